// ThreadSanitizer driver for the service's /delete route
// (tests/test_delete_service.py). A stand-alone program: built with
// -fsanitize=thread from csrc/service/*.cpp, the CPU test double
// tests/delete/fake_engine_delete.cpp and this file.
//
// Threads run /upsert, /search (plain and filtered) and /delete (by ids and by
// filter) on one Dot collection at once. Every point's vector is a function of
// its id (exact in fp32: small multiples of 1/8) and its payload names its id,
// so each search answer can be held to ONE version of the collection: for
// every hit, payload.pid equals the id (id and payload of the same row), and
// the score equals the exact dot of the query with that id's vector (the row
// the engine scored is the row the id was decoded from). A delete renumbering
// ids apart from the engine's move, or a search decoding after the lock was
// dropped, breaks one of the two. A thread also checks that ids it deleted
// never come back until it upserts them again.
// Exit status 0 and no TSAN report is the pass condition.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/vsearch_service.h"
#include "json.h"  // csrc/service (on the include path)

using vsjson::Json;

namespace {

constexpr int kDim = 16;
std::atomic<int> g_bad{0};

void bad(const char* what, const std::string& detail = "") {
  if (g_bad++ < 10) std::fprintf(stderr, "BAD %s %s\n", what, detail.c_str());
}

int call(vsvc* s, const char* method, const char* path, const std::string& body, std::string* out) {
  int status = 0;
  char* resp = nullptr;
  size_t len = 0;
  const char* ct = nullptr;
  if (vsvc_handle(s, method, path, body.data(), body.size(), &status, &resp, &len, &ct) != VS_OK)
    bad("vsvc_handle");
  if (out) out->assign(resp ? resp : "", resp ? len : 0);
  vsvc_free(resp);
  return status;
}

std::string uuid(uint32_t t, uint32_t j) {
  char b[40];
  std::snprintf(b, sizeof b, "%08x-0000-4000-8000-%012x", t, j);
  return b;
}

// component d of the vector of point (t, j): a multiple of 1/8 in [-1, 1]
float comp(uint32_t t, uint32_t j, int d) {
  uint64_t x = ((uint64_t)t << 40) ^ ((uint64_t)j << 8) ^ (uint64_t)d;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (float)((int)(x % 17) - 8) / 8.0f;
}

std::string vec_json(uint32_t t, uint32_t j) {
  std::string s = "[";
  for (int d = 0; d < kDim; ++d) {
    char b[32];
    std::snprintf(b, sizeof b, "%s%.3f", d ? "," : "", comp(t, j, d));
    s += b;
  }
  return s + "]";
}

bool parse_uuid(const std::string& id, uint32_t* t, uint32_t* j) {
  if (id.size() != 36) return false;
  *t = (uint32_t)std::strtoul(id.substr(0, 8).c_str(), nullptr, 16);
  *j = (uint32_t)std::strtoul(id.substr(24).c_str(), nullptr, 16);
  return uuid(*t, *j) == id;
}

// Holds a /search answer to one version; returns the ids it names.
std::set<std::string> check_answer(const std::string& resp, uint32_t qt, uint32_t qj,
                                   const char* group) {
  std::set<std::string> ids;
  Json root;
  std::string err;
  if (!vsjson::parse(resp.data(), resp.size(), &root, &err)) {
    bad("answer does not parse", resp);
    return ids;
  }
  const Json* res = root.get("results");
  if (!res || res->kind != Json::Array) {
    bad("no results", resp);
    return ids;
  }
  for (const Json& hit : res->arr) {
    const Json* id = hit.get("id");
    const Json* score = hit.get("score");
    const Json* pl = hit.get("payload");
    const Json* pid = pl ? pl->get("pid") : nullptr;
    uint32_t t = 0, j = 0;
    if (!id || !score || !pid || !parse_uuid(id->str, &t, &j)) {
      bad("malformed hit", resp);
      continue;
    }
    if (pid->str != id->str) bad("payload of another point", id->str + " vs " + pid->str);
    double want = 0;
    for (int d = 0; d < kDim; ++d) want += (double)comp(qt, qj, d) * (double)comp(t, j, d);
    if (score->num != want) bad("score of another row", id->str);
    if (group) {
      const Json* g = pl->get("g");
      if (!g || g->str != group) bad("hit outside the filter", id->str);
    }
    if (!ids.insert(id->str).second) bad("id twice in one answer", id->str);
  }
  return ids;
}

}  // namespace

int main(int argc, char** argv) {
  const int threads = argc > 1 ? std::atoi(argv[1]) : 8;
  const int iters = argc > 2 ? std::atoi(argv[2]) : 60;
  vs_engine* eng = nullptr;
  if (vs_open(nullptr, &eng) != VS_OK) return 2;
  const char* cfg =
      "{\"collections\":[{\"name\":\"a\",\"dim\":16,\"metric\":\"Dot\"}],"
      "\"batching\":{\"enabled\":true,\"max_batch\":16,\"max_wait_us\":200,\"workers\":2},"
      "\"filter\":\"match\"}";
  vsvc* svc = nullptr;
  if (vsvc_open(eng, cfg, &svc) != VS_OK) return 3;
  std::atomic<long> n_del{0}, n_hits{0};

  std::vector<std::thread> pool;
  for (int ti = 0; ti < threads; ++ti)
    pool.emplace_back([&, ti] {
      const uint32_t t = 0x100 + (uint32_t)ti;  // this thread's ids: uuid(t, *)
      std::mt19937 rng(77 + ti);
      std::vector<uint32_t> live;  // own points in the collection
      std::vector<uint32_t> gone;  // own points deleted and not upserted again
      uint32_t next = 0;
      auto group_of = [&](uint32_t j) { return "g" + std::to_string(t) + "-" + std::to_string(j / 4); };
      auto upsert = [&](const std::vector<uint32_t>& js) {
        std::string body = "{\"collection\":\"a\",\"points\":[";
        for (size_t p = 0; p < js.size(); ++p)
          body += std::string(p ? "," : "") + "{\"id\":\"" + uuid(t, js[p]) + "\",\"vector\":" +
                  vec_json(t, js[p]) + ",\"payload\":{\"pid\":\"" + uuid(t, js[p]) + "\",\"g\":\"" +
                  group_of(js[p]) + "\"}}";
        body += "]}";
        if (call(svc, "POST", "/upsert", body, nullptr) != 200) bad("upsert status");
      };
      auto search = [&](uint32_t qt, uint32_t qj, int k, const char* group) {
        std::string body = "{\"collection\":\"a\",\"query\":" + vec_json(qt, qj) +
                           ",\"top_k\":" + std::to_string(k);
        if (group) body += std::string(",\"filter\":{\"g\":\"") + group + "\"}";
        body += "}";
        std::string resp;
        if (call(svc, "POST", "/search", body, &resp) != 200) bad("search status", resp);
        auto ids = check_answer(resp, qt, qj, group);
        n_hits += (long)ids.size();
        return ids;
      };
      auto deleted_count = [&](const std::string& resp) {
        Json root;
        std::string err;
        const Json* d = vsjson::parse(resp.data(), resp.size(), &root, &err) ? root.get("deleted")
                                                                              : nullptr;
        return d ? (long)d->num : -1L;
      };
      auto stay_gone = [&] {  // none of this thread's deleted ids is ever returned
        if (gone.empty()) return;
        const uint32_t j = gone[rng() % gone.size()];
        const auto ids = search(t, j, 1024, nullptr);
        for (uint32_t g : gone)
          if (ids.count(uuid(t, g))) bad("a deleted id came back", uuid(t, g));
      };
      for (int i = 0; i < iters; ++i) {
        switch ((i + ti) % 6) {
          case 0:
          case 1: {  // four new points (one group), or a deleted id again: a new point
            std::vector<uint32_t> js;
            if (!gone.empty() && i % 4 == 1) {
              js.push_back(gone.back());
              gone.pop_back();
            } else {
              for (int p = 0; p < 4; ++p) js.push_back(next++);
            }
            upsert(js);
            live.insert(live.end(), js.begin(), js.end());
            break;
          }
          case 2: {  // search near one of the own points, or anywhere
            if (live.empty()) break;
            search(t, live[rng() % live.size()], 1 + i % 9, nullptr);
            stay_gone();
            break;
          }
          case 3: {  // delete two own points and an id nobody has
            if (live.size() < 2) break;
            std::string body = "{\"collection\":\"a\",\"ids\":[\"" + uuid(0xdead, (uint32_t)i) + "\"";
            for (int p = 0; p < 2; ++p) {
              const size_t at = rng() % live.size();
              body += ",\"" + uuid(t, live[at]) + "\"";
              gone.push_back(live[at]);
              live.erase(live.begin() + (long)at);
            }
            body += "]}";
            std::string resp;
            if (call(svc, "POST", "/delete", body, &resp) != 200) bad("delete status", resp);
            if (deleted_count(resp) != 2) bad("deleted count", resp);
            n_del += 2;
            stay_gone();
            break;
          }
          case 4: {  // delete one own group by filter
            if (live.empty()) break;
            const std::string g = group_of(live[rng() % live.size()]);
            long want = 0;
            for (size_t at = 0; at < live.size();)
              if (group_of(live[at]) == g) {
                gone.push_back(live[at]);
                live.erase(live.begin() + (long)at);
                ++want;
              } else {
                ++at;
              }
            std::string resp;
            if (call(svc, "POST", "/delete",
                     "{\"collection\":\"a\",\"filter\":{\"g\":\"" + g + "\"}}", &resp) != 200)
              bad("delete status", resp);
            if (deleted_count(resp) != want) bad("deleted-by-filter count", resp);
            n_del += want;
            stay_gone();
            break;
          }
          default: {  // filtered search of an own group: exactly its live points
            if (live.empty()) break;
            const uint32_t j = live[rng() % live.size()];
            const std::string g = group_of(j);
            const auto ids = search(t, j, 8, g.c_str());
            std::set<std::string> want;
            for (uint32_t l : live)
              if (group_of(l) == g) want.insert(uuid(t, l));
            if (ids != want) bad("filtered answer is not the group", g);
            if (call(svc, "GET", "/delete", "", nullptr) != 405) bad("405");
            break;
          }
        }
      }
    });
  for (auto& th : pool) th.join();
  vsvc_close(svc);
  vs_close(eng);
  if (g_bad.load()) {
    std::fprintf(stderr, "violations: %d\n", g_bad.load());
    return 9;
  }
  if (n_del.load() == 0 || n_hits.load() == 0) return 10;
  std::printf("ok %d threads x %d iterations, %ld deleted, %ld hits checked\n", threads, iters,
              n_del.load(), n_hits.load());
  return 0;
}
