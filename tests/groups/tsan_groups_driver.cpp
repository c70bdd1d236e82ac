// ThreadSanitizer driver for /search's "group_by" (tests/test_groups_service.py).
// A stand-alone program: built with -fsanitize=thread from csrc/service/*.cpp,
// the CPU test double tests/groups/fake_engine_groups.cpp and this file.
//
// Threads run grouped searches, /upsert and /delete (by ids and by filter) on
// one Dot collection at once, as tests/delete/tsan_delete_driver.cpp does for
// plain searches. Every point's vector is a function of its id (exact in fp32:
// multiples of 1/8) and its payload names its id and its group, so each grouped
// answer can be held to ONE version of the collection:
//   * for every hit, payload.pid equals the id and the score equals the exact
//     dot of the query with that id's vector;
//   * "results" is flat in the order of "groups": each group's hits are
//     adjacent, carry its id in payload.g, number groups[j].hits (1..size),
//     and fall in score; the groups' best scores fall too; no group twice.
// The grouping cached by the service is rebuilt after every /upsert and
// /delete; a search that reached the engine with a grouping built for another
// state of the collection is counted by the double (fake_stale_groupings) and
// fails the run. Exit status 0 and no TSAN report is the pass condition.
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

extern "C" uint64_t fake_stale_groupings(void);

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

// Holds a grouped /search answer to one version; returns the ids it names.
std::set<std::string> check_answer(const std::string& resp, uint32_t qt, uint32_t qj, int top_k,
                                   int size) {
  std::set<std::string> ids;
  Json root;
  std::string err;
  if (!vsjson::parse(resp.data(), resp.size(), &root, &err)) {
    bad("answer does not parse", resp);
    return ids;
  }
  const Json* res = root.get("results");
  const Json* groups = root.get("groups");
  const Json* count = root.get("count");
  if (!res || res->kind != Json::Array || !groups || groups->kind != Json::Array || !count) {
    bad("no results / groups / count", resp);
    return ids;
  }
  if ((size_t)count->num != res->arr.size()) bad("count is not the results' length", resp);
  if (groups->arr.size() > (size_t)top_k) bad("more groups than top_k", resp);
  size_t at = 0;
  double prev_head = 1e300;
  std::set<std::string> seen;
  for (const Json& g : groups->arr) {
    const Json* gid = g.get("id");
    const Json* nh = g.get("hits");
    if (!gid || gid->kind != Json::String || !nh || nh->num < 1 || nh->num > size ||
        at + (size_t)nh->num > res->arr.size()) {
      bad("malformed group", resp);
      return ids;
    }
    if (!seen.insert(gid->str).second) bad("a group twice in one answer", gid->str);
    double prev = 1e300;
    for (size_t h = 0; h < (size_t)nh->num; ++h, ++at) {
      const Json& hit = res->arr[at];
      const Json* id = hit.get("id");
      const Json* score = hit.get("score");
      const Json* pl = hit.get("payload");
      const Json* pid = pl ? pl->get("pid") : nullptr;
      const Json* pg = pl ? pl->get("g") : nullptr;
      uint32_t t = 0, j = 0;
      if (!id || !score || !pid || !pg || !parse_uuid(id->str, &t, &j)) {
        bad("malformed hit", resp);
        continue;
      }
      if (pid->str != id->str) bad("payload of another point", id->str + " vs " + pid->str);
      if (pg->str != gid->str) bad("hit outside its group", id->str);
      double want = 0;
      for (int d = 0; d < kDim; ++d) want += (double)comp(qt, qj, d) * (double)comp(t, j, d);
      if (score->num != want) bad("score of another row", id->str);
      if (score->num > prev) bad("a group's hits do not fall in score", id->str);
      prev = score->num;
      if (h == 0) {
        if (score->num > prev_head) bad("the groups' best scores do not fall", gid->str);
        prev_head = score->num;
      }
      if (!ids.insert(id->str).second) bad("id twice in one answer", id->str);
    }
  }
  if (at != res->arr.size()) bad("results outside the groups", resp);
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
      std::mt19937 rng(99 + ti);
      std::vector<uint32_t> live, gone;
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
      auto search = [&](uint32_t qj, int k, int size) {
        const std::string body = "{\"collection\":\"a\",\"query\":" + vec_json(t, qj) +
                                 ",\"top_k\":" + std::to_string(k) + ",\"group_by\":\"g\"," +
                                 "\"group_size\":" + std::to_string(size) + "}";
        std::string resp;
        if (call(svc, "POST", "/search", body, &resp) != 200) bad("search status", resp);
        auto ids = check_answer(resp, t, qj, k, size);
        n_hits += (long)ids.size();
        for (uint32_t g : gone)
          if (ids.count(uuid(t, g))) bad("a deleted id came back", uuid(t, g));
        return ids;
      };
      for (int i = 0; i < iters; ++i) {
        switch ((i + ti) % 5) {
          case 0: {  // four new points: one group
            std::vector<uint32_t> js;
            for (int p = 0; p < 4; ++p) js.push_back(next++);
            upsert(js);
            live.insert(live.end(), js.begin(), js.end());
            break;
          }
          case 1:
          case 2: {  // grouped search near an own point
            if (live.empty()) break;
            search(live[rng() % live.size()], 1 + i % 9, 1 + i % 4);
            break;
          }
          case 3: {  // delete one own point by id
            if (live.empty()) break;
            const size_t at = rng() % live.size();
            const std::string body =
                "{\"collection\":\"a\",\"ids\":[\"" + uuid(t, live[at]) + "\"]}";
            gone.push_back(live[at]);
            live.erase(live.begin() + (long)at);
            std::string resp;
            if (call(svc, "POST", "/delete", body, &resp) != 200) bad("delete status", resp);
            ++n_del;
            if (!live.empty()) search(live[0], 128, 16);
            break;
          }
          default: {  // delete one own group by filter, then look for it
            if (live.empty()) break;
            const std::string g = group_of(live[rng() % live.size()]);
            for (size_t at = 0; at < live.size();)
              if (group_of(live[at]) == g) {
                gone.push_back(live[at]);
                live.erase(live.begin() + (long)at);
                ++n_del;
              } else {
                ++at;
              }
            std::string resp;
            if (call(svc, "POST", "/delete",
                     "{\"collection\":\"a\",\"filter\":{\"g\":\"" + g + "\"}}", &resp) != 200)
              bad("delete status", resp);
            if (!live.empty()) search(live[rng() % live.size()], 5, 3);
            break;
          }
        }
      }
    });
  for (auto& th : pool) th.join();
  vsvc_close(svc);
  vs_close(eng);
  if (fake_stale_groupings()) bad("a stale grouping id reached the engine");
  if (g_bad.load()) {
    std::fprintf(stderr, "violations: %d\n", g_bad.load());
    return 9;
  }
  if (n_del.load() == 0 || n_hits.load() == 0) return 10;
  std::printf("ok %d threads x %d iterations, %ld deleted, %ld hits checked\n", threads, iters,
              n_del.load(), n_hits.load());
  return 0;
}
