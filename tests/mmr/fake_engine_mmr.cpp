// TEST DOUBLE: tests/delete/fake_engine_delete.cpp plus vs_search_mmr by the
// rule of include/vsearch.h, and a log of every search call the service makes,
// for the CPU tests of /search's "mmr" object (tests/test_mmr_service.py).
// Never linked into the product. The three plain search entry points are the
// double's own, renamed and wrapped so that each call leaves one log line;
// fake_calls() hands the log over and clears it.
#define vs_search vs_search_plain
#define vs_search_filtered vs_search_filtered_plain
#define vs_search_filter_id vs_search_filter_id_plain
#include "../delete/fake_engine_delete.cpp"
#undef vs_search
#undef vs_search_filtered
#undef vs_search_filter_id

#include <cinttypes>

namespace {

std::mutex g_log_mu;
std::string g_log;

// FNV-1a of the query bytes: two calls carried the same floats iff equal
uint64_t bytes_hash(const void* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  return h;
}

void log_call(const char* what, const char* coll, const float* q, uint32_t nq, uint32_t dim,
              uint32_t k, const std::string& extra) {
  char line[256];
  std::snprintf(line, sizeof line, "%s %s nq=%u dim=%u k=%u q=%016" PRIx64 "%s\n", what, coll, nq,
                dim, k, bytes_hash(q, (size_t)nq * dim * 4), extra.c_str());
  std::lock_guard<std::mutex> g(g_log_mu);
  g_log += line;
}

}  // namespace

extern "C" {

// Copies the log (NUL-terminated, truncated to len - 1) and clears it.
size_t fake_calls(char* buf, size_t len) {
  std::lock_guard<std::mutex> g(g_log_mu);
  const size_t n = std::min(g_log.size(), len ? len - 1 : 0);
  if (len) {
    std::memcpy(buf, g_log.data(), n);
    buf[n] = 0;
  }
  g_log.clear();
  return n;
}

int vs_search(vs_engine* e, const char* coll, const float* q, uint32_t nq, uint32_t dim,
              uint32_t k, float* os, uint64_t* orow, uint32_t* ocnt) {
  log_call("vs_search", coll, q, nq, dim, k, "");
  return vs_search_plain(e, coll, q, nq, dim, k, os, orow, ocnt);
}

int vs_search_filtered(vs_engine* e, const char* coll, const float* q, uint32_t nq, uint32_t dim,
                       uint32_t k, const uint64_t* allow, uint64_t words, float* os,
                       uint64_t* orow, uint32_t* ocnt) {
  log_call("vs_search_filtered", coll, q, nq, dim, k, "");
  return vs_search_filtered_plain(e, coll, q, nq, dim, k, allow, words, os, orow, ocnt);
}

int vs_search_filter_id(vs_engine* e, const char* coll, const float* q, uint32_t nq, uint32_t dim,
                        uint32_t k, uint64_t id, float* os, uint64_t* orow, uint32_t* ocnt) {
  log_call("vs_search_filter_id", coll, q, nq, dim, k, " filter=" + std::to_string(id));
  return vs_search_filter_id_plain(e, coll, q, nq, dim, k, id, os, orow, ocnt);
}

int vs_search_mmr(vs_engine* e, const char* coll, const float* q, uint32_t nq, uint32_t dim,
                  uint32_t k, uint32_t F, float d, uint64_t filter_id, float* os, uint64_t* orow,
                  uint32_t* ocnt) {
  char extra[96];
  std::snprintf(extra, sizeof extra, " F=%u d=%.9g filter=%" PRIu64, F, (double)d, filter_id);
  log_call("vs_search_mmr", coll, q, nq, dim, k, extra);
  if (k == 0 || k > VS_MMR_MAX_CANDIDATES) return fail(VS_ERR_INVALID_ARG, "k");
  if (F == 0) F = std::min<uint32_t>(4 * k, VS_MMR_MAX_CANDIDATES);
  if (F > VS_MMR_MAX_CANDIDATES || k > F) return fail(VS_ERR_INVALID_ARG, "candidates_limit");
  if (!(d >= 0.f && d <= 1.f)) return fail(VS_ERR_INVALID_ARG, "diversity");
  // the candidates: the double's own search with k = F, under the filter
  std::vector<float> cs((size_t)nq * F);
  std::vector<uint64_t> cr((size_t)nq * F);
  std::vector<uint32_t> cc(nq);
  const int rc = filter_id
                     ? vs_search_filter_id_plain(e, coll, q, nq, dim, F, filter_id, cs.data(),
                                                 cr.data(), cc.data())
                     : vs_search_plain(e, coll, q, nq, dim, F, cs.data(), cr.data(), cc.data());
  if (rc != VS_OK) return rc;
  std::shared_lock<std::shared_mutex> g(e->mu);
  const Coll& c = *e->colls.find(coll)->second;
  const float a = 1.0f - d;
  for (uint32_t i = 0; i < nq; ++i) {
    const uint32_t n = cc[i];
    const float* s = cs.data() + (size_t)i * F;
    const uint64_t* r = cr.data() + (size_t)i * F;
    std::vector<float> pen(n, -INFINITY);
    std::vector<char> used(n, 0);
    uint32_t m = 0;
    for (; m < std::min(k, n); ++m) {
      uint32_t best = n;
      float bv = 0;
      for (uint32_t j = 0; j < n; ++j) {
        if (used[j]) continue;
        const float p1 = a * s[j], p2 = d * pen[j];  // two roundings, then the difference
        const float v = m == 0 ? 0.f : p1 - p2;
        if (best == n || v > bv) best = j, bv = v;
      }
      used[best] = 1;
      os[(size_t)i * k + m] = s[best];
      orow[(size_t)i * k + m] = r[best];
      for (uint32_t j = 0; j < n; ++j)
        pen[j] = std::max(pen[j], dot(c.rows.data() + r[j] * dim, c.rows.data() + r[best] * dim, dim));
    }
    ocnt[i] = m;
    for (uint32_t j = m; j < k; ++j) os[(size_t)i * k + j] = 0.f, orow[(size_t)i * k + j] = 0;
  }
  return VS_OK;
}

}  // extern "C"
