// TEST DOUBLE: tests/mmr/fake_engine_mmr.cpp (the logging double of the C-ABI)
// plus vs_search_fused by the rule of include/vsearch.h, for the CPU tests of
// /search's "fusion" object (tests/test_fuse_service.py). Never linked into the
// product. A fused call leaves one log line that carries every argument and a
// hash of each sub-query's bytes, in order.
#include "../mmr/fake_engine_mmr.cpp"

#include <map>

extern "C" int vs_search_fused(vs_engine* e, const char* coll, const float* q, uint32_t nq,
                               uint32_t n_sub, uint32_t dim, uint32_t k, uint32_t F, int fusion,
                               uint32_t rrf_k, uint64_t filter_id, float* os, uint64_t* orow,
                               uint32_t* ocnt) {
  {  // log_call's line is too short for eight hashes: the line is built here
    char buf[160];
    std::snprintf(buf, sizeof buf,
                  "vs_search_fused %s nq=%u n_sub=%u dim=%u k=%u F=%u fusion=%d rrf_k=%u filter=%" PRIu64,
                  coll, nq, n_sub, dim, k, F, fusion, rrf_k, filter_id);
    std::string line = buf;
    for (uint64_t l = 0; l < (uint64_t)nq * n_sub; ++l) {
      std::snprintf(buf, sizeof buf, " q=%016" PRIx64, bytes_hash(q + (size_t)l * dim, (size_t)dim * 4));
      line += buf;
    }
    std::lock_guard<std::mutex> g(g_log_mu);
    g_log += line + "\n";
  }
  if (n_sub == 0 || n_sub > VS_FUSE_MAX_LISTS) return fail(VS_ERR_INVALID_ARG, "n_sub");
  if (k == 0 || k > VS_FUSE_MAX_LIMIT) return fail(VS_ERR_INVALID_ARG, "k");
  if (F == 0) F = std::min<uint32_t>(4 * k, VS_FUSE_MAX_LIMIT);
  if (F > VS_FUSE_MAX_LIMIT || k > F) return fail(VS_ERR_INVALID_ARG, "prefetch_limit");
  if (fusion != VS_FUSION_RRF && fusion != VS_FUSION_DBSF) return fail(VS_ERR_INVALID_ARG, "fusion");
  if (rrf_k > 65536 || (fusion == VS_FUSION_DBSF && rrf_k)) return fail(VS_ERR_INVALID_ARG, "rrf_k");
  const uint32_t K = rrf_k ? rrf_k : 2, nsq = nq * n_sub;
  // the lists: the double's own search of all sub-queries with k = F, under the filter
  std::vector<float> cs((size_t)nsq * F);
  std::vector<uint64_t> cr((size_t)nsq * F);
  std::vector<uint32_t> cc(nsq);
  const int rc = filter_id
                     ? vs_search_filter_id_plain(e, coll, q, nsq, dim, F, filter_id, cs.data(),
                                                 cr.data(), cc.data())
                     : vs_search_plain(e, coll, q, nsq, dim, F, cs.data(), cr.data(), cc.data());
  if (rc != VS_OK) return rc;
  for (uint32_t i = 0; i < nq; ++i) {
    std::map<uint64_t, float> fused;  // row -> sum, terms added in ascending l
    for (uint32_t l = 0; l < n_sub; ++l) {
      const uint32_t li = i * n_sub + l, n = cc[li];
      const float* s = cs.data() + (size_t)li * F;
      double mu = 0, var = 0;
      for (uint32_t p = 0; p < n; ++p) mu += s[p];
      if (n) mu /= n;
      for (uint32_t p = 0; p < n; ++p) var += ((double)s[p] - mu) * ((double)s[p] - mu);
      const double sigma = n > 1 ? std::sqrt(var / (n - 1)) : 0.0;
      for (uint32_t p = 0; p < n; ++p) {
        float t;
        if (fusion == VS_FUSION_RRF) t = 1.0f / (float)(p + K);
        else t = sigma > 0 ? (float)(((double)s[p] - (mu - 3 * sigma)) / (6 * sigma)) : 0.5f;
        auto it = fused.find(cr[(size_t)li * F + p]);
        if (it == fused.end()) fused[cr[(size_t)li * F + p]] = t;
        else it->second = it->second + t;
      }
    }
    std::vector<std::pair<float, uint64_t>> v;
    for (auto& kv : fused) v.push_back({kv.second, kv.first});
    std::sort(v.begin(), v.end(), [](const auto& a, const auto& b) {
      return a.first > b.first || (a.first == b.first && a.second < b.second);
    });
    const uint32_t m = (uint32_t)std::min<size_t>(k, v.size());
    for (uint32_t j = 0; j < k; ++j) {
      os[(size_t)i * k + j] = j < m ? v[j].first : 0.f;
      orow[(size_t)i * k + j] = j < m ? v[j].second : 0;
    }
    ocnt[i] = m;
  }
  return VS_OK;
}
