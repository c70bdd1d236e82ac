// TEST DOUBLE: tests/mmr/fake_engine_mmr.cpp plus vs_grouping_create,
// vs_grouping_drop and vs_search_groups by the rule of include/vsearch.h, for
// the CPU tests of /search's "group_by" (tests/test_groups_service.py) and
// their ThreadSanitizer driver (tests/groups/tsan_groups_driver.cpp). Never
// linked into the product. Every grouping call leaves a log line (fake_calls()
// of the MMR double hands the log over); vs_delete and vs_collection_drop are
// the doubles' own, wrapped so that they drop the collection's groupings as the
// engine does; fake_stale_groupings() counts the searches that arrived with a
// grouping built for another state of the collection.
#define vs_delete vs_delete_plain
#define vs_collection_drop vs_collection_drop_plain
#include "../mmr/fake_engine_mmr.cpp"
#undef vs_delete
#undef vs_collection_drop

#include <atomic>

namespace {

struct Grouping {
  vs_engine* eng;
  std::string coll;
  uint64_t rows;
  uint32_t n_groups;
  std::vector<uint32_t> gor;
};

std::mutex g_grp_mu;
std::map<uint64_t, Grouping> g_groupings;
uint64_t g_next_grouping = 1;
std::atomic<uint64_t> g_stale{0};

void log_line(const std::string& line) {
  std::lock_guard<std::mutex> g(g_log_mu);
  g_log += line + "\n";
}

void drop_groupings_of(vs_engine* e, const char* coll) {
  std::lock_guard<std::mutex> g(g_grp_mu);
  for (auto it = g_groupings.begin(); it != g_groupings.end();)
    it = it->second.eng == e && it->second.coll == coll ? g_groupings.erase(it) : std::next(it);
}

}  // namespace

extern "C" {

uint64_t fake_stale_groupings(void) { return g_stale.load(); }

int vs_delete(vs_engine* e, const char* coll, uint64_t n, const uint64_t* rows,
              uint64_t* moved_from, uint64_t* moved_to, uint64_t* n_moved) {
  const int rc = vs_delete_plain(e, coll, n, rows, moved_from, moved_to, n_moved);
  if (rc == VS_OK && n) drop_groupings_of(e, coll ? coll : "");
  return rc;
}

int vs_collection_drop(vs_engine* e, const char* name) {
  const int rc = vs_collection_drop_plain(e, name);
  if (rc == VS_OK) drop_groupings_of(e, name);
  return rc;
}

int vs_grouping_create(vs_engine* e, const char* coll, const uint32_t* gor, uint64_t n_rows,
                       uint32_t n_groups, uint64_t* id) {
  std::shared_lock<std::shared_mutex> g(e->mu);
  auto it = e->colls.find(coll ? coll : "");
  if (it == e->colls.end()) return fail(VS_ERR_NOT_FOUND, "not found");
  if (n_rows != it->second->n()) return fail(VS_ERR_INVALID_ARG, "grouping: wrong row count");
  if (n_groups > std::max<uint64_t>(n_rows, 1)) return fail(VS_ERR_INVALID_ARG, "n_groups");
  for (uint64_t r = 0; r < n_rows; ++r)
    if (gor[r] >= n_groups && gor[r] != VS_GROUP_NONE) return fail(VS_ERR_INVALID_ARG, "group id");
  std::lock_guard<std::mutex> gg(g_grp_mu);
  *id = g_next_grouping++;
  g_groupings[*id] = Grouping{e, coll, n_rows, n_groups, std::vector<uint32_t>(gor, gor + n_rows)};
  log_line("vs_grouping_create " + std::string(coll) + " rows=" + std::to_string(n_rows) +
           " groups=" + std::to_string(n_groups) + " id=" + std::to_string(*id));
  return VS_OK;
}

int vs_grouping_drop(vs_engine*, uint64_t id) {
  std::lock_guard<std::mutex> g(g_grp_mu);
  log_line("vs_grouping_drop id=" + std::to_string(id));
  return g_groupings.erase(id) ? VS_OK : fail(VS_ERR_NOT_FOUND, "no grouping");
}

int vs_search_groups(vs_engine* e, const char* coll, const float* q, uint32_t nq, uint32_t dim,
                     uint32_t limit, uint32_t S, uint64_t grouping_id, uint64_t filter_id,
                     uint32_t* og, uint32_t* oh, float* os, uint64_t* orow, uint32_t* ocnt) {
  char extra[96];
  std::snprintf(extra, sizeof extra, " S=%u grouping=%" PRIu64 " filter=%" PRIu64, S, grouping_id,
                filter_id);
  log_call("vs_search_groups", coll, q, nq, dim, limit, extra);
  if (limit == 0 || limit > VS_GROUPS_MAX_LIMIT) return fail(VS_ERR_INVALID_ARG, "limit");
  if (S == 0 || S > VS_GROUPS_MAX_SIZE) return fail(VS_ERR_INVALID_ARG, "group_size");
  std::shared_lock<std::shared_mutex> g(e->mu);
  auto it = e->colls.find(coll ? coll : "");
  if (it == e->colls.end()) return fail(VS_ERR_NOT_FOUND, "not found");
  const Coll& c = *it->second;
  if (dim != c.dim) return fail(VS_ERR_DIM_MISMATCH, "dim");
  std::vector<uint32_t> gor;
  {
    std::lock_guard<std::mutex> gg(g_grp_mu);
    auto gi = g_groupings.find(grouping_id);
    if (gi == g_groupings.end()) {
      ++g_stale;
      return fail(VS_ERR_NOT_FOUND, "no grouping");
    }
    if (gi->second.eng != e || gi->second.coll != coll || gi->second.rows != c.n()) {
      ++g_stale;
      return fail(VS_ERR_INVALID_ARG, "stale grouping");
    }
    gor = gi->second.gor;
  }
  const uint64_t* allow = nullptr;
  if (filter_id) {
    auto f = e->filters.find(filter_id);
    if (f == e->filters.end() || f->second.coll != coll || f->second.rows != c.n())
      return fail(VS_ERR_INVALID_ARG, "stale filter");
    allow = f->second.bits.data();
  }
  std::vector<float> qq(dim);
  for (uint32_t i = 0; i < nq; ++i) {
    std::memcpy(qq.data(), q + (size_t)i * dim, dim * sizeof(float));
    if (c.metric == VS_METRIC_COSINE) normalise(qq.data(), dim);
    std::vector<std::pair<float, uint64_t>> hits;  // the eligible rows, ranked
    for (uint64_t r = 0; r < c.n(); ++r) {
      if (gor[r] == VS_GROUP_NONE) continue;
      if (allow && !((allow[r / 64] >> (r % 64)) & 1)) continue;
      hits.push_back({dot(c.rows.data() + r * dim, qq.data(), dim), r});
    }
    std::sort(hits.begin(), hits.end(), [](auto& a, auto& b) {
      return a.first != b.first ? a.first > b.first : a.second < b.second;
    });
    // walking the ranking meets every group at its best row first
    uint32_t* G = og + (size_t)i * limit;
    uint32_t* H = oh + (size_t)i * limit;
    float* Sc = os + (size_t)i * limit * S;
    uint64_t* R = orow + (size_t)i * limit * S;
    std::fill(G, G + limit, 0u);
    std::fill(H, H + limit, 0u);
    std::fill(Sc, Sc + (size_t)limit * S, 0.f);
    std::fill(R, R + (size_t)limit * S, 0ull);
    uint32_t ng = 0;
    std::map<uint32_t, uint32_t> slot;
    for (const auto& h : hits) {
      const uint32_t grp = gor[h.second];
      auto s = slot.find(grp);
      if (s == slot.end()) {
        if (ng == limit) continue;
        s = slot.emplace(grp, ng).first;
        G[ng++] = grp;
      }
      const uint32_t j = s->second;
      if (H[j] == S) continue;
      Sc[(size_t)j * S + H[j]] = h.first;
      R[(size_t)j * S + H[j]] = h.second;
      ++H[j];
    }
    ocnt[i] = ng;
  }
  return VS_OK;
}

}  // extern "C"
