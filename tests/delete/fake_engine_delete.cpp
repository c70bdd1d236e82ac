// TEST DOUBLE: tests/tsan/fake_engine.cpp plus vs_delete, for the CPU tests of
// the service's /delete route (tests/test_delete_service.py) and their
// ThreadSanitizer driver (tests/delete/tsan_delete_driver.cpp). Never linked
// into the product. vs_delete follows the rule of include/vsearch.h: holes
// below the new row count take the surviving tail rows, both ascending, and
// the collection is truncated; the collection's filters are dropped.
#include "../tsan/fake_engine.cpp"

#include <set>

extern "C" int vs_delete(vs_engine* e, const char* coll, uint64_t n, const uint64_t* rows,
                         uint64_t* moved_from, uint64_t* moved_to, uint64_t* n_moved) {
  if (n_moved) *n_moved = 0;
  std::unique_lock<std::shared_mutex> g(e->mu);
  auto it = e->colls.find(coll ? coll : "");
  if (it == e->colls.end()) return fail(VS_ERR_NOT_FOUND, "not found");
  if (n == 0) return VS_OK;
  Coll& c = *it->second;
  const uint64_t N = c.n();
  std::set<uint64_t> del(rows, rows + n);
  if (*del.rbegin() >= N) return fail(VS_ERR_INVALID_ARG, "delete: row past the rows");
  const uint64_t Nn = N - del.size();
  uint64_t p = 0, t = Nn;
  for (uint64_t h : del) {
    if (h >= Nn) break;
    while (del.count(t)) ++t;
    std::memcpy(c.rows.data() + h * c.dim, c.rows.data() + t * c.dim, c.dim * sizeof(float));
    moved_from[p] = t++;
    moved_to[p++] = h;
  }
  c.rows.resize(Nn * c.dim);
  *n_moved = p;
  for (auto f = e->filters.begin(); f != e->filters.end();)
    f = f->second.coll == coll ? e->filters.erase(f) : std::next(f);
  return VS_OK;
}
