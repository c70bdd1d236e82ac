// TEST DOUBLE: tests/delete/fake_engine_delete.cpp whose vs_delete can be told
// to fail AFTER it compacted the rows (fake_fail_next_delete(1)), as the engine
// does when a device error loses the moved pairs: the service must not go on
// serving ids that no longer match the engine's rows.
#define vs_delete vs_delete_compacting
#include "fake_engine_delete.cpp"
#undef vs_delete

static int g_fail_next = 0;

extern "C" void fake_fail_next_delete(int on) { g_fail_next = on; }

extern "C" int vs_delete(vs_engine* e, const char* coll, uint64_t n, const uint64_t* rows,
                         uint64_t* moved_from, uint64_t* moved_to, uint64_t* n_moved) {
  const int rc = vs_delete_compacting(e, coll, n, rows, moved_from, moved_to, n_moved);
  if (rc != VS_OK || !g_fail_next) return rc;
  g_fail_next = 0;
  *n_moved = 0;
  return fail(VS_ERR_DEVICE, "injected: the rows were already compacted");
}
