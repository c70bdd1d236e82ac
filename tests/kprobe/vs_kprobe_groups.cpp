// vs_kprobe_groups.cpp — test-only C entry points over the grouped-search
// launchers of csrc/vs_kernels.h (vs_group.hip) and the merge that follows
// them. tests/test_groups_stages_gpu.py is the user, through
// tests/kprobe/groups.py.
//
// Host C++ only, as vs_kprobe.cpp: raw device addresses, stream 0, the
// launcher's hipError_t back as an int. Built by build.py into
// lib/libvs_kprobe_groups.so, linked against libvsearch.so; not part of the
// product library.
#include <stdint.h>

#include "vs_kernels.h"

namespace {
template <class T>
T* P(uint64_t a) {
  return (T*)(uintptr_t)a;
}
}  // namespace

extern "C" {

uint32_t kpg_group_none() { return vsk::kGroupNone; }
uint32_t kpg_max_limit() { return vsk::kGroupsMaxLimit; }
uint32_t kpg_max_size() { return vsk::kGroupsMaxSize; }
uint32_t kpg_max_lists() { return vsk::kGroupsMaxLists; }
uint32_t kpg_rsel_bins() { return (uint32_t)vsk::kRselBins; }
uint32_t kpg_group_lists(uint32_t n_rows) { return vsk::group_lists(n_rows); }

int kpg_group_best(uint64_t sc, uint64_t gid, uint32_t n_rows, uint32_t row_base,
                   uint32_t n_groups, uint64_t best, uint64_t hist) {
  return (int)vsk::launch_group_best(P<const uint32_t>(sc), P<const uint32_t>(gid), n_rows,
                                     row_base, n_groups, P<uint64_t>(best), P<uint32_t>(hist),
                                     nullptr);
}

int kpg_group_heads(uint64_t sc, uint64_t gid, uint64_t best, uint32_t n_rows, uint32_t row_base,
                    uint32_t n_groups, uint32_t limit, uint64_t lists) {
  return (int)vsk::launch_group_heads(P<const uint32_t>(sc), P<const uint32_t>(gid),
                                      P<const uint64_t>(best), n_rows, row_base, n_groups, limit,
                                      P<uint64_t>(lists), nullptr);
}

int kpg_group_members(uint64_t sc, uint64_t gid, uint64_t best, uint32_t n_rows,
                      uint32_t row_base, uint32_t n_groups, uint64_t heads, uint32_t limit,
                      uint32_t group_size, uint64_t lists, uint64_t groups) {
  return (int)vsk::launch_group_members(P<const uint32_t>(sc), P<const uint32_t>(gid),
                                        P<const uint64_t>(best), n_rows, row_base, n_groups,
                                        P<const uint64_t>(heads), limit, group_size,
                                        P<uint64_t>(lists), P<uint32_t>(groups), nullptr);
}

int kpg_group_clear(uint64_t best, uint32_t n_groups) {
  return (int)vsk::launch_group_clear(P<uint64_t>(best), n_groups, nullptr);
}

int kpg_merge(uint64_t lists, uint32_t L, uint64_t lstride, uint64_t qstride, uint32_t nq,
              uint32_t kin, uint32_t k, uint64_t out) {
  return (int)vsk::launch_merge(P<const uint64_t>(lists), L, lstride, qstride, nq, kin, k,
                                P<uint64_t>(out), nullptr);
}

}  // extern "C"
