// vs_kprobe_runif.cpp — one more test-only C entry point beside vs_kprobe.cpp:
// the int8 pass with its run_if word (the launch stands down when the word
// is 0), which kp_mfma_cand_q8 does not pass on. tests/test_q8_split_wg_gpu.py
// is the user.
//
// Host C++ only, as vs_kprobe.cpp: raw device addresses, stream 0, the
// launcher's hipError_t back as an int. Built by build.py into
// lib/libvs_kprobe_runif.so, linked against libvsearch.so; not part of the
// product library.
#include <stdint.h>

#include "vs_kernels.h"

namespace {
template <class T>
T* P(uint64_t a) {
  return (T*)(uintptr_t)a;
}
}  // namespace

extern "C" int kpr_mfma_cand_q8(uint64_t X8, uint32_t dim, uint32_t n_rows, uint32_t row_base,
                                uint64_t Q8, uint32_t nq_valid, uint32_t k, uint64_t init_score,
                                uint64_t q8par, uint64_t q8glob, uint64_t slabs, uint64_t slab_tile,
                                uint32_t cand_cap, uint64_t cand_cnt, uint64_t cand_max,
                                uint32_t max_lists, uint32_t* nlists, uint64_t gate, uint64_t allow,
                                uint64_t run_if) {
  return (int)vsk::launch_mfma_cand_q8(P<const void>(X8), dim, n_rows, row_base, P<const void>(Q8),
                                       nq_valid, k, P<const float>(init_score),
                                       P<const float>(q8par), P<const float>(q8glob),
                                       P<float>(slabs), P<uint32_t>(slab_tile), cand_cap,
                                       P<uint32_t>(cand_cnt), P<uint32_t>(cand_max), max_lists,
                                       nlists, P<uint32_t>(gate), nullptr, P<const uint64_t>(allow),
                                       P<const uint32_t>(run_if));
}
