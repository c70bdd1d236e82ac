// vs_kprobe.cpp — test-only C entry points over the C++ launchers of
// csrc/vs_kernels.h (namespace vsk), so the suite can run each stage of the
// int8 prefilter on inputs of its own (tests/kprobe/__init__.py is the ctypes
// loader; tests/test_q8_stages_gpu.py, test_spec_verify_gpu.py,
// test_sample_bound_gpu.py and, for the single-query int8 scan and finish,
// test_q8_gemv_stages_gpu.py are the users), and each piece of the large-k
// path (test_rsel_stages_gpu.py: both selections on score images the test
// builds; test_large_k_stages_gpu.py: the score pass, the key sort, the sort
// merge and the key remap), and the plain one-query scan
// (test_gemv_stages_gpu.py: launch_gemv with and without a row list,
// launch_gemv_one, launch_gemv_small, launch_compact_rows). The sort merge's
// walk used to end at the first 256-key chunk that kept nothing, which a key
// repeated in more than 256 lists produces with distinct keys still behind it;
// it now ends at the zero padding.
//
// Host C++ only: no kernels and no HIP runtime call. Every pointer is a raw
// device address (uint64_t, a torch tensor's data_ptr()), every launch goes to
// stream 0, and the launcher's hipError_t comes back as an int. The caller
// synchronises. Built by build.py into lib/libvs_kprobe.so, linked against
// libvsearch.so; not part of the product library.
#include <stddef.h>
#include <stdint.h>

#include "vs_kernels.h"

namespace {
template <class T>
T* P(uint64_t a) {
  return (T*)(uintptr_t)a;
}
const hipStream_t kSt = nullptr;
}  // namespace

extern "C" {

// ---- layout the tests read instead of hard-coding ---------------------------
uint64_t kp_q8_glob_bytes() { return vsk::kQ8GlobBytes; }
uint64_t kp_q8_spec_stat_off() { return vsk::kQ8SpecStatOff; }
uint64_t kp_q8_spec_k_off() { return vsk::kQ8SpecKOff; }
uint64_t kp_q8_spec_k_size() { return sizeof(vsk::Q8SpecK); }
uint64_t kp_q8_spec_k_count() { return vsk::kQ8SpecK; }
uint64_t kp_q8_spec_stat_size() { return sizeof(vsk::Q8SpecStat); }
// Q8SpecK fields / Q8SpecStat fields, byte offsets inside the struct
uint64_t kp_spec_k_ratio_off() { return offsetof(vsk::Q8SpecK, ratio); }
uint64_t kp_spec_k_backoff_off() { return offsetof(vsk::Q8SpecK, backoff); }
uint64_t kp_spec_k_loose_off() { return offsetof(vsk::Q8SpecK, loose); }
uint64_t kp_spec_k_since_off() { return offsetof(vsk::Q8SpecK, since); }
uint64_t kp_spec_stat_tries_off() { return offsetof(vsk::Q8SpecStat, tries); }
uint64_t kp_spec_stat_fails_off() { return offsetof(vsk::Q8SpecStat, fails); }
uint64_t kp_spec_stat_skipped_off() { return offsetof(vsk::Q8SpecStat, skipped); }
uint64_t kp_q8_par_bytes() { return vsk::kQ8ParBytes; }
uint32_t kp_gate_verdict() { return vsk::kGateVerdict; }
uint32_t kp_gate_forced() { return vsk::kGateForced; }
uint32_t kp_gate_go() { return vsk::kGateGo; }
uint32_t kp_q8_spec_probe() { return vsk::kQ8SpecProbe; }
uint32_t kp_q8_spec_max_backoff() { return vsk::kQ8SpecMaxBackoff; }
uint32_t kp_mfma_query_slots() { return vsk::kMfmaQueries; }
uint32_t kp_mfma_max_k() { return vsk::kMfmaMaxK; }
uint32_t kp_mfma_max_cand_cap() { return vsk::kMfmaMaxCandCap; }

// ---- helpers ----------------------------------------------------------------
void kp_mfma_grid(uint32_t n_rows, uint32_t* nwg, uint32_t* rows_per_wg) {
  vsk::mfma_grid(n_rows, nwg, rows_per_wg);
}
uint32_t kp_mfma_max_lists(uint32_t n_rows) { return vsk::mfma_max_lists(n_rows); }
uint32_t kp_mfma_tiles_per_wg(uint32_t n_rows) { return vsk::mfma_tiles_per_wg(n_rows); }
uint32_t kp_mfma_sample_tiles(uint32_t n_rows, uint32_t dim, int f32) {
  return vsk::mfma_sample_tiles(n_rows, dim, f32 != 0);
}
uint32_t kp_mfma_cand_cap(uint32_t n_rows, uint32_t k, uint32_t sample_tiles, double scale) {
  return vsk::mfma_cand_cap(n_rows, k, sample_tiles, scale);
}
uint32_t kp_mfma_queries(uint32_t dim, int f32) { return vsk::mfma_queries(dim, f32 != 0); }
int kp_mfma_supported(uint32_t dim, int f32) { return vsk::mfma_supported(dim, f32 != 0) ? 1 : 0; }
int kp_q8_supported(uint32_t dim, int f32) { return vsk::q8_supported(dim, f32 != 0) ? 1 : 0; }
int kp_sample_bound_passes() { return vsk::sample_bound_passes(); }

// ---- store side -------------------------------------------------------------
int kp_q8_absmax(uint64_t X, int f32, uint64_t n, uint64_t glob) {
  return (int)vsk::launch_q8_absmax(P<const void>(X), f32 != 0, n, P<float>(glob), kSt);
}
int kp_q8_set_scale(uint64_t glob) { return (int)vsk::launch_q8_set_scale(P<float>(glob), kSt); }
int kp_q8_quantize(uint64_t X, int f32, uint32_t n_rows, uint32_t dim, uint64_t tiles, uint32_t t0,
                   uint32_t ntiles, uint64_t X8, uint64_t meta, uint64_t glob) {
  return (int)vsk::launch_q8_quantize(P<const void>(X), f32 != 0, n_rows, dim,
                                      P<const uint32_t>(tiles), t0, ntiles, P<int8_t>(X8),
                                      P<float>(meta), P<float>(glob), kSt);
}

// ---- query side -------------------------------------------------------------
int kp_query_prep(uint64_t in, uint32_t n, uint32_t dim, int cosine, int round_qp, uint64_t qp,
                  uint64_t qb) {
  return (int)vsk::launch_query_prep(P<const float>(in), n, dim, cosine != 0, round_qp != 0,
                                     P<float>(qp), P<uint16_t>(qb), kSt);
}
int kp_q8_query(uint64_t q, int f32, uint32_t nq, uint32_t dim, uint64_t glob, uint64_t q8,
                uint64_t q8par, uint64_t gate) {
  return (int)vsk::launch_q8_query(P<const void>(q), f32 != 0, nq, dim, P<const float>(glob),
                                   P<int8_t>(q8), P<float>(q8par), P<uint32_t>(gate), kSt);
}
int kp_q8_query_spec(uint64_t q, int f32, uint32_t nq, uint32_t dim, uint64_t glob, uint64_t q8,
                     uint64_t q8par, uint64_t gate, uint64_t ratio, uint64_t bound, uint64_t spec_k,
                     uint64_t stat, int force) {
  return (int)vsk::launch_q8_query(P<const void>(q), f32 != 0, nq, dim, P<const float>(glob),
                                   P<int8_t>(q8), P<float>(q8par), P<uint32_t>(gate), kSt,
                                   P<const float>(ratio), P<float>(bound), P<vsk::Q8SpecK>(spec_k),
                                   P<vsk::Q8SpecStat>(stat), force != 0);
}
int kp_q8_prep_query(uint64_t in, int cosine, int round_qp, uint64_t qp, uint64_t qbf, int f32,
                     uint32_t nq, uint32_t dim, uint64_t glob, uint64_t q8, uint64_t q8par,
                     uint64_t gate, uint64_t ratio, uint64_t bound, uint64_t spec_k, uint64_t stat,
                     int force) {
  return (int)vsk::launch_q8_prep_query(P<const float>(in), cosine != 0, round_qp != 0, P<float>(qp),
                                        P<uint16_t>(qbf), f32 != 0, nq, dim, P<const float>(glob),
                                        P<int8_t>(q8), P<float>(q8par), P<uint32_t>(gate), kSt,
                                        P<const float>(ratio), P<float>(bound),
                                        P<vsk::Q8SpecK>(spec_k), P<vsk::Q8SpecStat>(stat), force != 0);
}
int kp_sample_bound_q8(uint64_t tmax, uint32_t m, uint32_t nq_bound, uint32_t k, uint64_t bound,
                       uint64_t q, int f32, uint32_t nq, uint32_t dim, uint64_t glob, uint64_t q8,
                       uint64_t q8par, uint64_t gate) {
  return (int)vsk::launch_sample_bound_q8(P<const float>(tmax), m, nq_bound, k, P<float>(bound),
                                          P<const void>(q), f32 != 0, nq, dim, P<const float>(glob),
                                          P<int8_t>(q8), P<float>(q8par), P<uint32_t>(gate), kSt);
}

// ---- sample pass and bound --------------------------------------------------
int kp_mfma_sample(uint64_t X, int f32, uint32_t dim, uint32_t n_rows, uint32_t row_base, uint64_t Q,
                   uint32_t nq_valid, uint32_t k, uint32_t max_tiles, uint64_t tmax,
                   uint32_t max_lists, uint32_t* nlists, uint64_t allow) {
  return (int)vsk::launch_mfma_sample(P<const void>(X), f32 != 0, dim, n_rows, row_base,
                                      P<const void>(Q), nq_valid, k, max_tiles, P<float>(tmax),
                                      max_lists, nlists, kSt, P<const uint64_t>(allow));
}
int kp_sample_bound(uint64_t tmax, uint32_t m, uint32_t nq, uint32_t k, uint64_t bound) {
  return (int)vsk::launch_sample_bound(P<const float>(tmax), m, nq, k, P<float>(bound), kSt);
}

// ---- main passes and selects ------------------------------------------------
int kp_mfma_cand(uint64_t X, int f32, uint32_t dim, uint32_t n_rows, uint32_t row_base, uint64_t Q,
                 uint32_t nq_valid, uint32_t k, uint64_t init_score, uint64_t slabs,
                 uint64_t slab_tile, uint32_t cand_cap, uint64_t cand_cnt, uint32_t max_lists,
                 uint32_t* nlists, uint64_t allow, uint64_t cand_max) {
  return (int)vsk::launch_mfma_cand(P<const void>(X), f32 != 0, dim, n_rows, row_base,
                                    P<const void>(Q), nq_valid, k, P<const float>(init_score),
                                    P<float>(slabs), P<uint32_t>(slab_tile), cand_cap,
                                    P<uint32_t>(cand_cnt), max_lists, nlists, kSt,
                                    P<const uint64_t>(allow), P<uint32_t>(cand_max));
}
int kp_select_slabs(uint64_t slabs, uint64_t slab_tile, uint64_t cand_cnt, uint32_t nwg, uint32_t cap,
                    uint32_t nq, uint32_t k, uint64_t out, uint32_t row_base, uint64_t allow,
                    uint64_t cand_max) {
  return (int)vsk::launch_select_slabs(P<const float>(slabs), P<const uint32_t>(slab_tile),
                                       P<const uint32_t>(cand_cnt), nwg, cap, nq, k,
                                       P<uint64_t>(out), kSt, row_base, P<const uint64_t>(allow),
                                       P<const uint32_t>(cand_max));
}
int kp_mfma_cand_q8(uint64_t X8, uint32_t dim, uint32_t n_rows, uint32_t row_base, uint64_t Q8,
                    uint32_t nq_valid, uint32_t k, uint64_t init_score, uint64_t q8par,
                    uint64_t q8glob, uint64_t slabs, uint64_t slab_tile, uint32_t cand_cap,
                    uint64_t cand_cnt, uint64_t cand_max, uint32_t max_lists, uint32_t* nlists,
                    uint64_t gate, uint64_t allow) {
  return (int)vsk::launch_mfma_cand_q8(P<const void>(X8), dim, n_rows, row_base, P<const void>(Q8),
                                       nq_valid, k, P<const float>(init_score),
                                       P<const float>(q8par), P<const float>(q8glob),
                                       P<float>(slabs), P<uint32_t>(slab_tile), cand_cap,
                                       P<uint32_t>(cand_cnt), P<uint32_t>(cand_max), max_lists,
                                       nlists, P<uint32_t>(gate), kSt, P<const uint64_t>(allow));
}
// With vq and ticket non-zero the select's last workgroup does the batch's
// check (check != 0) or record, as launch_q8_verify_record would after it.
int kp_select_q8(uint64_t slabs, uint64_t slab_tile, uint64_t cand_cnt, uint64_t cand_max,
                 uint32_t nwg, uint32_t cap, uint32_t nq, uint32_t k, uint64_t out, uint32_t row_base,
                 uint64_t X, uint64_t qb, int f32, uint32_t dim, uint64_t q8par, uint64_t q8glob,
                 uint64_t meta, uint64_t bound, uint64_t X8, uint64_t Q8, uint64_t allow,
                 uint32_t n_rows, int check, uint64_t gate, uint64_t spec_k, uint64_t stat,
                 uint64_t advice, uint64_t vq, uint64_t ticket) {
  vsk::SpecVerifyArgs va{check ? 1u : 0u,
                         dim,
                         P<const float>(bound),
                         P<const float>(q8par),
                         P<const float>(q8glob),
                         P<uint32_t>(gate),
                         P<vsk::Q8SpecK>(spec_k),
                         P<vsk::Q8SpecStat>(stat),
                         P<uint32_t>(advice),
                         P<float4>(vq),
                         P<uint32_t>(ticket)};
  const bool verify = vq != 0 && ticket != 0;
  return (int)vsk::launch_select_q8(
      P<const float>(slabs), P<const uint32_t>(slab_tile), P<const uint32_t>(cand_cnt),
      P<const uint32_t>(cand_max), nwg, cap, nq, k, P<uint64_t>(out), row_base, P<const void>(X),
      P<const void>(qb), f32 != 0, dim, P<const float>(q8par), P<const float>(q8glob),
      P<const float>(meta), P<const float>(bound), P<const void>(X8), P<const void>(Q8),
      P<const uint64_t>(allow), n_rows, kSt, nullptr, nullptr, nullptr, verify ? &va : nullptr);
}

// ---- single query: the plain GEMV and the int8 scan + finish ------------------
uint32_t kp_gemv_max_lists(uint32_t dim, int bf16, uint32_t n_rows, uint32_t k) {
  return vsk::gemv_max_lists(dim, bf16 != 0, n_rows, k);
}
int kp_gemv_one(uint64_t X, int bf16, uint32_t dim, uint32_t n_rows, uint32_t row_base,
                uint64_t q_raw, int cosine, uint64_t allow, uint32_t k, uint64_t lists,
                uint32_t max_lists, uint32_t* nlists) {
  return (int)vsk::launch_gemv_one(P<const void>(X), bf16 != 0, dim, n_rows, row_base,
                                   P<const float>(q_raw), cosine != 0, P<const uint64_t>(allow), k,
                                   P<uint64_t>(lists), max_lists, kSt, nlists, nullptr);
}
int kp_merge(uint64_t lists, uint32_t L, uint64_t lstride, uint64_t qstride, uint32_t nq,
             uint32_t kin, uint32_t k, uint64_t out) {
  return (int)vsk::launch_merge(P<const uint64_t>(lists), L, lstride, qstride, nq, kin, k,
                                P<uint64_t>(out), kSt);
}
uint32_t kp_gemv_q8_lists(uint32_t n_rows) { return vsk::gemv_q8_lists(n_rows); }
uint64_t kp_gemv_q8_scratch_bytes(uint32_t n_rows, uint32_t k) {
  return vsk::gemv_q8_scratch_bytes(n_rows, k);
}
// the launcher's own scratch layout (gemv_q8_layout): byte offsets, and KP
uint64_t kp_gemv_q8_ulist_off(uint32_t n_rows, uint32_t k) {
  return vsk::gemv_q8_layout(n_rows, k).ulist_off;
}
uint64_t kp_gemv_q8_lbest_off(uint32_t n_rows, uint32_t k) {
  return vsk::gemv_q8_layout(n_rows, k).lbest_off;
}
uint64_t kp_gemv_q8_cand_off(uint32_t n_rows, uint32_t k) {
  return vsk::gemv_q8_layout(n_rows, k).cand_off;
}
uint32_t kp_gemv_q8_kp(uint32_t n_rows, uint32_t k) { return vsk::gemv_q8_layout(n_rows, k).kp; }
// part: 1 = scan, 2 = finish, 3 = both; no completion flag, no stage clocks
int kp_gemv_q8(int part, uint64_t X, int bf16, uint64_t X8, uint64_t meta, uint64_t glob,
               uint32_t dim, uint32_t n_rows, uint32_t row_base, uint64_t q_raw, int cosine,
               uint64_t allow, uint32_t k, uint64_t scratch, uint64_t scratch_bytes, uint64_t ctr,
               uint64_t dst, uint64_t stats) {
  return (int)vsk::launch_gemv_q8(part, P<const void>(X), bf16 != 0, P<const int8_t>(X8),
                                  P<const float>(meta), P<const float>(glob), dim, n_rows, row_base,
                                  P<const float>(q_raw), cosine != 0, P<const uint64_t>(allow), k,
                                  P<void>(scratch), (size_t)scratch_bytes, P<uint32_t>(ctr),
                                  P<uint64_t>(dst), kSt, nullptr, 0, P<uint32_t>(stats), nullptr);
}

// ---- large k: score pass, selections, sort, sort merge, remap ------------------
uint32_t kp_rsel_bins() { return vsk::kRselBins; }
uint32_t kp_max_k() { return vsk::kMaxK; }
uint64_t kp_rsel_state_size() { return sizeof(vsk::RselState); }
uint64_t kp_rsel_state_thr_off() { return offsetof(vsk::RselState, thr); }
uint64_t kp_rsel_state_krem_off() { return offsetof(vsk::RselState, krem); }
uint64_t kp_rsel_state_done_off() { return offsetof(vsk::RselState, done); }
uint64_t kp_rsel_state_count_off() { return offsetof(vsk::RselState, count); }
uint32_t kp_device_cu_count() { return (uint32_t)vsk::device_cu_count(); }
int kp_gemv_scores(uint64_t X, int bf16, uint32_t dim, uint32_t n_rows, uint64_t q, uint64_t allow,
                   uint64_t sc, uint64_t hist) {
  return (int)vsk::launch_gemv_scores(P<const void>(X), bf16 != 0, dim, n_rows, P<const float>(q),
                                      P<const uint64_t>(allow), P<uint32_t>(sc), P<uint32_t>(hist),
                                      kSt);
}
// q is the preprocessed query; no row list (rows null)
int kp_gemv(uint64_t X, int bf16, uint32_t dim, uint32_t n_rows, uint32_t row_base, uint64_t q,
            uint32_t k, uint64_t out, uint32_t max_lists, uint32_t* nlists, uint64_t allow) {
  return (int)vsk::launch_gemv(P<const void>(X), bf16 != 0, dim, n_rows, row_base, P<const float>(q),
                               k, P<uint64_t>(out), max_lists, nlists, kSt,
                               P<const uint64_t>(allow), nullptr);
}
// ---- the plain one-query family (test_gemv_stages_gpu.py) -----------------------
uint32_t kp_gemv_small_arg_dim() { return vsk::kGemvSmallArgDim; }
uint32_t kp_gemv_small_max_rows() { return vsk::kGemvSmallMaxRows; }
uint32_t kp_gemv_small_max_k() { return vsk::kGemvSmallMaxK; }
uint32_t kp_gemv_small_max_parts() { return vsk::kGemvSmallMaxParts; }
// rows: n_rows local row indices on the device; the scan gathers them
int kp_gemv_gather(uint64_t X, int bf16, uint32_t dim, uint32_t n_rows, uint32_t row_base,
                   uint64_t q, uint32_t k, uint64_t out, uint32_t max_lists, uint32_t* nlists,
                   uint64_t rows) {
  return (int)vsk::launch_gemv(P<const void>(X), bf16 != 0, dim, n_rows, row_base, P<const float>(q),
                               k, P<uint64_t>(out), max_lists, nlists, kSt, nullptr,
                               P<const uint32_t>(rows));
}
uint32_t kp_compact_scratch_words(uint32_t n_rows) { return vsk::compact_scratch_words(n_rows); }
int kp_compact_rows(uint64_t allow, uint32_t n_rows, uint64_t rows, uint64_t scratch) {
  return (int)vsk::launch_compact_rows(P<const uint64_t>(allow), n_rows, P<uint32_t>(rows),
                                       P<uint32_t>(scratch), kSt);
}
int kp_gemv_small_ok(uint32_t dim, uint32_t n_rows, uint32_t k) {
  return vsk::gemv_small_ok(dim, n_rows, k) ? 1 : 0;
}
uint32_t kp_gemv_small_parts(uint32_t dim, int bf16, uint32_t n_rows) {
  return vsk::gemv_small_parts(dim, bf16 != 0, n_rows);
}
int kp_gemv_one_ok(uint32_t dim, uint32_t k) { return vsk::gemv_one_ok(dim, k) ? 1 : 0; }
// part / counter: 0 = one workgroup; q_host: a HOST address (0 = read q_raw on
// the device); no completion word
int kp_gemv_small(uint64_t X, int bf16, uint32_t dim, uint32_t n_rows, uint32_t row_base,
                  uint64_t q_raw, int cosine, uint32_t k, uint64_t out, uint64_t part,
                  uint64_t counter, uint64_t q_host) {
  return (int)vsk::launch_gemv_small(P<const void>(X), bf16 != 0, dim, n_rows, row_base,
                                     P<const float>(q_raw), cosine != 0, k, P<uint64_t>(out), kSt,
                                     P<uint64_t>(part), P<uint32_t>(counter), nullptr, 0,
                                     P<const float>(q_host));
}
// kp_gemv_one with the raw query at a HOST address (it travels in the kernel arguments)
int kp_gemv_one_host(uint64_t X, int bf16, uint32_t dim, uint32_t n_rows, uint32_t row_base,
                     uint64_t q_host, int cosine, uint64_t allow, uint32_t k, uint64_t lists,
                     uint32_t max_lists, uint32_t* nlists) {
  return (int)vsk::launch_gemv_one(P<const void>(X), bf16 != 0, dim, n_rows, row_base, nullptr,
                                   cosine != 0, P<const uint64_t>(allow), k, P<uint64_t>(lists),
                                   max_lists, kSt, nlists, P<const float>(q_host));
}
int kp_rsel(uint64_t sc, uint32_t n_rows, uint32_t row_base, uint32_t keff, uint64_t hist,
            uint64_t state, uint64_t sel) {
  return (int)vsk::launch_rsel(P<const uint32_t>(sc), n_rows, row_base, keff, P<uint32_t>(hist),
                               P<vsk::RselState>(state), P<uint64_t>(sel), kSt);
}
int kp_rsel_fused(uint64_t sc, uint32_t n_rows, uint32_t row_base, uint32_t keff, uint64_t hist,
                  uint64_t hist1, uint64_t ctr, uint64_t sel, uint64_t cand) {
  return (int)vsk::launch_rsel_fused(P<const uint32_t>(sc), n_rows, row_base, keff,
                                     P<uint32_t>(hist), P<uint32_t>(hist1), P<uint32_t>(ctr),
                                     P<uint64_t>(sel), P<uint64_t>(cand), kSt);
}
uint64_t kp_sort_keys_temp_bytes(uint64_t n) { return vsk::sort_keys_temp_bytes(n); }
int kp_sort_keys_desc(uint64_t in, uint64_t out, uint64_t n, uint64_t temp, uint64_t temp_bytes) {
  return (int)vsk::launch_sort_keys_desc(P<const uint64_t>(in), P<uint64_t>(out), n, P<void>(temp),
                                         (size_t)temp_bytes, kSt);
}
uint64_t kp_merge_large_scratch(uint32_t L, uint32_t nq, uint32_t kin) {
  return vsk::merge_large_scratch(L, nq, kin);
}
int kp_merge_large(uint64_t lists, uint32_t L, uint64_t lstride, uint64_t qstride, uint32_t nq,
                   uint32_t kin, uint32_t k, uint64_t out, uint64_t scratch,
                   uint64_t scratch_bytes) {
  return (int)vsk::launch_merge_large(P<const uint64_t>(lists), L, lstride, qstride, nq, kin, k,
                                      P<uint64_t>(out), P<void>(scratch), (size_t)scratch_bytes,
                                      kSt);
}
int kp_remap_keys(uint64_t keys, uint64_t n, uint32_t stride, uint32_t offset, uint32_t base) {
  return (int)vsk::launch_remap_keys(P<uint64_t>(keys), n, stride, offset, base, kSt);
}

// ---- the speculative check / record ----------------------------------------
int kp_q8_verify_record(uint64_t keys, uint32_t nq, uint32_t k, uint32_t dim, uint64_t bound,
                        uint64_t q8par, uint64_t glob, int check, uint64_t gate, uint64_t spec_k,
                        uint64_t stat, uint64_t advice) {
  return (int)vsk::launch_q8_verify_record(P<const uint64_t>(keys), nq, k, dim,
                                           P<const float>(bound), P<const float>(q8par),
                                           P<const float>(glob), check != 0, P<uint32_t>(gate),
                                           P<vsk::Q8SpecK>(spec_k), P<vsk::Q8SpecStat>(stat),
                                           P<uint32_t>(advice), kSt);
}

}  // extern "C"
