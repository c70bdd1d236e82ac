// vs_fuse.hip — device side of vs_search_fused / vs_fuse_keys (include/vsearch.h
// "Fused search"): one workgroup of four waves per fused query turns its n_sub
// candidate lists (at most 8 x 128 keys) into the k rows with the largest fused
// score. Everything lives in LDS; nothing but the two key arrays is touched.
//
//  0. DBSF only: wave w reduces lists w and w + 4 in fp64 (mean, two-pass
//     sample variance) and leaves mu - 3 sigma and 6 sigma per list.
//  1. every non-empty slot (l, p) becomes the composite row << 32 | slot, with
//     slot = l * k_in + p, and its term goes to s_term[slot]; empty slots are
//     ~0, which sorts last.
//  2. a bitonic sort, ascending: the entries of one row become one run, in
//     ascending l (slot grows with l).
//  3. the first element of each run walks its run SEQUENTIALLY and adds the
//     terms in that order, starting from the first term: this fixes the fp32
//     summation order the header promises. No atomics, no tree.
//  4. heads become ~vs_key_encode(fused, row), every other slot ~0; the same
//     ascending sort then orders the keys descending with the empty slots last.
//  5. the first k, complemented back, are written out (0 past the count).
//
// A row repeated inside one list only makes a run longer than n_sub: the walk
// is bounded by the sorted array, so the result is unspecified but nothing
// faults or hangs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vs_kernels.h"

// The rule rounds every operation once: no fused multiply-add anywhere below.
#pragma clang fp contract(off)

namespace vsk {

namespace {

constexpr int kFuseThreads = 256;
constexpr int kFuseSlots = (int)(kFuseMaxLists * kFuseMaxLimit);  // 1024
constexpr int kFuseIters = kFuseSlots / kFuseThreads;             // slots a thread owns
constexpr uint64_t kEmpty = ~0ull;

// vs_key_score / the order-preserving image of a float (include/vsearch.h)
__device__ __forceinline__ float key_score(uint64_t key) {
  const uint32_t o = (uint32_t)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ uint32_t float_ord(float v) {
  const uint32_t u = __float_as_uint(v == 0.0f ? 0.0f : v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Ascending bitonic sort of a[0 .. P), P a power of two <= kFuseSlots, by the
// whole workgroup. Ends with a barrier.
__device__ __forceinline__ void sort_asc(uint64_t* a, uint32_t P, int tid) {
  for (uint32_t size = 2; size <= P; size <<= 1) {
    for (uint32_t j = size >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < (P >> 1); t += kFuseThreads) {
        const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));  // bit j clear
        const uint32_t hi = lo | j;
        const uint64_t x = a[lo], y = a[hi];
        const bool up = (lo & size) == 0;
        if ((x > y) == up) {
          a[lo] = y;
          a[hi] = x;
        }
      }
      __syncthreads();
    }
  }
}

template <bool DBSF>
__global__ __launch_bounds__(kFuseThreads) void fuse_kernel(
    const uint64_t* __restrict__ lists, uint32_t n_sub, uint32_t k_in, uint32_t k, uint32_t rrf_k,
    uint32_t P, uint64_t* __restrict__ out) {
  __shared__ uint64_t s_a[kFuseSlots];
  __shared__ float s_term[kFuseSlots];
  __shared__ double s_lo[kFuseMaxLists];   // mu - 3 sigma
  __shared__ double s_den[kFuseMaxLists];  // 6 sigma; 0: every term of the list is 0.5
  const int tid = threadIdx.x;
  const uint32_t N = n_sub * k_in;  // <= kFuseSlots <= P rounded up (launch_fuse)
  const uint64_t* in = lists + (size_t)blockIdx.x * N;

  // ---- 0. per-list statistics (DBSF) ---------------------------------------
  if constexpr (DBSF) {
    const uint32_t lane = tid & 63, wave = tid >> 6;
    for (uint32_t l = wave; l < n_sub; l += kFuseThreads / 64) {
      const uint64_t k0 = lane < k_in ? in[l * k_in + lane] : 0ull;
      const uint64_t k1 = lane + 64 < k_in ? in[l * k_in + lane + 64] : 0ull;
      const uint32_t n = (uint32_t)__popcll(__ballot(k0 != 0)) + (uint32_t)__popcll(__ballot(k1 != 0));
      const double v0 = k0 ? (double)key_score(k0) : 0.0, v1 = k1 ? (double)key_score(k1) : 0.0;
      double lo = 0.0, den = 0.0;
      if (n > 1) {  // wave-uniform
        const double mu = wave_sum_f64(v0 + v1) / (double)n;
        const double d0 = k0 ? v0 - mu : 0.0, d1 = k1 ? v1 - mu : 0.0;
        const double var = wave_sum_f64(d0 * d0 + d1 * d1) / (double)(n - 1);
        const double sigma = sqrt(var);
        if (sigma > 0.0) {  // false for 0 and for NaN
          lo = mu - 3.0 * sigma;
          den = 6.0 * sigma;
        }
      }
      if (lane == 0) {
        s_lo[l] = lo;
        s_den[l] = den;
      }
    }
    __syncthreads();
  }

  // ---- 1. composites and terms ----------------------------------------------
#pragma unroll
  for (int it = 0; it < kFuseIters; ++it) {
    const uint32_t i = (uint32_t)it * kFuseThreads + tid;
    if (i < P) {
      uint64_t comp = kEmpty;
      if (i < N) {
        const uint64_t key = in[i];
        if (key != 0) {
          const uint32_t l = i / k_in, p = i - l * k_in;
          float term;
          if constexpr (DBSF) {
            const double den = s_den[l];
            term = den > 0.0 ? (float)(((double)key_score(key) - s_lo[l]) / den) : 0.5f;
          } else {
            term = 1.0f / (float)(p + rrf_k);  // IEEE division, rounded once
          }
          s_term[i] = term;
          comp = (uint64_t)(0xFFFFFFFFu - (uint32_t)key) << 32 | i;
        }
      }
      s_a[i] = comp;
    }
  }
  __syncthreads();

  // ---- 2. runs of equal rows, ascending l inside a run ------------------------
  sort_asc(s_a, P, tid);

  // ---- 3 + 4. heads sum their runs in order and become keys -------------------
  uint64_t fused[kFuseIters];
#pragma unroll
  for (int it = 0; it < kFuseIters; ++it) {
    const uint32_t i = (uint32_t)it * kFuseThreads + tid;
    fused[it] = kEmpty;
    if (i < P) {
      const uint64_t c = s_a[i];
      const uint32_t row = (uint32_t)(c >> 32);
      if (c != kEmpty && (i == 0 || (uint32_t)(s_a[i - 1] >> 32) != row)) {
        float sum = s_term[(uint32_t)c & (kFuseSlots - 1)];
        for (uint32_t j = i + 1; j < P; ++j) {
          const uint64_t cj = s_a[j];
          if (cj == kEmpty || (uint32_t)(cj >> 32) != row) break;
          sum = sum + s_term[(uint32_t)cj & (kFuseSlots - 1)];
        }
        fused[it] = ~((uint64_t)float_ord(sum) << 32 | (0xFFFFFFFFu - row));
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < kFuseIters; ++it) {
    const uint32_t i = (uint32_t)it * kFuseThreads + tid;
    if (i < P) s_a[i] = fused[it];
  }
  __syncthreads();

  // ---- 5. descending by key, the first k out -----------------------------------
  sort_asc(s_a, P, tid);
  for (uint32_t j = tid; j < k; j += kFuseThreads)
    out[(size_t)blockIdx.x * k + j] = j < P ? ~s_a[j] : 0ull;
}

}  // namespace

hipError_t launch_fuse(const uint64_t* lists, uint32_t nq, uint32_t n_sub, uint32_t k_in,
                       uint32_t k, bool dbsf, uint32_t rrf_k, uint64_t* out, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (n_sub == 0 || n_sub > kFuseMaxLists || k_in == 0 || k_in > kFuseMaxLimit || k == 0 ||
      k > k_in || !lists || !out)
    return hipErrorInvalidValue;
  if (dbsf ? rrf_k != 0 : (rrf_k == 0 || rrf_k > 65536u)) return hipErrorInvalidValue;
  uint32_t P = 1;
  while (P < n_sub * k_in) P <<= 1;  // <= 1024
  if (dbsf)
    hipLaunchKernelGGL(fuse_kernel<true>, dim3(nq), dim3(kFuseThreads), 0, st, lists, n_sub, k_in,
                       k, rrf_k, P, out);
  else
    hipLaunchKernelGGL(fuse_kernel<false>, dim3(nq), dim3(kFuseThreads), 0, st, lists, n_sub, k_in,
                       k, rrf_k, P, out);
  return hipGetLastError();
}

}  // namespace vsk
