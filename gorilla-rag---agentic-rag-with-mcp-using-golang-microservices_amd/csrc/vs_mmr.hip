// vs_mmr.hip — device side of vs_search_mmr / vs_mmr_keys (include/vsearch.h
// "MMR search"): one workgroup of four waves per query turns a candidate key
// list into the MMR selection. Three stages, all inside the one launch:
//
//  1. gather + Gram matrix. The candidates' stored rows are streamed through
//     LDS in 256-byte K-chunks (128 bf16 / 64 fp32 elements a row; 8-byte
//     loads, which every legal dim keeps aligned; the K tail and the rows of
//     empty slots are zeros). Wave w owns the 64 x 64 quadrant (w >> 1, w & 1)
//     of G = X X^T as 4 x 4 tiles of v_mfma_f32_16x16x32_bf16 (bf16 rows) or
//     v_mfma_f32_16x16x4_f32 (fp32 rows), accumulators in registers for the
//     whole K loop. A and B are rows of the same matrix read the same way, so
//     any k order inside a step is valid as long as both take the same one:
//     the fp32 form reads four k per lane in one 16-byte LDS read.
//  2. G goes to LDS (it reuses the staging area), and wave 0 runs the greedy
//     loop: lane l holds candidates l and l + 64 in named registers (score,
//     running-max penalty, free flag), one 64-bit wave max per step picks the
//     largest v (ties: the lower candidate), and every lane folds row `sel`
//     of G into its two penalties. No register is indexed dynamically.
//  3. the keys of the selected candidates are written in selection order.
//
// A slot whose key is 0, or whose row lies outside [row_base, row_base +
// n_rows), is empty: it is never dereferenced and never selected.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vs_kernels.h"

namespace vsk {

namespace {

constexpr int kMmrThreads = 256;
constexpr int kMmrF = (int)kMmrMaxCand;   // 128 candidate slots
constexpr int kChunkBytes = 256;          // K-chunk of one row in LDS
constexpr int kRowStride = kChunkBytes + 16;  // 68 dwords: rows 4 banks apart
constexpr int kStageBytes = kMmrF * kRowStride;
constexpr int kGramBytes = kMmrF * kMmrF * 4;
constexpr int kGatherIters = kMmrF * (kChunkBytes / 8) / kMmrThreads;  // 16 8-byte loads a thread

using frag_bf16 = __attribute__((ext_vector_type(8))) short;
using frag_acc = __attribute__((ext_vector_type(4))) float;

// vs_key_score / the order-preserving image of a float (include/vsearch.h)
__device__ __forceinline__ float key_score(uint64_t key) {
  const uint32_t o = (uint32_t)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ uint32_t float_ord(float v) {
  const uint32_t u = __float_as_uint(v == 0.0f ? 0.0f : v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = __shfl_xor((unsigned long long)v, off);
    v = o > v ? o : v;
  }
  return v;
}

// One 64-byte k-step of a 16 x 16 tile pair: a / b are the lanes' 16 bytes.
template <bool BF16>
__device__ __forceinline__ frag_acc mma_step(const uint4& a, const uint4& b, frag_acc c) {
  if constexpr (BF16) {
    union { uint4 u; frag_bf16 f; } fa, fb;
    fa.u = a;
    fb.u = b;
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa.f, fb.f, c, 0, 0, 0);
  } else {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
    return c;
  }
}

template <bool BF16>
__global__ __launch_bounds__(kMmrThreads) void mmr_kernel(
    const char* __restrict__ X, uint32_t row_bytes, uint32_t n_rows, uint32_t row_base,
    const uint64_t* __restrict__ cand, uint32_t n_cand, uint32_t k, float diversity,
    uint64_t* __restrict__ out) {
  // staging rows during the K loop, then the Gram matrix
  __shared__ __attribute__((aligned(16))) char smem[kGramBytes > kStageBytes ? kGramBytes
                                                                             : kStageBytes];
  __shared__ uint64_t s_key[kMmrF];
  __shared__ uint64_t s_off[kMmrF];  // byte offset of the slot's row; ~0 = empty slot
  __shared__ uint32_t s_sel[kMmrF];
  __shared__ uint32_t s_cnt;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  const uint32_t fr = (n_cand + 15u) & ~15u;  // slots the tiles cover

  if (tid < kMmrF) {
    uint64_t key = 0, off = ~0ull;
    if ((uint32_t)tid < n_cand) {
      key = cand[(size_t)q * n_cand + tid];
      const uint32_t row = 0xFFFFFFFFu - (uint32_t)key;
      const uint32_t local = row - row_base;
      if (key != 0 && row >= row_base && local < n_rows)
        off = (uint64_t)local * row_bytes;
      else
        key = 0;
    }
    s_key[tid] = key;
    s_off[tid] = off;
  }
  __syncthreads();

  // ---- 1. gather + Gram -------------------------------------------------
  const int qi = wave >> 1, qj = wave & 1;
  frag_acc acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = frag_acc{0.f, 0.f, 0.f, 0.f};

  const uint32_t n_chunks = (row_bytes + kChunkBytes - 1) / kChunkBytes;
  const uint32_t n_units = fr * (kChunkBytes / 8);  // 8-byte units of one chunk
  uint2 stg[kGatherIters];
  auto gather = [&](uint32_t chunk) {
#pragma unroll
    for (int it = 0; it < kGatherIters; ++it) {
      const uint32_t u = (uint32_t)it * kMmrThreads + tid;
      uint2 v = make_uint2(0u, 0u);
      if (u < n_units) {
        const uint32_t r = u >> 5, col = chunk * kChunkBytes + (u & 31u) * 8u;
        const uint64_t off = s_off[r];
        if (off != ~0ull && col < row_bytes) v = *(const uint2*)(X + off + col);
      }
      stg[it] = v;
    }
  };
  const bool quad_live = (uint32_t)(qi * 64) < fr && (uint32_t)(qj * 64) < fr;
  if (n_chunks) gather(0);
  for (uint32_t chunk = 0; chunk < n_chunks; ++chunk) {
#pragma unroll
    for (int it = 0; it < kGatherIters; ++it) {
      const uint32_t u = (uint32_t)it * kMmrThreads + tid;
      if (u < n_units) *(uint2*)(smem + (u >> 5) * kRowStride + (u & 31u) * 8u) = stg[it];
    }
    __syncthreads();
    if (chunk + 1 < n_chunks) gather(chunk + 1);  // in flight across the MFMAs
    if (quad_live) {
      const uint32_t left = row_bytes - chunk * kChunkBytes;  // bytes of this chunk that hold data
#pragma unroll
      for (int kk = 0; kk < kChunkBytes / 64; ++kk) {
        if ((uint32_t)(kk * 64) < left) {
          const int lo = (lane & 15) * kRowStride + kk * 64 + (lane >> 4) * 16;
          uint4 fa[4], fb[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            fa[a] = make_uint4(0u, 0u, 0u, 0u);
            if ((uint32_t)((qi * 4 + a) * 16) < fr)
              fa[a] = *(const uint4*)(smem + (qi * 4 + a) * 16 * kRowStride + lo);
          }
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            fb[b] = make_uint4(0u, 0u, 0u, 0u);
            if ((uint32_t)((qj * 4 + b) * 16) < fr)
              fb[b] = *(const uint4*)(smem + (qj * 4 + b) * 16 * kRowStride + lo);
          }
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
              if ((uint32_t)((qi * 4 + a) * 16) < fr && (uint32_t)((qj * 4 + b) * 16) < fr)
                acc[a][b] = mma_step<BF16>(fa[a], fb[b], acc[a][b]);
        }
      }
    }
    __syncthreads();  // the staging rows are rewritten by the next chunk (or by G)
  }

  // ---- 2. G to LDS, greedy loop in wave 0 --------------------------------
  float* G = (float*)smem;
  if (quad_live) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const uint32_t r0 = (qi * 4 + a) * 16, c0 = (qj * 4 + b) * 16;
        if (r0 < fr && c0 < fr) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            G[(r0 + (lane >> 4) * 4 + r) * kMmrF + c0 + (lane & 15)] = acc[a][b][r];
        }
      }
  }
  __syncthreads();

  if (wave == 0) {
    const uint64_t key0 = s_key[lane], key1 = s_key[lane + 64];
    bool free0 = key0 != 0, free1 = key1 != 0;
    const float s0 = key_score(key0), s1 = key_score(key1);
    float p0 = -INFINITY, p1 = -INFINITY;
    const float d = diversity, a = 1.0f - d;
    const uint32_t n_valid = (uint32_t)__popcll(__ballot(free0)) + (uint32_t)__popcll(__ballot(free1));
    const uint32_t steps = k < n_valid ? k : n_valid;
    const uint32_t id0 = 0xFFFFFFFFu - (uint32_t)lane, id1 = id0 - 64u;
    uint32_t t = 0;
    for (; t < steps; ++t) {
      uint64_t m0 = 0, m1 = 0;
      if (t == 0) {  // the first candidate: the lowest valid slot
        m0 = free0 ? (0xFFFFFFFFull << 32 | id0) : 0;
        m1 = free1 ? (0xFFFFFFFFull << 32 | id1) : 0;
      } else {       // v = (1 - d) s - d max sim, every operation rounded once
        const float v0 = __fsub_rn(__fmul_rn(a, s0), __fmul_rn(d, p0));
        const float v1 = __fsub_rn(__fmul_rn(a, s1), __fmul_rn(d, p1));
        m0 = free0 ? ((uint64_t)float_ord(v0) << 32 | id0) : 0;
        m1 = free1 ? ((uint64_t)float_ord(v1) << 32 | id1) : 0;
      }
      const uint64_t m = wave_max_u64(m0 > m1 ? m0 : m1);
      if (m == 0) break;  // only NaN scores are left
      const uint32_t sel = 0xFFFFFFFFu - (uint32_t)m;  // < kMmrF: built from a lane id
      if (sel == (uint32_t)lane) free0 = false;
      if (sel == (uint32_t)lane + 64u) free1 = false;
      if (lane == 0) s_sel[t] = sel;
      p0 = fmaxf(p0, G[sel * kMmrF + lane]);
      p1 = fmaxf(p1, G[sel * kMmrF + lane + 64]);
    }
    if (lane == 0) s_cnt = t;
  }
  __syncthreads();

  // ---- 3. keys in selection order, 0-padded -------------------------------
  const uint32_t cnt = s_cnt;
  for (uint32_t j = tid; j < k; j += kMmrThreads)
    out[(size_t)q * k + j] = j < cnt ? s_key[s_sel[j]] : 0ull;
}

}  // namespace

hipError_t launch_mmr(const void* X, bool bf16, uint32_t dim, uint32_t n_rows, uint32_t row_base,
                      const uint64_t* cand, uint32_t nq, uint32_t n_cand, uint32_t k,
                      float diversity, uint64_t* out, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (n_cand == 0 || n_cand > kMmrMaxCand || k == 0 || k > n_cand || !cand || !out)
    return hipErrorInvalidValue;
  if (!(diversity >= 0.0f && diversity <= 1.0f)) return hipErrorInvalidValue;
  const uint64_t row_bytes = (uint64_t)dim * (bf16 ? 2 : 4);
  // 8-byte loads: bf16 dim % 4 == 0, fp32 dim % 2 == 0 (the engine's own rule)
  if (row_bytes == 0 || row_bytes % 8 != 0 || row_bytes > 0xFFFFFFFFull) return hipErrorInvalidValue;
  if (n_rows && (!X || (uintptr_t)X % 8 != 0)) return hipErrorInvalidValue;
  if (bf16)
    hipLaunchKernelGGL(mmr_kernel<true>, dim3(nq), dim3(kMmrThreads), 0, st, (const char*)X,
                       (uint32_t)row_bytes, n_rows, row_base, cand, n_cand, k, diversity, out);
  else
    hipLaunchKernelGGL(mmr_kernel<false>, dim3(nq), dim3(kMmrThreads), 0, st, (const char*)X,
                       (uint32_t)row_bytes, n_rows, row_base, cand, n_cand, k, diversity, out);
  return hipGetLastError();
}

}  // namespace vsk
