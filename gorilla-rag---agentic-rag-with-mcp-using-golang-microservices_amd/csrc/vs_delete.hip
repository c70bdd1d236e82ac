// vs_delete.hip — device side of vs_delete (include/vsearch.h "point
// deletion"): the deleted rows' bitmap, the two ascending compactions (holes
// below the new row count, survivors at or above it), the row move and the
// de-duplicated list of int8 tiles the move touched. Launchers are declared in
// vs_kernels.h; everything is ordered on the caller's stream and nothing here
// waits for the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "vs_kernels.h"

namespace vsk {

namespace {

constexpr int kDelThreads = 256;

// Bit r of bits[r / 64] for every rows[i] < n_rows. Several threads may hit
// one word (and repeats one bit): a device-scope atomic OR on the vector
// memory path, nothing else writes the bitmap.
__global__ __launch_bounds__(kDelThreads) void delete_mark_kernel(
    const uint64_t* __restrict__ rows, uint64_t n, uint32_t n_rows,
    unsigned long long* __restrict__ bits) {
  const uint64_t step = (uint64_t)gridDim.x * kDelThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kDelThreads + threadIdx.x; i < n; i += step) {
    const uint64_t r = rows[i];
    if (r < n_rows) atomicOr(&bits[r >> 6], 1ull << (r & 63));
  }
}

// The bits of word wi (rows 64 wi ..) that lie in [lo, hi), of the bitmap or,
// with `invert`, of its complement. wi < ceil(hi / 64) words are read.
__device__ __forceinline__ uint64_t ranged_word(const uint64_t* __restrict__ bits, uint32_t wi,
                                                uint32_t lo, uint32_t hi, bool invert) {
  const uint64_t b0 = (uint64_t)wi * 64;
  if (b0 >= hi || b0 + 64 <= lo) return 0;
  uint64_t w = bits[wi];
  if (invert) w = ~w;
  if (lo > b0) w &= ~0ull << (lo - b0);
  if (hi < b0 + 64) w &= (1ull << (hi - b0)) - 1;
  return w;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(v, off);
    if (lane >= off) v += t;
  }
  return v;
}

// The ranged twin of vs_kernels.hip's filter compaction: words w0 + j of the
// range, kDelThreads of them a block. Per-block counts ...
__global__ __launch_bounds__(kDelThreads) void range_count_kernel(
    const uint64_t* __restrict__ bits, uint32_t lo, uint32_t hi, uint32_t invert, uint32_t w0,
    uint32_t* __restrict__ block_cnt) {
  __shared__ uint32_t part[kDelThreads / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t wi = w0 + blockIdx.x * kDelThreads + threadIdx.x;
  const uint32_t c = (uint32_t)__popcll(ranged_word(bits, wi, lo, hi, invert != 0));
  const uint32_t t = wave_incl_scan(c, lane);
  if (lane == 63) part[w] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
    for (int v = 0; v < kDelThreads / 64; ++v) sum += part[v];
    block_cnt[blockIdx.x] = sum;
  }
}

// ... their exclusive scan in place by one workgroup (*total = their sum) ...
__global__ __launch_bounds__(kDelThreads) void range_scan_kernel(uint32_t* __restrict__ block_cnt,
                                                                 uint32_t n,
                                                                 uint64_t* __restrict__ total) {
  __shared__ uint32_t part[kDelThreads / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < n; b0 += kDelThreads) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t c = i < n ? block_cnt[i] : 0;
    const uint32_t inc = wave_incl_scan(c, lane);
    if (lane == 63) part[w] = inc;
    __syncthreads();
    uint32_t base = carry, tot = 0;
    for (int v = 0; v < kDelThreads / 64; ++v) {
      if (v < w) base += part[v];
      tot += part[v];
    }
    if (i < n) block_cnt[i] = base + inc - c;
    carry += tot;
    __syncthreads();  // part[] is rewritten by the next chunk
  }
  if (threadIdx.x == 0) *total = carry;
}

// ... and each block places its set bits' numbers, ascending.
template <typename T>
__global__ __launch_bounds__(kDelThreads) void range_place_kernel(
    const uint64_t* __restrict__ bits, uint32_t lo, uint32_t hi, uint32_t invert, uint32_t w0,
    const uint32_t* __restrict__ block_base, T* __restrict__ out) {
  __shared__ uint32_t part[kDelThreads / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t wi = w0 + blockIdx.x * kDelThreads + threadIdx.x;
  uint64_t word = ranged_word(bits, wi, lo, hi, invert != 0);
  const uint32_t c = (uint32_t)__popcll(word);
  const uint32_t inc = wave_incl_scan(c, lane);
  if (lane == 63) part[w] = inc;
  __syncthreads();
  uint32_t o = block_base[blockIdx.x] + inc - c;
  for (int v = 0; v < w; ++v) o += part[v];
  while (word) {
    out[o++] = (T)((uint64_t)wi * 64u + (uint32_t)(__ffsll((unsigned long long)word) - 1));
    word &= word - 1;
  }
}

// One wave per pair: row src_rows[i] of src (row i when src_rows is null) ->
// row dst_rows[i] of dst, V at a time, lane j on elements j, j + 64, ... so a
// wave's access is one contiguous run of the row (16-byte lanes: 1 KiB).
// In place (src == dst, a delete on one device) this needs no second buffer:
// every source row is at or above the new row count and every destination
// below it, and both lists are duplicate-free, so no row is both read and
// written and none is written twice.
template <typename V>
__global__ __launch_bounds__(kDelThreads) void move_rows_kernel(
    const char* __restrict__ src, const uint64_t* __restrict__ src_rows, char* __restrict__ dst,
    const uint64_t* __restrict__ dst_rows, uint32_t row_bytes, uint32_t n_pairs) {
  const int lane = threadIdx.x & 63;
  const uint32_t waves = kDelThreads / 64;
  const uint32_t nv = row_bytes / (uint32_t)sizeof(V);
  for (uint32_t i = blockIdx.x * waves + (threadIdx.x >> 6); i < n_pairs; i += gridDim.x * waves) {
    const uint64_t sr = src_rows ? src_rows[i] : i;
    const V* s = (const V*)(src + sr * row_bytes);
    V* d = (V*)(dst + dst_rows[i] * row_bytes);
    for (uint32_t j = lane; j < nv; j += 64) d[j] = s[j];
  }
}

// Bit t of tbits for the 32-row tile t of every dst_rows[i], and of last_tile.
__global__ __launch_bounds__(kDelThreads) void mark_tiles_kernel(
    const uint64_t* __restrict__ dst_rows, uint32_t n_pairs, uint32_t last_tile, uint32_t mark_last,
    unsigned long long* __restrict__ tbits) {
  const uint32_t step = gridDim.x * kDelThreads;
  const uint32_t t0 = blockIdx.x * kDelThreads + threadIdx.x;
  if (t0 == 0 && mark_last) atomicOr(&tbits[last_tile >> 6], 1ull << (last_tile & 63));
  for (uint32_t i = t0; i < n_pairs; i += step) {
    const uint64_t t = dst_rows[i] >> 5;
    atomicOr(&tbits[t >> 6], 1ull << (t & 63));
  }
}

uint32_t grid_for(uint64_t n, uint32_t per_block) {
  return (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(1, (n + per_block - 1) / per_block));
}

}  // namespace

hipError_t launch_delete_mark(const uint64_t* rows, uint64_t n, uint32_t n_rows, uint64_t* bits,
                              hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(delete_mark_kernel, dim3(grid_for(n, kDelThreads)), dim3(kDelThreads), 0, st,
                     rows, n, n_rows, (unsigned long long*)bits);
  return hipGetLastError();
}

uint32_t compact_range_scratch_words(uint32_t lo, uint32_t hi) {
  if (lo >= hi) return 1;
  const uint32_t words = (hi + 63) / 64 - lo / 64;
  return (words + kDelThreads - 1) / kDelThreads;
}

hipError_t launch_compact_range(const uint64_t* bits, uint32_t lo, uint32_t hi, bool invert,
                                uint64_t* out64, uint32_t* out32, uint32_t* scratch,
                                uint64_t* total, hipStream_t st) {
  if (!out64 == !out32) return hipErrorInvalidValue;
  if (lo >= hi) return hipMemsetAsync(total, 0, 8, st);
  const uint32_t nb = compact_range_scratch_words(lo, hi), w0 = lo / 64, inv = invert ? 1u : 0u;
  hipLaunchKernelGGL(range_count_kernel, dim3(nb), dim3(kDelThreads), 0, st, bits, lo, hi, inv, w0,
                     scratch);
  hipLaunchKernelGGL(range_scan_kernel, dim3(1), dim3(kDelThreads), 0, st, scratch, nb, total);
  if (out64)
    hipLaunchKernelGGL(range_place_kernel<uint64_t>, dim3(nb), dim3(kDelThreads), 0, st, bits, lo,
                       hi, inv, w0, scratch, out64);
  else
    hipLaunchKernelGGL(range_place_kernel<uint32_t>, dim3(nb), dim3(kDelThreads), 0, st, bits, lo,
                       hi, inv, w0, scratch, out32);
  return hipGetLastError();
}

hipError_t launch_move_rows(const void* src, const uint64_t* src_rows, void* dst,
                            const uint64_t* dst_rows, uint32_t row_bytes, uint32_t n_pairs,
                            hipStream_t st) {
  if (n_pairs == 0) return hipSuccess;
  if (row_bytes == 0 || (row_bytes & 1)) return hipErrorInvalidValue;
  const dim3 grid(grid_for(n_pairs, kDelThreads / 64)), block(kDelThreads);
  const uintptr_t align = (uintptr_t)src | (uintptr_t)dst | row_bytes;
  if (align % 16 == 0)
    hipLaunchKernelGGL(move_rows_kernel<uint4>, grid, block, 0, st, (const char*)src, src_rows,
                       (char*)dst, dst_rows, row_bytes, n_pairs);
  else if (align % 4 == 0)  // element-granular: fp32 elements, or bf16 pairs
    hipLaunchKernelGGL(move_rows_kernel<uint32_t>, grid, block, 0, st, (const char*)src, src_rows,
                       (char*)dst, dst_rows, row_bytes, n_pairs);
  else
    hipLaunchKernelGGL(move_rows_kernel<uint16_t>, grid, block, 0, st, (const char*)src, src_rows,
                       (char*)dst, dst_rows, row_bytes, n_pairs);
  return hipGetLastError();
}

hipError_t launch_mark_tiles(const uint64_t* dst_rows, uint32_t n_pairs, uint32_t n_rows,
                             uint64_t* tbits, hipStream_t st) {
  if (n_pairs == 0 && n_rows == 0) return hipSuccess;
  hipLaunchKernelGGL(mark_tiles_kernel, dim3(grid_for(n_pairs, kDelThreads)), dim3(kDelThreads), 0,
                     st, dst_rows, n_pairs, n_rows ? (n_rows - 1) / 32 : 0u, n_rows ? 1u : 0u,
                     (unsigned long long*)tbits);
  return hipGetLastError();
}

}  // namespace vsk
