// vs_group.hip — device side of vs_search_groups / vs_group_keys
// (include/vsearch.h "Grouped search"): the exact top `limit` groups of one
// query and the `group_size` best rows of each, from the score images the
// large-k score pass leaves (vs_kernels.h launch_gemv_scores: sc[r] = the
// result key's high word, 0 = masked) and one group id per row.
//
// A row is eligible when its image is not 0 and its id is a group (< n_groups;
// VS_GROUP_NONE and any other id are "no group", never used as an index). Its
// key is (image << 32) | (0xFFFFFFFF - (row_base + r)): keys are distinct.
//
//  1. group_best_kernel: best[g] = the largest key of group g. Each wave takes
//     64 consecutive rows; a segmented max scan over the lanes folds every run
//     of equal ids into its last lane, which issues the run's one 64-bit
//     atomic max; the run that ends a wave's 64 rows is held back and folded
//     into the wave's next rows when they go on with the same id, so a wave
//     issues one atomic per run of its own rows (it walks 256 consecutive rows
//     a step). Documents are appended chunk after chunk, so a 10 000-chunk
//     document costs ~40 atomics and a single group holding every row one per
//     wave; any other id layout only has shorter runs (one group per row: one
//     atomic a row, each to its own word). The same launch clears the score
//     pass's digit histogram.
//  2. group_top_kernel<false>: a row is its group's head iff best[gid[r]] is
//     its own key. Every workgroup keeps the `limit` largest head keys of its
//     rows; launch_merge makes the global list (0-padded).
//  3. group_top_kernel<true>: a row belongs to a returned group iff
//     best[gid[r]] >= the last returned head; its slot is the position of
//     best[gid[r]] in that list. Every workgroup keeps, per slot, the
//     `group_size` largest keys of its rows; launch_merge with one "query" per
//     slot makes out[limit][group_size]. Workgroup 0 also writes the groups.
//
// 2 and 3 are one kernel: "the S largest keys of each of `nslots` segments".
// A workgroup holds that table (nslots * S <= 2048 keys) in LDS. Rows stream
// by in 1024-row chunks; a candidate above its slot's current S-th key is
// appended to an LDS buffer, and when the buffer could overflow (and at the
// end) table and buffer are sorted together by (slot, key descending) and the
// first S of every slot become the new table. After the first flush the
// table's S-th keys reject almost every row, so the cost is the stream: one
// group holding every row and one group per row both stay linear in the rows.
// launch_group_clear restores best with one memset of its n_groups words: at
// most the 8 bytes a row the passes read, and far fewer with document-like
// groups, where a pass that revisits only the written entries would stream
// every row's image and id once more.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vs_kernels.h"

namespace vsk {

namespace {

constexpr int kGrpThreads = 256;
constexpr uint32_t kGrpRowsPerThread = 4;
constexpr uint32_t kGrpChunk = kGrpThreads * kGrpRowsPerThread;  // rows a workgroup step
constexpr uint32_t kGrpTab = kGroupsMaxLimit * kGroupsMaxSize;   // 2048 table keys
constexpr uint32_t kGrpBuf = kGrpTab + 2 * kGrpChunk;            // 4096 sort entries
constexpr uint32_t kGrpBestWgs = 1024;
constexpr uint32_t kNoSlot = 0xFFFFu;

static_assert((kGrpBuf & (kGrpBuf - 1)) == 0, "the sort buffer is a power of two");
static_assert(kGrpTab + kGrpChunk <= kGrpBuf, "a chunk fits after a flush");

__device__ __forceinline__ uint64_t row_key(uint32_t image, uint32_t row_base, uint32_t r) {
  return ((uint64_t)image << 32) | (uint32_t)(0xFFFFFFFFu - (row_base + r));
}

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
  const uint32_t lo = __shfl_up((unsigned)(uint32_t)v, d, 64);
  const uint32_t hi = __shfl_up((unsigned)(uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int ln) {
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, ln);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), ln);
  return ((uint64_t)hi << 32) | lo;
}

// One wave, 64 consecutive rows, lane l holding row r of them. (carry_g,
// carry_key) is the wave's pending run, wave-uniform: the last run of the
// rows it has seen, whose atomic is held back because the next rows may go on
// with the same id (carry_g == kGroupNone: none pending).
__device__ __forceinline__ void best_step(uint32_t image, uint32_t g, bool valid, uint32_t r,
                                          uint32_t row_base, unsigned long long* best, int lane,
                                          uint32_t& carry_g, uint64_t& carry_key) {
  if (!valid) g = kGroupNone;
  uint64_t key = valid ? row_key(image, row_base, r) : 0ull;
  const uint32_t gp = __shfl_up(g, 1, 64);
  const bool head = lane == 0 || gp != g;
  const uint64_t heads = __ballot(head);  // bit 0 is always set
  // first lane of this lane's run: the highest head bit at or below the lane
  const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = shfl_up_u64(key, d);
    if (lane - d >= start && o > key) key = o;
  }
  // the last lane of every run now holds the run's largest key
  const uint64_t tails = (heads >> 1) | (1ull << 63);
  if (carry_g != kGroupNone) {
    const int end0 = __builtin_ctzll(tails);  // the first run is lanes [0, end0]
    const uint32_t g0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
    if (g0 == carry_g) {  // wave-uniform: the pending run goes on
      if (lane == end0 && carry_key > key) key = carry_key;
    } else if (lane == 0) {
      atomicMax(best + carry_g, (unsigned long long)carry_key);
    }
  }
  // the run that ends the wave's rows stays pending instead
  carry_g = (uint32_t)__builtin_amdgcn_readlane((int)g, 63);
  carry_key = readlane_u64(key, 63);
  if (((tails >> lane) & 1ull) && lane != 63 && key != 0)
    atomicMax(best + g, (unsigned long long)key);
}

__global__ __launch_bounds__(kGrpThreads) void group_best_kernel(
    const uint32_t* __restrict__ sc, const uint32_t* __restrict__ gid, uint32_t n_rows,
    uint32_t row_base, uint32_t n_groups, unsigned long long* __restrict__ best,
    uint32_t* __restrict__ hist) {
  const int lane = threadIdx.x & 63;
  if (hist)
    for (uint32_t i = blockIdx.x * kGrpThreads + threadIdx.x; i < (uint32_t)kRselBins;
         i += gridDim.x * kGrpThreads)
      hist[i] = 0;
  // a wave owns 256 consecutive rows a step: four 64-row loads in flight
  const uint64_t wave = (uint64_t)blockIdx.x * (kGrpThreads / 64) + (threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (kGrpThreads / 64);
  uint32_t carry_g = kGroupNone;
  uint64_t carry_key = 0;
  for (uint64_t b = wave * 256; b < n_rows; b += waves * 256) {
    uint32_t im[4], g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t r = b + j * 64 + lane;
      const bool in = r < n_rows;
      im[j] = in ? sc[r] : 0u;
      g[j] = in ? gid[r] : kGroupNone;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (b + j * 64 >= n_rows) break;  // wave-uniform
      const uint32_t r = (uint32_t)(b + j * 64 + lane);
      best_step(im[j], g[j], im[j] != 0 && g[j] < n_groups, r, row_base, best, lane, carry_g,
                carry_key);
    }
  }
  if (carry_g != kGroupNone && lane == 0) atomicMax(best + carry_g, (unsigned long long)carry_key);
}

struct GroupLds {
  uint64_t sk[kGrpBuf];   // sort buffer: keys
  uint64_t tab[kGrpTab];  // [nslots][S], every slot descending, 0-padded
  uint64_t hk[kGroupsMaxLimit];  // members: the returned heads, descending
  uint16_t ss[kGrpBuf];   // sort buffer: slots
  uint32_t cnt, nh;
};

// (slot, key) order of the flush: slot ascending, key descending; padding
// (kNoSlot, 0) last.
__device__ __forceinline__ bool grp_before(uint32_t sa, uint64_t ka, uint32_t sb, uint64_t kb) {
  return sa < sb || (sa == sb && ka > kb);
}

// Table + buffer -> table. Every thread of the workgroup calls it.
__device__ __forceinline__ void group_flush(GroupLds& L, uint32_t nslots, uint32_t S) {
  const uint32_t T = nslots * S, t = threadIdx.x;
  __syncthreads();
  if (L.cnt == 0) return;  // uniform: nothing new, the table stands
  __syncthreads();
  for (uint32_t i = t; i < T; i += kGrpThreads) {
    const uint64_t v = L.tab[i];
    if (v) {
      const uint32_t p = atomicAdd(&L.cnt, 1u);
      L.sk[p] = v;
      L.ss[p] = (uint16_t)(i / S);
    }
  }
  __syncthreads();
  const uint32_t c = L.cnt;  // <= kGrpBuf: T + at most kGrpBuf - T candidates
  uint32_t n = 64;
  while (n < c) n <<= 1;
  for (uint32_t i = c + t; i < n; i += kGrpThreads) {
    L.sk[i] = 0;
    L.ss[i] = (uint16_t)kNoSlot;
  }
  for (uint32_t i = t; i < T; i += kGrpThreads) L.tab[i] = 0;
  __syncthreads();
  for (uint32_t k2 = 2; k2 <= n; k2 <<= 1)
    for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
      for (uint32_t i = t; i < n; i += kGrpThreads) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const uint32_t sa = L.ss[i], sb = L.ss[l];
          const uint64_t ka = L.sk[i], kb = L.sk[l];
          const bool up = (i & k2) == 0;
          if (up ? grp_before(sb, kb, sa, ka) : grp_before(sa, ka, sb, kb)) {
            L.ss[i] = (uint16_t)sb, L.ss[l] = (uint16_t)sa;
            L.sk[i] = kb, L.sk[l] = ka;
          }
        }
      }
      __syncthreads();
    }
  // entry i is among the first S of its slot iff the entry S places above is
  // of another slot; its rank is its distance from the slot's first entry
  for (uint32_t i = t; i < c; i += kGrpThreads) {
    const uint32_t s = L.ss[i];
    if (i >= S && L.ss[i - S] == s) continue;
    uint32_t lo = i >= S ? i - S + 1 : 0, hi = i;  // first entry of slot s is in [lo, hi]
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (L.ss[mid] < s) lo = mid + 1; else hi = mid;
    }
    L.tab[s * S + (i - lo)] = L.sk[i];
  }
  __syncthreads();
  if (t == 0) L.cnt = 0;
  __syncthreads();
}

// MEMBERS = false: nslots = 1, S = limit, candidates are the head rows.
// MEMBERS = true: nslots = limit, S = group_size, candidates are the rows of
// the groups in `heads` ([nslots] keys, descending, 0-padded); workgroup 0
// writes groups[nslots]. lists: [gridDim.x][nslots * S].
template <bool MEMBERS>
__global__ __launch_bounds__(kGrpThreads) void group_top_kernel(
    const uint32_t* __restrict__ sc, const uint32_t* __restrict__ gid,
    const unsigned long long* __restrict__ best, uint32_t n_rows, uint32_t row_base,
    uint32_t n_groups, const uint64_t* __restrict__ heads, uint32_t nslots, uint32_t S,
    uint64_t* __restrict__ lists, uint32_t* __restrict__ groups) {
  __shared__ GroupLds L;
  const uint32_t t = threadIdx.x, T = nslots * S;
  for (uint32_t i = t; i < T; i += kGrpThreads) L.tab[i] = 0;
  if (t == 0) L.cnt = 0, L.nh = 0;
  if (MEMBERS && t < nslots) L.hk[t] = heads[t];
  __syncthreads();
  uint64_t hmin = 0;
  uint32_t nh = 0;
  if constexpr (MEMBERS) {
    if (t < nslots && L.hk[t] != 0 && (t + 1 == nslots || L.hk[t + 1] == 0)) L.nh = t + 1;
    __syncthreads();
    nh = L.nh;
    if (blockIdx.x == 0 && t < nslots) {
      // a head's row is a row of the collection: best held its key
      const uint32_t r = 0xFFFFFFFFu - (uint32_t)L.hk[t] - row_base;
      groups[t] = t < nh && r < n_rows ? gid[r] : kGroupNone;
    }
    if (nh) hmin = L.hk[nh - 1];
  }
  uint64_t* out = lists + (uint64_t)blockIdx.x * T;
  if (MEMBERS && nh == 0) {  // no group returned: nothing to look for
    for (uint32_t i = t; i < T; i += kGrpThreads) out[i] = 0;
    return;
  }
  for (uint64_t base = (uint64_t)blockIdx.x * kGrpChunk; base < n_rows;
       base += (uint64_t)gridDim.x * kGrpChunk) {
    const uint32_t pending = L.cnt;
    __syncthreads();  // every thread has read the same count before anyone appends
    if (pending + kGrpChunk > kGrpBuf - T) group_flush(L, nslots, S);
    const uint64_t r0 = base + (uint64_t)t * kGrpRowsPerThread;
    uint32_t im[4] = {0, 0, 0, 0}, g[4] = {kGroupNone, kGroupNone, kGroupNone, kGroupNone};
    if (r0 + 3 < n_rows) {  // 16-byte loads: r0 is a multiple of 4
      const uint4 a = *reinterpret_cast<const uint4*>(sc + r0);
      const uint4 b = *reinterpret_cast<const uint4*>(gid + r0);
      im[0] = a.x, im[1] = a.y, im[2] = a.z, im[3] = a.w;
      g[0] = b.x, g[1] = b.y, g[2] = b.z, g[3] = b.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (r0 + j < n_rows) im[j] = sc[r0 + j], g[j] = gid[r0 + j];
    }
    uint64_t bg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bg[j] = im[j] != 0 && g[j] < n_groups ? best[g[j]] : 0ull;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (im[j] == 0 || g[j] >= n_groups) continue;
      const uint64_t key = row_key(im[j], row_base, (uint32_t)(r0 + j));
      uint32_t slot = 0;
      if constexpr (MEMBERS) {
        if (bg[j] < hmin) continue;
        uint32_t lo = 0, hi = nh;  // slot = heads above the group's best
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (L.hk[mid] > bg[j]) lo = mid + 1; else hi = mid;
        }
        if (lo >= nh || L.hk[lo] != bg[j]) continue;  // not a returned head
        slot = lo;
      } else {
        if (bg[j] != key) continue;
      }
      if (key > L.tab[slot * S + S - 1]) {
        const uint32_t p = atomicAdd(&L.cnt, 1u);
        L.sk[p] = key;
        L.ss[p] = (uint16_t)slot;
      }
    }
    __syncthreads();
  }
  group_flush(L, nslots, S);
  for (uint32_t i = t; i < T; i += kGrpThreads) out[i] = L.tab[i];
}

// the 16-byte loads of sc and gid
bool grp_aligned(const void* a, const void* b) {
  return (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

}  // namespace

uint32_t group_lists(uint32_t n_rows) {
  const uint32_t chunks = (n_rows + kGrpChunk - 1) / kGrpChunk;
  return chunks < 1 ? 1 : (chunks < kGroupsMaxLists ? chunks : kGroupsMaxLists);
}

hipError_t launch_group_best(const uint32_t* sc, const uint32_t* gid, uint32_t n_rows,
                             uint32_t row_base, uint32_t n_groups, uint64_t* best, uint32_t* hist,
                             hipStream_t st) {
  if (n_rows == 0 || (uint64_t)row_base + n_rows > 0xFFFFFFFFull) return hipErrorInvalidValue;
  const uint32_t steps = (n_rows + kGrpChunk - 1) / kGrpChunk;
  const uint32_t nwg = steps < kGrpBestWgs ? steps : kGrpBestWgs;
  hipLaunchKernelGGL(group_best_kernel, dim3(nwg), dim3(kGrpThreads), 0, st, sc, gid, n_rows,
                     row_base, n_groups, (unsigned long long*)best, hist);
  return hipGetLastError();
}

hipError_t launch_group_heads(const uint32_t* sc, const uint32_t* gid, const uint64_t* best,
                              uint32_t n_rows, uint32_t row_base, uint32_t n_groups,
                              uint32_t limit, uint64_t* lists, hipStream_t st) {
  if (n_rows == 0 || (uint64_t)row_base + n_rows > 0xFFFFFFFFull || limit == 0 ||
      limit > kGroupsMaxLimit || !grp_aligned(sc, gid))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(group_top_kernel<false>, dim3(group_lists(n_rows)), dim3(kGrpThreads), 0, st,
                     sc, gid, (const unsigned long long*)best, n_rows, row_base, n_groups,
                     (const uint64_t*)nullptr, 1u, limit, lists, (uint32_t*)nullptr);
  return hipGetLastError();
}

hipError_t launch_group_members(const uint32_t* sc, const uint32_t* gid, const uint64_t* best,
                                uint32_t n_rows, uint32_t row_base, uint32_t n_groups,
                                const uint64_t* heads, uint32_t limit, uint32_t group_size,
                                uint64_t* lists, uint32_t* groups, hipStream_t st) {
  if (n_rows == 0 || (uint64_t)row_base + n_rows > 0xFFFFFFFFull || limit == 0 ||
      limit > kGroupsMaxLimit || group_size == 0 || group_size > kGroupsMaxSize ||
      !grp_aligned(sc, gid))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(group_top_kernel<true>, dim3(group_lists(n_rows)), dim3(kGrpThreads), 0, st,
                     sc, gid, (const unsigned long long*)best, n_rows, row_base, n_groups, heads,
                     limit, group_size, lists, groups);
  return hipGetLastError();
}

hipError_t launch_group_clear(uint64_t* best, uint32_t n_groups, hipStream_t st) {
  if (n_groups == 0) return hipSuccess;
  return hipMemsetAsync(best, 0, (size_t)n_groups * 8, st);
}

}  // namespace vsk
