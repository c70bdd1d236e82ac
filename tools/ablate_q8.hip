// ablate_q8.hip — where the int8 prefilter pass's time goes (r05; VERDICT r04
// item 2). Builds the pass in several modes and times them interleaved in
// one process on one resident corpus, each timing a burst of back-to-back
// launches (sustained clocks, the serving regime):
//   prod     mfma_topk_kernel<768, 0, 2304, 2, false, true>: the 8-wave
//            workgroup, the product until the split workgroups replaced it
//            (prod-sw below is what the library launches)
//   noapp    the same, never appending (timing only: wrong answers)
//   noepi    MODE 1: no epilogue at all (MFMA + LDS reads + stream + barriers)
//   stream   the bf16 kernel at D = 384 (768-B rows: the int8 pass's byte
//            stream and chunk geometry) in MODE 2: the LDS-DMA stream alone
//   mfma     the same in MODE 4: MFMAs (16x16x32 bf16, 16 cycles each: the
//            int8 pass's count and cycles) + LDS reads + barriers, no stream
//   mfma-nb  MODE 5: MODE 4 without barriers
//   mfma8    the int8 instance itself in MODE 4 (its own LDS reads and MFMAs)
//   *-rm     prod, noapp, noepi and mfma8 on the row-major mapping the
//            query-half mapping replaced (VAR 4096: 32 queries x 32 rows a
//            wave, two ds_read_b128 a step; the same bytes out). The library
//            launches the query-half kernel only.
//   *-sw     prod, noapp, noepi, stream8 and mfma8 as split workgroups (VAR
//            268435456: two 4-wave blocks per logical workgroup, 2 x nwg
//            blocks of 256 threads, a 72 KiB ring each; the same bytes out),
//            next to the 8-wave arms in the same rotation. stream8 is the
//            int8 instance's own LDS-DMA stream alone (MODE 2). prod-sw is
//            the product; the 8-wave instance stays in this tool only.
// After the timings: one launch of each of the 8-wave and split clock arms
// (VAR 8192); the split one also reports where the hardware placed the
// blocks (q8-sw_resident_*: all blocks started before any ended, blocks per
// CU, and whether every SIMD of a CU holds one wave of each of its blocks).
// noepi and stream use the product's branch-free stream, as every mode of the
// kernel that streams. The experiment arms once timed here (pair, epipipe,
// spread, prea, split, pd2/pd3, stag, pair+epi, the sample pass's early ring
// fill) were all slower than prod or within noise of it and are out of the
// kernel: DESIGN.md, "Experiments removed from the MFMA scan"; their records
// are profiles/r05_ablate_q8*.json.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ablate_q8.hip -o tools/ablate_q8
//   ablate_q8 [ROWS=10000000] [REPS=5] [BURST=20] [ARM: that arm alone]
#include "../gorilla-rag---agentic-rag-with-mcp-using-golang-microservices_amd/csrc/vs_kernels.hip"
#include "../gorilla-rag---agentic-rag-with-mcp-using-golang-microservices_amd/csrc/vs_q8.hip"

#include <algorithm>
#include <cstdio>
#include <string>
#include <cstdlib>
#include <vector>

using namespace vsk;

#define CK(x)                                                        \
  do {                                                               \
    hipError_t e = (x);                                              \
    if (e != hipSuccess) {                                           \
      printf("HIP %s @%d\n", hipGetErrorString(e), __LINE__);        \
      return 1;                                                      \
    }                                                                \
  } while (0)

struct Ctx {
  MfArgs q8, bf;  // int8 pass arguments; the D = 384 bf16 skeleton's
  uint32_t nwg;
  int burst;
  hipEvent_t a, b;
};

template <int D, int MODE, int VAR, bool I8>
static float run(const Ctx& c) {
  const MfArgs& a = I8 ? c.q8 : c.bf;
  hipEventRecord(c.a, 0);
  constexpr bool kSw = (VAR & kMfVarSplit) != 0;  // split workgroups: twice the blocks of 4 waves
  for (int i = 0; i < c.burst; ++i)
    hipLaunchKernelGGL((mfma_topk_kernel<D, MODE, VAR, 2, false, I8>), dim3(kSw ? 2 * c.nwg : c.nwg),
                       dim3(kSw ? 256 : 512), 0, 0, a);
  hipEventRecord(c.b, 0);
  hipEventSynchronize(c.b);
  float ms = 0;
  hipEventElapsedTime(&ms, c.a, c.b);
  return ms / c.burst;
}

struct Arm {
  const char* name;
  float (*fn)(const Ctx&);
  std::vector<float> t;
};

int main(int argc, char** argv) {
  const uint32_t n = argc > 1 ? (uint32_t)atol(argv[1]) : 10000000u;
  const int reps = argc > 2 ? atoi(argv[2]) : 5;
  const int burst = argc > 3 ? atoi(argv[3]) : 20;
  const uint32_t k = 10, dim = 768;
  uint16_t *X, *Q;
  int8_t *X8, *Q8;
  float *meta, *glob, *par, *tmax, *bnd, *slabs;
  uint32_t *tiles, *cnt, *cmx;
  CK(hipMalloc(&X, ((size_t)n + 32) * dim * 2));
  CK(hipMemset(X, 0, ((size_t)n + 32) * dim * 2));
  CK(hipMalloc(&X8, ((size_t)n + 32) * dim));
  CK(hipMemset(X8, 0, ((size_t)n + 32) * dim));
  CK(hipMalloc(&Q, 256 * dim * 2));
  CK(hipMalloc(&Q8, 256 * dim));
  CK(hipMalloc(&meta, ((size_t)n / 32 + 2) * 8));
  CK(hipMalloc(&glob, 16));
  CK(hipMalloc(&par, 256 * 16 + 64));
  uint32_t* gate = (uint32_t*)(par + 4 * 256);
  CK(launch_generate(0x5EED, 0, n, dim, true, X, 0, 0));
  CK(launch_generate(0xC0FFEE, 0, 256, dim, true, Q, 0, 0));
  CK(hipMemset(glob, 0, 16));
  CK(launch_q8_absmax(X, false, (uint64_t)n * dim, glob, 0));
  CK(launch_q8_set_scale(glob, 0));
  CK(launch_q8_quantize(X, false, n, dim, nullptr, 0, (n + 31) / 32, X8, meta, glob, 0));
  Ctx c{};
  c.burst = burst;
  device_cu_count();
  uint32_t rpw;
  mfma_grid(n, &c.nwg, &rpw);
  const uint32_t st = mfma_sample_tiles(n), cap = mfma_cand_cap(n, k, st, 8.0);
  CK(hipMalloc(&slabs, (size_t)c.nwg * 256 * cap * 32));
  CK(hipMalloc(&tiles, (size_t)c.nwg * 256 * cap * 4));
  CK(hipMalloc(&cnt, (size_t)c.nwg * 256 * 16));
  CK(hipMalloc(&cmx, (size_t)c.nwg * 256 * 16));
  // room for the sample-pass sweep below, which runs 1, 2 and 4 tiles whatever st is
  CK(hipMalloc(&tmax, (size_t)c.nwg * 256 * std::max(st, 4u) * 4));
  CK(hipMalloc(&bnd, 256 * 4));
  uint32_t L = 0;
  CK(launch_mfma_sample(X, false, dim, n, 0, Q, 256, k, st, tmax, c.nwg, &L, 0));
  CK(launch_sample_bound_q8(tmax, L * st, 256, k, bnd, Q, false, 256, dim, glob, Q8, par, gate, 0));
  CK(hipDeviceSynchronize());
  MfArgs& a = c.q8;
  a.X = X8, a.Q = Q8, a.init_score = bnd, a.cand = (uint64_t*)slabs, a.cand_tile = tiles;
  a.cand_cnt = cnt, a.cand_max = cmx, a.n_rows = n, a.row_base = 0, a.rows_per_wg = rpw;
  a.nq_valid = 256, a.k = k, a.cand_cap = cap, a.q8par = par, a.q8glob = glob, a.gate = gate;
  // the bf16 skeleton over the same bytes: 768-B rows read as D = 384 bf16
  MfArgs& f = c.bf;
  f = a;
  f.X = X8, f.Q = Q, f.q8par = nullptr, f.q8glob = nullptr, f.init_score = nullptr;
  hipEventCreate(&c.a);
  hipEventCreate(&c.b);
  std::vector<Arm> arms = {
      {"prod", run<768, 0, 2304, true>, {}},
      {"noapp", run<768, 0, 2304 + 16777216, true>, {}},
      {"noepi", run<768, 1, 2304, true>, {}},
      {"stream", run<384, 2, 2304, false>, {}},
      {"mfma", run<384, 4, 2304, false>, {}},
      {"mfma-nb", run<384, 5, 2304, false>, {}},
      {"mfma8", run<768, 4, 2304, true>, {}},
      {"prod-rm", run<768, 0, 2304 + 4096, true>, {}},
      {"noapp-rm", run<768, 0, 2304 + 4096 + 16777216, true>, {}},
      {"noepi-rm", run<768, 1, 2304 + 4096, true>, {}},
      {"mfma8-rm", run<768, 4, 2304 + 4096, true>, {}},
      {"stream8", run<768, 2, 2304, true>, {}},
      {"prod-sw", run<768, 0, 2304 + kMfVarSplit, true>, {}},
      {"noapp-sw", run<768, 0, 2304 + kMfVarSplit + 16777216, true>, {}},
      {"noepi-sw", run<768, 1, 2304 + kMfVarSplit, true>, {}},
      {"stream8-sw", run<768, 2, 2304 + kMfVarSplit, true>, {}},
      {"mfma8-sw", run<768, 4, 2304 + kMfVarSplit, true>, {}},
  };
  // an arm's name as the 4th argument: that arm alone (PMC passes), R x B launches
  if (argc > 4) {
    for (auto& arm : arms) {
      if (std::string(argv[4]) != arm.name) continue;
      for (int r = 0; r < reps; ++r) arm.t.push_back(arm.fn(c));
      std::sort(arm.t.begin(), arm.t.end());
      printf("{\"rows\": %u, \"%s_ms\": %.4f}\n", n, arm.name, arm.t[arm.t.size() / 2]);
      return 0;
    }
    printf("no arm %s\n", argv[4]);
    return 1;
  }
  for (auto& arm : arms) arm.fn(c);  // warm every arm once
  for (int r = 0; r < reps; ++r)
    for (size_t i = 0; i < arms.size(); ++i) {
      const size_t j = (i + (size_t)r) % arms.size();  // rotate the order per rep
      arms[j].t.push_back(arms[j].fn(c));
    }
  const double bytes = (double)n * dim + 256.0 * dim + 256.0 * k * 12;
  printf("{\"rows\": %u, \"reps\": %d, \"burst\": %d, \"nwg\": %u", n, reps, burst, c.nwg);
  for (auto& arm : arms) {
    std::sort(arm.t.begin(), arm.t.end());
    const double ms = arm.t[arm.t.size() / 2];
    printf(", \"%s_ms\": %.4f, \"%s_hbm_frac\": %.4f", arm.name, ms, arm.name, bytes / (ms * 1e-3) / 8e12);
  }
  // the sample pass (MODE 3, bf16 rows) at 1, 2, 4, 8 tiles per workgroup
  // (the N = 8 share uses 4), timed in bursts, and one launch with the
  // per-workgroup clocks (VAR 8192: start, prologue done, tiles done, end)
  {
    MfArgs sa{};
    sa.X = X, sa.Q = Q, sa.tmax = tmax, sa.n_rows = n, sa.rows_per_wg = rpw;
    sa.nq_valid = 256, sa.k = k;
    const uint32_t sts[4] = {1, 2, 4, 8};
    for (uint32_t st2 : sts) {
      if (st2 > st && st2 > 4) break;  // tmax holds nwg * st tiles per query
      sa.max_tiles = st2;
      std::vector<float> ts;
      for (int r = 0; r < reps; ++r) {
        hipEventRecord(c.a, 0);
        for (int i = 0; i < burst; ++i)
          hipLaunchKernelGGL((mfma_topk_kernel<768, 3, 2304, 2, false, false>), dim3(c.nwg), dim3(512), 0, 0,
                             sa);
        hipEventRecord(c.b, 0);
        hipEventSynchronize(c.b);
        float ms = 0;
        hipEventElapsedTime(&ms, c.a, c.b);
        ts.push_back(ms / burst);
      }
      std::sort(ts.begin(), ts.end());
      printf(", \"sample_st%u_us\": %.2f", st2, ts[ts.size() / 2] * 1e3);
    }
    uint64_t* clkb;
    CK(hipMalloc(&clkb, (size_t)c.nwg * 4 * 8));
    sa.max_tiles = 4 < st ? 4 : st;
    sa.lists = clkb;
    for (int i = 0; i < 3; ++i)
      hipLaunchKernelGGL((mfma_topk_kernel<768, 3, 2304 + 8192, 2, false, false>), dim3(c.nwg), dim3(512), 0, 0,
                         sa);
    CK(hipDeviceSynchronize());
    std::vector<uint64_t> h((size_t)c.nwg * 4);
    CK(hipMemcpy(h.data(), clkb, h.size() * 8, hipMemcpyDeviceToHost));
    uint64_t t0 = ~0ull;
    for (uint32_t b = 0; b < c.nwg; ++b) t0 = std::min(t0, h[4 * b]);
    const char* nm[4] = {"start", "prologue", "tiles", "end"};
    for (int j = 0; j < 4; ++j) {
      std::vector<double> v;
      for (uint32_t b = 0; b < c.nwg; ++b) v.push_back((h[4 * b + j] - t0) * 0.01);
      std::sort(v.begin(), v.end());
      printf(", \"sample_clk_%s_us_med\": %.2f, \"sample_clk_%s_us_max\": %.2f", nm[j], v[v.size() / 2], nm[j],
             v.back());
    }
  }
  // the int8 pass's own clocks, both mappings (the query-half prologue loads
  // 64 queries' fragments a wave, the row-major one 32)
  {
    uint64_t* clkb;
    CK(hipMalloc(&clkb, (size_t)c.nwg * 4 * 8));
    MfArgs qa = c.q8;
    qa.lists = clkb;
    for (int rm = 0; rm < 2; ++rm) {
      for (int i = 0; i < 3; ++i) {
        if (rm)
          hipLaunchKernelGGL((mfma_topk_kernel<768, 0, 2304 + 4096 + 8192, 2, false, true>), dim3(c.nwg),
                             dim3(512), 0, 0, qa);
        else
          hipLaunchKernelGGL((mfma_topk_kernel<768, 0, 2304 + 8192, 2, false, true>), dim3(c.nwg), dim3(512),
                             0, 0, qa);
      }
      CK(hipDeviceSynchronize());
      std::vector<uint64_t> h((size_t)c.nwg * 4);
      CK(hipMemcpy(h.data(), clkb, h.size() * 8, hipMemcpyDeviceToHost));
      std::vector<double> v;  // prologue: start -> fragments and bounds loaded, per workgroup
      for (uint32_t b = 0; b < c.nwg; ++b) v.push_back((h[4 * b + 1] - h[4 * b]) * 0.01);
      std::sort(v.begin(), v.end());
      printf(", \"q8%s_clk_prologue_us_med\": %.2f, \"q8%s_clk_prologue_us_max\": %.2f", rm ? "-rm" : "",
             v[v.size() / 2], rm ? "-rm" : "", v.back());
    }
  }
  // the split instance's clocks and residency: 8 words per physical block
  // (4 clocks, then the hardware id of each of its 4 waves)
  {
    const uint32_t nb = 2 * c.nwg;
    uint64_t* clkb;
    CK(hipMalloc(&clkb, (size_t)nb * 8 * 8));
    MfArgs qa = c.q8;
    qa.lists = clkb;
    for (int i = 0; i < 3; ++i)
      hipLaunchKernelGGL((mfma_topk_kernel<768, 0, 2304 + kMfVarSplit + 8192, 2, false, true>), dim3(nb),
                         dim3(256), 0, 0, qa);
    CK(hipDeviceSynchronize());
    std::vector<uint64_t> h((size_t)nb * 8);
    CK(hipMemcpy(h.data(), clkb, h.size() * 8, hipMemcpyDeviceToHost));
    uint64_t last_start = 0, first_end = ~0ull;
    std::vector<double> v;
    for (uint32_t b = 0; b < nb; ++b) {
      last_start = std::max(last_start, h[8 * b]);
      first_end = std::min(first_end, h[8 * b + 3]);
      v.push_back((h[8 * b + 1] - h[8 * b]) * 0.01);
    }
    std::sort(v.begin(), v.end());
    // a CU: (XCC, SE, SH, CU) of the id word; a block's four waves must sit on
    // one CU, on four different SIMDs
    std::vector<std::pair<uint32_t, uint32_t>> cu_of;  // (cu key, simd mask) per block
    bool one_cu = true;
    for (uint32_t b = 0; b < nb; ++b) {
      uint32_t key0 = 0, mask = 0;
      for (int wv = 0; wv < 4; ++wv) {
        const uint64_t id = h[8 * b + 4 + wv];
        const uint32_t hw = (uint32_t)id, xcc = (uint32_t)(id >> 32) & 0xFu;
        const uint32_t key = (xcc << 16) | (hw & 0xFF00u);
        if (wv == 0) key0 = key;
        one_cu &= key == key0;
        mask |= 1u << ((hw >> 4) & 3u);
      }
      cu_of.push_back({key0, mask});
    }
    std::sort(cu_of.begin(), cu_of.end());
    uint32_t cus = 0, min_b = ~0u, max_b = 0, simd_ok = 1;
    for (size_t i = 0; i < cu_of.size();) {
      size_t j = i;
      while (j < cu_of.size() && cu_of[j].first == cu_of[i].first) {
        simd_ok &= cu_of[j].second == 0xFu;  // one wave of this block on every SIMD
        ++j;
      }
      ++cus;
      min_b = std::min(min_b, (uint32_t)(j - i));
      max_b = std::max(max_b, (uint32_t)(j - i));
      i = j;
    }
    printf(", \"q8-sw_clk_prologue_us_med\": %.2f, \"q8-sw_clk_prologue_us_max\": %.2f", v[v.size() / 2],
           v.back());
    printf(", \"q8-sw_resident_blocks\": %u, \"q8-sw_resident_all_started_before_any_end\": %d, "
           "\"q8-sw_resident_start_to_first_end_us\": %.2f, \"q8-sw_resident_cus\": %u, "
           "\"q8-sw_resident_blocks_per_cu_min\": %u, \"q8-sw_resident_blocks_per_cu_max\": %u, "
           "\"q8-sw_resident_block_on_one_cu\": %d, \"q8-sw_resident_one_wave_per_simd\": %u",
           nb, (int)(last_start < first_end), ((double)first_end - (double)last_start) * 0.01, cus, min_b,
           max_b, (int)one_cu, simd_ok);
  }
  printf("}\n");
  return 0;
}
