// plf_kernels.hip -- launchers of the fused PLF kernels for CDNA4 (gfx950).
//
// One kernel replaces the reference's whole accelerator pipeline for one PLF
// call: the PL input movers (hls/src/mm2sleft_memDNAwindowComb.cpp:16-100,
// mm2sright_*, transpose.cpp:6-24), the AIE lane chain mmul_branch x2 ->
// combine -> ev (aie/src/128x9DNAwindow8192Comb/kernels/*.cpp) and the PL
// output mover with the underflow test/rescale and the char scaler
// (hls/src/s2mm_memDNAwindowComb.cpp:45-99), plus the host's weighted scaler
// reduction (app/src/host_mem.cpp:384-388).  Arithmetic follows the CPU
// definition plf() (app/src/plf.cpp:19-65) operation for operation.  The
// device code and its mapping are documented in plf_dna.hpp / DESIGN.md.
//
// Grids: grid-stride kernels launch at most the co-resident block count
// (occupancy x CUs, plf_launch.hpp grid_x); batched launches spread those
// blocks over the batch's nodes (blockIdx.y = node).  Run-time choices (dtype,
// scaler sum, tips, depth) become template arguments through dispatch().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "plf_dna.hpp"
#include "plf_kernels.hpp"
#include "plf_launch.hpp"
#include "plf_lnl.hpp"
#include "plf_pmat.hpp"
#include "plf_prot.hpp"

namespace plfx {
namespace {

using dev::kBlock;
using dev::kWavesPerBlock;
static_assert(kBlockThreads == kBlock, "block size mismatch");
static_assert(kWsWords == dev::kWsWords, "workspace size mismatch");
static_assert(kMaxBatch == dev::kMaxBatch, "batch size mismatch");
static_assert(sizeof(NodeDescH) == sizeof(dev::NodeDesc), "node descriptor mismatch");
static_assert(sizeof(TripleDescH) == sizeof(dev::TripleDesc), "triple descriptor mismatch");
static_assert(kMaxTriples == dev::kMaxTriples && 3 * kMaxTriples <= kMaxBatch, "triple batch size");
static_assert(sizeof(SeptetDescH) == sizeof(dev::SeptetDesc), "septet descriptor mismatch");
static_assert(kMaxSeptets == dev::kMaxSeptets, "septet batch size");
static_assert(kDeepQueueRegion == dev::kDeepQueueRegion, "deep queue region");
static_assert(sizeof(DeepDescH) == sizeof(dev::DeepDesc), "deep descriptor mismatch");
static_assert(kProtCombos == dev::kProtCombos, "combination count");

// Tuned on MI355X (tools/tune_plf.hip@f9b3af3, profiles/r01_tune.log):
// f64 lane-pair kernel, 2 x 16-site steps per trip, non-temporal CLV loads
// and stores, grid = resident blocks.
constexpr int kU64 = 2, kU32 = 4;
constexpr bool kNt = true;   // f32: NT CLV loads (74.8% vs 70.2% of HBM peak, r01_tune_f32.log)
constexpr bool kNtl64 = true;
constexpr int kMinWaves = 1;
constexpr int kBlocksPerCu32 = 2;  // f32 node kernel grid (launch_cat)
constexpr int kTripleU = 1;  // fused level pairs: 16 sites per trip (tools/tune_triple.hip@f9b3af3)
constexpr int kTripleUTips = 2;  // with coded tips: 32 sites per trip (+13-19 % for 2 tip
                                 // children, equal for 1; profiles/r01_ab_fused_tips.log)
constexpr int kTripleU32 = 2;
// fused three-level subtrees: 2 x 8-site blocks per trip, matrices re-read from
// LDS, next trip's loads in flight (tools/tune_septet.hip@f9b3af3, r01_tune_septet.log)
constexpr int kSeptetU = 2;
constexpr int kSeptetU32 = 2;  // f32 (lane = category): 2 x 16-site blocks per trip
constexpr int kDeepU32 = 2;    // f32 six-level pass: 2 x 16-site blocks per trip

// Node kernels switch to the XCD-segmented site mapping (plf_dna.hpp
// wave_sites, kSegL2 = 3) from min_sites up, or always / never with
// DnaArgs::segments.  The thresholds are measured, segmented vs not on the same
// buffers, calls alternating (tools/max_sites.py --ab, three boxes,
// profiles/r05_node_segments_ab.log): f32 +3-4 % at 2^25 sites, +9-29 % from
// 5e7 up; f64 -2 to +1 % at 2^25, +1 % at 2^26, +5-12 % from 1e8 up -- and both
// 6-8 % SLOWER at 2^24, equal below.  Round 6 (tools/node_placement.py, three
// fresh buffer sets per size in one process, profiles/r06_node_placement*.log):
// f64 at 5e7 sites +8-9 % with segments (0.74-0.77 vs 0.68-0.71), so f64 now
// switches from 2^25 as f32 does.  Returns the segmented launch's grid -- the capped grid
// gx rounded down to a multiple of 8 (blocks b and b + 8 share an XCD) -- or
// 0: not segmented.  Never more blocks than gx: below 8 (a small node, or a
// PLFX_MAX_BLOCKS cap < 8) the one-window mapping runs instead.
constexpr int64_t kSegMinSites32 = int64_t(1) << 25, kSegMinSites64 = int64_t(1) << 25;
int64_t segment_grid(const DnaArgs &a, int64_t gx, int64_t min_sites) {
  if (a.segments == 0 || (a.segments < 0 && a.n < min_sites) || gx < 8) return 0;
  return gx - gx % 8;
}

template <typename T, bool kSum>
hipError_t launch_cat(const DnaArgs &a, int max_blocks, hipStream_t s) {
  static int cache = 0;
  auto kernel = &dev::plf_dna_kernel<T, kU32, kSum, kNt, kMinWaves>;
  // 2 blocks per CU rather than the 3 co-resident ones: at 2^20 sites U = 4
  // leaves 5.33 trips per wave at 3/CU (a sixth trip for a third of the waves)
  // and exactly 8 at 2/CU -- 35.4 vs 35.8 us, and 68.4 vs 69.2 us at 2^21
  // (tools/ab_defer.hip@f9b3af3, tools/tune_f32.hip@f9b3af3; profiles/r02_tune_f32.log)
  // With `streams` calls in flight each takes 1/streams of it: two f32 nodes
  // on two streams at 256 blocks each run 0.773 of the HBM peak in 20-step
  // regions vs 0.746 at 512 (tools/probes/node_grid_lanes_f32.sh,
  // profiles/r06_probe_node_grid_lanes.log)
  const int64_t gx = grid_x((const void *)kernel, cache, a.n, kWavesPerBlock * 16 * kU32, 1,
                            max_blocks > 0 ? max_blocks
                                           : std::max(1, kBlocksPerCu32 * cu_count() / std::max(1, a.streams)));
  const int64_t gs = segment_grid(a, gx, kSegMinSites32);
  if (gs) kernel = &dev::plf_dna_kernel<T, kU32, kSum, kNt, kMinWaves, 3>;
  return launch_node<T>(kernel, gs ? gs : gx, s, a);
}

template <bool kSum>
hipError_t launch_pair(const DnaArgs &a, int max_blocks, hipStream_t s) {
  static int cache = 0;
  auto kernel = &dev::plf_dna_f64_pair_kernel<kU64, kSum, kMinWaves, kNtl64>;
  // resident blocks / streams: two 2^20-site nodes in flight on two streams at
  // 512 blocks each (16 trips per block) run 0.775 in 20-step regions and 0.80
  // in 200-step ones, vs 0.750 / 0.778 at 1024 (8 trips); one node alone at
  // 512 runs 0.64 (tools/probes/node_grid_lanes.sh, profiles/r06_probe_node_grid_lanes.log)
  const int64_t gx = grid_x((const void *)kernel, cache, a.n, kWavesPerBlock * 16 * kU64,
                            std::max(1, a.streams), max_blocks);
  const int64_t gs = segment_grid(a, gx, kSegMinSites64);
  if (gs) kernel = &dev::plf_dna_f64_pair_kernel<kU64, kSum, kMinWaves, kNtl64, 3>;
  return launch_node<double>(kernel, gs ? gs : gx, s, a);
}

// One template per batched launcher, f32 and f64: EV and tipvec are values of T.
template <typename T, bool kSum, int kTips>
hipError_t launch_dna_batch_t(const dev::NodeBatch &b, int count, const void *EV, const int32_t *wgt,
                              int64_t n, unsigned long long *ws, int max_blocks, hipStream_t s,
                              const void *tipvec, int share) {
  static int cache = 0;
  auto kernel = [] {
    if constexpr (sizeof(T) == 8) return &dev::plf_dna_f64_pair_batch_kernel<kU64, kSum, kMinWaves, kNtl64, kTips>;
    else return &dev::plf_dna_batch_kernel<T, kU32, kSum, kNt, kMinWaves, kTips>;
  }();
  constexpr int U = sizeof(T) == 8 ? kU64 : kU32;
  // share: batches the caller keeps in flight on as many streams (plfx_ctx_set_streams)
  const int64_t gx = grid_x((const void *)kernel, cache, n, kWavesPerBlock * 16 * U,
                            count * std::max(1, share), max_blocks);
  return launch(kernel, dim3((unsigned)gx, (unsigned)count), kBlock, s, b, (const T *)EV, wgt, n, ws,
                (const T *)tipvec);
}

template <typename T, int S, int C>
hipError_t launch_lnl_t(const T *x, int64_t n, const double *catw, const double *freq,
                        const int32_t *wgt, const int64_t *sums, int nsums, double *partials,
                        unsigned long long *ticket, double *out, double *site_lnl, hipStream_t s) {
  static int cache = 0;
  auto kernel = &dev::root_lnl_kernel<T, S, C>;
  // C steps of 64/C sites per wave trip; 2 blocks per CU (more trips per wave: the
  // kernel is short and its ramp and final reduction weigh; tools/ab_lnl.hip@f9b3af3)
  int64_t gx = grid_x((const void *)kernel, cache, n, kWavesPerBlock * 64, 1, 0);
  gx = std::min<int64_t>({gx, 2 * (int64_t)cu_count(), kLnlMaxGrid});
  return launch(kernel, dim3((unsigned)gx), kBlock, s, x, n, catw, freq, wgt, sums, nsums, partials, ticket,
                out, site_lnl);
}

// protein root lnL: 64-site LDS tiles, the co-resident grid (plf_lnl.hpp
// root_lnl_prot_kernel; the C-lanes form took 94 us for 2^18 f64 sites)
template <typename T>
hipError_t launch_lnl_prot_t(const T *x, int64_t n, const double *catw, const double *freq,
                             const int32_t *wgt, const int64_t *sums, int nsums, double *partials,
                             unsigned long long *ticket, double *out, double *site_lnl, hipStream_t s) {
  static int cache = 0;
  auto kernel = &dev::root_lnl_prot_kernel<T>;
  const int64_t gx = std::min<int64_t>(grid_x((const void *)kernel, cache, n, 64, 1, 0), kLnlMaxGrid);
  return launch(kernel, dim3((unsigned)gx), kBlock, s, x, n, catw, freq, wgt, sums, nsums, partials, ticket,
                out, site_lnl);
}

template <typename T, bool kFma, bool kSum, int kTips>
hipError_t launch_prot_t(const DnaArgs &a, int max_blocks, hipStream_t s, const void *tipvec) {
  static_assert(sizeof(T) == 4, "f32 protein; f64 runs launch_prot_mfma_t / launch_prot_exact64_t");
  static int cache = 0;
  // f32: FMA mode on the matrix cores (v_mfma_f32_16x16x4_f32 = fmaf chain;
  // rows 16..19 of the products and the back-transform on 4x4x1_16b, kQ = 2:
  // 52.4 -> 46.5 us at 2^18, profiles/r02_tune_protein_f32_q.log), exact mode
  // on the LDS-matrix kernel (4-row groups, tile prefetch)
  // (tools/tune_prot32.hip@f9b3af3, profiles/r02_tune_protein_f32.log)
  if constexpr (kFma) {
    auto kernel = &dev::plf_prot_mfma32_kernel<kSum, 3, kTips>;
    // with `streams` calls in flight: the resident blocks per CU / streams,
    // rounded UP to whole blocks per CU (3 per CU -> 2 at two streams: 0.743-
    // 0.746 vs 0.728-0.730 at the full grid and 0.737 at 1.5 per CU;
    // profiles/r06_probe_prot_grid_lanes.log)
    int cap = max_blocks;
    if (cap <= 0 && a.streams > 1) {
      const int cus = cu_count(), per_cu = std::max(1, resident_blocks((const void *)kernel, kBlock, 2, cache) / cus);
      cap = cus * ((per_cu + a.streams - 1) / a.streams);
    }
    return launch_node<T>(kernel, grid_x((const void *)kernel, cache, a.n, 64, 1, cap), s, a, tipvec);
  } else {
    auto kernel = &dev::plf_prot_lds_kernel<T, kSum, 2, kTips, 4, false>;
    return launch_node<T>(kernel, grid_x((const void *)kernel, cache, a.n, 64, 1, max_blocks), s, a, tipvec);
  }
}

template <bool kSum, int kTips>
hipError_t launch_prot_mfma_t(const DnaArgs &a, int max_blocks, hipStream_t s, const void *tipvec) {
  static int cache = 0;
  // X3 to LDS through permuted back-transform rows (kX3 = 2: conflict-free
  // b128 writes; 90.2 vs 91.2 us at 2^18, 342 vs 345 at 2^20, tools/tune_prot.hip@f9b3af3,
  // profiles/r02_tune_protein_v3.log); first tile's loads before the matrix fragments.
  // From 32 tiles per block (2^20 sites at 512 blocks) on, tiles come from the
  // device-wide queue (kDyn, plf_prot.hpp ProtQueue): 2^20 -3..-5 %, 2^22 -10 %
  // dense, tip/inner -8 / -14 %; below that, and for tip/tip nodes at any size,
  // the fixed stride is as fast or faster (tools/tune_prot64d.hip@f9b3af3,
  // profiles/r03_tune_protein_dyn.log)
  auto kernel = &dev::plf_prot_mfma_kernel<kSum, 2, kTips, false>;
  // resident blocks / streams (two 2^18-site nodes in flight: 256 blocks each,
  // +1-2 %; the VALU protein kernels keep their full grid, which measured best
  // with two in flight too -- tools/probes/prot_grid_lanes.sh,
  // profiles/r06_probe_prot_grid_lanes.log)
  const int64_t gx = grid_x((const void *)kernel, cache, a.n, 64, std::max(1, a.streams), max_blocks);
  if constexpr (kTips < 2)  // the queue form exists for dense and tip/inner nodes only
    if (a.ws && (a.n + 63) / 64 >= 32 * gx) kernel = &dev::plf_prot_mfma_kernel<kSum, 2, kTips, true>;
  return launch_node<double>(kernel, gx, s, a, tipvec);
}

template <bool kSum, int kTips>
hipError_t launch_prot_exact64_t(const DnaArgs &a, int max_blocks, hipStream_t s, const void *tipvec) {
  static int cache = 0;
  // 10-row groups + tile prefetch (tools/tune_prot.hip@f9b3af3, profiles/r02_tune_protein_exact_rows.log)
  auto kernel = &dev::plf_prot_lds_kernel<double, kSum, 2, kTips, 10, true>;
  return launch_node<double>(kernel, grid_x((const void *)kernel, cache, a.n, 64, 1, max_blocks), s, a, tipvec);
}

template <typename T, bool kSum, int kTips>
hipError_t launch_triples_t(const dev::TripleBatch &b, int count, const void *EV, const int32_t *wgt,
                            int64_t n, unsigned long long *ws, int max_blocks, hipStream_t s,
                            const void *tipvec) {
  static int cache = 0;
  constexpr int U = sizeof(T) == 4 ? kTripleU32 : kTips ? kTripleUTips : kTripleU;
  auto kernel = [] {
    if constexpr (sizeof(T) == 8) return &dev::plf_dna_f64_triple_kernel<kSum, 1, kNtl64, kTips, U>;
    else return &dev::plf_dna_cat_triple_kernel<T, kSum, 1, kNt, kTips, U>;
  }();
  const int64_t gx = grid_x((const void *)kernel, cache, n, kWavesPerBlock * 16 * U, count, max_blocks);
  return launch(kernel, dim3((unsigned)gx, (unsigned)count), kBlock, s, b, (const T *)EV, wgt, n, ws,
                (const T *)tipvec);
}

template <typename T, bool kSum, int kTips>
hipError_t launch_septets_t(const dev::SeptetBatch &b, int count, const void *EV, const int32_t *wgt,
                            int64_t n, unsigned long long *ws, int max_blocks, hipStream_t s,
                            const void *tipvec) {
  static int cache = 0;
  auto kernel = [] {
    // f64: next-trip prefetch for dense leaves only: with coded leaves the pass is
    // write-bound and the prefetch registers cost 4-4.5 % (r01_ab_fused_tips.log)
    if constexpr (sizeof(T) == 8) return &dev::plf_dna_f64_septet_kernel<kSum, 1, kNtl64, kTips, kSeptetU, kTips == 0>;
    else return &dev::plf_dna_cat_septet_kernel<T, kSum, 1, kNt, kTips, kSeptetU32>;
  }();
  constexpr int kSites = sizeof(T) == 8 ? kWavesPerBlock * 8 * kSeptetU : kWavesPerBlock * 16 * kSeptetU32;
  const int64_t gx = grid_x((const void *)kernel, cache, n, kSites, count, max_blocks);
  return launch(kernel, dim3((unsigned)gx, (unsigned)count), kBlock, s, b, (const T *)EV, wgt, n, ws,
                (const T *)tipvec);
}

// fused six-level subtrees: 512-thread blocks (one LDS copy of the 63 nodes'
// matrices per 8 waves), 2 x 8-site blocks per trip, grid = co-resident blocks
// (tools/gpu_deep.sh@f9b3af3, profiles/r01_deep.log)
constexpr int kDeepThreads = 512;
template <int D, typename T, bool kSum, int kTips>
hipError_t launch_deep_t(const dev::DeepDesc &d, const void *EV, const int32_t *wgt, int64_t n,
                         unsigned long long *ws, int max_blocks, hipStream_t s, const void *tipvec) {
  // chunks from the wave-level queue (plf_dna.hpp WaveQueue, kDyn) whenever there is
  // a workspace: the fixed stride left wave exits spread over 2.61-3.36 ms of a
  // 2^20-site f64 pass (same process: 3358 -> 3116 us,
  // profiles/r03_tune_deep_dyn.log; bench tree64 f64 --tips 1688 -> 1643 us,
  // f32 --tips 875 -> 861, f32 dense equal, profiles/r03_ab_deep_dyn.log)
  // (the traversal always has a stream workspace when it launches a pass)
  if (!ws) return hipErrorInvalidValue;
  static int cache = 0;
  // coded leaves, f32: 4 x 16-site blocks per trip, as f64: tree64 f32 --tips
  // 0.664 (U = 2) -> 0.707 same box, U = 1 0.673; three-level passes 0.633
  // (profiles/r03_ab_deep_tips_u_f32.log)
  // coded leaves, f64: 4 x 8-site blocks per trip (every output stream gets 4 KiB
  // runs per wave and trip; the pass is write-bound): 0.693 -> 0.727 of
  // peak on tree64 --tips same box, U = 1 0.637; U = 6/8 spill
  // (profiles/r03_ab_deep_tips_u.log)
  constexpr int U = kTips == 2 ? 4 : sizeof(T) == 8 ? 2 : kDeepU32;
  // f64: lane pairs, 8 sites per wave instruction; f32: lane = category, 16
  auto kernel = [] {
    if constexpr (sizeof(T) == 8) return &dev::plf_dna_f64_deep_kernel<D, kSum, kNtl64, U, kDeepThreads, kTips, true>;
    else return &dev::plf_dna_cat_deep_kernel<D, T, kSum, kNt, U, kDeepThreads, kTips, true>;
  }();
  constexpr int kSitesPerWave = sizeof(T) == 8 ? 8 : 16;
  const int64_t gx = grid_x((const void *)kernel, cache, n, (kDeepThreads / 64) * kSitesPerWave * U, 1,
                            max_blocks, kDeepThreads, 1);
  return launch(kernel, dim3((unsigned)gx), kDeepThreads, s, d, (const T *)EV, wgt, n, ws, (const T *)tipvec);
}

// Protein batches: grid (resident blocks, count) -- every node gets the grid a
// one-node launch would (the kernels keep their one-node grid stride) and the
// nodes' blocks follow each other through the co-resident slots.
template <typename T, bool kFma, bool kSum, int kTips>
hipError_t launch_prot_batch_t(const dev::NodeBatch &b, int count, const void *EV, const int32_t *wgt,
                               int64_t n, unsigned long long *ws, int max_blocks, hipStream_t s,
                               const void *tipvec) {
  static int cache = 0;
  auto kernel = [] {
    if constexpr (sizeof(T) == 8 && kFma) return &dev::plf_prot_mfma_batch_kernel<kSum, 2, kTips>;
    else if constexpr (sizeof(T) == 8) return &dev::plf_prot_lds_batch_kernel<double, kSum, 2, kTips, 10, true>;
    else if constexpr (kFma) return &dev::plf_prot_mfma32_batch_kernel<kSum, 3, kTips>;
    else return &dev::plf_prot_lds_batch_kernel<float, kSum, 2, kTips, 4, false>;
  }();
  const int64_t gx = grid_x((const void *)kernel, cache, n, 64, 1, max_blocks);
  return launch(kernel, dim3((unsigned)gx, (unsigned)count), kBlock, s, b, (const T *)EV, wgt, n, ws,
                (const T *)tipvec);
}

template <typename T, bool kFma, bool kSum>
hipError_t launch_prot_tab_t(const dev::ProtTabBatch &b, int count, const void *EV, const int32_t *wgt,
                             int64_t n, unsigned long long *ws, int max_blocks, hipStream_t s) {
  static int cache = 0;
  auto kernel = [] {
    // exact: the exact bodies' shapes (launch_prot_t / launch_prot_exact64_t)
    if constexpr (sizeof(T) == 8 && kFma) return &dev::plf_prot_mfma_tab_batch_kernel<kSum>;
    else if constexpr (sizeof(T) == 8) return &dev::plf_prot_lds_tab_batch_kernel<double, kSum, 10, true>;
    else if constexpr (kFma) return &dev::plf_prot_mfma32_tab_batch_kernel<kSum>;
    else return &dev::plf_prot_lds_tab_batch_kernel<float, kSum, 4, false>;
  }();
  const int64_t gx = grid_x((const void *)kernel, cache, n, 64, 1, max_blocks);  // full grid per node
  return launch(kernel, dim3((unsigned)gx, (unsigned)count), kBlock, s, b, (const T *)EV, wgt, n, ws);
}

using bools = among<false, true>;
const auto node_sum = [](const auto &d) { return d.scaler_sum != nullptr; };

}  // namespace

hipError_t launch_plf_dna_deep(int dtype, int depth, const DeepDescH *t, const void *EV,
                               const int32_t *wgt, int64_t n, unsigned long long *ws, int max_blocks,
                               hipStream_t s, int tips, const void *tipvec) {
  if (depth < 4 || depth > 6) return hipErrorInvalidValue;
  dev::DeepDesc d;
  __builtin_memcpy(&d, t, sizeof(d));
  bool any_sum = false;
  for (int q = 0; q < (1 << depth) - 1; q++) any_sum |= t->ss[q] != nullptr;
  // tips: every leaf dense (0) or every leaf coded (2)
  return dispatch(
      [&](auto kD, auto k64, auto kSum, auto kTips) {
        return launch_deep_t<kD(), real_t<k64()>, kSum(), kTips()>(d, EV, wgt, n, ws, max_blocks, s, tipvec);
      },
      among<4, 5, 6>{depth}, bools{dtype == 1}, bools{any_sum}, among<0, 2>{tips});
}

hipError_t launch_plf_dna_septets(int dtype, const SeptetDescH *t, int count, const void *EV,
                                  const int32_t *wgt, int64_t n, unsigned long long *ws,
                                  int max_blocks, hipStream_t s, int tips, const void *tipvec) {
  if (count < 1 || count > kMaxSeptets || tips < 0 || tips > 2) return hipErrorInvalidValue;
  const auto p = pack<dev::SeptetBatch>(t, count, [](const SeptetDescH &d) {
    return std::any_of(d.ss, d.ss + 7, [](const int64_t *ss) { return ss != nullptr; });
  });
  return dispatch(
      [&](auto k64, auto kSum, auto kTips) {
        return launch_septets_t<real_t<k64()>, kSum(), kTips()>(p.b, count, EV, wgt, n, ws, max_blocks, s, tipvec);
      },
      bools{dtype == 1}, bools{p.any_sum}, among<0, 1, 2>{tips});
}

hipError_t launch_plf_dna_triples(int dtype, const TripleDescH *t, int count, const void *EV,
                                  const int32_t *wgt, int64_t n, unsigned long long *ws,
                                  int max_blocks, hipStream_t s, int tips, const void *tipvec) {
  if (count < 1 || count > kMaxTriples || tips < 0 || tips > 2) return hipErrorInvalidValue;
  const auto p = pack<dev::TripleBatch>(t, count, [](const TripleDescH &d) { return d.ssa || d.ssb || d.ssp; });
  return dispatch(
      [&](auto k64, auto kSum, auto kTips) {
        return launch_triples_t<real_t<k64()>, kSum(), kTips()>(p.b, count, EV, wgt, n, ws, max_blocks, s, tipvec);
      },
      bools{dtype == 1}, bools{p.any_sum}, among<0, 1, 2>{tips});
}

hipError_t launch_plf_prot_batch(int dtype, bool fma, const NodeDescH *nodes, int count, const void *EV,
                                 const int32_t *wgt, int64_t n, unsigned long long *ws, int max_blocks,
                                 hipStream_t s, int tips, const void *tipvec) {
  if (count < 1 || count > kMaxBatch || tips < 0 || tips > 2) return hipErrorInvalidValue;
  const auto p = pack<dev::NodeBatch>(nodes, count, node_sum);
  return dispatch(
      [&](auto k64, auto kFma, auto kSum, auto kTips) {
        // tips == 2 runs only as the combination tables of tip/tip nodes (trav_lower.hpp
        // kLaunchProtTipTip), which carry no sum: a tip/tip node's sum comes from the
        // gather, so the summing tip/tip forms are not built
        if constexpr (kTips() == 2 && kSum()) return hipErrorInvalidValue;
        else
          return launch_prot_batch_t<real_t<k64()>, kFma(), kSum(), kTips()>(p.b, count, EV, wgt, n, ws,
                                                                              max_blocks, s, tipvec);
      },
      bools{dtype == 1}, bools{fma}, bools{p.any_sum}, among<0, 1, 2>{tips});
}

hipError_t launch_prot_tiptip_gather(int dtype, const ProtGatherDescH *d, int count, const int32_t *wgt,
                                     int64_t n, unsigned long long *ws, int max_blocks, hipStream_t s) {
  if (count < 1 || count > kMaxBatch) return hipErrorInvalidValue;
  const auto p = pack<dev::ProtGatherBatch>(d, count, node_sum);
  return dispatch(
      [&](auto k64, auto kSum) {
        static int cache = 0;
        auto kernel = &dev::prot_tiptip_gather_kernel<real_t<k64()>, kSum()>;
        const int64_t gx = grid_x((const void *)kernel, cache, n, 64, 1, max_blocks);
        return launch(kernel, dim3((unsigned)gx, (unsigned)count), kBlock, s, p.b, wgt, n, ws);
      },
      bools{dtype == 1}, bools{p.any_sum});
}

hipError_t launch_prot_tab_batch(int dtype, bool fma, const ProtTabDescH *d, int count, const void *EV,
                                 const int32_t *wgt, int64_t n, unsigned long long *ws, int max_blocks,
                                 hipStream_t s) {
  if (count < 1 || count > kMaxBatch) return hipErrorInvalidValue;
  const auto p = pack<dev::ProtTabBatch>(d, count, node_sum);
  return dispatch(
      [&](auto k64, auto kFma, auto kSum) {
        return launch_prot_tab_t<real_t<k64()>, kFma(), kSum()>(p.b, count, EV, wgt, n, ws, max_blocks, s);
      },
      bools{dtype == 1}, bools{fma}, bools{p.any_sum});
}

hipError_t launch_plf_prot(int dtype, bool fma, const DnaArgs &a, int max_blocks, hipStream_t s,
                           int tips, const void *tipvec) {
  // tip/tip nodes (tips == 2) always go through the combination tables of the
  // stream's workspace (launch_plf_prot_batch over the 576 code pairs, then
  // launch_prot_tiptip_gather), never a one-node kernel
  return dispatch(
      [&](auto k64, auto kFma, auto kSum, auto kTips) {
        // f64 FMA on the matrix cores: bit-identical to the fused VALU chain;
        // f64 exact: matrices broadcast from LDS (plf_prot.hpp)
        if constexpr (k64() && kFma()) return launch_prot_mfma_t<kSum(), kTips()>(a, max_blocks, s, tipvec);
        else if constexpr (k64()) return launch_prot_exact64_t<kSum(), kTips()>(a, max_blocks, s, tipvec);
        else return launch_prot_t<float, kFma(), kSum(), kTips()>(a, max_blocks, s, tipvec);
      },
      bools{dtype == 1}, bools{fma}, bools{a.scaler_sum != nullptr}, among<0, 1>{tips});
}

hipError_t launch_plf_dna_f32(const DnaArgs &a, int max_blocks, hipStream_t s) {
  return dispatch([&](auto kSum) { return launch_cat<float, kSum()>(a, max_blocks, s); },
                  bools{a.scaler_sum != nullptr});
}

hipError_t launch_plf_dna_f64(const DnaArgs &a, int max_blocks, hipStream_t s) {
  return dispatch([&](auto kSum) { return launch_pair<kSum()>(a, max_blocks, s); },
                  bools{a.scaler_sum != nullptr});
}

hipError_t launch_plf_dna_batch(int dtype, const NodeDescH *nodes, int count, const void *EV,
                                const int32_t *wgt, int64_t n, unsigned long long *ws,
                                int max_blocks, hipStream_t s, int tips, const void *tipvec,
                                int share) {
  if (count < 1 || count > kMaxBatch || tips < 0 || tips > 2) return hipErrorInvalidValue;
  const auto p = pack<dev::NodeBatch>(nodes, count, node_sum);
  return dispatch(
      [&](auto k64, auto kSum, auto kTips) {
        return launch_dna_batch_t<real_t<k64()>, kSum(), kTips()>(p.b, count, EV, wgt, n, ws, max_blocks, s,
                                                                 tipvec, share);
      },
      bools{dtype == 1}, bools{p.any_sum}, among<0, 1, 2>{tips});
}

hipError_t launch_root_lnl(int dtype, int states, const void *x, int64_t n, const double *catw,
                           const double *freq, const int32_t *wgt, const int64_t *scaler_sums,
                           int nsums, double *partials, unsigned long long *ticket, double *out,
                           double *site_lnl, hipStream_t s) {
  return dispatch(
      [&](auto kStates, auto kDtype) {
        using T = real_t<kDtype() == 1>;
        if constexpr (kStates() == 4)
          return launch_lnl_t<T, 4, 4>((const T *)x, n, catw, freq, wgt, scaler_sums, nsums, partials, ticket,
                                       out, site_lnl, s);
        else
          return launch_lnl_prot_t<T>((const T *)x, n, catw, freq, wgt, scaler_sums, nsums, partials, ticket,
                                      out, site_lnl, s);
      },
      among<4, 20>{states}, among<0, 1>{dtype});
}

hipError_t launch_scaler_sum(const uint8_t *scaler, const int32_t *wgt, int64_t n, int64_t *out,
                             unsigned long long *ws, int max_blocks, hipStream_t s) {
  int64_t blocks = (n + kBlock - 1) / kBlock;
  const int64_t cap = max_blocks > 0 ? max_blocks : 2048;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return launch(dev::scaler_sum_kernel, dim3((unsigned)blocks), kBlock, s, scaler, wgt, n, ws, out);
}

hipError_t launch_pmatrix(int dtype, bool eigen_conv, const double *eigen, int S,
                          const double *rates, int ncat, const double *blen, int64_t nbranch,
                          void *out, hipStream_t s) {
  const int64_t total = nbranch * ncat * S * S;
  int64_t blocks = (total + kBlock - 1) / kBlock;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  return dispatch(
      [&](auto k64, auto kConv) {
        using T = real_t<k64()>;
        return launch(&dev::pmatrix_kernel<T, kConv()>, dim3((unsigned)blocks), kBlock, s, eigen, S, rates, ncat,
                      blen, nbranch, (T *)out);
      },
      bools{dtype == 1}, bools{eigen_conv});
}

}  // namespace plfx
