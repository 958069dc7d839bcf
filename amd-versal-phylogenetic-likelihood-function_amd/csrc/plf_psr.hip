// plf_psr.hip -- launchers of the per-site-rate kernels (plf_psr.hpp: the DNA
// node, the root lnL, the sum table -- one and batched --, the edge sums and
// the branch-length loop on the device, with one rate category per site,
// plfx.h section 11).
//
// Built into a library of its own, plfx/libplfx_psr.so, which libplfx.so
// links, as plf_edge.hip is: libplfx.so's code objects and the pinned kernel
// list (tests/golden/kernel_symbols.txt) stay as they are.  The C ABI
// (plfx_*_psr*) is in plfx_api.hip like every other entry point.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#define PLFX_SECONDARY_TU  // plf_dna.hpp's non-template kernel lives in plf_kernels.hip
#include "plf_psr.hpp"
#include "plf_kernels.hpp"
#include "plf_launch.hpp"

namespace plfx {
namespace {

using dev::kBlock;
static_assert(kBlockThreads == kBlock, "block size mismatch");
static_assert(dev::kMaxBatch == kMaxBatch && dev::kWsWords == kWsWords, "batch constants");
using bools = among<false, true>;

// sites per lane and trip: 128 B (f64) / 64 B (f32) of child loads in flight per lane
template <typename T>
constexpr int kNodeU = sizeof(T) == 8 ? 2 : 4;
constexpr int kStreamU = 4;  // root lnL, edge sums: one 32-B / 16-B load per site
constexpr int kScanU = 2;    // rate scan: candidates of a site per trip, their loads issued together

// The node is an HBM stream: the share of the co-resident blocks its node
// count leaves each node (grid_x), node = blockIdx.y.
template <typename T, bool T1, bool T2>
hipError_t launch_plf_psr_t(const NodeDescH *nodes, int count, const void *EV, const uint8_t *rate_cat, int ncat,
                            const int32_t *wgt, int64_t n, const void *tipvec, unsigned long long *ws,
                            int max_blocks, hipStream_t s) {
  constexpr int U = kNodeU<T>;
  const auto p = pack<dev::NodeBatch>(nodes, count, [](const NodeDescH &d) { return d.scaler_sum != nullptr; });
  static int cache[2] = {0, 0};
  auto go = [&](auto kSum) {
    auto kernel = &dev::plf_psr_kernel<T, U, kSum(), T1, T2>;
    const int64_t gx = grid_x((const void *)kernel, cache[kSum() ? 1 : 0], n, kBlock * U, count, max_blocks);
    return launch(kernel, dim3((unsigned)gx, (unsigned)count), kBlock, s, p.b, (const T *)EV, rate_cat, ncat, wgt,
                  n, ws, (const T *)tipvec);
  };
  return p.any_sum ? go(std::true_type{}) : go(std::false_type{});
}

// Fused level pairs: a triple's share of the co-resident blocks, triple =
// blockIdx.y, the node kernel's sites per lane and trip.
template <typename T, int kTips>
hipError_t launch_plf_psr_triples_t(const TripleDescH *t, int count, const void *EV, const uint8_t *rate_cat,
                                    int ncat, const int32_t *wgt, int64_t n, const void *tipvec,
                                    unsigned long long *ws, int max_blocks, hipStream_t s) {
  constexpr int U = kNodeU<T>;
  static_assert(dev::PsrTripleLds<T, kTips>::kValues * sizeof(T) <= 160 * 1024, "LDS of a gfx950 workgroup");
  const auto p = pack<dev::TripleBatch>(t, count, [](const TripleDescH &d) { return d.ssa || d.ssb || d.ssp; });
  static int cache[2] = {0, 0};
  auto go = [&](auto kSum) {
    auto kernel = &dev::plf_psr_triple_kernel<T, U, kSum(), kTips>;
    const int64_t gx = grid_x((const void *)kernel, cache[kSum() ? 1 : 0], n, kBlock * U, count, max_blocks);
    return launch(kernel, dim3((unsigned)gx, (unsigned)count), kBlock, s, p.b, (const T *)EV, rate_cat, ncat, wgt,
                  n, ws, (const T *)tipvec);
  };
  return p.any_sum ? go(std::true_type{}) : go(std::false_type{});
}

template <typename K>
int64_t lnl_grid(K kernel, int &cache, int64_t n, int max_blocks) {
  return lnl_cap(grid_x((const void *)kernel, cache, n, kBlock * kStreamU, 1, max_blocks));
}

// The grid of the edge sums, from edge_deriv_psr_kernel's occupancy: also the
// one-edge grid of the device loop, whose sums then have that kernel's slots
// and order.
template <typename T>
int64_t edge_deriv_psr_grid(int64_t n, int max_blocks) {
  static int cache = 0;
  return lnl_grid(&dev::edge_deriv_psr_kernel<T, kStreamU>, cache, n, max_blocks);
}

// the chunks of 4 x 16 B per thread a block of the sum-table kernels covers per trip, in sites
template <typename T>
constexpr int kSumtabSitesPerTrip = kBlock * 4 / (4 * (int)sizeof(T) / 16);

}  // namespace

hipError_t launch_plf_psr(int dtype, int tips, const NodeDescH *nodes, int count, const void *EV,
                          const uint8_t *rate_cat, int ncat, const int32_t *wgt, int64_t n, const void *tipvec,
                          unsigned long long *ws, int max_blocks, hipStream_t s) {
  if (count < 1 || count > kMaxBatch || ncat < 1 || ncat > dev::kPsrMaxCats || n < 1) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64, auto kT1, auto kT2) {
        return launch_plf_psr_t<real_t<k64()>, kT1(), kT2()>(nodes, count, EV, rate_cat, ncat, wgt, n, tipvec, ws,
                                                            max_blocks, s);
      },
      bools{dtype == 1}, bools{(tips & 1) != 0}, bools{(tips & 2) != 0});
}

hipError_t launch_plf_psr_triples(int dtype, int tips, const TripleDescH *t, int count, const void *EV,
                                  const uint8_t *rate_cat, int ncat, const int32_t *wgt, int64_t n,
                                  const void *tipvec, unsigned long long *ws, int max_blocks, hipStream_t s) {
  static_assert(dev::kMaxTriples == kMaxTriples, "triple batch size");
  if (count < 1 || count > kMaxTriples || ncat < 1 || ncat > dev::kPsrMaxCats || n < 1) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64, auto kTips) {
        return launch_plf_psr_triples_t<real_t<k64()>, kTips()>(t, count, EV, rate_cat, ncat, wgt, n, tipvec, ws,
                                                                max_blocks, s);
      },
      bools{dtype == 1}, among<0, 1, 2>{tips});
}

hipError_t launch_root_lnl_psr(int dtype, const void *x, int64_t n, const double *freq, const int32_t *wgt,
                               const int64_t *scaler_sums, int nsums, double *partials,
                               unsigned long long *ticket, double *out, double *site_lnl, int max_blocks,
                               hipStream_t s) {
  return dispatch(
      [&](auto k64) {
        using T = real_t<k64()>;
        static int cache = 0;
        auto kernel = &dev::root_lnl_psr_kernel<T, kStreamU>;
        const int64_t gx = lnl_grid(kernel, cache, n, max_blocks);
        return launch(kernel, dim3((unsigned)gx), kBlock, s, (const T *)x, n, freq, wgt, scaler_sums, nsums,
                      partials, ticket, out, site_lnl);
      },
      bools{dtype == 1});
}

hipError_t launch_edge_sumtable_psr(int dtype, bool tip, const void *x1, const void *x2, int64_t n,
                                    const void *tipvec, void *sumtab, int max_blocks, hipStream_t s) {
  return dispatch(
      [&](auto k64, auto kTip) {
        using T = real_t<k64()>;
        static int cache = 0;
        auto kernel = &dev::edge_sumtable_psr_kernel<T, kTip()>;
        const int64_t gx = grid_x((const void *)kernel, cache, n, kSumtabSitesPerTrip<T>, 1, max_blocks);
        return launch(kernel, dim3((unsigned)gx), kBlock, s, x1, (const T *)x2, n, (const T *)tipvec, (T *)sumtab);
      },
      bools{dtype == 1}, bools{tip});
}

hipError_t launch_edge_sumtable_psr_batch(int dtype, bool tip, const PsrEdgeDescH *edges, int count, int64_t n,
                                          const void *tipvec, int max_blocks, hipStream_t s) {
  if (count < 1 || count > kMaxBatch || n < 1) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64, auto kTip) {
        using T = real_t<k64()>;
        static int cache = 0;
        auto kernel = &dev::edge_sumtable_psr_batch_kernel<T, kTip()>;
        const auto p = pack<dev::PsrEdgeBatch>(edges, count, [](const PsrEdgeDescH &) { return false; });
        // an edge's share of the co-resident blocks, as a node's in launch_plf_psr_t
        const int64_t gx = grid_x((const void *)kernel, cache, n, kSumtabSitesPerTrip<T>, count, max_blocks);
        return launch(kernel, dim3((unsigned)gx, (unsigned)count), kBlock, s, p.b, n, (const T *)tipvec);
      },
      bools{dtype == 1}, bools{tip});
}

hipError_t launch_edge_derivatives_psr(int dtype, const void *sumtab, int64_t n, const double *lambda,
                                       const double *rates, int ncat, const uint8_t *rate_cat,
                                       const int32_t *wgt, const double *t, const int64_t *scaler_sums, int nsums,
                                       double *partials, unsigned long long *ticket, double *out3,
                                       double *site_lnl, int max_blocks, hipStream_t s) {
  if (ncat < 1 || ncat > dev::kPsrMaxCats) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64) {
        using T = real_t<k64()>;
        const int64_t gx = edge_deriv_psr_grid<T>(n, max_blocks);
        return launch(&dev::edge_deriv_psr_kernel<T, kStreamU>, dim3((unsigned)gx), kBlock, s, (const T *)sumtab, n,
                      lambda, rates, ncat, rate_cat, wgt, t, scaler_sums, nsums, partials, ticket, out3, site_lnl);
      },
      bools{dtype == 1});
}

// The device loop (edge_opt_loop) of edge_opt_psr_kernel.
hipError_t launch_edge_optimize_psr(int dtype, const void *const *sumtabs, int count, int64_t n,
                                    const double *lambda, const double *rates, int ncat,
                                    const uint8_t *rate_cat, const int32_t *wgt, const double *t0, double tmin,
                                    double tmax, int max_evals, void *state, double *partials,
                                    unsigned long long *ws, double *t_opt, double *out3, int32_t *evals,
                                    int max_blocks, hipStream_t s) {
  if (count < 1 || count > kMaxBatch || ncat < 1 || ncat > dev::kPsrMaxCats) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64) {
        using T = real_t<k64()>;
        return edge_opt_loop<dev::EdgeOptTabs>(
            sumtabs, count, max_evals, edge_deriv_psr_grid<T>(n, max_blocks),
            [&](dim3 grid, const dev::EdgeOptTabs &a, int first) {
              return launch(&dev::edge_opt_psr_kernel<T, kStreamU>, grid, kBlock, s, a, n, lambda, rates, ncat,
                            rate_cat, wgt, t0, tmin, tmax, max_evals, first, static_cast<EdgeNewtonStep *>(state),
                            partials, ws, t_opt, out3, evals);
            });
      },
      bools{dtype == 1});
}

// ---- plfx.h section 12 ----

// One block per kBlock sites, capped at the co-resident blocks and at the
// partial slots of lnl_finish.
hipError_t launch_psr_site_lnl(int dtype, const void *x, int64_t n, const double *freq, const uint8_t *scalers,
                               int nsc, int64_t stride, double *site_lnl, int max_blocks, hipStream_t s) {
  if (n < 1) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64) {
        using T = real_t<k64()>;
        static int cache = 0;
        auto kernel = &dev::psr_site_lnl_kernel<T, false, 1>;
        const int64_t gx = grid_x((const void *)kernel, cache, n, kBlock, 1, max_blocks);
        return launch(kernel, dim3((unsigned)gx), kBlock, s, (const T *)x, n, 1, freq, scalers, nsc, stride, 0, 1,
                      site_lnl, (double *)nullptr, (int32_t *)nullptr, (const int32_t *)nullptr, (double *)nullptr,
                      (unsigned long long *)nullptr, (double *)nullptr);
      },
      bools{dtype == 1});
}

hipError_t launch_psr_scan_pass(int dtype, const void *x, int64_t n, int gc, const double *freq,
                                const uint8_t *scalers, int nsc, int64_t stride, int k0, bool first,
                                double *all_lnl, double *best_lnl, int32_t *best_idx, const int32_t *wgt,
                                double *partials, unsigned long long *ticket, double *out, int max_blocks,
                                hipStream_t s) {
  if (n < 1 || gc < 1) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64) {
        using T = real_t<k64()>;
        static int cache = 0;
        auto kernel = &dev::psr_site_lnl_kernel<T, true, kScanU>;
        const int64_t gx = lnl_cap(grid_x((const void *)kernel, cache, n, kBlock, 1, max_blocks));
        return launch(kernel, dim3((unsigned)gx), kBlock, s, (const T *)x, n, gc, freq, scalers, nsc, stride, k0,
                      (int)first, all_lnl, best_lnl, best_idx, wgt, partials, ticket, out);
      },
      bools{dtype == 1});
}

hipError_t launch_psr_tile(const PsrTileDescH *tips, int count, int64_t n, int group, uint8_t *cat, int max_blocks,
                           hipStream_t s) {
  if (count < 0 || count > kMaxBatch || (count == 0 && !cat) || n < 1 || group < 1) return hipErrorInvalidValue;
  static int cache = 0;
  const auto p = pack<dev::PsrTileBatch>(tips, count, [](const PsrTileDescH &) { return false; });
  const int rows = count + (cat ? 1 : 0);
  const int64_t gx = grid_x((const void *)&dev::psr_tile_kernel, cache, (int64_t)group * n, kBlock, rows, max_blocks);
  return launch(&dev::psr_tile_kernel, dim3((unsigned)gx, (unsigned)rows), kBlock, s, p.b, count, n, group, cat);
}

}  // namespace plfx
