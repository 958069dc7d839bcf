// plf_psr_prot.hip -- launchers of the protein per-site-rate kernels
// (plf_psr_prot.hpp: the node and the root lnL with one rate category per site
// and 20 states, plfx.h section 11b; the sum table -- one and batched --, the
// edge sums and the branch-length loop on the device, section 11c; the rate
// scan's per-site lnL and argmax, section 12b).
//
// Built into a library of its own, plfx/libplfx_psr_prot.so, which libplfx.so
// links, as plf_psr.hip and plf_edge.hip are: the code objects of the other
// three libraries and the pinned kernel list
// (tests/golden/kernel_symbols.txt) stay as they are.  The C ABI
// (plfx_*_psr_gen) is in plfx_api.hip like every other entry point.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "plf_psr_prot.hpp"
#include "plf_kernels.hpp"
#include "plf_launch.hpp"

namespace plfx {
namespace {

using dev::kBlock;
static_assert(kBlockThreads == kBlock, "block size mismatch");
static_assert(dev::kMaxBatch == kMaxBatch && dev::kWsWords == kWsWords, "batch constants");
using bools = among<false, true>;

// A block's four waves own 64 sites each per trip; the grid is a node's share
// of the co-resident blocks (grid_x), node = blockIdx.y, as the DNA PSR node's.
template <typename T, bool T1, bool T2>
hipError_t launch_plf_psr_prot_t(const NodeDescH *nodes, int count, const void *EV, const uint8_t *rate_cat,
                                 int ncat, const int32_t *wgt, int64_t n, const void *tipvec,
                                 unsigned long long *ws, int max_blocks, hipStream_t s) {
  static_assert((dev::kWavesPerBlock * dev::PsrProtTile<T>::kChunks + dev::PsrProtTile<T>::kTabChunks) * 16 <=
                    64 * 1024,
                "static LDS of a workgroup");
  const auto p = pack<dev::NodeBatch>(nodes, count, [](const NodeDescH &d) { return d.scaler_sum != nullptr; });
  static int cache[2] = {0, 0};
  auto go = [&](auto kSum) {
    auto kernel = &dev::plf_psr_prot_kernel<T, kSum(), T1, T2>;
    const int64_t gx = grid_x((const void *)kernel, cache[kSum() ? 1 : 0], n, kBlock, count, max_blocks);
    return launch(kernel, dim3((unsigned)gx, (unsigned)count), kBlock, s, p.b, (const T *)EV, rate_cat, ncat, wgt,
                  n, ws, (const T *)tipvec);
  };
  return p.any_sum ? go(std::true_type{}) : go(std::false_type{});
}

// The grid of the edge sums, from edge_deriv_psr_prot_kernel's occupancy: one
// site per lane and trip, capped at the partial slots of lnl_finish.  Also the
// one-edge grid of the device loop, whose sums then have that kernel's slots
// and order.
template <typename T>
int64_t edge_deriv_psr_prot_grid(int64_t n, int max_blocks) {
  static int cache = 0;
  return lnl_cap(grid_x((const void *)&dev::edge_deriv_psr_prot_kernel<T>, cache, n, kBlock, 1, max_blocks));
}

// 16-B chunks of a table of n sites, and those a block of the sum-table kernels covers per trip
template <typename T>
int64_t sumtab_chunks(int64_t n) {
  return n * dev::PsrProtTile<T>::kChunksPerSite;
}
constexpr int kSumtabChunksPerTrip = kBlock * 4;

}  // namespace

hipError_t launch_plf_psr_prot(int dtype, int tips, const NodeDescH *nodes, int count, const void *EV,
                               const uint8_t *rate_cat, int ncat, const int32_t *wgt, int64_t n,
                               const void *tipvec, unsigned long long *ws, int max_blocks, hipStream_t s) {
  if (count < 1 || count > kMaxBatch || ncat < 1 || ncat > dev::kPsrProtMaxCats || n < 1)
    return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64, auto kT1, auto kT2) {
        return launch_plf_psr_prot_t<real_t<k64()>, kT1(), kT2()>(nodes, count, EV, rate_cat, ncat, wgt, n, tipvec,
                                                                 ws, max_blocks, s);
      },
      bools{dtype == 1}, bools{(tips & 1) != 0}, bools{(tips & 2) != 0});
}

hipError_t launch_root_lnl_psr_prot(int dtype, const void *x, int64_t n, const double *freq, const int32_t *wgt,
                                    const int64_t *scaler_sums, int nsums, double *partials,
                                    unsigned long long *ticket, double *out, double *site_lnl, int max_blocks,
                                    hipStream_t s) {
  return dispatch(
      [&](auto k64) {
        using T = real_t<k64()>;
        static int cache = 0;
        auto kernel = &dev::root_lnl_psr_prot_kernel<T>;
        const int64_t gx = lnl_cap(grid_x((const void *)kernel, cache, n, kBlock, 1, max_blocks));
        return launch(kernel, dim3((unsigned)gx), kBlock, s, (const T *)x, n, freq, wgt, scaler_sums, nsums,
                      partials, ticket, out, site_lnl);
      },
      bools{dtype == 1});
}

hipError_t launch_edge_sumtable_psr_prot(int dtype, bool tip, const void *x1, const void *x2, int64_t n,
                                         const void *tipvec, void *sumtab, int max_blocks, hipStream_t s) {
  if (n < 1) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64, auto kTip) {
        using T = real_t<k64()>;
        static int cache = 0;
        auto kernel = &dev::edge_sumtable_psr_prot_kernel<T, kTip()>;
        const int64_t gx = grid_x((const void *)kernel, cache, sumtab_chunks<T>(n), kSumtabChunksPerTrip, 1, max_blocks);
        return launch(kernel, dim3((unsigned)gx), kBlock, s, x1, (const T *)x2, n, (const T *)tipvec, (T *)sumtab);
      },
      bools{dtype == 1}, bools{tip});
}

hipError_t launch_edge_sumtable_psr_prot_batch(int dtype, bool tip, const PsrEdgeDescH *edges, int count, int64_t n,
                                               const void *tipvec, int max_blocks, hipStream_t s) {
  if (count < 1 || count > kMaxBatch || n < 1) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64, auto kTip) {
        using T = real_t<k64()>;
        static int cache = 0;
        auto kernel = &dev::edge_sumtable_psr_prot_batch_kernel<T, kTip()>;
        const auto p = pack<dev::PsrProtEdgeBatch>(edges, count, [](const PsrEdgeDescH &) { return false; });
        // an edge's share of the co-resident blocks, as a node's in launch_plf_psr_prot_t
        const int64_t gx =
            grid_x((const void *)kernel, cache, sumtab_chunks<T>(n), kSumtabChunksPerTrip, count, max_blocks);
        return launch(kernel, dim3((unsigned)gx, (unsigned)count), kBlock, s, p.b, n, (const T *)tipvec);
      },
      bools{dtype == 1}, bools{tip});
}

hipError_t launch_edge_derivatives_psr_prot(int dtype, const void *sumtab, int64_t n, const double *lambda,
                                            const double *rates, int ncat, const uint8_t *rate_cat,
                                            const int32_t *wgt, const double *t, const int64_t *scaler_sums,
                                            int nsums, double *partials, unsigned long long *ticket, double *out3,
                                            double *site_lnl, int max_blocks, hipStream_t s) {
  if (ncat < 1 || ncat > dev::kPsrProtMaxCats) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64) {
        using T = real_t<k64()>;
        const int64_t gx = edge_deriv_psr_prot_grid<T>(n, max_blocks);
        return launch(&dev::edge_deriv_psr_prot_kernel<T>, dim3((unsigned)gx), kBlock, s, (const T *)sumtab, n, lambda,
                      rates, ncat, rate_cat, wgt, t, scaler_sums, nsums, partials, ticket, out3, site_lnl);
      },
      bools{dtype == 1});
}

// The device loop (edge_opt_loop) of edge_opt_psr_prot_kernel.
hipError_t launch_edge_optimize_psr_prot(int dtype, const void *const *sumtabs, int count, int64_t n,
                                         const double *lambda, const double *rates, int ncat,
                                         const uint8_t *rate_cat, const int32_t *wgt, const double *t0, double tmin,
                                         double tmax, int max_evals, void *state, double *partials,
                                         unsigned long long *ws, double *t_opt, double *out3, int32_t *evals,
                                         int max_blocks, hipStream_t s) {
  if (count < 1 || count > kMaxBatch || ncat < 1 || ncat > dev::kPsrProtMaxCats) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64) {
        using T = real_t<k64()>;
        return edge_opt_loop<dev::EdgeOptTabs>(
            sumtabs, count, max_evals, edge_deriv_psr_prot_grid<T>(n, max_blocks),
            [&](dim3 grid, const dev::EdgeOptTabs &a, int first) {
              return launch(&dev::edge_opt_psr_prot_kernel<T>, grid, kBlock, s, a, n, lambda, rates, ncat, rate_cat,
                            wgt, t0, tmin, tmax, max_evals, first, static_cast<EdgeNewtonStep *>(state), partials, ws,
                            t_opt, out3, evals);
            });
      },
      bools{dtype == 1});
}

// ---- plfx.h section 12b ----

// launch_psr_site_lnl and launch_psr_scan_pass (plf_psr.hip) for rows of 20
// values: one block per kBlock sites, capped at the co-resident blocks and,
// for the pass that sums, at the partial slots of lnl_finish.
hipError_t launch_psr_site_lnl_prot(int dtype, const void *x, int64_t n, const double *freq, const uint8_t *scalers,
                                    int nsc, int64_t stride, double *site_lnl, int max_blocks, hipStream_t s) {
  if (n < 1) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64) {
        using T = real_t<k64()>;
        static int cache = 0;
        auto kernel = &dev::psr_site_lnl_prot_kernel<T, false>;
        const int64_t gx = grid_x((const void *)kernel, cache, n, kBlock, 1, max_blocks);
        return launch(kernel, dim3((unsigned)gx), kBlock, s, (const T *)x, n, 1, freq, scalers, nsc, stride, 0, 1,
                      site_lnl, (double *)nullptr, (int32_t *)nullptr, (const int32_t *)nullptr, (double *)nullptr,
                      (unsigned long long *)nullptr, (double *)nullptr);
      },
      bools{dtype == 1});
}

hipError_t launch_psr_scan_pass_prot(int dtype, const void *x, int64_t n, int gc, const double *freq,
                                     const uint8_t *scalers, int nsc, int64_t stride, int k0, bool first,
                                     double *all_lnl, double *best_lnl, int32_t *best_idx, const int32_t *wgt,
                                     double *partials, unsigned long long *ticket, double *out, int max_blocks,
                                     hipStream_t s) {
  if (n < 1 || gc < 1) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64) {
        using T = real_t<k64()>;
        static int cache = 0;
        auto kernel = &dev::psr_site_lnl_prot_kernel<T, true>;
        const int64_t gx = lnl_cap(grid_x((const void *)kernel, cache, n, kBlock, 1, max_blocks));
        return launch(kernel, dim3((unsigned)gx), kBlock, s, (const T *)x, n, gc, freq, scalers, nsc, stride, k0,
                      (int)first, all_lnl, best_lnl, best_idx, wgt, partials, ticket, out);
      },
      bools{dtype == 1});
}

}  // namespace plfx
