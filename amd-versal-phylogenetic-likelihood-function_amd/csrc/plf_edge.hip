// plf_edge.hip -- launchers of the edge kernels (plf_edge.hpp: the sum table
// and the derivatives of one branch between two fixed CLVs, plfx.h section 10).
//
// Built into a library of its own, plfx/libplfx_edge.so, which libplfx.so
// links: libplfx.so's three gfx950 code objects hold the node, traversal and
// root-lnL kernels that the PMC records and the pinned kernel list
// (tests/golden/kernel_symbols.txt) are tied to, and stay as they are; the
// edge kernels are a separate code object loaded with it.  The C ABI
// (plfx_edge_*) is in plfx_api.hip like every other entry point.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#define PLFX_SECONDARY_TU  // plf_dna.hpp's non-template kernel lives in plf_kernels.hip
#include "plf_edge.hpp"
#include "plf_kernels.hpp"
#include "plf_launch.hpp"

namespace plfx {
namespace {

using dev::kBlock;
using dev::kWavesPerBlock;
static_assert(kBlockThreads == kBlock, "block size mismatch");
using bools = among<false, true>;

// Edge sum table: an HBM stream (two reads, one write; one read with a coded
// side), 4 x 16-B chunks per thread and trip, the co-resident grid.
template <typename T, int S, bool kTip>
hipError_t launch_edge_sumtable_t(const void *x1, const void *x2, int64_t n, const void *tipvec, void *out,
                                  int max_blocks, hipStream_t s) {
  static int cache = 0;
  auto kernel = &dev::edge_sumtable_kernel<T, S, kTip>;
  constexpr int kSitesPerTrip = kBlock * 4 / (4 * S * (int)sizeof(T) / 16);  // rounded down
  const int64_t gx = grid_x((const void *)kernel, cache, n, kSitesPerTrip, 1, max_blocks);
  return launch(kernel, dim3((unsigned)gx), kBlock, s, x1, (const T *)x2, n, (const T *)tipvec, (T *)out);
}

// Edge derivatives: the grids of the root-lnL kernels they are modelled on
// (launch_lnl_t, launch_lnl_prot_t), under the context's grid cap.
// (edge_deriv_grid: also the one-edge grid of the device loop below, whose
// sums then have the derivative kernels' slots and order.)
template <typename T>
int64_t edge_deriv_grid(int states, int64_t n, int max_blocks) {
  static int cache4 = 0, cache20 = 0;
  if (states == 4) {
    auto kernel = &dev::edge_deriv_kernel<T, 4, 4>;
    int64_t gx = grid_x((const void *)kernel, cache4, n, kWavesPerBlock * 64, 1, max_blocks);
    if (max_blocks <= 0) gx = std::min<int64_t>(gx, 2 * (int64_t)cu_count());
    return lnl_cap(gx);
  }
  auto kernel = &dev::edge_deriv_prot_kernel<T>;
  return lnl_cap(grid_x((const void *)kernel, cache20, n, 64, 1, max_blocks));
}

template <typename T>
hipError_t launch_edge_deriv_t(int states, const T *st, int64_t n, const double *lambda, const double *rates,
                               const double *catw, const int32_t *wgt, const double *t, const int64_t *sums,
                               int nsums, double *partials, unsigned long long *ticket, double *out,
                               double *site_lnl, int max_blocks, hipStream_t s) {
  const int64_t gx = edge_deriv_grid<T>(states, n, max_blocks);
  if (states == 4)
    return launch(&dev::edge_deriv_kernel<T, 4, 4>, dim3((unsigned)gx), kBlock, s, st, n, lambda, rates, catw,
                  wgt, t, sums, nsums, partials, ticket, out, site_lnl);
  return launch(&dev::edge_deriv_prot_kernel<T>, dim3((unsigned)gx), kBlock, s, st, n, lambda, rates, catw, wgt,
                t, sums, nsums, partials, ticket, out, site_lnl);
}

// The device loop (edge_opt_loop) of edge_opt_kernel.
template <typename T, int S>
hipError_t launch_edge_opt_t(const void *const *tabs, int count, int64_t n, const double *lambda,
                             const double *rates, const double *catw, const int32_t *wgt, const double *t0,
                             double tmin, double tmax, int max_evals, void *state, double *partials,
                             unsigned long long *ws, double *t_opt, double *out3, int32_t *evals,
                             int max_blocks, hipStream_t s) {
  static_assert(dev::kMaxBatch == kMaxBatch && dev::kWsWords == kWsWords, "batch constants");
  return edge_opt_loop<dev::EdgeOptTabs>(
      tabs, count, max_evals, edge_deriv_grid<T>(S, n, max_blocks),
      [&](dim3 grid, const dev::EdgeOptTabs &a, int first) {
        return launch(&dev::edge_opt_kernel<T, S>, grid, kBlock, s, a, n, lambda, rates, catw, wgt, t0, tmin, tmax,
                      max_evals, first, static_cast<EdgeNewtonStep *>(state), partials, ws, t_opt, out3, evals);
      });
}

}  // namespace

hipError_t launch_edge_sumtable(int dtype, int states, bool tip, const void *x1, const void *x2, int64_t n,
                                const void *tipvec, void *sumtab, int max_blocks, hipStream_t s) {
  return dispatch(
      [&](auto kStates, auto k64, auto kTip) {
        return launch_edge_sumtable_t<real_t<k64()>, kStates(), kTip()>(x1, x2, n, tipvec, sumtab, max_blocks, s);
      },
      among<4, 20>{states}, bools{dtype == 1}, bools{tip});
}

hipError_t launch_edge_derivatives(int dtype, int states, const void *sumtab, int64_t n, const double *lambda,
                                   const double *rates, const double *catw, const int32_t *wgt,
                                   const double *t, const int64_t *scaler_sums, int nsums, double *partials,
                                   unsigned long long *ticket, double *out3, double *site_lnl,
                                   int max_blocks, hipStream_t s) {
  if (states != 4 && states != 20) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64) {
        using T = real_t<k64()>;
        return launch_edge_deriv_t<T>(states, (const T *)sumtab, n, lambda, rates, catw, wgt, t, scaler_sums,
                                      nsums, partials, ticket, out3, site_lnl, max_blocks, s);
      },
      bools{dtype == 1});
}

hipError_t launch_edge_optimize(int dtype, int states, const void *const *sumtabs, int count, int64_t n,
                                const double *lambda, const double *rates, const double *catw,
                                const int32_t *wgt, const double *t0, double tmin, double tmax, int max_evals,
                                void *state, double *partials, unsigned long long *ws, double *t_opt,
                                double *out3, int32_t *evals, int max_blocks, hipStream_t s) {
  if (count < 1 || count > kMaxBatch) return hipErrorInvalidValue;
  return dispatch(
      [&](auto kStates, auto k64) {
        return launch_edge_opt_t<real_t<k64()>, kStates()>(sumtabs, count, n, lambda, rates, catw, wgt, t0, tmin,
                                                           tmax, max_evals, state, partials, ws, t_opt, out3,
                                                           evals, max_blocks, s);
      },
      among<4, 20>{states}, bools{dtype == 1});
}

}  // namespace plfx
