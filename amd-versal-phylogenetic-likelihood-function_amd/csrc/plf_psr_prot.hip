// plf_psr_prot.hip -- launchers of the protein per-site-rate kernels
// (plf_psr_prot.hpp: the node and the root lnL with one rate category per site
// and 20 states, plfx.h section 11b).
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
        const int64_t gx =
            std::min<int64_t>(grid_x((const void *)kernel, cache, n, kBlock, 1, max_blocks), kLnlMaxGrid);
        return launch(kernel, dim3((unsigned)gx), kBlock, s, (const T *)x, n, freq, wgt, scaler_sums, nsums,
                      partials, ticket, out, site_lnl);
      },
      bools{dtype == 1});
}

}  // namespace plfx
