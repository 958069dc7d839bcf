// plf_psr_prot_mfma.hip -- launcher of the protein per-site-rate node in FMA
// mode on the f64 matrix cores (plf_psr_prot_mfma.hpp, plfx.h section 11d).
//
// Built into a library of its own, plfx/libplfx_psr_prot_mfma.so, which
// libplfx.so links, as plf_psr_prot.hip is: the code objects of the other
// libraries and the pinned kernel list (tests/golden/kernel_symbols.txt) stay
// as they are.  The C ABI (plfx_*_psr_ex) is in plfx_api.hip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "plf_psr_prot_mfma.hpp"
#include "plf_kernels.hpp"
#include "plf_launch.hpp"

namespace plfx {
namespace {

using dev::kBlock;
static_assert(kBlockThreads == kBlock, "block size mismatch");
static_assert(dev::kMaxBatch == kMaxBatch && dev::kWsWords == kWsWords, "batch constants");
using bools = among<false, true>;

// The grid is the exact node's (launch_plf_psr_prot_t): a block's four waves
// own 64 sites each per trip, a node's share of the co-resident blocks,
// node = blockIdx.y.
template <bool T1, bool T2>
hipError_t launch_plf_psr_prot_mfma_t(const NodeDescH *nodes, int count, const void *EV, const uint8_t *rate_cat,
                                      int ncat, const int32_t *wgt, int64_t n, const void *tipvec,
                                      unsigned long long *ws, int max_blocks, hipStream_t s) {
  static_assert((dev::kWavesPerBlock * dev::PsrProtTile<double>::kChunks + dev::PsrProtTile<double>::kTabChunks) * 16 <=
                    64 * 1024,
                "static LDS of a workgroup");
  const auto p = pack<dev::NodeBatch>(nodes, count, [](const NodeDescH &d) { return d.scaler_sum != nullptr; });
  static int cache[2] = {0, 0};
  auto go = [&](auto kSum) {
    auto kernel = &dev::plf_psr_prot_mfma_kernel<kSum(), T1, T2>;
    const int64_t gx = grid_x((const void *)kernel, cache[kSum() ? 1 : 0], n, kBlock, count, max_blocks);
    return launch(kernel, dim3((unsigned)gx, (unsigned)count), kBlock, s, p.b, (const double *)EV, rate_cat, ncat,
                  wgt, n, ws, (const double *)tipvec);
  };
  return p.any_sum ? go(std::true_type{}) : go(std::false_type{});
}

}  // namespace

hipError_t launch_plf_psr_prot_mfma(int tips, const NodeDescH *nodes, int count, const void *EV,
                                    const uint8_t *rate_cat, int ncat, const int32_t *wgt, int64_t n,
                                    const void *tipvec, unsigned long long *ws, int max_blocks, hipStream_t s) {
  if (count < 1 || count > kMaxBatch || ncat < 1 || ncat > dev::kPsrProtMaxCats || n < 1)
    return hipErrorInvalidValue;
  return dispatch(
      [&](auto kT1, auto kT2) {
        return launch_plf_psr_prot_mfma_t<kT1(), kT2()>(nodes, count, EV, rate_cat, ncat, wgt, n, tipvec, ws,
                                                        max_blocks, s);
      },
      bools{(tips & 1) != 0}, bools{(tips & 2) != 0});
}

}  // namespace plfx
