// plf_psr_branch.hip -- launchers of the all-branch kernels of plfx.h section
// 13 (plf_psr_branch.hpp: the fused sibling pair and the counters' pass).
//
// Built into a library of its own, plfx/libplfx_psr_branch.so, which
// libplfx.so links, as plf_psr.hip is: libplfx.so's code objects and the pinned
// kernel list (tests/golden/kernel_symbols.txt) stay as they are.  The C ABI
// (plfx_branch_sumtables_psr) is in plfx_api.hip like every other entry point.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#define PLFX_SECONDARY_TU  // plf_dna.hpp's non-template kernel lives in plf_kernels.hip
#define PLFX_PSR_NO_TILE_KERNEL  // and plf_psr.hpp's in plf_psr.hip
#include "plf_psr_branch.hpp"
#include "plf_kernels.hpp"
#include "plf_launch.hpp"

namespace plfx {
namespace {

using dev::kBlock;
static_assert(kBlockThreads == kBlock, "block size mismatch");
static_assert(dev::kMaxPairs == kMaxPairs && dev::kScaleChunk == kScaleChunk, "batch constants");
static_assert(sizeof(dev::BranchPairBatch) <= 2048 && sizeof(dev::BranchScaleBatch) <= 3072,
              "descriptors travel in the kernel arguments (4 KB)");
using bools = among<false, true>;

// plf_psr.hip's kNodeU: 128 B (f64) / 64 B (f32) of loads per child in flight per lane
template <typename T>
constexpr int kPairU = sizeof(T) == 8 ? 2 : 4;

template <typename T, int kTips>
hipError_t launch_pairs_t(const BranchPairDescH *pairs, int count, const void *EV, const uint8_t *rate_cat, int ncat,
                          const int32_t *wgt, int64_t n, const void *tipvec, unsigned long long *ws, int max_blocks,
                          hipStream_t s) {
  constexpr int U = kPairU<T>;
  static_assert(dev::PsrBranchLds<T, kTips>::kValues * sizeof(T) <= 64 * 1024, "LDS of a workgroup");
  const auto p = pack<dev::BranchPairBatch>(pairs, count, [](const BranchPairDescH &d) { return d.ss1 || d.ss2; });
  static int cache[2] = {0, 0};
  auto go = [&](auto kSum) {
    auto kernel = &dev::psr_branch_pair_kernel<T, U, kSum(), kTips>;
    const int64_t gx = grid_x((const void *)kernel, cache[kSum() ? 1 : 0], n, kBlock * U, count, max_blocks);
    return launch(kernel, dim3((unsigned)gx, (unsigned)count), kBlock, s, p.b, (const T *)EV, rate_cat, ncat, wgt,
                  n, ws, (const T *)tipvec);
  };
  return p.any_sum ? go(std::true_type{}) : go(std::false_type{});
}

}  // namespace

int psr_branch_sites_per_lane(int dtype) { return dtype == 1 ? kPairU<double> : kPairU<float>; }

hipError_t launch_psr_branch_pairs(int dtype, int tips, const BranchPairDescH *pairs, int count, const void *EV,
                                   const uint8_t *rate_cat, int ncat, const int32_t *wgt, int64_t n,
                                   const void *tipvec, unsigned long long *ws, int max_blocks, hipStream_t s) {
  if (count < 1 || count > kMaxPairs || ncat < 1 || ncat > dev::kPsrMaxCats || n < 1) return hipErrorInvalidValue;
  return dispatch(
      [&](auto k64, auto kTips) {
        return launch_pairs_t<real_t<k64()>, kTips()>(pairs, count, EV, rate_cat, ncat, wgt, n, tipvec, ws,
                                                      max_blocks, s);
      },
      bools{dtype == 1}, among<0, 1, 2>{tips});
}

hipError_t launch_psr_branch_counts(bool outer_pass, const BranchScaleDescH *ops, int first, int count,
                                    const int64_t *scaler_sums, const int64_t *wsum, int64_t *sub, int64_t *outer,
                                    int64_t *edge_scale, hipStream_t s) {
  if (count < 1 || count > kScaleChunk || first < 0) return hipErrorInvalidValue;
  const auto p = pack<dev::BranchScaleBatch>(ops, count, [](const BranchScaleDescH &) { return false; });
  if (!outer_pass)
    return launch(&dev::psr_branch_sub_kernel, dim3(1), kBlock, s, p.b, first, count, scaler_sums, sub);
  return launch(&dev::psr_branch_scale_kernel, dim3(1), kBlock, s, p.b, first, count, wsum, (const int64_t *)sub, outer,
                edge_scale);
}

}  // namespace plfx
