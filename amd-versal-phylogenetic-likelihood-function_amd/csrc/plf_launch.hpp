// plf_launch.hpp -- host-side helpers shared by the launchers of the HIP
// translation units (plf_kernels.hip, plf_prot_valu.hip,
// plf_prot_valu_exact.hip, plf_edge.hip, plf_psr.hip, plf_psr_prot.hip,
// plf_psr_prot_mfma.hip, plf_psr_branch.hip): pick
// a grid, pick a kernel instantiation, launch.
// Internal to libplfx; no device code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "plf_kernels.hpp"

namespace plfx {

// threads of every block but the deep passes' (= dev::kBlock, asserted in plf_kernels.hip;
// no device header here: plf_dna.hpp defines a kernel, for one translation unit only)
constexpr int kBlockThreads = 256;

inline int cu_count() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus < 1) cus = 256;
  }
  return cus;
}

// Co-resident blocks of `threads` threads of `kernel` on the current device
// (occupancy x CUs; fallback_per_cu blocks per CU if the occupancy query
// fails), cached in `cache`: one per kernel instantiation, kept by the caller.
inline int resident_blocks(const void *kernel, int threads, int fallback_per_cu, int &cache) {
  if (!cache) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess || per_cu < 1)
      per_cu = fallback_per_cu;
    cache = per_cu * cu_count();
  }
  return cache;
}

// blocks along x for `count` nodes of n sites each: one block per
// sites_per_block sites, at most max_blocks or, without a cap, the node's share
// of the co-resident blocks
inline int64_t grid_x(const void *kernel, int &cache, int64_t n, int sites_per_block, int count,
                      int max_blocks, int threads = kBlockThreads, int fallback_per_cu = 2) {
  int64_t blocks = (n + sites_per_block - 1) / sites_per_block;
  const int64_t resident = resident_blocks(kernel, threads, fallback_per_cu, cache);
  // floor: count x cap blocks must fit in one wave of resident blocks (a ceil
  // would leave a few blocks for a second, nearly empty wave: +30% on a
  // 10-node batch)
  const int64_t cap = max_blocks > 0 ? max_blocks : std::max<int64_t>(1, resident / count);
  if (blocks > cap) blocks = cap;
  return blocks < 1 ? 1 : blocks;
}

// the grid of a kernel whose blocks each own a slot of the kLnlMaxGrid partial sums
inline int64_t lnl_cap(int64_t gx) { return std::min<int64_t>(gx, kLnlMaxGrid); }

template <typename K, typename... A>
hipError_t launch(K kernel, dim3 grid, int threads, hipStream_t s, const A &...args) {
  hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, s, args...);
  return hipGetLastError();
}

// The branch-length loop on the device: max_evals launches over the group's
// `count` edges (blockIdx.y), the first of which initialises the per-edge
// state.  Tabs: the device's struct of the tables' pointers (no device header
// here); eval(grid, tabs, first) enqueues one launch of the caller's kernel.
// The per-edge grid is the one-edge grid gx1 unless the group's 3 * gx * count
// slots would not fit the 3 * kLnlMaxGrid doubles of the partials.
template <typename Tabs, typename Eval>
hipError_t edge_opt_loop(const void *const *tabs, int count, int max_evals, int64_t gx1, Eval eval) {
  Tabs a{};
  for (int j = 0; j < count; j++) a.st[j] = tabs[j];
  const int64_t gx = std::max<int64_t>(1, std::min<int64_t>(gx1, kLnlMaxGrid / count));
  for (int i = 0; i < max_evals; i++) {
    hipError_t e = eval(dim3((unsigned)gx, (unsigned)count), a, (int)(i == 0));
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// A node kernel over gx blocks: DnaArgs as the kernel's argument list, the
// values as T; tipvec (none, or one const void *) goes last, as T too.
template <typename T, typename K, typename... V>
hipError_t launch_node(K kernel, int64_t gx, hipStream_t s, const DnaArgs &a, V... tipvec) {
  return launch(kernel, dim3((unsigned)gx), kBlockThreads, s, (const T *)a.x1, (const T *)a.x2, (T *)a.x3,
                (const T *)a.EV, (const T *)a.left, (const T *)a.right, a.wgt, a.scaler, a.n, a.ws,
                a.scaler_sum, (const T *)tipvec...);
}

// Run-time values to template arguments: dispatch(f, among<Vs...>{v}, ...)
// calls f(std::integral_constant<., V>{}, ...) with the V equal to each v, or
// returns hipErrorInvalidValue when some v is none of its Vs.  Only the
// combinations f's body names (outside a discarded `if constexpr`) are built.
template <auto... Vs>
struct among {
  std::common_type_t<decltype(Vs)...> v;
};
template <bool k64>
using real_t = std::conditional_t<k64, double, float>;  // among<false, true>{dtype == 1}

template <typename F>
hipError_t dispatch(F &&f) {
  return f();
}
template <typename F, auto... Vs, typename... Rest>
hipError_t dispatch(F &&f, among<Vs...> c, Rest... rest) {
  hipError_t e = hipErrorInvalidValue;
  auto with = [&](auto k) { return dispatch([&](auto... r) { return f(k, r...); }, rest...); };
  (void)((c.v == Vs && ((e = with(std::integral_constant<decltype(Vs), Vs>{})), true)) || ...);
  return e;
}

// The descriptors of one launch in the device's batch struct (same layout,
// asserted), and whether any of them asks for a scaler sum.
template <typename Batch>
struct Packed {
  Batch b;
  bool any_sum;
};
template <typename Batch, typename Desc, typename F>
Packed<Batch> pack(const Desc *descs, int count, F any_sum_of) {
  Packed<Batch> p{};
  static_assert(sizeof(p.b.d[0]) == sizeof(Desc), "layout");
  for (int i = 0; i < count; i++) {
    __builtin_memcpy(&p.b.d[i], &descs[i], sizeof(Desc));
    p.any_sum |= any_sum_of(descs[i]);
  }
  return p;
}

}  // namespace plfx
