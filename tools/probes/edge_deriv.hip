// edge_deriv.hip -- probe (not product code): what bounds the DNA edge-derivative
// kernel (csrc/plf_edge.hpp edge_deriv_kernel) at 2^20 f64 sites?  Times, back
// to back in one process, the product kernel at 2 and 3 blocks per CU and
// copies of it with the quad broadcasts of the three category sums as __shfl
// or as DPP moves, at 2 / 3 / 4 blocks per CU, and without the two divisions
// and the log.  profiles/r07_probe_edge_deriv.log: DPP 27.6 us against 28.9
// with __shfl; dropping the divisions and the log changes nothing (27.5-27.6);
// more blocks per CU are slower (29.4-29.9) -- the per-site arithmetic does not
// bound the kernel, the cross-lane moves cost ~1.3 us, the rest is the stream.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include <algorithm>
#include "plf_edge.hpp"

using namespace plfx::dev;

template <int k>
__device__ __forceinline__ double quad_bcast(double x, int lane, bool dpp) {
  return dpp ? dpp_f64<k * 0x55>(x) : __shfl(x, (lane / 4) * 4 + k);
}

template <bool kDpp, bool kNoDiv, bool kNoLog, int kMinBlocks>
__global__ void __launch_bounds__(kBlock, kMinBlocks)
probe_kernel(const double *__restrict__ st, int64_t n, const double *__restrict__ lambda,
             const double *__restrict__ rates, const double *__restrict__ catw,
             const int32_t *__restrict__ wgt, const double *__restrict__ tp,
             const int64_t *__restrict__ scaler_sums, int nsums, double *partials,
             unsigned long long *ticket, double *out, double *__restrict__ site_lnl) {
  constexpr int S = 4, C = 4, V = 16, SPW = 16;
  const int lane = threadIdx.x & 63;
  const int c = lane % C;
  const int q = lane / C;
  double e0[S], e1[S], e2[S];
  {
    const double t = *tp, r = rates[c];
#pragma unroll
    for (int k = 0; k < S; k++) edge_factors(lambda[k], r, t, e0[k], e1[k], e2[k]);
  }
  double cw[C];
#pragma unroll
  for (int k = 0; k < C; k++) cw[k] = catw ? catw[k] : 1.0 / C;
  double acc[3] = {0.0, 0.0, 0.0};
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock * SPW * C;
  const int64_t nlast = n - 1;
  for (int64_t base = wave * SPW * C; base < n; base += stride) {
    double v[C][S];
#pragma unroll
    for (int u = 0; u < C; u++) {
      const int64_t site = base + u * SPW + q;
      const double *xs = st + (site < n ? site : nlast) * V + c * S;
#pragma unroll
      for (int s = 0; s < S; s += 2) {
        const f64x2 w = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(xs + s));
        v[u][s] = w.x;
        v[u][s + 1] = w.y;
      }
    }
    const int64_t site = base + c * SPW + q;
    const bool valid = site < n;
    const int wv = wgt_at(wgt, valid ? site : nlast, partials);
    __builtin_amdgcn_sched_barrier(0);
    double m0 = 1.0, m1 = 0.0, m2 = 0.0;
#pragma unroll
    for (int u = 0; u < C; u++) {
      double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
      for (int k = 0; k < S; k++) {
        const double x = v[u][k];
        t0 += x * e0[k];
        t1 += x * e1[k];
        t2 += x * e2[k];
      }
      double L0 = 0.0, L1 = 0.0, L2 = 0.0;
      L0 += cw[0] * quad_bcast<0>(t0, lane, kDpp); L1 += cw[0] * quad_bcast<0>(t1, lane, kDpp); L2 += cw[0] * quad_bcast<0>(t2, lane, kDpp);
      L0 += cw[1] * quad_bcast<1>(t0, lane, kDpp); L1 += cw[1] * quad_bcast<1>(t1, lane, kDpp); L2 += cw[1] * quad_bcast<1>(t2, lane, kDpp);
      L0 += cw[2] * quad_bcast<2>(t0, lane, kDpp); L1 += cw[2] * quad_bcast<2>(t1, lane, kDpp); L2 += cw[2] * quad_bcast<2>(t2, lane, kDpp);
      L0 += cw[3] * quad_bcast<3>(t0, lane, kDpp); L1 += cw[3] * quad_bcast<3>(t1, lane, kDpp); L2 += cw[3] * quad_bcast<3>(t2, lane, kDpp);
      if (u == c) { m0 = L0; m1 = L1; m2 = L2; }
    }
    if (valid) {
      const double l = kNoLog ? m0 : log(m0);
      const double r1 = kNoDiv ? m1 : m1 / m0, r2 = kNoDiv ? m2 : m2 / m0;
      acc[0] += (double)wv * l;
      acc[1] += (double)wv * r1;
      acc[2] += (double)wv * (r2 - r1 * r1);
      if (site_lnl) site_lnl[site] = l;
    }
  }
  lnl_finish<3>(acc, partials, ticket, out, scaler_sums, nsums);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
  const int64_t n = 1 << 20;
  std::vector<double> h(n * 16);
  unsigned s = 1;
  for (auto &x : h) { s = s * 1664525u + 1013904223u; x = 0.1 + (s >> 8) * (1.0 / (1 << 24)); }
  double *st, *lam, *rates, *t, *partials, *out;
  unsigned long long *ticket;
  int32_t *wgt;
  CK(hipMalloc(&st, h.size() * 8)); CK(hipMemcpy(st, h.data(), h.size() * 8, hipMemcpyHostToDevice));
  const double hl[4] = {0.0, -0.9, -1.1, -1.4}, hr[4] = {0.03, 0.28, 0.9, 2.8}, ht = 0.2;
  CK(hipMalloc(&lam, 32)); CK(hipMemcpy(lam, hl, 32, hipMemcpyHostToDevice));
  CK(hipMalloc(&rates, 32)); CK(hipMemcpy(rates, hr, 32, hipMemcpyHostToDevice));
  CK(hipMalloc(&t, 8)); CK(hipMemcpy(t, &ht, 8, hipMemcpyHostToDevice));
  CK(hipMalloc(&partials, 3 * 4096 * 8)); CK(hipMalloc(&out, 24));
  CK(hipMalloc(&ticket, 33 * 16 * 8)); CK(hipMemset(ticket, 0, 33 * 16 * 8));
  CK(hipMalloc(&wgt, n * 4));
  std::vector<int32_t> hw(n, 1);
  CK(hipMemcpy(wgt, hw.data(), n * 4, hipMemcpyHostToDevice));
  int cus = 0;
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  hipEvent_t b, f;
  CK(hipEventCreate(&b)); CK(hipEventCreate(&f));
  struct Var { const char *name; void (*k)(const double *, int64_t, const double *, const double *, const double *, const int32_t *, const double *, const int64_t *, int, double *, unsigned long long *, double *, double *); int per_cu; };
  std::vector<Var> vars = {
      {"product kernel 2/CU", edge_deriv_kernel<double, 4, 4>, 2},
      {"product kernel 3/CU", edge_deriv_kernel<double, 4, 4>, 3},
      {"shfl   2/CU", probe_kernel<false, false, false, 1>, 2},
      {"dpp    2/CU", probe_kernel<true, false, false, 1>, 2},
      {"dpp    3/CU", probe_kernel<true, false, false, 1>, 3},
      {"dpp    4/CU (launch bounds 4)", probe_kernel<true, false, false, 4>, 4},
      {"dpp nodiv 2/CU", probe_kernel<true, true, false, 1>, 2},
      {"dpp nodiv nolog 2/CU", probe_kernel<true, true, true, 1>, 2},
      {"shfl nodiv nolog 2/CU", probe_kernel<false, true, true, 1>, 2},
  };
  for (int round = 0; round < 4; round++) {
    for (auto &v : vars) {
      const int grid = (int)std::min<int64_t>((n + 255) / 256, (int64_t)v.per_cu * cus);
      const int calls = 100;
      CK(hipEventRecord(b, 0));
      for (int i = 0; i < calls; i++)
        hipLaunchKernelGGL(v.k, dim3(grid), dim3(256), 0, 0, st, n, lam, rates, nullptr, wgt, t, nullptr, 0, partials, ticket, out, nullptr);
      CK(hipEventRecord(f, 0));
      CK(hipEventSynchronize(f));
      CK(hipGetLastError());
      float ms = 0;
      CK(hipEventElapsedTime(&ms, b, f));
      double ho[3];
      CK(hipMemcpy(ho, out, 24, hipMemcpyDeviceToHost));
      if (round) printf("round %d %-32s grid %4d %7.2f us/call  out %.12g %.12g %.12g\n", round, v.name, grid, ms * 1e3 / calls, ho[0], ho[1], ho[2]);
    }
  }
  return 0;
}
