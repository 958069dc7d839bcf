// plf_edge.hpp -- one branch with the CLVs at its two ends held fixed: the
// sum table and the log-likelihood with its first two derivatives in the
// branch length (extension: RAxML's makenewz next to plf() = newview and
// plf_lnl.hpp = evaluate; the reference has neither).
//
// CLVs in eigen coordinates (PLFX_PMAT_EIGEN, V^T Pi V = I): for the two ends
// a, b of a branch of length t
//   st[i][c][k] = a[i][c][k] * b[i][c][k]                  (one multiply in T)
//   L_i(t)      = sum_c catw[c] * sum_k st[i][c][k] * exp(lambda_k r_c t)
// so the t-dependence is a diagonal and one pass over st gives, in f64,
//   x_ck = lambda_k r_c,  e = exp(x t),  e1 = e x,  e2 = e1 x
//   L, L1, L2 = sum_c catw[c] * sum_k st * {e, e1, e2}   (ascending k from +0.0,
//                                                         then ascending c)
//   out[0] = sum_i w_i log L_i + (sum of scaler_sums) * log(2^-32)
//   out[1] = sum_i w_i L1/L                  = d lnL / dt
//   out[2] = sum_i w_i (L2/L - (L1/L)^2)     = d2 lnL / dt2
// Scaling multiplies L, L1 and L2 of a site alike, so it cancels in out[1],
// out[2].  The three sums share plf_lnl.hpp's fixed-order reduction (N = 3).
// At the end of the file: the branch-length iteration over these sums with the
// loop on the device (edge_opt_kernel, plfx_edge_optimize_dev).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "edge_newton_step.hpp"
#include "plf_lnl.hpp"

namespace plfx {
namespace dev {

// Sum table, elementwise over 16-B chunks (ProtTile's chunk type; a site's
// row needs no transposition here, so the chunks go straight from registers
// to the store).  A trip's loads are all issued before its stores.  kTip:
// side 1 is one uint8 code per site, x1[i][c][k] = tipvec[row(code_i)][k] --
// DNA row = code & 15 (16 x 4), protein row = min(code, 23) (24 x 20).
template <typename T, int S, bool kTip>
__global__ void __launch_bounds__(kBlock)
edge_sumtable_kernel(const void *__restrict__ x1, const T *__restrict__ x2, int64_t n,
                     const T *__restrict__ tipvec, T *__restrict__ out) {
  using V = typename ProtTile<T>::V;
  constexpr int kVals = 16 / (int)sizeof(T);  // values per chunk
  constexpr int kRow = S / kVals;             // chunks per (site, category) row
  constexpr int kSite = 4 * kRow;             // chunks per site
  static_assert(S % kVals == 0, "a row is whole chunks");
  static_assert(S != 20 || kSite == ProtTile<T>::kChunksPerSite, "the protein tile's chunking");
  constexpr int U = 4;
  const int64_t total = n * kSite;
  const V *a = static_cast<const V *>(x1);
  const uint8_t *codes = static_cast<const uint8_t *>(x1);
  const V *b = reinterpret_cast<const V *>(x2);
  V *o = reinterpret_cast<V *>(out);
  const int64_t stride = (int64_t)gridDim.x * (kBlock * U);
  for (int64_t base = (int64_t)blockIdx.x * (kBlock * U); base < total; base += stride) {
    V va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t j = base + u * kBlock + threadIdx.x;
      if (j >= total) continue;
      vb[u] = __builtin_nontemporal_load(b + j);
      if constexpr (kTip) {
        const int64_t site = j / kSite;
        const int q = (int)(j - site * kSite);
        const int code = codes[site];
        const int row = S == 4 ? (code & 15) : prot_code((uint8_t)code);
        const T *tv = tipvec + row * S + (q % kRow) * kVals;
#pragma unroll
        for (int e = 0; e < kVals; e++) va[u][e] = tv[e];
      } else {
        va[u] = __builtin_nontemporal_load(a + j);
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t j = base + u * kBlock + threadIdx.x;
      if (j < total) __builtin_nontemporal_store(va[u] * vb[u], o + j);
    }
  }
}

// the three factors of category rate r at branch length t
__device__ __forceinline__ void edge_factors(double lambda, double r, double t, double &e0, double &e1,
                                             double &e2) {
  const double x = lambda * r;
  e0 = exp(x * t);
  e1 = e0 * x;
  e2 = e1 * x;
}

// one site's terms into the three accumulators; returns log L
__device__ __forceinline__ double edge_site(double L, double L1, double L2, int w, double (&acc)[3]) {
  const double l = log(L), r1 = L1 / L, r2 = L2 / L;
  acc[0] += (double)w * l;
  acc[1] += (double)w * r1;
  acc[2] += (double)w * (r2 - r1 * r1);
  return l;
}

// sum_k cw[k] * (t of lane k of this lane's quad), ascending k from +0.0.  The
// quad broadcasts are DPP moves: as __shfl (two LDS-crossbar permutes per
// double, 96 per trip for the three sums) the kernel ran 28.9 us per 2^20 f64
// sites against 27.6 with these, same bits (tools/probes/edge_deriv.hip,
// profiles/r07_probe_edge_deriv.log).  Every lane of the wave is active where
// this is called.
__device__ __forceinline__ double quad_cat_sum(const double (&cw)[4], double t) {
  double L = 0.0;
  L += cw[0] * dpp_f64<0x00>(t);  // quad_perm [0,0,0,0]
  L += cw[1] * dpp_f64<0x55>(t);  // [1,1,1,1]
  L += cw[2] * dpp_f64<0xAA>(t);  // [2,2,2,2]
  L += cw[3] * dpp_f64<0xFF>(t);  // [3,3,3,3]
  return L;
}

// S = 4: root_lnl_kernel's arrangement (C lanes per site, lane = category,
// lane c takes the log and the two quotients of step c's site).  A lane's
// table is its category's 3 x S factors, in registers.  The block's share of
// the sites into acc, at branch length t: the body of edge_deriv_kernel and
// of edge_opt_kernel (blocks along x).  partials: only a readable word here
// (wgt_at's dummy).
template <typename T, int S, int C>
__device__ __forceinline__ void edge_deriv_sites(const T *__restrict__ st, int64_t n,
                                                 const double *__restrict__ lambda,
                                                 const double *__restrict__ rates,
                                                 const double *__restrict__ catw,
                                                 const int32_t *__restrict__ wgt, const double t,
                                                 const double *partials, double *__restrict__ site_lnl,
                                                 double (&acc)[3]) {
  static_assert(C == 4, "a site's categories are the lanes of a quad (quad_cat_sum)");
  constexpr int V = S * C;
  constexpr int SPW = 64 / C;  // sites per wave step
  const int lane = threadIdx.x & 63;
  const int c = lane % C;
  const int q = lane / C;
  double e0[S], e1[S], e2[S];
  {
    const double r = rates[c];
#pragma unroll
    for (int k = 0; k < S; k++) edge_factors(lambda[k], r, t, e0[k], e1[k], e2[k]);
  }
  double cw[C];
#pragma unroll
  for (int k = 0; k < C; k++) cw[k] = catw ? catw[k] : 1.0 / C;

  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock * SPW * C;
  const int64_t nlast = n - 1;
  for (int64_t base = wave * SPW * C; base < n; base += stride) {
    // every load of the trip first (clamped to the last site), as root_lnl_kernel
    T v[C][S];
#pragma unroll
    for (int u = 0; u < C; u++) {
      const int64_t site = base + u * SPW + q;
      const T *xs = st + (site < n ? site : nlast) * V + c * S;  // 16-B aligned: S*sizeof(T) % 16 == 0
      if constexpr (sizeof(T) == 8) {
#pragma unroll
        for (int s = 0; s < S; s += 2) {
          const f64x2 w = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(xs + s));
          v[u][s] = w.x;
          v[u][s + 1] = w.y;
        }
      } else {
#pragma unroll
        for (int s = 0; s < S; s += 4) {
          const f32x4 w = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(xs + s));
          v[u][s] = w.x; v[u][s + 1] = w.y; v[u][s + 2] = w.z; v[u][s + 3] = w.w;
        }
      }
    }
    const int64_t site = base + c * SPW + q;  // this lane's site (step c)
    const bool valid = site < n;
    const int wv = wgt_at(wgt, valid ? site : nlast, partials);
    __builtin_amdgcn_sched_barrier(0);  // keeps the weight load with the table loads
    double m0 = 1.0, m1 = 0.0, m2 = 0.0;  // L, L1, L2 of step c's site
#pragma unroll
    for (int u = 0; u < C; u++) {
      double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
      for (int k = 0; k < S; k++) {
        const double x = (double)v[u][k];
        t0 += x * e0[k];
        t1 += x * e1[k];
        t2 += x * e2[k];
      }
      const double L0 = quad_cat_sum(cw, t0), L1 = quad_cat_sum(cw, t1), L2 = quad_cat_sum(cw, t2);
      if (u == c) {
        m0 = L0;
        m1 = L1;
        m2 = L2;
      }
    }
    if (valid) {
      const double l = edge_site(m0, m1, m2, wv, acc);
      if (site_lnl) site_lnl[site] = l;
    }
  }
}

template <typename T, int S, int C>
__global__ void __launch_bounds__(kBlock)
edge_deriv_kernel(const T *__restrict__ st, int64_t n, const double *__restrict__ lambda,
                  const double *__restrict__ rates, const double *__restrict__ catw,
                  const int32_t *__restrict__ wgt, const double *__restrict__ tp,
                  const int64_t *__restrict__ scaler_sums, int nsums, double *partials,
                  unsigned long long *ticket, double *out, double *__restrict__ site_lnl) {
  double acc[3] = {0.0, 0.0, 0.0};
  edge_deriv_sites<T, S, C>(st, n, lambda, rates, catw, wgt, *tp, partials, site_lnl, acc);
  lnl_finish<3>(acc, partials, ticket, out, scaler_sums, nsums);
}

// S = 20, C = 4: root_lnl_prot_kernel's arrangement (64-site tiles staged
// through LDS with coalesced loads, the next tile in flight in registers,
// wave w = category w, lane = site).  The block's 3 x 4 x 20 table is formed
// in LDS and stays there: a wave reads its category's 60 factors per tile at
// wave-uniform addresses (broadcast reads; in registers they cost 120 VGPRs
// and left one block per CU).  The category sums meet in LDS and wave 0 forms
// L, L1, L2 and the site's terms.
template <typename T>
__device__ __forceinline__ void edge_deriv_prot_sites(const T *__restrict__ st, int64_t n,
                                                      const double *__restrict__ lambda,
                                                      const double *__restrict__ rates,
                                                      const double *__restrict__ catw,
                                                      const int32_t *__restrict__ wgt, const double t,
                                                      const double *partials, double *__restrict__ site_lnl,
                                                      double (&acc)[3]) {
  constexpr int S = 20, C = 4;
  using PT = ProtTile<T>;
  constexpr int K = PT::kChunks / kBlock;
  const int c = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  __shared__ double tab[3][C][S];
  if (threadIdx.x < C * S) {
    const int tc_ = threadIdx.x / S, tk = threadIdx.x % S;
    double a0, a1, a2;
    edge_factors(lambda[tk], rates[tc_], t, a0, a1, a2);
    tab[0][tc_][tk] = a0;
    tab[1][tc_][tk] = a1;
    tab[2][tc_][tk] = a2;
  }
  double cw[C];
#pragma unroll
  for (int k = 0; k < C; k++) cw[k] = catw ? catw[k] : 1.0 / C;
  __shared__ typename PT::V tile[64 * PT::kStride];
  __shared__ double tc[3][C][64];
  const int64_t stride = (int64_t)gridDim.x * 64;
  typename PT::V pf[K];
  if ((int64_t)blockIdx.x * 64 < n) tile_fetch<T>(st, (int64_t)blockIdx.x * 64, n, pf);
  for (int64_t base = (int64_t)blockIdx.x * 64; base < n; base += stride) {
    const int64_t site = base + lane;
    const bool valid = site < n;
    const int wv = wgt_at(wgt, valid ? site : n - 1, partials);
    tile_put<T>(tile, pf);
    __syncthreads();
    if (base + stride < n) tile_fetch<T>(st, base + stride, n, pf);
    T v[S];
    row_read<T>(tile, lane, c, v);
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int k = 0; k < S; k++) {
      const double x = (double)v[k];
      t0 += x * tab[0][c][k];
      t1 += x * tab[1][c][k];
      t2 += x * tab[2][c][k];
    }
    tc[0][c][lane] = t0;
    tc[1][c][lane] = t1;
    tc[2][c][lane] = t2;
    __syncthreads();  // also: every wave is done reading the tile
    if (c == 0 && valid) {
      double L0 = 0.0, L1 = 0.0, L2 = 0.0;
#pragma unroll
      for (int k = 0; k < C; k++) {
        L0 += cw[k] * tc[0][k][lane];
        L1 += cw[k] * tc[1][k][lane];
        L2 += cw[k] * tc[2][k][lane];
      }
      const double l = edge_site(L0, L1, L2, wv, acc);
      if (site_lnl) site_lnl[site] = l;
    }
    __syncthreads();  // tc is rewritten by the next trip
  }
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
edge_deriv_prot_kernel(const T *__restrict__ st, int64_t n, const double *__restrict__ lambda,
                       const double *__restrict__ rates, const double *__restrict__ catw,
                       const int32_t *__restrict__ wgt, const double *__restrict__ tp,
                       const int64_t *scaler_sums, int nsums, double *partials,
                       unsigned long long *ticket, double *out, double *__restrict__ site_lnl) {
  double acc[3] = {0.0, 0.0, 0.0};
  edge_deriv_prot_sites<T>(st, n, lambda, rates, catw, wgt, *tp, partials, site_lnl, acc);
  lnl_finish<3>(acc, partials, ticket, out, scaler_sums, nsums);
}

// ---- the branch-length loop on the device (plfx_edge_optimize_dev) ----
//
// One launch = one evaluation of every edge of a group that has not stopped
// (blockIdx.y = edge, gridDim.x blocks per edge) and, in the thread that holds
// the edge's totals, one step of its bracket (edge_newton_step.hpp).  The host
// enqueues max_evals such launches; nothing waits inside a launch.
//
// Per edge j: its state state[j] (the stepper struct, in the stream
// workspace), its ticket words ws + j * kWsWords and its 3 * gridDim.x partial
// slots.  The first launch of a call (first != 0) does not read the state: t
// is t0[j] clamped into [tmin, tmax] and the electing thread initialises the
// state before it steps, so a replayed graph needs no reset.  In later
// launches every block reads the edge's flags and t at entry; the state was
// written by an earlier launch of the same stream, so all blocks of the edge
// agree, and a stopped edge's blocks return before they touch partials or
// tickets.  Within a launch the state is written only after every block of the
// edge has drawn its ticket, i.e. after every entry read.  The thread that
// stops an edge writes t_opt[j], out3[3j..], evals[j] (the last two optional).
struct EdgeOptTabs {
  const void *st[kMaxBatch];
};
static_assert(sizeof(EdgeNewtonStep) == 32, "plf_kernels.hpp kEdgeStateBytes");

__device__ __forceinline__ double edge_opt_entry(const EdgeNewtonStep *sp, const double *t0,
                                                 double tmin, double tmax, int first, bool &done) {
  const int j = blockIdx.y;
  done = false;
  if (first) {
    const double t = t0[j];
    return !(t >= tmin) ? tmin : (t > tmax ? tmax : t);  // a NaN starts at tmin
  }
  done = (__hip_atomic_load(&sp->flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & EdgeNewtonStep::kDone) != 0;
  return __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const unsigned long long *>(&sp->t),
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// the electing thread: acc holds the edge's lnL, d1, d2 at t
__device__ __forceinline__ void edge_opt_step(EdgeNewtonStep *sp, const double (&acc)[3], double t, double tmin,
                                              double tmax, int max_evals, int first, double *t_opt,
                                              double *out3, int32_t *evals) {
  const int j = blockIdx.y;
  EdgeNewtonStep s;
  if (first) s.init(t, tmin, tmax);
  else s = *sp;
  if (!s.advance(acc[1], acc[2], max_evals)) {
    s.flags |= EdgeNewtonStep::kDone;
    t_opt[j] = s.t;
    if (out3) {
      out3[3 * j] = acc[0];
      out3[3 * j + 1] = acc[1];
      out3[3 * j + 2] = acc[2];
    }
    if (evals) evals[j] = s.evals;
  }
  *sp = s;
}

template <typename T, int S>
__global__ void __launch_bounds__(kBlock)
edge_opt_kernel(const EdgeOptTabs tabs, int64_t n, const double *__restrict__ lambda,
                const double *__restrict__ rates, const double *__restrict__ catw,
                const int32_t *__restrict__ wgt, const double *t0, double tmin, double tmax,
                int max_evals, int first, EdgeNewtonStep *state, double *partials, unsigned long long *ws,
                double *t_opt, double *out3, int32_t *evals) {
  EdgeNewtonStep *sp = state + blockIdx.y;
  bool done;
  const double t = edge_opt_entry(sp, t0, tmin, tmax, first, done);
  if (done) return;
  const T *st = static_cast<const T *>(tabs.st[blockIdx.y]);
  double *part = partials + (size_t)blockIdx.y * 3 * gridDim.x;
  double acc[3] = {0.0, 0.0, 0.0};
  if constexpr (S == 4) edge_deriv_sites<T, 4, 4>(st, n, lambda, rates, catw, wgt, t, part, nullptr, acc);
  else edge_deriv_prot_sites<T>(st, n, lambda, rates, catw, wgt, t, part, nullptr, acc);
  if (lnl_finish<3, false>(acc, part, ws + (size_t)blockIdx.y * kWsWords, nullptr, nullptr, 0))
    edge_opt_step(sp, acc, t, tmin, tmax, max_evals, first, t_opt, out3, evals);
}

}  // namespace dev
}  // namespace plfx
