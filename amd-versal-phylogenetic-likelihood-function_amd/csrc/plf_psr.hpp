// plf_psr.hpp -- device code of the per-site-rate (PSR, "CAT") DNA mode,
// plfx.h section 11: every site belongs to exactly one of ncat rate
// categories, so a CLV is x[site*4 + state] -- a quarter of the Gamma layout
// -- and a site's P matrices are chosen by its category byte,
// c = min(rate_cat[site], ncat - 1).
//
// Node update, in plf()'s operation order with no contraction:
//   umpL[k] = sum_l x1[i][l] * left[c*16 + k*4 + l]   (from +0.0, ascending l)
//   x3[i][l] = sum_k (umpL[k] * umpR[k]) * EV[4k + l] (from +0.0, ascending k)
// then the 2^-32 rescale over the site's four values.  One lane owns one site:
// its children are 16 (f32) or 32 (f64) contiguous bytes, the scale test needs
// no cross-lane step, and the only thing that is not wave-uniform any more --
// the two matrices -- comes from LDS, where the block stages both tables once.
//
// LDS rows.  A lane reads its category's 16 values per side as ds_read_b128
// (16-lane groups, sixteen 16-B slots per LDS cycle).  With the natural row
// stride (128 B in f64, 64 B in f32) chunk j of every row falls on 2 (f64) or
// 4 (f32) of the sixteen slots, so a group whose lanes sit in different
// categories would serialise 8- or 4-fold.  One 16-B chunk of padding per row
// makes the stride 9 (f64) or 5 (f32) slots, odd, so 16 consecutive
// categories cover all sixteen slots: what is left is the chance collision of
// random categories (ncat / 16 rows share a slot).  EV is wave-uniform and
// stays in scalar registers.
//
// A coded child's ump depends only on (category, code): the block forms
// tab[(c*16 + code)*4 + k] = sum_l tipvec[code][l] * P_c[k][l] in the same
// order, so results are bit-identical to the dense computation on the
// expanded child (as plf_dna.hpp build_tip_table does per Gamma category).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "plf_edge.hpp"

namespace plfx {
namespace dev {

constexpr int kPsrMaxCats = 32;  // PLFX_PSR_MAX_CATS (asserted in plfx_api.hip)

template <typename T>
struct PsrRow {
  static constexpr int kChunk = 16 / (int)sizeof(T);  // values per 16-B chunk
  static constexpr int kStride = 16 + kChunk;         // values per staged matrix row (one chunk of padding)
  using V = std::conditional_t<sizeof(T) == 8, f64x2, f32x4>;
};

__device__ __forceinline__ int psr_cat(int byte, int ncat) { return byte < ncat ? byte : ncat - 1; }

// both tables of a node into LDS, padded rows; the caller synchronises
template <typename T>
__device__ __forceinline__ void psr_stage(const T *__restrict__ P, int ncat, T *sP) {
  for (int i = threadIdx.x; i < ncat * 16; i += kBlock) sP[(i >> 4) * PsrRow<T>::kStride + (i & 15)] = P[i];
}

// tab[(c*16 + code)*4 + k] of a coded child (tv NULL: the 0/1 indicator)
template <typename T>
__device__ __forceinline__ void psr_tip_table(const T *__restrict__ P, const T *__restrict__ tv, int ncat,
                                              T *tab) {
  for (int i = threadIdx.x; i < ncat * 64; i += kBlock) {
    const int c = i >> 6, code = (i >> 2) & 15, k = i & 3;
    T v = T(0);
#pragma unroll
    for (int l = 0; l < 4; l++) v += (tv ? tv[code * 4 + l] : T((code >> l) & 1)) * P[c * 16 + k * 4 + l];
    tab[i] = v;
  }
}

// a 16-B aligned LDS row of N values as 16-B reads
template <typename T, int N>
__device__ __forceinline__ void psr_lds_row(const T *row, T (&m)[N]) {
  using V = typename PsrRow<T>::V;
  constexpr int kChunk = PsrRow<T>::kChunk;
  static_assert(N % kChunk == 0, "whole chunks");
  const V *r = reinterpret_cast<const V *>(row);
#pragma unroll
  for (int j = 0; j < N / kChunk; j++) {
    const V v = r[j];
#pragma unroll
    for (int e = 0; e < kChunk; e++) m[j * kChunk + e] = v[e];
  }
}

// Up to kMaxBatch nodes per launch, node = blockIdx.y, sharing EV, n, wgt and
// rate_cat; T1 / T2: child 1 / 2 of every node of the launch is coded (the
// descriptor's x1 / x2 then point at uint8 codes).  U sites per lane and trip,
// all their loads issued first (clamped to the last site, results unused past
// n).  kSum: some node of the launch wants its weighted scaler sum.
template <typename T, int U, bool kSum, bool T1, bool T2>
__global__ void __launch_bounds__(kBlock)
plf_psr_kernel(const NodeBatch nodes, const T *__restrict__ EV, const uint8_t *__restrict__ rate_cat, int ncat,
               const int32_t *__restrict__ wgt, int64_t n, unsigned long long *ws,
               const T *__restrict__ tipvec) {
  constexpr int kStride = PsrRow<T>::kStride;
  const NodeDesc &d = nodes.d[blockIdx.y];
  const T *__restrict__ x1 = static_cast<const T *>(d.x1);
  const T *__restrict__ x2 = static_cast<const T *>(d.x2);
  const uint8_t *__restrict__ tip1 = static_cast<const uint8_t *>(d.x1);
  const uint8_t *__restrict__ tip2 = static_cast<const uint8_t *>(d.x2);
  T *__restrict__ x3 = static_cast<T *>(d.x3);
  uint8_t *__restrict__ scaler = d.scaler;
  unsigned long long *wsn = ws + (size_t)blockIdx.y * kWsWords;

  __shared__ __attribute__((aligned(16))) T sL[T1 ? 4 : kPsrMaxCats * kStride];
  __shared__ __attribute__((aligned(16))) T sR[T2 ? 4 : kPsrMaxCats * kStride];
  __shared__ __attribute__((aligned(16))) T tab1[T1 ? kPsrMaxCats * 64 : 4];
  __shared__ __attribute__((aligned(16))) T tab2[T2 ? kPsrMaxCats * 64 : 4];
  if constexpr (T1) psr_tip_table<T>(static_cast<const T *>(d.left), tipvec, ncat, tab1);
  else psr_stage<T>(static_cast<const T *>(d.left), ncat, sL);
  if constexpr (T2) psr_tip_table<T>(static_cast<const T *>(d.right), tipvec, ncat, tab2);
  else psr_stage<T>(static_cast<const T *>(d.right), ncat, sR);
  __syncthreads();

  T E[16];
#pragma unroll
  for (int i = 0; i < 16; i++) E[i] = EV[i];  // uniform: scalar loads
  const T m = Num<T>::minlik();

  long long acc = 0;
  const int64_t stride = (int64_t)gridDim.x * (kBlock * U);
  const int64_t nlast = n - 1;
  for (int64_t base = (int64_t)blockIdx.x * (kBlock * U); base < n; base += stride) {
    T a[U][4], b[U][4];
    int cat[U], k1[U], k2[U], w[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t site = base + u * kBlock + threadIdx.x;
      const int64_t ld = site < n ? site : nlast;
      cat[u] = rate_cat[ld];
      if constexpr (T1) k1[u] = tip1[ld] & 15;
      else Num<T>::template load4<true>(x1 + ld * 4, a[u]);
      if constexpr (T2) k2[u] = tip2[ld] & 15;
      else Num<T>::template load4<true>(x2 + ld * 4, b[u]);
      if (kSum) w[u] = wgt_at(wgt, ld, ws);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t site = base + u * kBlock + threadIdx.x;
      const int c = psr_cat(cat[u], ncat);
      T u1[4], u2[4];
      if constexpr (T1) {
        psr_lds_row<T, 4>(tab1 + (c * 16 + k1[u]) * 4, u1);
      } else {
        T PL[16];
        psr_lds_row<T, 16>(sL + c * kStride, PL);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          u1[k] = T(0);
#pragma unroll
          for (int l = 0; l < 4; l++) u1[k] += a[u][l] * PL[k * 4 + l];
        }
      }
      if constexpr (T2) {
        psr_lds_row<T, 4>(tab2 + (c * 16 + k2[u]) * 4, u2);
      } else {
        T PR[16];
        psr_lds_row<T, 16>(sR + c * kStride, PR);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          u2[k] = T(0);
#pragma unroll
          for (int l = 0; l < 4; l++) u2[k] += b[u][l] * PR[k * 4 + l];
        }
      }
      T o[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const T p = u1[k] * u2[k];
#pragma unroll
        for (int l = 0; l < 4; l++) o[l] += p * E[4 * k + l];
      }
      const bool sc = (Num<T>::abs(o[0]) < m) && (Num<T>::abs(o[1]) < m) && (Num<T>::abs(o[2]) < m) &&
                      (Num<T>::abs(o[3]) < m);
#pragma unroll
      for (int l = 0; l < 4; l++) {
        const T s = o[l] * Num<T>::two32();  // exact: power-of-two scaling
        o[l] = sc ? s : o[l];
      }
      if (site < n) {
        Num<T>::store4_nt(x3 + site * 4, o);
        if (scaler) scaler[site] = (uint8_t)sc;
        if (kSum) acc += sc ? (long long)w[u] : 0ll;
      }
    }
  }
  if constexpr (kSum) block_ticket_sum(acc, wsn, d.scaler_sum);
}

// One site of one node, plf_psr_kernel's arithmetic restated for the fused
// kernel below (the node kernel keeps its own statement: routed through this
// function its register allocation changes, f64 dense/dense 91 -> 112 VGPRs):
// o = the (possibly rescaled) parent values, returns the site's scale flag.  row1 / row2: the side's LDS row -- the category's padded
// matrix row (dense child a / b) or the 4 products of (category, code) when
// the side is coded (T1 / T2; a / b are then unused).
template <typename T, bool T1, bool T2>
__device__ __forceinline__ bool psr_site(const T (&a)[4], const T (&b)[4], const T *row1, const T *row2,
                                         const T (&E)[16], T m, T (&o)[4]) {
  T u1[4], u2[4];
  if constexpr (T1) {
    psr_lds_row<T, 4>(row1, u1);
  } else {
    T PL[16];
    psr_lds_row<T, 16>(row1, PL);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      u1[k] = T(0);
#pragma unroll
      for (int l = 0; l < 4; l++) u1[k] += a[l] * PL[k * 4 + l];
    }
  }
  if constexpr (T2) {
    psr_lds_row<T, 4>(row2, u2);
  } else {
    T PR[16];
    psr_lds_row<T, 16>(row2, PR);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      u2[k] = T(0);
#pragma unroll
      for (int l = 0; l < 4; l++) u2[k] += b[l] * PR[k * 4 + l];
    }
  }
#pragma unroll
  for (int l = 0; l < 4; l++) o[l] = T(0);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const T p = u1[k] * u2[k];
#pragma unroll
    for (int l = 0; l < 4; l++) o[l] += p * E[4 * k + l];
  }
  const bool sc = (Num<T>::abs(o[0]) < m) && (Num<T>::abs(o[1]) < m) && (Num<T>::abs(o[2]) < m) &&
                  (Num<T>::abs(o[3]) < m);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const T s = o[l] * Num<T>::two32();  // exact: power-of-two scaling
    o[l] = sc ? s : o[l];
  }
  return sc;
}

// Fused level pair of a PSR traversal (plfx_traverse_psr): ops A and B of one
// level and the op P of the next that reads both, in one pass.  The lane that
// owns a site computes A from (a1, a2) and B from (b1, b2) as psr_site does,
// stores both, and computes P from the (rescaled) values it still holds, so
// P's children are written once and never read back: 4 leaf reads + 3 writes
// per site instead of 6 reads + 3 writes.  Every node keeps its own scale
// test, scaler byte and weighted sum: the bits of three plf_psr_kernel
// launches.  Up to kMaxTriples per launch, triple = blockIdx.y, each with
// three consecutive ticket regions of ws.
// kTips: 0 the four leaves are dense; 1 a1 and b1 are coded (the lowering puts
// the coded child first); 2 all four are coded.  LDS: a (category, code) table
// per coded leaf, a padded matrix table per dense leaf, and P's two matrix
// tables -- in f64 at most 27 KB (kTips 0), 50 KB (1), 73 KB (2), half of
// that in f32.
template <typename T, int kTips>
struct PsrTripleLds {
  static constexpr int kMat = kPsrMaxCats * PsrRow<T>::kStride;  // a staged matrix table
  static constexpr int kTab = kPsrMaxCats * 64;                  // a coded leaf's table
  static constexpr int kSide1 = kTips >= 1 ? kTab : kMat, kSide2 = kTips == 2 ? kTab : kMat;
  static constexpr int kValues = 2 * kSide1 + 2 * kSide2 + 2 * kMat;
};

template <typename T, int U, bool kSum, int kTips>
__global__ void __launch_bounds__(kBlock)
plf_psr_triple_kernel(const TripleBatch tb, const T *__restrict__ EV, const uint8_t *__restrict__ rate_cat,
                      int ncat, const int32_t *__restrict__ wgt, int64_t n, unsigned long long *ws,
                      const T *__restrict__ tipvec) {
  constexpr bool T1 = kTips >= 1, T2 = kTips == 2;
  constexpr int kStride = PsrRow<T>::kStride;
  using Lds = PsrTripleLds<T, kTips>;
  const TripleDesc &d = tb.d[blockIdx.y];

  __shared__ __attribute__((aligned(16))) T lds[Lds::kValues];
  T *const sA1 = lds, *const sB1 = sA1 + Lds::kSide1, *const sA2 = sB1 + Lds::kSide1;
  T *const sB2 = sA2 + Lds::kSide2, *const sLP = sB2 + Lds::kSide2, *const sRP = sLP + Lds::kMat;
  if constexpr (T1) {
    psr_tip_table<T>((const T *)d.la, tipvec, ncat, sA1);
    psr_tip_table<T>((const T *)d.lb, tipvec, ncat, sB1);
  } else {
    psr_stage<T>((const T *)d.la, ncat, sA1);
    psr_stage<T>((const T *)d.lb, ncat, sB1);
  }
  if constexpr (T2) {
    psr_tip_table<T>((const T *)d.ra, tipvec, ncat, sA2);
    psr_tip_table<T>((const T *)d.rb, tipvec, ncat, sB2);
  } else {
    psr_stage<T>((const T *)d.ra, ncat, sA2);
    psr_stage<T>((const T *)d.rb, ncat, sB2);
  }
  psr_stage<T>((const T *)d.lp, ncat, sLP);
  psr_stage<T>((const T *)d.rp, ncat, sRP);
  __syncthreads();

  T E[16];
#pragma unroll
  for (int i = 0; i < 16; i++) E[i] = EV[i];  // uniform: scalar loads
  const T m = Num<T>::minlik();
  const T *__restrict__ xa1 = (const T *)d.a1, *__restrict__ xa2 = (const T *)d.a2;
  const T *__restrict__ xb1 = (const T *)d.b1, *__restrict__ xb2 = (const T *)d.b2;
  const uint8_t *__restrict__ ta1 = (const uint8_t *)d.a1, *__restrict__ ta2 = (const uint8_t *)d.a2;
  const uint8_t *__restrict__ tb1 = (const uint8_t *)d.b1, *__restrict__ tb2 = (const uint8_t *)d.b2;
  T *__restrict__ xa = (T *)d.xa, *__restrict__ xb = (T *)d.xb, *__restrict__ xp = (T *)d.xp;

  long long accA = 0, accB = 0, accP = 0;
  const int64_t stride = (int64_t)gridDim.x * (kBlock * U);
  const int64_t nlast = n - 1;
  for (int64_t base = (int64_t)blockIdx.x * (kBlock * U); base < n; base += stride) {
    T va1[U][4], va2[U][4], vb1[U][4], vb2[U][4];
    int cat[U], ka1[U], ka2[U], kb1[U], kb2[U], w[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t site = base + u * kBlock + threadIdx.x;
      const int64_t ld = site < n ? site : nlast;
      cat[u] = rate_cat[ld];
      if constexpr (T1) {
        ka1[u] = ta1[ld] & 15;
        kb1[u] = tb1[ld] & 15;
      } else {
        Num<T>::template load4<true>(xa1 + ld * 4, va1[u]);
        Num<T>::template load4<true>(xb1 + ld * 4, vb1[u]);
      }
      if constexpr (T2) {
        ka2[u] = ta2[ld] & 15;
        kb2[u] = tb2[ld] & 15;
      } else {
        Num<T>::template load4<true>(xa2 + ld * 4, va2[u]);
        Num<T>::template load4<true>(xb2 + ld * 4, vb2[u]);
      }
      if (kSum) w[u] = wgt_at(wgt, ld, ws);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t site = base + u * kBlock + threadIdx.x;
      const int c = psr_cat(cat[u], ncat);
      T oA[4], oB[4], oP[4];
      const bool sA = psr_site<T, T1, T2>(va1[u], va2[u], T1 ? sA1 + (c * 16 + ka1[u]) * 4 : sA1 + c * kStride,
                                          T2 ? sA2 + (c * 16 + ka2[u]) * 4 : sA2 + c * kStride, E, m, oA);
      const bool sB = psr_site<T, T1, T2>(vb1[u], vb2[u], T1 ? sB1 + (c * 16 + kb1[u]) * 4 : sB1 + c * kStride,
                                          T2 ? sB2 + (c * 16 + kb2[u]) * 4 : sB2 + c * kStride, E, m, oB);
      const bool sP = psr_site<T, false, false>(oA, oB, sLP + c * kStride, sRP + c * kStride, E, m, oP);
      if (site < n) {
        Num<T>::store4_nt(xa + site * 4, oA);
        Num<T>::store4_nt(xb + site * 4, oB);
        Num<T>::store4_nt(xp + site * 4, oP);
        if (d.sa) d.sa[site] = (uint8_t)sA;
        if (d.sb) d.sb[site] = (uint8_t)sB;
        if (d.sp) d.sp[site] = (uint8_t)sP;
        if (kSum) {
          accA += sA ? (long long)w[u] : 0ll;
          accB += sB ? (long long)w[u] : 0ll;
          accP += sP ? (long long)w[u] : 0ll;
        }
      }
    }
  }
  if constexpr (kSum)
    block_ticket_sum3(accA, accB, accP, ws + (size_t)blockIdx.y * 3 * kWsWords, d.ssa, d.ssb, d.ssp);
}

// Root lnL of a PSR CLV: L_i = sum_s freq[s] * x[i][s] (from +0.0, ascending
// s, in f64), one lane per site, U sites per lane and trip; the sum over the
// sites through plf_lnl.hpp's fixed-order reduction.
template <typename T, int U>
__global__ void __launch_bounds__(kBlock)
root_lnl_psr_kernel(const T *__restrict__ x, int64_t n, const double *__restrict__ freq,
                    const int32_t *__restrict__ wgt, const int64_t *__restrict__ scaler_sums, int nsums,
                    double *partials, unsigned long long *ticket, double *out, double *__restrict__ site_lnl) {
  double fr[4];
#pragma unroll
  for (int s = 0; s < 4; s++) fr[s] = freq ? freq[s] : 0.25;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * (kBlock * U);
  const int64_t nlast = n - 1;
  for (int64_t base = (int64_t)blockIdx.x * (kBlock * U); base < n; base += stride) {
    T v[U][4];
    int w[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t site = base + u * kBlock + threadIdx.x;
      const int64_t ld = site < n ? site : nlast;
      Num<T>::template load4<true>(x + ld * 4, v[u]);
      w[u] = wgt_at(wgt, ld, partials);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t site = base + u * kBlock + threadIdx.x;
      double L = 0.0;
#pragma unroll
      for (int s = 0; s < 4; s++) L += fr[s] * (double)v[u][s];
      if (site < n) {
        const double l = log(L);
        if (site_lnl) site_lnl[site] = l;
        acc += (double)w[u] * l;
      }
    }
  }
  lnl_finish(acc, partials, ticket, out, scaler_sums, nsums);
}

// Sum table of a PSR branch: x1 * x2 over n * 4 values, 16-B chunks, U chunks
// per thread and trip (plf_edge.hpp edge_sumtable_kernel for one category).
// kTip: side 1 is one code per site, x1[i][k] = tipvec[(code & 15)*4 + k].
template <typename T, bool kTip>
__device__ __forceinline__ void edge_sumtable_psr_chunks(const void *__restrict__ x1, const T *__restrict__ x2,
                                                         int64_t n, const T *__restrict__ tipvec,
                                                         T *__restrict__ out) {
  using V = typename PsrRow<T>::V;
  constexpr int kVals = PsrRow<T>::kChunk;
  constexpr int kSite = 4 / kVals;  // chunks per site
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
        const T *tv = tipvec + (codes[site] & 15) * 4 + (int)(j - site * kSite) * kVals;
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

template <typename T, bool kTip>
__global__ void __launch_bounds__(kBlock)
edge_sumtable_psr_kernel(const void *__restrict__ x1, const T *__restrict__ x2, int64_t n,
                         const T *__restrict__ tipvec, T *__restrict__ out) {
  edge_sumtable_psr_chunks<T, kTip>(x1, x2, n, tipvec, out);
}

// Up to kMaxBatch sum tables per launch (plfx_edge_sumtable_psr_batch), edge =
// blockIdx.y, all with the same kind of side 1 (kTip: x1 names the codes):
// each edge's table is the one-edge kernel's, chunk for chunk.
struct PsrEdgeDesc {
  const void *x1, *x2;
  void *out;
};
struct PsrEdgeBatch {
  PsrEdgeDesc d[kMaxBatch];
};

template <typename T, bool kTip>
__global__ void __launch_bounds__(kBlock)
edge_sumtable_psr_batch_kernel(const PsrEdgeBatch edges, int64_t n, const T *__restrict__ tipvec) {
  const PsrEdgeDesc &d = edges.d[blockIdx.y];
  edge_sumtable_psr_chunks<T, kTip>(d.x1, static_cast<const T *>(d.x2), n, tipvec, static_cast<T *>(d.out));
}

// The three edge sums of a PSR branch.  x_k = lambda_k * rates[c_i]; the
// ncat x 4 factor triples {e, e x, e x x} are formed once per block from the
// device t into LDS (rows of 12 doubles padded to 14: a stride of 7 slots,
// odd, as the node's tables) and a lane reads its site's row.  L, L1, L2 =
// sum_k st[i][k] * {e, e1, e2} from +0.0, ascending k, in f64; the sums over
// the sites as plf_edge.hpp's (edge_site, lnl_finish<3>).  n == 0: one block,
// out = {correction, 0, 0}.
//
// edge_deriv_psr_sites: the block's factor table at branch length t and its
// share of the sites into acc (blocks along x) -- edge_deriv_psr_kernel's
// lines, statement for statement, as the body of edge_opt_psr_kernel.  The
// derivative kernel keeps its own statement below: routed through this
// function its register allocation changes (f64 110 -> 116 VGPRs, f32 98 ->
// 104; LDS 3688 B and 4 waves per SIMD either way), as the node kernel's does
// through psr_site.  The bits are the same: no contraction, one order.
// partials: only a readable word here (wgt_at's dummy).
constexpr int kPsrFactorStride = 14;
template <typename T, int U>
__device__ __forceinline__ void edge_deriv_psr_sites(const T *__restrict__ st, int64_t n,
                                                     const double *__restrict__ lambda,
                                                     const double *__restrict__ rates, int ncat,
                                                     const uint8_t *__restrict__ rate_cat,
                                                     const int32_t *__restrict__ wgt, const double t,
                                                     const double *partials, double *__restrict__ site_lnl,
                                                     double (&acc)[3]) {
  __shared__ __attribute__((aligned(16))) double tab[kPsrMaxCats * kPsrFactorStride];
  for (int i = threadIdx.x; i < ncat * 4; i += kBlock) {
    const int c = i >> 2, k = i & 3;
    double e0, e1, e2;
    edge_factors(lambda[k], rates[c], t, e0, e1, e2);
    tab[c * kPsrFactorStride + k] = e0;
    tab[c * kPsrFactorStride + 4 + k] = e1;
    tab[c * kPsrFactorStride + 8 + k] = e2;
  }
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * (kBlock * U);
  const int64_t nlast = n - 1;
  for (int64_t base = (int64_t)blockIdx.x * (kBlock * U); base < n; base += stride) {
    T v[U][4];
    int cat[U], w[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t site = base + u * kBlock + threadIdx.x;
      const int64_t ld = site < n ? site : nlast;
      cat[u] = rate_cat[ld];
      Num<T>::template load4<true>(st + ld * 4, v[u]);
      w[u] = wgt_at(wgt, ld, partials);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t site = base + u * kBlock + threadIdx.x;
      double f[12];
      psr_lds_row<double, 12>(tab + psr_cat(cat[u], ncat) * kPsrFactorStride, f);
      double L = 0.0, L1 = 0.0, L2 = 0.0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const double x = (double)v[u][k];
        L += x * f[k];
        L1 += x * f[4 + k];
        L2 += x * f[8 + k];
      }
      if (site < n) {
        const double l = edge_site(L, L1, L2, w[u], acc);
        if (site_lnl) site_lnl[site] = l;
      }
    }
  }
}

template <typename T, int U>
__global__ void __launch_bounds__(kBlock)
edge_deriv_psr_kernel(const T *__restrict__ st, int64_t n, const double *__restrict__ lambda,
                      const double *__restrict__ rates, int ncat, const uint8_t *__restrict__ rate_cat,
                      const int32_t *__restrict__ wgt, const double *__restrict__ tp,
                      const int64_t *__restrict__ scaler_sums, int nsums, double *partials,
                      unsigned long long *ticket, double *out, double *__restrict__ site_lnl) {
  __shared__ __attribute__((aligned(16))) double tab[kPsrMaxCats * kPsrFactorStride];
  const double t = *tp;
  for (int i = threadIdx.x; i < ncat * 4; i += kBlock) {
    const int c = i >> 2, k = i & 3;
    double e0, e1, e2;
    edge_factors(lambda[k], rates[c], t, e0, e1, e2);
    tab[c * kPsrFactorStride + k] = e0;
    tab[c * kPsrFactorStride + 4 + k] = e1;
    tab[c * kPsrFactorStride + 8 + k] = e2;
  }
  __syncthreads();
  double acc[3] = {0.0, 0.0, 0.0};
  const int64_t stride = (int64_t)gridDim.x * (kBlock * U);
  const int64_t nlast = n - 1;
  for (int64_t base = (int64_t)blockIdx.x * (kBlock * U); base < n; base += stride) {
    T v[U][4];
    int cat[U], w[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t site = base + u * kBlock + threadIdx.x;
      const int64_t ld = site < n ? site : nlast;
      cat[u] = rate_cat[ld];
      Num<T>::template load4<true>(st + ld * 4, v[u]);
      w[u] = wgt_at(wgt, ld, partials);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t site = base + u * kBlock + threadIdx.x;
      double f[12];
      psr_lds_row<double, 12>(tab + psr_cat(cat[u], ncat) * kPsrFactorStride, f);
      double L = 0.0, L1 = 0.0, L2 = 0.0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const double x = (double)v[u][k];
        L += x * f[k];
        L1 += x * f[4 + k];
        L2 += x * f[8 + k];
      }
      if (site < n) {
        const double l = edge_site(L, L1, L2, w[u], acc);
        if (site_lnl) site_lnl[site] = l;
      }
    }
  }
  lnl_finish<3>(acc, partials, ticket, out, scaler_sums, nsums);
}

// The branch-length loop on the device for PSR branches
// (plfx_edge_optimize_psr_dev): plf_edge.hpp's edge_opt_kernel with the site
// loop above.  One launch = one evaluation of every edge of the group that has
// not stopped (blockIdx.y = edge, gridDim.x blocks per edge) and one step of
// its bracket in the thread that holds the edge's totals; the state, ticket
// and partial regions, the entry read and the step are that kernel's
// (edge_opt_entry, edge_opt_step).  A stopped edge's blocks return before any
// barrier, LDS write, partial or ticket.  Every block forms the factor table
// from its edge's own t.
template <typename T, int U>
__global__ void __launch_bounds__(kBlock)
edge_opt_psr_kernel(const EdgeOptTabs tabs, int64_t n, const double *__restrict__ lambda,
                    const double *__restrict__ rates, int ncat, const uint8_t *__restrict__ rate_cat,
                    const int32_t *__restrict__ wgt, const double *t0, double tmin, double tmax, int max_evals,
                    int first, EdgeNewtonStep *state, double *partials, unsigned long long *ws, double *t_opt,
                    double *out3, int32_t *evals) {
  EdgeNewtonStep *sp = state + blockIdx.y;
  bool done;
  const double t = edge_opt_entry(sp, t0, tmin, tmax, first, done);
  if (done) return;
  const T *st = static_cast<const T *>(tabs.st[blockIdx.y]);
  double *part = partials + (size_t)blockIdx.y * 3 * gridDim.x;
  double acc[3] = {0.0, 0.0, 0.0};
  edge_deriv_psr_sites<T, U>(st, n, lambda, rates, ncat, rate_cat, wgt, t, part, nullptr, acc);
  if (lnl_finish<3, false>(acc, part, ws + (size_t)blockIdx.y * kWsWords, nullptr, nullptr, 0))
    edge_opt_step(sp, acc, t, tmin, tmax, max_evals, first, t_opt, out3, evals);
}

// ---- plfx.h section 12: the per-site rate scan ----
//
// Per-site lnL with the site's own scaling correction over a "virtual
// alignment" of G segments of n sites (virtual site g * n + i = site i under
// candidate k0 + g), and the running argmax over the candidates.  One lane
// owns site i and walks g:
//   L   = sum_s freq[s] * x[(g*n + i)*4 + s]    root_lnl_psr_kernel's statement
//   cnt = sum_{j < nsc} (scalers[j*stride + g*n + i] != 0)
//   lnl = log(L) + (double)cnt * log(2^-32)     one multiply, one add
// A wave's 64 lanes read 64 consecutive bytes of a scaler row and 64
// consecutive CLV rows: the kernel streams nsc + 4 * sizeof(T) bytes per
// virtual site.  U candidates per trip, all their loads issued first (clamped
// to the last candidate, results unused past G).
// kBest: candidate k0 + g replaces (best_lnl, best_idx) iff lnl > best_lnl
// (ties keep the lower index, a NaN never wins), from (-inf, 0) when `first`,
// else from what the earlier passes left; out != NULL (the last pass): out =
// sum_i wgt_i * best_lnl[i] through lnl_finish.  all_lnl may be NULL.
template <typename T, bool kBest, int U>
__global__ void __launch_bounds__(kBlock)
psr_site_lnl_kernel(const T *__restrict__ x, int64_t n, int G, const double *__restrict__ freq,
                    const uint8_t *__restrict__ scalers, int nsc, int64_t stride, int k0, int first,
                    double *__restrict__ all_lnl, double *best_lnl, int32_t *best_idx,
                    const int32_t *__restrict__ wgt, double *partials, unsigned long long *ticket, double *out) {
  double fr[4];
#pragma unroll
  for (int s = 0; s < 4; s++) fr[s] = freq ? freq[s] : 0.25;
  double acc = 0.0;
  const int64_t step = (int64_t)gridDim.x * kBlock;
  for (int64_t site = (int64_t)blockIdx.x * kBlock + threadIdx.x; site < n; site += step) {
    double bl = -__builtin_inf();
    int bi = 0;
    if constexpr (kBest) {
      if (!first) {
        bl = best_lnl[site];
        bi = best_idx[site];
      }
    }
    for (int g0 = 0; g0 < G; g0 += U) {
      T v[U][4];
      int cnt[U];
      int64_t vs[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int g = g0 + u < G ? g0 + u : G - 1;
        vs[u] = (int64_t)g * n + site;
        Num<T>::template load4<true>(x + vs[u] * 4, v[u]);
        cnt[u] = 0;
      }
#pragma unroll 4
      for (int j = 0; j < nsc; j++) {
        const uint8_t *row = scalers + (int64_t)j * stride;
#pragma unroll
        for (int u = 0; u < U; u++) cnt[u] += row[vs[u]] != 0 ? 1 : 0;
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        double L = 0.0;
#pragma unroll
        for (int s = 0; s < 4; s++) L += fr[s] * (double)v[u][s];
        const double corr = (double)cnt[u] * kLogMinLik;
        const double l = log(L) + corr;
        if (g0 + u < G) {
          if (all_lnl) all_lnl[(int64_t)(k0 + g0 + u) * n + site] = l;
          if (kBest && l > bl) {
            bl = l;
            bi = k0 + g0 + u;
          }
        }
      }
    }
    if constexpr (kBest) {
      best_lnl[site] = bl;
      best_idx[site] = bi;
      if (out) acc += (double)wgt_at(wgt, site, partials) * bl;
    }
  }
  if constexpr (kBest) {
    if (out) lnl_finish(acc, partials, ticket, out, nullptr, 0);  // uniform: a kernel argument
  }
}

// The scan's set-up: tip t of the launch (blockIdx.y < count) tiled G times,
// dst[g*n + i] = src[i]; blockIdx.y == count (launched when cat != NULL): the
// category bytes cat[g*n + i] = g.
struct PsrTileDesc {
  const uint8_t *src;
  uint8_t *dst;
};
struct PsrTileBatch {
  PsrTileDesc d[kMaxBatch];
};

#ifndef PLFX_PSR_NO_TILE_KERNEL  // a translation unit that only borrows this header's device functions
__global__ void __launch_bounds__(kBlock)
psr_tile_kernel(const PsrTileBatch tips, int count, int64_t n, int G, uint8_t *__restrict__ cat) {
  const int64_t total = (int64_t)G * n;
  const int64_t step = (int64_t)gridDim.x * kBlock;
  const bool is_cat = (int)blockIdx.y >= count;
  const PsrTileDesc &d = tips.d[is_cat ? 0 : blockIdx.y];
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < total; v += step) {
    const int64_t g = v / n;
    if (is_cat) cat[v] = (uint8_t)g;
    else d.dst[v] = d.src[v - g * n];
  }
}
#endif

}  // namespace dev
}  // namespace plfx
