// plf_psr_branch.hpp -- device code of plfx.h section 13: the outer CLVs and
// sum tables of the two branches below one op of a per-site-rate DNA tree in
// one pass, and the integer pass that turns the scaler sums into one count per
// branch.
//
// Fused sibling pair, op (v, c1, c2): the lane that owns a site reads W(v),
// x_c1 and x_c2 once, forms
//   umpU = Pup  * W(v)     umpA = P_c1 * x_c1     umpB = P_c2 * x_c2
// and from them both outer CLVs, each with its own rescale test,
//   W(c1) = EV^T (umpU o umpB)        W(c2) = EV^T (umpU o umpA)
// in plf_psr_kernel's operation order (ump from +0.0 ascending l, the product
// rounded once, the EV sum from +0.0 ascending k; no contraction), and both
// tables x_c o W(c), one multiply rounded in T.  Every value is what one
// plf_psr_kernel launch per W and one edge_sumtable_psr launch per table
// write: 3 CLV reads + 4 writes per site instead of 8 + 4.  A coded child
// (kTips 1: c1; 2: both -- the lowering puts the coded child first) is a code
// byte; its ump comes from the (category, code) table psr_tip_table forms of
// its matrix, its table side from tipvec, and its W is never written.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "plf_psr.hpp"

namespace plfx {
namespace dev {

struct BranchPairDesc {
  const void *wv, *c1, *c2;
  const void *pup, *p1, *p2;
  void *w1, *w2, *t1, *t2;
  int64_t *ss1, *ss2;
};
constexpr int kMaxPairs = 16;
struct BranchPairBatch {
  BranchPairDesc d[kMaxPairs];
};

// Two independent sums (consecutive kWsWords regions of ws), published by
// threads 0 and 1 in parallel (block_ticket_sum3 for two).
__device__ inline void block_ticket_sum2(long long v0, long long v1, unsigned long long *wsu, int64_t *o0,
                                         int64_t *o1) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v0 += __shfl_xor(v0, off);
    v1 += __shfl_xor(v1, off);
  }
  __shared__ long long part2[2][kWavesPerBlock];
  if ((threadIdx.x & 63) == 0) {
    part2[0][threadIdx.x >> 6] = v0;
    part2[1][threadIdx.x >> 6] = v1;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= 2) return;
  long long tot = 0;
#pragma unroll
  for (int i = 0; i < kWavesPerBlock; i++) tot += part2[t][i];
  ticket_publish(tot, wsu + (size_t)t * kWsWords, t == 0 ? o0 : o1);
}

// ump[k] = sum_l x[l] * P[k][l] from the category's padded LDS row
template <typename T>
__device__ __forceinline__ void psr_ump(const T (&x)[4], const T *row, T (&u)[4]) {
  T P[16];
  psr_lds_row<T, 16>(row, P);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    u[k] = T(0);
#pragma unroll
    for (int l = 0; l < 4; l++) u[k] += x[l] * P[k * 4 + l];
  }
}

// o = EV^T (u1 o u2) with the 2^-32 rescale; returns the site's scale flag
template <typename T>
__device__ __forceinline__ bool psr_outer(const T (&u1)[4], const T (&u2)[4], const T (&E)[16], T m, T (&o)[4]) {
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

// LDS: Pup's padded matrix table, per child a padded matrix table (dense) or a
// (category, code) table (coded), and tipvec's 64 values when a child is
// coded -- in f64 13.5 KB (kTips 0), 25.5 KB (1), 37.5 KB (2), half in f32.
template <typename T, int kTips>
struct PsrBranchLds {
  static constexpr int kMat = kPsrMaxCats * PsrRow<T>::kStride;
  static constexpr int kTab = kPsrMaxCats * 64;
  static constexpr int kSide1 = kTips >= 1 ? kTab : kMat, kSide2 = kTips == 2 ? kTab : kMat;
  static constexpr int kTipvec = kTips >= 1 ? 64 : 0;
  static constexpr int kValues = kMat + kSide1 + kSide2 + kTipvec;
};

// Up to kMaxPairs ops per launch, op = blockIdx.y, two consecutive ticket
// regions of ws each.  One lane per site, U sites per lane and trip, all their
// loads issued first (clamped to the last site, results unused past n).
template <typename T, int U, bool kSum, int kTips>
__global__ void __launch_bounds__(kBlock)
psr_branch_pair_kernel(const BranchPairBatch pb, const T *__restrict__ EV, const uint8_t *__restrict__ rate_cat,
                       int ncat, const int32_t *__restrict__ wgt, int64_t n, unsigned long long *ws,
                       const T *__restrict__ tipvec) {
  constexpr bool T1 = kTips >= 1, T2 = kTips == 2;
  constexpr int kStride = PsrRow<T>::kStride;
  using Lds = PsrBranchLds<T, kTips>;
  const BranchPairDesc &d = pb.d[blockIdx.y];

  __shared__ __attribute__((aligned(16))) T lds[Lds::kValues];
  T *const sU = lds, *const s1 = sU + Lds::kMat, *const s2 = s1 + Lds::kSide1, *const stv = s2 + Lds::kSide2;
  psr_stage<T>((const T *)d.pup, ncat, sU);
  if constexpr (T1) psr_tip_table<T>((const T *)d.p1, tipvec, ncat, s1);
  else psr_stage<T>((const T *)d.p1, ncat, s1);
  if constexpr (T2) psr_tip_table<T>((const T *)d.p2, tipvec, ncat, s2);
  else psr_stage<T>((const T *)d.p2, ncat, s2);
  if constexpr (T1) {
    if (threadIdx.x < 64) stv[threadIdx.x] = tipvec[threadIdx.x];
  }
  __syncthreads();

  T E[16];
#pragma unroll
  for (int i = 0; i < 16; i++) E[i] = EV[i];  // uniform: scalar loads
  const T m = Num<T>::minlik();
  const T *__restrict__ xv = (const T *)d.wv;
  const T *__restrict__ x1 = (const T *)d.c1, *__restrict__ x2 = (const T *)d.c2;
  const uint8_t *__restrict__ tip1 = (const uint8_t *)d.c1, *__restrict__ tip2 = (const uint8_t *)d.c2;
  T *__restrict__ w1 = (T *)d.w1, *__restrict__ w2 = (T *)d.w2;
  T *__restrict__ t1 = (T *)d.t1, *__restrict__ t2 = (T *)d.t2;

  long long acc1 = 0, acc2 = 0;
  const int64_t stride = (int64_t)gridDim.x * (kBlock * U);
  const int64_t nlast = n - 1;
  for (int64_t base = (int64_t)blockIdx.x * (kBlock * U); base < n; base += stride) {
    T v[U][4], a[U][4], b[U][4];
    int cat[U], k1[U], k2[U], w[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t site = base + u * kBlock + threadIdx.x;
      const int64_t ld = site < n ? site : nlast;
      cat[u] = rate_cat[ld];
      Num<T>::template load4<true>(xv + ld * 4, v[u]);
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
      T uU[4], uA[4], uB[4];
      psr_ump<T>(v[u], sU + c * kStride, uU);
      if constexpr (T1) {
        psr_lds_row<T, 4>(s1 + (c * 16 + k1[u]) * 4, uA);
        psr_lds_row<T, 4>(stv + k1[u] * 4, a[u]);  // the coded child's side of its table
      } else {
        psr_ump<T>(a[u], s1 + c * kStride, uA);
      }
      if constexpr (T2) {
        psr_lds_row<T, 4>(s2 + (c * 16 + k2[u]) * 4, uB);
        psr_lds_row<T, 4>(stv + k2[u] * 4, b[u]);
      } else {
        psr_ump<T>(b[u], s2 + c * kStride, uB);
      }
      T o1[4], o2[4];
      const bool sc1 = psr_outer<T>(uU, uB, E, m, o1);
      const bool sc2 = psr_outer<T>(uU, uA, E, m, o2);
      T q1[4], q2[4];
#pragma unroll
      for (int l = 0; l < 4; l++) {
        q1[l] = a[u][l] * o1[l];
        q2[l] = b[u][l] * o2[l];
      }
      if (site < n) {
        if constexpr (!T1) Num<T>::store4_nt(w1 + site * 4, o1);
        if constexpr (!T2) Num<T>::store4_nt(w2 + site * 4, o2);
        Num<T>::store4_nt(t1 + site * 4, q1);
        Num<T>::store4_nt(t2 + site * 4, q2);
        if (kSum) {
          acc1 += sc1 ? (long long)w[u] : 0ll;
          acc2 += sc2 ? (long long)w[u] : 0ll;
        }
      }
    }
  }
  if constexpr (kSum) block_ticket_sum2(acc1, acc2, ws + (size_t)blockIdx.y * 2 * kWsWords, d.ss1, d.ss2);
}

// ---- the counters ----
// One block, thread t = op first + t of a chunk of the op list.  The values a
// chunk needs of other chunks come from global memory (an earlier launch wrote
// them), the chain inside the chunk runs in LDS in thread 0: integer sums,
// exact in any order.
//   sub[j]         = scaler_sums[j] + sub[w1] + sub[w2]               (ops ascending)
//   outer[2j + s]  = wsum[2j + s] + outer[up] + sub[sibling of s]     (ops descending; the root op: sub[sibling])
//   edge_scale[e]  = outer[e] + sub[child of e]
struct BranchScaleDesc {
  int32_t w1, w2, up;
};
constexpr int kScaleChunk = 256;
struct BranchScaleBatch {
  BranchScaleDesc d[kScaleChunk];
};
static_assert(kScaleChunk == kBlock, "one thread per op of a chunk");

__global__ void __launch_bounds__(kBlock)
psr_branch_sub_kernel(const BranchScaleBatch sb, int first, int count, const int64_t *__restrict__ scaler_sums,
                      int64_t *sub) {
  __shared__ long long a[kScaleChunk];
  const int t = threadIdx.x;
  if (t < count) {
    const BranchScaleDesc d = sb.d[t];
    long long v = scaler_sums[first + t];
    if (d.w1 >= 0 && d.w1 < first) v += sub[d.w1];
    if (d.w2 >= 0 && d.w2 < first) v += sub[d.w2];
    a[t] = v;
  }
  __syncthreads();
  if (t == 0) {
    for (int i = 0; i < count; i++) {
      const BranchScaleDesc d = sb.d[i];
      long long v = a[i];
      if (d.w1 >= first) v += a[d.w1 - first];
      if (d.w2 >= first) v += a[d.w2 - first];
      a[i] = v;
    }
  }
  __syncthreads();
  if (t < count) sub[first + t] = a[t];
}

__global__ void __launch_bounds__(kBlock)
psr_branch_scale_kernel(const BranchScaleBatch sb, int first, int count, const int64_t *__restrict__ wsum,
                        const int64_t *__restrict__ sub, int64_t *outer, int64_t *__restrict__ edge_scale) {
  __shared__ long long b[2][kScaleChunk];
  const int t = threadIdx.x, j = first + t;
  long long s1 = 0, s2 = 0;
  if (t < count) {
    const BranchScaleDesc d = sb.d[t];
    if (d.w1 >= 0) s1 = sub[d.w1];
    if (d.w2 >= 0) s2 = sub[d.w2];
    long long o1 = s2, o2 = s1;
    if (d.up >= 0) {
      o1 += wsum[2 * j];
      o2 += wsum[2 * j + 1];
      if ((d.up >> 1) >= first + count) {
        const long long o = outer[d.up];
        o1 += o;
        o2 += o;
      }
    }
    b[0][t] = o1;
    b[1][t] = o2;
  }
  __syncthreads();
  if (t == 0) {
    for (int i = count - 1; i >= 0; i--) {
      const int up = sb.d[i].up;
      if (up >= 0 && (up >> 1) < first + count) {
        const long long o = b[up & 1][(up >> 1) - first];
        b[0][i] += o;
        b[1][i] += o;
      }
    }
  }
  __syncthreads();
  if (t < count) {
    outer[2 * j] = b[0][t];
    outer[2 * j + 1] = b[1][t];
    edge_scale[2 * j] = b[0][t] + s1;
    edge_scale[2 * j + 1] = b[1][t] + s2;
  }
}

}  // namespace dev
}  // namespace plfx
