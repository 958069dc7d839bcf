// plf_psr_prot.hpp -- device code of the protein per-site-rate (PSR, "CAT")
// mode, plfx.h section 11b: a CLV is x[site*20 + state], n * 20 values, and a
// site's two 20 x 20 matrices are chosen by its category byte,
// c = min(rate_cat[site], ncat - 1).
//
// Node update, plf()'s loop with one category and no contraction:
//   umpL[k]  = sum_l x1[i][l] * left[c*400 + k*20 + l]   (from +0.0, ascending l)
//   x3[i][l] = sum_k (umpL[k] * umpR[k]) * EV[20k + l]   (from +0.0, ascending k)
// then the 2^-32 rescale over the site's twenty values.
//
// The DNA kernel (plf_psr.hpp) stages both matrix tables in LDS and every lane
// reads its category's rows.  That does not carry over: 32 categories x 2
// sides x 400 f64 are 200 KB.  The matrices stay what they are in the Gamma
// protein kernels (plf_prot_valu.hpp) -- wave-uniform scalar operands -- and
// the category is made wave-uniform by looping over it:
//   * one lane owns one site, a wave 64 consecutive sites, a block 4 waves =
//     256 sites per trip; the waves of a block share nothing but the coded
//     children's tip table and the final sum, so no trip has a block barrier;
//   * a dense child's 64 rows reach the lanes through the wave's LDS tile:
//     coalesced 16-B non-temporal loads, rows of 10 (f64) / 5 (f32) chunks at
//     an odd chunk stride (11 / 5), so the lanes' ds_read_b128 of their own
//     rows are conflict-free; a coded child's row is gathered from the 24 x 20
//     tip table the block stages once (rows at the same odd stride).  The
//     arithmetic on a gathered row is the dense child's: bit-identical by
//     construction, with no (category, code) table;
//   * per side: todo = the lanes whose site is < n; while todo != 0, c = the
//     category of todo's first lane (a scalar), the lanes of that category run
//     the twenty dot products against P + c*400 (scalar loads, SGPR operands,
//     the chains of plf_prot_valu.hpp's exact mode) and leave todo;
//   * phase 3 (EV, wave-uniform) runs once for all lanes; the scale test is
//     the lane's own twenty values; x3 leaves through the tile, coalesced.
// A wave whose 64 sites share a category makes one pass per side, a wave with
// k distinct categories k: correct for any site order, fast for sites sorted
// by category (plfx_psr_site_order).
//
// At the end of the file: the branch-length half (plfx.h section 11c) -- the
// sum table, one and batched, the three edge sums and the branch-length loop
// on the device, over tables of n * 20 values -- and the rate scan's per-site
// lnL and argmax kernel (section 12b).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#define PLFX_SECONDARY_TU  // plf_dna.hpp's non-template kernel lives in plf_kernels.hip
#include "plf_edge.hpp"
#include "plf_lnl.hpp"
#include "plf_prot.hpp"

namespace plfx {
namespace dev {

constexpr int kPsrProtMaxCats = 32;  // PLFX_PSR_MAX_CATS (asserted in plfx_api.hip)

__device__ __forceinline__ int psr_prot_cat(int byte, int ncat) { return byte < ncat ? byte : ncat - 1; }

template <typename T>
struct PsrProtTile {
  static constexpr int kChunksPerSite = 20 * (int)sizeof(T) / 16;  // 10 (f64) / 5 (f32)
  static constexpr int kStride = kChunksPerSite | 1;               // odd: 11 / 5
  static constexpr int kChunks = 64 * kStride;                     // of one wave's tile
  static constexpr int kTabChunks = kProtCodes * kStride;          // of the tip table
  using V = std::conditional_t<sizeof(T) == 8, f64x2, f32x4>;
};

// The waves of a block work on their own tiles: what orders a wave's LDS
// writes before the reads of its other lanes is the wave's own program order,
// which this keeps the compiler from changing.
__device__ __forceinline__ void psr_prot_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The wave's 64 rows from wbase on into its tile: chunk j = lane + 64 i is
// site j / kChunksPerSite's chunk j % kChunksPerSite, all loads issued before
// the first LDS write.  The chunks of sites past n are zero (never used).
template <typename T>
__device__ __forceinline__ void psr_prot_tile_load(const T *__restrict__ g, int64_t wbase, int64_t n, int lane,
                                                   typename PsrProtTile<T>::V *tile) {
  using PT = PsrProtTile<T>;
  using V = typename PT::V;
  const V *src = reinterpret_cast<const V *>(g) + wbase * PT::kChunksPerSite + lane;
  V v[PT::kChunksPerSite];
  if (wbase + 64 <= n) {
#pragma unroll
    for (int i = 0; i < PT::kChunksPerSite; i++) v[i] = __builtin_nontemporal_load(src + 64 * i);
  } else {
    const int lim = (int)(n - wbase) * PT::kChunksPerSite;  // chunks of valid sites
#pragma unroll
    for (int i = 0; i < PT::kChunksPerSite; i++) {
      v[i] = V{};
      if (lane + 64 * i < lim) v[i] = __builtin_nontemporal_load(src + 64 * i);
    }
  }
#pragma unroll
  for (int i = 0; i < PT::kChunksPerSite; i++) {
    const int j = lane + 64 * i, s = j / PT::kChunksPerSite, q = j - s * PT::kChunksPerSite;
    tile[s * PT::kStride + q] = v[i];
  }
}

template <typename T>
__device__ __forceinline__ void psr_prot_tile_store(T *__restrict__ g, int64_t wbase, int64_t n, int lane,
                                                    const typename PsrProtTile<T>::V *tile) {
  using PT = PsrProtTile<T>;
  using V = typename PT::V;
  V *dst = reinterpret_cast<V *>(g) + wbase * PT::kChunksPerSite + lane;
  V v[PT::kChunksPerSite];
#pragma unroll
  for (int i = 0; i < PT::kChunksPerSite; i++) {
    const int j = lane + 64 * i, s = j / PT::kChunksPerSite, q = j - s * PT::kChunksPerSite;
    v[i] = tile[s * PT::kStride + q];
  }
  if (wbase + 64 <= n) {
#pragma unroll
    for (int i = 0; i < PT::kChunksPerSite; i++) __builtin_nontemporal_store(v[i], dst + 64 * i);
  } else {
    const int lim = (int)(n - wbase) * PT::kChunksPerSite;
#pragma unroll
    for (int i = 0; i < PT::kChunksPerSite; i++)
      if (lane + 64 * i < lim) __builtin_nontemporal_store(v[i], dst + 64 * i);
  }
}

// psr_prot_tile_load in two steps, for a loop that keeps its next tile in
// flight in registers while it works on this one (the edge sums below): the
// same chunks from the same addresses into v, then v into the tile.
template <typename T>
__device__ __forceinline__ void psr_prot_tile_fetch(const T *__restrict__ g, int64_t wbase, int64_t n, int lane,
                                                    typename PsrProtTile<T>::V (&v)[PsrProtTile<T>::kChunksPerSite]) {
  using PT = PsrProtTile<T>;
  using V = typename PT::V;
  const V *src = reinterpret_cast<const V *>(g) + wbase * PT::kChunksPerSite + lane;
  if (wbase + 64 <= n) {
#pragma unroll
    for (int i = 0; i < PT::kChunksPerSite; i++) v[i] = __builtin_nontemporal_load(src + 64 * i);
  } else {
    const int lim = (int)(n - wbase) * PT::kChunksPerSite;  // chunks of valid sites
#pragma unroll
    for (int i = 0; i < PT::kChunksPerSite; i++) {
      v[i] = V{};
      if (lane + 64 * i < lim) v[i] = __builtin_nontemporal_load(src + 64 * i);
    }
  }
}

template <typename T>
__device__ __forceinline__ void psr_prot_tile_put(
    const typename PsrProtTile<T>::V (&v)[PsrProtTile<T>::kChunksPerSite], int lane,
    typename PsrProtTile<T>::V *tile) {
  using PT = PsrProtTile<T>;
#pragma unroll
  for (int i = 0; i < PT::kChunksPerSite; i++) {
    const int j = lane + 64 * i, s = j / PT::kChunksPerSite, q = j - s * PT::kChunksPerSite;
    tile[s * PT::kStride + q] = v[i];
  }
}

// a row of 20 values at an LDS chunk address <-> registers
template <typename T>
__device__ __forceinline__ void psr_prot_row_read(const typename PsrProtTile<T>::V *r, T (&v)[20]) {
  constexpr int kVals = 16 / (int)sizeof(T);
#pragma unroll
  for (int i = 0; i < PsrProtTile<T>::kChunksPerSite; i++) {
    const typename PsrProtTile<T>::V t = r[i];
#pragma unroll
    for (int e = 0; e < kVals; e++) v[i * kVals + e] = t[e];
  }
}

template <typename T>
__device__ __forceinline__ void psr_prot_row_write(typename PsrProtTile<T>::V *r, const T (&v)[20]) {
  constexpr int kVals = 16 / (int)sizeof(T);
#pragma unroll
  for (int i = 0; i < PsrProtTile<T>::kChunksPerSite; i++) {
    typename PsrProtTile<T>::V t;
#pragma unroll
    for (int e = 0; e < kVals; e++) t[e] = v[i * kVals + e];
    r[i] = t;
  }
}

// fn(k, sum_l x[l] * P[k][l]) for the twenty rows k: plf()'s separate multiply
// and add from +0.0 (kept: +0.0 + -0.0 is +0.0), ascending l; P is
// wave-uniform (scalar loads, SGPR operands), kRows chains side by side and
// kCols columns of operands loaded ahead, as plf_prot_valu.hpp's exact mode.
// The matrix is read through a constant-address-space pointer: the node's
// matrices come from the descriptor, not from a __restrict__ kernel argument,
// and without this the compiler cannot rule out that a store of the kernel
// changes them -- it then reads them with 400 vector loads per side and pass
// instead of scalar ones.  (They are inputs: no launch writes them.)
template <typename T, int kRows, int kCols, typename F>
__device__ __forceinline__ void psr_prot_dot(const T *__restrict__ P, const T (&x)[20], F &&fn) {
  constexpr int S = 20;
  static_assert(S % kRows == 0 && S % kCols == 0, "row groups and column chunks divide 20");
  using CP = const T __attribute__((address_space(4))) *;
#pragma unroll
  for (int gk = 0; gk < S / kRows; gk++) {
    const CP G = reinterpret_cast<CP>(reinterpret_cast<uintptr_t>(P + gk * kRows * S));
    T u[kRows], cur[kRows][kCols], nxt[kRows][kCols];
#pragma unroll
    for (int j = 0; j < kRows; j++)
#pragma unroll
      for (int q = 0; q < kCols; q++) cur[j][q] = G[j * S + q];
#pragma unroll
    for (int lc = 0; lc < S; lc += kCols) {
      if (lc + kCols < S) {
#pragma unroll
        for (int j = 0; j < kRows; j++)
#pragma unroll
          for (int q = 0; q < kCols; q++) nxt[j][q] = G[j * S + lc + kCols + q];
      }
#pragma unroll
      for (int q = 0; q < kCols; q++) {
        T pr[kRows];
#pragma unroll
        for (int j = 0; j < kRows; j++) pr[j] = x[lc + q] * cur[j][q];
        pin_chains(pr);
#pragma unroll
        for (int j = 0; j < kRows; j++) u[j] = (lc + q == 0 ? T(0) : u[j]) + pr[j];
      }
      pin_chains(u);
#pragma unroll
      for (int j = 0; j < kRows; j++)
#pragma unroll
        for (int q = 0; q < kCols; q++) cur[j][q] = nxt[j][q];
    }
#pragma unroll
    for (int j = 0; j < kRows; j++) fn(gk * kRows + j, u[j]);
  }
}

// One side of a node for the wave's 64 sites: every lane of `valid` gets
// fn(k, ump[k]) exactly once, from the pass of its own category.
template <typename T, typename F>
__device__ __forceinline__ void psr_prot_side(const T *__restrict__ P, const T (&x)[20], int cat,
                                              unsigned long long valid, bool mine_valid, F &&fn) {
  unsigned long long todo = valid;
  while (todo) {
    const int first = __builtin_ctzll(todo);
    const int c = __builtin_amdgcn_readlane(cat, first);
    const bool mine = mine_valid && cat == c;
    // Inside the branch cat == c, and the compiler would replace the scalar c
    // by the lane's cat: the matrix address would be a vector, its reads
    // vector loads.  The empty asm keeps c a scalar of its own.
    int cs = c;
    asm volatile("" : "+s"(cs));
    if (mine) psr_prot_dot<T, 4, 2>(P + cs * 400, x, fn);
    todo &= ~__ballot(mine);
  }
}

// One node: x1 / x2 name the uint8 codes of a coded child (T1 / T2).  The
// pointers are __restrict__ parameters, so that the matrices stay scalar loads
// after the first store of a trip.
template <typename T, bool kSum, bool T1, bool T2>
__device__ __forceinline__ void psr_prot_body(const void *__restrict__ c1, const void *__restrict__ c2,
                                              T *__restrict__ x3, const T *__restrict__ EV,
                                              const T *__restrict__ left, const T *__restrict__ right,
                                              const uint8_t *__restrict__ rate_cat, int ncat,
                                              const int32_t *__restrict__ wgt, uint8_t *__restrict__ scaler,
                                              int64_t n, unsigned long long *ws, int64_t *scaler_sum,
                                              const T *__restrict__ tipvec) {
  constexpr int S = 20, kPh3 = 10;
  using PT = PsrProtTile<T>;
  using V = typename PT::V;
  const T *__restrict__ x1 = static_cast<const T *>(c1);
  const T *__restrict__ x2 = static_cast<const T *>(c2);
  const uint8_t *__restrict__ tip1 = static_cast<const uint8_t *>(c1);
  const uint8_t *__restrict__ tip2 = static_cast<const uint8_t *>(c2);

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  __shared__ V tiles[kWavesPerBlock * PT::kChunks];
  __shared__ V tab[(T1 || T2) ? PT::kTabChunks : 1];
  V *const tile = tiles + wave * PT::kChunks;
  if constexpr (T1 || T2) {
    T *t = reinterpret_cast<T *>(tab);
    constexpr int kRowVals = PT::kStride * 16 / (int)sizeof(T);
    for (int e = threadIdx.x; e < kProtCodes * S; e += kBlock) {
      const int code = e / S, l = e - code * S;
      t[code * kRowVals + l] = prot_tip_value<T>(tipvec, code, l);
    }
    __syncthreads();
  }
  const T m = Num<T>::minlik();

  long long acc = 0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += stride) {
    const int64_t wbase = base + wave * 64;
    if (wbase >= n) continue;  // wave-uniform: none of the wave's sites exists
    const int64_t site = wbase + lane;
    const bool in = site < n;
    const int64_t ld = in ? site : n - 1;
    const int cat = psr_prot_cat(rate_cat[ld], ncat);
    const int w = kSum ? wgt_at(wgt, ld, ws) : 0;
    const unsigned long long valid = __ballot(in);

    T U[S];
    {
      T a[S];
      if constexpr (T1) {
        psr_prot_row_read<T>(tab + prot_code(tip1[ld]) * PT::kStride, a);
      } else {
        psr_prot_tile_load<T>(x1, wbase, n, lane, tile);
        psr_prot_wave_sync();
        psr_prot_row_read<T>(tile + lane * PT::kStride, a);
        psr_prot_wave_sync();  // every lane holds its row before the tile is written again
      }
      psr_prot_side<T>(left, a, cat, valid, in, [&](int k, T u) { U[k] = u; });
    }
    {
      T b[S];
      if constexpr (T2) {
        psr_prot_row_read<T>(tab + prot_code(tip2[ld]) * PT::kStride, b);
      } else {
        psr_prot_tile_load<T>(x2, wbase, n, lane, tile);
        psr_prot_wave_sync();
        psr_prot_row_read<T>(tile + lane * PT::kStride, b);
        psr_prot_wave_sync();
      }
      psr_prot_side<T>(right, b, cat, valid, in, [&](int k, T u) { U[k] = U[k] * u; });  // umpL[k] * umpR[k]
    }
    if (!in) {
#pragma unroll
      for (int k = 0; k < S; k++) U[k] = T(0);  // a lane without a site took no part
    }
    // phase 3: O[l] = sum_k U[k] * EV[k][l], separate multiply and add, from +0.0
    T O[S];
    {
      T tok = T(0);
#pragma unroll
      for (int h = 0; h < S / kPh3; h++) {
        T v[kPh3];
#pragma unroll
        for (int j = 0; j < kPh3; j++) v[j] = T(0);
#pragma unroll
        for (int k = 0; k < S; k++) {
          int so = 0;
          asm volatile("" : "+s"(so) : "v"(tok));  // EV row k after the previous row's chains
          const T *er = EV + so + k * S + h * kPh3;
          T pr[kPh3];
#pragma unroll
          for (int j = 0; j < kPh3; j++) pr[j] = U[k] * er[j];
          pin_chains(pr);
#pragma unroll
          for (int j = 0; j < kPh3; j++) v[j] += pr[j];
          pin_chains(v);
          tok = v[kPh3 - 1];
        }
#pragma unroll
        for (int j = 0; j < kPh3; j++) O[h * kPh3 + j] = v[j];
      }
    }
    bool sc = in;
#pragma unroll
    for (int l = 0; l < S; l++) sc = sc && (Num<T>::abs(O[l]) < m);
#pragma unroll
    for (int l = 0; l < S; l++) {
      const T s = O[l] * Num<T>::two32();  // exact: power-of-two scaling
      O[l] = sc ? s : O[l];
    }
    psr_prot_row_write<T>(tile + lane * PT::kStride, O);
    if (in) {
      if (scaler) scaler[site] = (uint8_t)sc;
      if (kSum) acc += sc ? (long long)w : 0ll;
    }
    psr_prot_wave_sync();
    psr_prot_tile_store<T>(x3, wbase, n, lane, tile);
    psr_prot_wave_sync();  // the tile is the next trip's
  }
  if constexpr (kSum) block_ticket_sum(acc, ws, scaler_sum);
}

// Up to kMaxBatch nodes per launch, node = blockIdx.y, sharing EV, n, wgt and
// rate_cat; T1 / T2: child 1 / 2 of every node of the launch is coded (the
// descriptor's x1 / x2 then point at uint8 codes).  kSum: some node of the
// launch wants its weighted scaler sum.  Each node has its own ticket region.
// 3 waves per SIMD: what the f64 tiles of a CU's blocks allow (3 x 45-49 KB of
// 160 KB), and 168 VGPRs; f32 spills when it is held to the 128 of 4 waves.
constexpr int kPsrProtMinWaves = 3;

template <typename T, bool kSum, bool T1, bool T2>
__global__ void __launch_bounds__(kBlock, kPsrProtMinWaves)
plf_psr_prot_kernel(const NodeBatch nodes, const T *__restrict__ EV, const uint8_t *__restrict__ rate_cat,
                    int ncat, const int32_t *__restrict__ wgt, int64_t n, unsigned long long *ws,
                    const T *__restrict__ tipvec) {
  const NodeDesc &d = nodes.d[blockIdx.y];
  psr_prot_body<T, kSum, T1, T2>(d.x1, d.x2, static_cast<T *>(d.x3), EV, static_cast<const T *>(d.left),
                                 static_cast<const T *>(d.right), rate_cat, ncat, wgt, d.scaler, n,
                                 ws + (size_t)blockIdx.y * kWsWords, d.scaler_sum, tipvec);
}

// Root lnL of a protein PSR CLV: L_i = sum_s freq[s] * x[i][s] (from +0.0,
// ascending s, in f64), one lane per site, its row read as 16-B chunks; the
// sum over the sites through plf_lnl.hpp's fixed-order reduction, as
// plf_psr.hpp root_lnl_psr_kernel.
template <typename T>
__global__ void __launch_bounds__(kBlock)
root_lnl_psr_prot_kernel(const T *__restrict__ x, int64_t n, const double *__restrict__ freq,
                         const int32_t *__restrict__ wgt, const int64_t *__restrict__ scaler_sums, int nsums,
                         double *partials, unsigned long long *ticket, double *out,
                         double *__restrict__ site_lnl) {
  using PT = PsrProtTile<T>;
  using V = typename PT::V;
  constexpr int kVals = 16 / (int)sizeof(T);
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t nlast = n - 1;
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += stride) {
    const int64_t site = base + threadIdx.x;
    const int64_t ld = site < n ? site : nlast;
    const V *row = reinterpret_cast<const V *>(x) + ld * PT::kChunksPerSite;
    V v[PT::kChunksPerSite];
#pragma unroll
    for (int i = 0; i < PT::kChunksPerSite; i++) v[i] = __builtin_nontemporal_load(row + i);
    const int w = wgt_at(wgt, ld, partials);
    double L = 0.0;
#pragma unroll
    for (int s = 0; s < 20; s++) L += (freq ? freq[s] : 0.05) * (double)v[s / kVals][s % kVals];
    if (site < n) {
      const double l = log(L);
      if (site_lnl) site_lnl[site] = l;
      acc += (double)w * l;
    }
  }
  lnl_finish(acc, partials, ticket, out, scaler_sums, nsums);
}

// ---- plfx.h section 11c: the branch-length half ----
//
// Sum table of a protein PSR branch: x1 * x2 over n * 20 values, 16-B chunks,
// 10 (f64) / 5 (f32) per site, U chunks per thread and trip, all of a trip's
// loads issued before its stores (plf_psr.hpp edge_sumtable_psr_chunks with 20
// states).  kTip: side 1 is one code per site, x1[i][k] =
// tipvec[min(code, 23)*20 + k].
template <typename T, bool kTip>
__device__ __forceinline__ void edge_sumtable_psr_prot_chunks(const void *__restrict__ x1,
                                                              const T *__restrict__ x2, int64_t n,
                                                              const T *__restrict__ tipvec,
                                                              T *__restrict__ out) {
  using V = typename PsrProtTile<T>::V;
  constexpr int kVals = 16 / (int)sizeof(T);
  constexpr int kSite = PsrProtTile<T>::kChunksPerSite;
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
        const T *tv = tipvec + prot_code(codes[site]) * 20 + (int)(j - site * kSite) * kVals;
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
edge_sumtable_psr_prot_kernel(const void *__restrict__ x1, const T *__restrict__ x2, int64_t n,
                              const T *__restrict__ tipvec, T *__restrict__ out) {
  edge_sumtable_psr_prot_chunks<T, kTip>(x1, x2, n, tipvec, out);
}

// Up to kMaxBatch sum tables per launch, edge = blockIdx.y, all with the same
// kind of side 1: each edge's table is the one-edge kernel's, chunk for chunk
// (plf_psr.hpp PsrEdgeBatch; the host's PsrEdgeDescH).
struct PsrProtEdgeDesc {
  const void *x1, *x2;
  void *out;
};
struct PsrProtEdgeBatch {
  PsrProtEdgeDesc d[kMaxBatch];
};

template <typename T, bool kTip>
__global__ void __launch_bounds__(kBlock)
edge_sumtable_psr_prot_batch_kernel(const PsrProtEdgeBatch edges, int64_t n, const T *__restrict__ tipvec) {
  const PsrProtEdgeDesc &d = edges.d[blockIdx.y];
  edge_sumtable_psr_prot_chunks<T, kTip>(d.x1, static_cast<const T *>(d.x2), n, tipvec, static_cast<T *>(d.out));
}

// The three edge sums of a protein PSR branch.  x_k = lambda_k * rates[c_i];
// the block forms the ncat x 20 factor triples {e, e x, e x x} once from the
// device t into LDS (edge_factors: the bits of the Gamma and DNA kernels), a
// category's row as e[0..20), e x[0..20), e x x[0..20): 60 doubles padded to 62
// = 31 16-B slots, odd, as plf_psr.hpp pads 12 to 14.  One lane owns one site,
// a wave 64 consecutive sites.  The wave's 64 rows reach the lanes through its
// LDS tile, as the node's dense children do (coalesced 16-B non-temporal
// loads, no block barrier in a trip), with the next tile's chunks in flight in
// registers meanwhile: read straight from global -- one 16-B load per lane at a
// 160-B lane stride, root_lnl_psr_prot_kernel's way -- the kernel took as long
// as the Gamma-4 kernel takes for four times the values.
// A lane reads its category's row two factors at a time; lanes of one category
// read the same addresses (broadcast), so a wave of category-sorted sites reads
// without a conflict.  L, L1, L2 = sum_k st[i][k] * {e, e x, e x x} from +0.0,
// ascending k, in f64; the sums over the sites as plf_edge.hpp's (edge_site,
// lnl_finish<3>).  Lane and trip of a site are what they were in the direct
// form, so every sum has the same bits.
//
// edge_deriv_psr_prot_sites: the block's factor table at branch length t and
// its share of the sites into acc (blocks along x): the body of
// edge_deriv_psr_prot_kernel and of edge_opt_psr_prot_kernel.  partials: only
// a readable word here (wgt_at's dummy).
constexpr int kPsrProtFactorStride = 62;
template <typename T>
__device__ __forceinline__ void edge_deriv_psr_prot_sites(const T *__restrict__ st, int64_t n,
                                                          const double *__restrict__ lambda,
                                                          const double *__restrict__ rates, int ncat,
                                                          const uint8_t *__restrict__ rate_cat,
                                                          const int32_t *__restrict__ wgt, const double t,
                                                          const double *partials, double *__restrict__ site_lnl,
                                                          double (&acc)[3]) {
  constexpr int S = 20;
  using PT = PsrProtTile<T>;
  using V = typename PT::V;
  static_assert(kPsrProtFactorStride >= 3 * S && kPsrProtFactorStride % 2 == 0 && (kPsrProtFactorStride / 2) % 2 == 1,
                "a row is whole 16-B slots, an odd number of them");
  __shared__ __attribute__((aligned(16))) double tab[kPsrProtMaxCats * kPsrProtFactorStride];
  for (int i = threadIdx.x; i < ncat * S; i += kBlock) {
    const int c = i / S, k = i - c * S;
    double e0, e1, e2;
    edge_factors(lambda[k], rates[c], t, e0, e1, e2);
    tab[c * kPsrProtFactorStride + k] = e0;
    tab[c * kPsrProtFactorStride + S + k] = e1;
    tab[c * kPsrProtFactorStride + 2 * S + k] = e2;
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  __shared__ V tiles[kWavesPerBlock * PT::kChunks];
  V *const tile = tiles + wave * PT::kChunks;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t nlast = n - 1;
  int64_t wbase = (int64_t)blockIdx.x * kBlock + wave * 64;  // wave-uniform, as the loop's trip count
  V pf[PT::kChunksPerSite];
  if (wbase < n) psr_prot_tile_fetch<T>(st, wbase, n, lane, pf);
  for (; wbase < n; wbase += stride) {
    const int64_t site = wbase + lane;
    const int64_t ld = site < n ? site : nlast;
    const int cat = rate_cat[ld];
    const int w = wgt_at(wgt, ld, partials);
    psr_prot_tile_put<T>(pf, lane, tile);
    psr_prot_wave_sync();
    if (wbase + stride < n) psr_prot_tile_fetch<T>(st, wbase + stride, n, lane, pf);
    T v[S];
    psr_prot_row_read<T>(tile + lane * PT::kStride, v);
    psr_prot_wave_sync();  // every lane holds its row before the tile is written again
    const f64x2 *f = reinterpret_cast<const f64x2 *>(tab + psr_prot_cat(cat, ncat) * kPsrProtFactorStride);
    double L = 0.0, L1 = 0.0, L2 = 0.0;
#pragma unroll
    for (int p = 0; p < S / 2; p++) {
      const f64x2 f0 = f[p], f1 = f[S / 2 + p], f2 = f[S + p];
      const double xa = (double)v[2 * p], xb = (double)v[2 * p + 1];
      L += xa * f0.x;
      L1 += xa * f1.x;
      L2 += xa * f2.x;
      L += xb * f0.y;
      L1 += xb * f1.y;
      L2 += xb * f2.y;
    }
    if (site < n) {
      const double l = edge_site(L, L1, L2, w, acc);
      if (site_lnl) site_lnl[site] = l;
    }
  }
}

// n == 0: one block, out = {correction, 0, 0}.
template <typename T>
__global__ void __launch_bounds__(kBlock)
edge_deriv_psr_prot_kernel(const T *__restrict__ st, int64_t n, const double *__restrict__ lambda,
                           const double *__restrict__ rates, int ncat, const uint8_t *__restrict__ rate_cat,
                           const int32_t *__restrict__ wgt, const double *__restrict__ tp,
                           const int64_t *__restrict__ scaler_sums, int nsums, double *partials,
                           unsigned long long *ticket, double *out, double *__restrict__ site_lnl) {
  double acc[3] = {0.0, 0.0, 0.0};
  edge_deriv_psr_prot_sites<T>(st, n, lambda, rates, ncat, rate_cat, wgt, *tp, partials, site_lnl, acc);
  lnl_finish<3>(acc, partials, ticket, out, scaler_sums, nsums);
}

// The branch-length loop on the device for protein PSR branches
// (plfx_edge_optimize_psr_dev_gen): plf_psr.hpp's edge_opt_psr_kernel with the
// site loop above.  One launch = one evaluation of every edge of the group that
// has not stopped (blockIdx.y = edge, gridDim.x blocks per edge) and one step
// of its bracket in the thread that holds the edge's totals (edge_opt_entry,
// edge_opt_step, unchanged).  A stopped edge's blocks return before any
// barrier, LDS write, partial or ticket.
template <typename T>
__global__ void __launch_bounds__(kBlock)
edge_opt_psr_prot_kernel(const EdgeOptTabs tabs, int64_t n, const double *__restrict__ lambda,
                         const double *__restrict__ rates, int ncat, const uint8_t *__restrict__ rate_cat,
                         const int32_t *__restrict__ wgt, const double *t0, double tmin, double tmax,
                         int max_evals, int first, EdgeNewtonStep *state, double *partials,
                         unsigned long long *ws, double *t_opt, double *out3, int32_t *evals) {
  EdgeNewtonStep *sp = state + blockIdx.y;
  bool done;
  const double t = edge_opt_entry(sp, t0, tmin, tmax, first, done);
  if (done) return;
  const T *st = static_cast<const T *>(tabs.st[blockIdx.y]);
  double *part = partials + (size_t)blockIdx.y * 3 * gridDim.x;
  double acc[3] = {0.0, 0.0, 0.0};
  edge_deriv_psr_prot_sites<T>(st, n, lambda, rates, ncat, rate_cat, wgt, t, part, nullptr, acc);
  if (lnl_finish<3, false>(acc, part, ws + (size_t)blockIdx.y * kWsWords, nullptr, nullptr, 0))
    edge_opt_step(sp, acc, t, tmin, tmax, max_evals, first, t_opt, out3, evals);
}

// ---- plfx.h section 12b: the protein per-site rate scan ----
//
// plf_psr.hpp's psr_site_lnl_kernel for rows of 20 values: per-site lnL with
// the site's own scaling correction over a "virtual alignment" of G segments
// of n sites (virtual site g * n + i = site i under candidate k0 + g), and the
// running argmax over the candidates.  One lane owns site i, a wave 64
// consecutive sites, and the wave walks g with (best lnL, index) in registers:
//   L   = sum_s freq[s] * x[(g*n + i)*20 + s]   root_lnl_psr_prot_kernel's statement
//   cnt = sum_{j < nsc} (scalers[j*stride + g*n + i] != 0)
//   lnl = log(L) + (double)cnt * log(2^-32)     one multiply, one add
// The 64 rows of segment g (base x + g*n*20: n * 20 values are whole 16-B
// chunks, so every segment is 16-B aligned) reach the lanes through the wave's
// own LDS tile, as the edge sums' rows do: coalesced 16-B non-temporal loads,
// no block barrier in the loop, and candidate g + 1's chunks in flight in
// registers while the lanes reduce candidate g.  The scaler bytes of candidate
// g + 1 -- 64 consecutive bytes per wave and row -- are issued behind those
// chunks, kPsrProtScanRows rows at a time, all loads of a strip before its
// first use (clamped to the last row, counted only below nsc).  The kernel
// streams nsc + 20 * sizeof(T) bytes per virtual site.
// kBest, `first`, all_lnl, out: psr_site_lnl_kernel's rules, word for word --
// candidate k0 + g replaces (best_lnl, best_idx) iff lnl > best_lnl (ties keep
// the lower index, a NaN never wins), from (-inf, 0) when `first`; out != NULL
// (the last pass): out = sum_i wgt_i * best_lnl[i] through lnl_finish.
constexpr int kPsrProtScanRows = 8;

__device__ __forceinline__ int psr_prot_scaler_count(const uint8_t *__restrict__ scalers, int nsc, int64_t stride,
                                                     int64_t vs) {
  int cnt = 0;
  for (int j0 = 0; j0 < nsc; j0 += kPsrProtScanRows) {
    uint8_t b[kPsrProtScanRows];
#pragma unroll
    for (int u = 0; u < kPsrProtScanRows; u++) {
      const int j = j0 + u < nsc ? j0 + u : nsc - 1;
      b[u] = scalers[(int64_t)j * stride + vs];
    }
#pragma unroll
    for (int u = 0; u < kPsrProtScanRows; u++) cnt += (j0 + u < nsc && b[u] != 0) ? 1 : 0;
  }
  return cnt;
}

template <typename T, bool kBest>
__global__ void __launch_bounds__(kBlock)
psr_site_lnl_prot_kernel(const T *__restrict__ x, int64_t n, int G, const double *__restrict__ freq,
                         const uint8_t *__restrict__ scalers, int nsc, int64_t stride, int k0, int first,
                         double *__restrict__ all_lnl, double *best_lnl, int32_t *best_idx,
                         const int32_t *__restrict__ wgt, double *partials, unsigned long long *ticket,
                         double *out) {
  constexpr int S = 20;
  using PT = PsrProtTile<T>;
  using V = typename PT::V;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  __shared__ V tiles[kWavesPerBlock * PT::kChunks];
  V *const tile = tiles + wave * PT::kChunks;
  const int64_t seg = n * S;  // values of a segment
  const int64_t step = (int64_t)gridDim.x * kBlock;
  const int64_t nlast = n - 1;
  double acc = 0.0;
  for (int64_t wbase = (int64_t)blockIdx.x * kBlock + wave * 64; wbase < n; wbase += step) {  // wave-uniform
    const int64_t site = wbase + lane;
    const bool in = site < n;
    const int64_t ld = in ? site : nlast;
    double bl = -__builtin_inf();
    int bi = 0;
    if constexpr (kBest) {
      if (!first) {
        bl = best_lnl[ld];
        bi = best_idx[ld];
      }
    }
    V pf[PT::kChunksPerSite];
    psr_prot_tile_fetch<T>(x, wbase, n, lane, pf);
    int cnt_next = psr_prot_scaler_count(scalers, nsc, stride, ld);
    for (int g = 0; g < G; g++) {
      const int cnt = cnt_next;
      psr_prot_tile_put<T>(pf, lane, tile);
      psr_prot_wave_sync();
      if (g + 1 < G) {
        psr_prot_tile_fetch<T>(x + (int64_t)(g + 1) * seg, wbase, n, lane, pf);
        cnt_next = psr_prot_scaler_count(scalers, nsc, stride, (int64_t)(g + 1) * n + ld);
      }
      T v[S];
      psr_prot_row_read<T>(tile + lane * PT::kStride, v);
      psr_prot_wave_sync();  // every lane holds its row before the tile is written again
      double L = 0.0;
#pragma unroll
      for (int s = 0; s < S; s++) L += (freq ? freq[s] : 0.05) * (double)v[s];
      const double corr = (double)cnt * kLogMinLik;
      const double l = log(L) + corr;
      if (in) {
        if (all_lnl) all_lnl[(int64_t)(k0 + g) * n + site] = l;
        if (kBest && l > bl) {
          bl = l;
          bi = k0 + g;
        }
      }
    }
    if constexpr (kBest) {
      if (in) {
        best_lnl[site] = bl;
        best_idx[site] = bi;
        if (out) acc += (double)wgt_at(wgt, site, partials) * bl;
      }
    }
  }
  if constexpr (kBest) {
    if (out) lnl_finish(acc, partials, ticket, out, nullptr, 0);  // uniform: a kernel argument
  }
}

}  // namespace dev
}  // namespace plfx
