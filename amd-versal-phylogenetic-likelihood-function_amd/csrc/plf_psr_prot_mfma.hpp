// plf_psr_prot_mfma.hpp -- the protein per-site-rate node in FMA mode on the
// f64 matrix cores (plfx.h section 11d): plf()'s loop with one category and
// every multiply-add fused, run on each site with its category's matrices,
//   umpL[k]  = fma chain over l ascending from +0.0 of x1[i][l] * left[c*400 + 20k + l]
//   p[k]     = umpL[k] * umpR[k]                       (one rounding)
//   x3[i][l] = fma chain over k ascending from +0.0 of p[k] * EV[20k + l]
// then section 11b's 2^-32 rescale.  f64 only.
//
// The arrangement is plf_psr_prot.hpp's: a wave owns 64 consecutive sites and
// its own PsrProtTile in LDS, a block 4 waves = 256 sites per trip, ordered by
// wave-level fences with no block barrier in a trip; dense children arrive by
// psr_prot_tile_fetch / _put, a coded child's rows are copied from the block's
// 24 x 20 tip table into the tile (the arithmetic on a copied row is the dense
// child's, so a coded child is bit-identical to its expansion).
//
// The products are plf_prot.hpp prot_mfma_body's, per 16-site sub-tile:
//   U^T = P . X^T   M = 20 as one v_mfma_f64_16x16x4_f64 tile plus rows 16..19
//                   on v_mfma_f64_4x4x4_4b_f64, K = 5 steps; B fragments from
//                   the LDS tile (site lane%16, state 4 st + lane/16)
//   p   = U_L o U_R in the accumulators
//   X3^T = EV^T . p with the accumulators as B fragments and the permuted EV
//                   rows that let a lane write four consecutive states.
// Both instructions are k-ordered fma chains from the accumulator
// (tools/probes/mfma_f64_numerics.hip, mfma_f64_4x4x4_numerics.hip), which is
// the statement above.  The EV A fragments are fixed for the whole kernel.
//
// What is new is that the A fragments of P_L and P_R depend on the site.  The
// category is made wave-uniform by looping, per side: while lanes are left, c =
// the category of the first (a readlane); the lanes load category c's A
// fragments (10 doubles per lane from P + c*400, L2-resident); every sub-tile
// that holds a site of category c runs the product, and a lane keeps the result
// only where its column's site (column = lane%16) has category c.  MFMA columns
// are independent, so the kept values do not depend on what other columns
// held.  Phase 3 and the scale test (the ballot over the four lanes that share
// a site) run once per sub-tile.  A wave of one category makes one pass per
// side, a wave with k categories k passes over the sub-tiles that need them:
// the same bits for any site order, fast for sites sorted by category.
//
// LDS: a B-fragment read is one ds_read_b64 per lane at double address
// 22 * (lane%16) + lane/16 + 4 st, i.e. dword 44 * (lane%16) + 2 * (lane/16).
// 44 * j mod 64 takes the sixteen multiples of 4, so lanes 0..31 (lane/16 = 0,
// 1) cover each of the 64 banks once, and so do lanes 32..63: conflict-free at
// PsrProtTile's 11-chunk stride, by the rules of tools/lds_banks.py (0 extra
// cycles), so the kernel needs no tile type of its own.  The compiler pairs
// k-steps 0,1 and 2,3 into ds_read2_b64, which the same rules charge 64 extra
// LDS cycles per side and 64-site tile (16 lanes a group over 32 banks:
// 12 j mod 32 repeats after 8 sites) against the 1680 matrix-core cycles of
// that side; not split.  The X3 writes: the two
// ds_write_b128 per sub-tile 0 extra cycles, the row-16..19 ds_write_b64 4.
#pragma once
#include "plf_psr_prot.hpp"

namespace plfx {
namespace dev {

// kPsrProtMfmaPrefetch: the next child tile's loads are in flight in registers
// under the products (x2 during side 1, the next trip's first dense child
// during side 2), which costs 40 VGPRs and one wave per SIMD: 2 waves.
// Without it a tile is loaded where it is used and 3 waves per SIMD (what the
// LDS tiles allow) hide the loads of one another.
#ifndef PLFX_PSR_PROT_MFMA_PREFETCH
#define PLFX_PSR_PROT_MFMA_PREFETCH 0
#endif
constexpr bool kPsrProtMfmaPrefetch = PLFX_PSR_PROT_MFMA_PREFETCH != 0;
constexpr int kPsrProtMfmaMinWaves = kPsrProtMfmaPrefetch ? 2 : 3;

template <bool kSum, bool T1, bool T2>
__device__ __forceinline__ void psr_prot_mfma_body(const void *__restrict__ c1, const void *__restrict__ c2,
                                                   double *__restrict__ x3, const double *__restrict__ EV,
                                                   const double *__restrict__ left,
                                                   const double *__restrict__ right,
                                                   const uint8_t *__restrict__ rate_cat, int ncat,
                                                   const int32_t *__restrict__ wgt, uint8_t *__restrict__ scaler,
                                                   int64_t n, unsigned long long *ws, int64_t *scaler_sum,
                                                   const double *__restrict__ tipvec) {
  constexpr int S = 20;
  using PT = PsrProtTile<double>;
  using V = typename PT::V;
  constexpr int kRow = 2 * PT::kStride;  // doubles per site in the LDS tile (22)
  const double *__restrict__ x1 = static_cast<const double *>(c1);
  const double *__restrict__ x2 = static_cast<const double *>(c2);
  const uint8_t *__restrict__ tip1 = static_cast<const uint8_t *>(c1);
  const uint8_t *__restrict__ tip2 = static_cast<const uint8_t *>(c2);

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int lo16 = lane & 15, g = lane >> 4;
  __shared__ V tiles[kWavesPerBlock * PT::kChunks];
  __shared__ V tab[(T1 || T2) ? PT::kTabChunks : 1];
  V *const tile = tiles + wave * PT::kChunks;
  const double *td = reinterpret_cast<const double *>(tile);
  double *tw = reinterpret_cast<double *>(tile);

  const int64_t stride = (int64_t)gridDim.x * kBlock;
  int64_t wbase = (int64_t)blockIdx.x * kBlock + wave * 64;  // wave-uniform, as the loop's trip count
  constexpr bool kPf = kPsrProtMfmaPrefetch;
  V pf[PT::kChunksPerSite];
  // the first dense child's first tile, before the table and the EV fragments
  if constexpr (kPf && !(T1 && T2)) {
    if (wbase < n) psr_prot_tile_fetch<double>(T1 ? x2 : x1, wbase, n, lane, pf);
  }
  if constexpr (T1 || T2) {
    double *t = reinterpret_cast<double *>(tab);
    for (int e = threadIdx.x; e < kProtCodes * S; e += kBlock) {
      const int code = e / S, l = e - code * S;
      t[code * kRow + l] = prot_tip_value<double>(tipvec, code, l);
    }
    __syncthreads();
  }
  // EV A fragments: [0][st] -> EV^T[l = 4 (lo16 % 4) + lo16 / 4][k = 4 st + g] (A row i of the
  // 16x16x4 tile computes state 4 (i % 4) + i / 4); [1][st] -> EV^T[l = 16 + lane % 4][k]
  double AE[2][5];
#pragma unroll
  for (int st = 0; st < 5; st++) {
    const int col = 4 * st + g;
    AE[0][st] = EV[col * S + 4 * (lo16 & 3) + (lo16 >> 2)];
    AE[1][st] = EV[col * S + 16 + (lane & 3)];
  }
  const double m = Num<double>::minlik();
  // a coded child's rows from the table into the tile: lane = site
  auto copy_rows = [&](int code) {
    double r[S];
    psr_prot_row_read<double>(tab + code * PT::kStride, r);
    psr_prot_row_write<double>(tile + lane * PT::kStride, r);
  };

  long long acc = 0;
  for (; wbase < n; wbase += stride) {
    const int64_t site = wbase + lane;
    const bool in = site < n;
    const int64_t ld = in ? site : n - 1;
    const int cat = psr_prot_cat(rate_cat[ld], ncat);
    const unsigned long long valid = __ballot(in);
    const int64_t next = wbase + stride;
    // the category of this lane's column in each sub-tile; -1: no site there
    int catT[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int ct = __shfl(cat, 16 * t + lo16);
      catT[t] = wbase + 16 * t + lo16 < n ? ct : -1;
    }

    f64x4 P0[4];  // per sub-tile: rows g + 4 r of U_L^T, then of p
    double P1[4];  // row 16 + g
#pragma unroll
    for (int t = 0; t < 4; t++) {
      P0[t] = f64x4{0.0, 0.0, 0.0, 0.0};
      P1[t] = 0.0;
    }
    // One side: fn(t, keep, u0, u1) for every sub-tile t with a site of the
    // pass's category; keep: this lane's column is such a site.
    auto side = [&](const double *__restrict__ Pm, auto &&fn) {
      unsigned long long todo = valid;
      while (todo) {
        const int c = __builtin_amdgcn_readlane(cat, __builtin_ctzll(todo));
        const double *__restrict__ Pc = Pm + c * (S * S);
        // A fragments of category c: [0] P[k = lo16][l = 4 st + g], [1] P[k = 16 + lane % 4][l]
        double A0[5], A1[5];
#pragma unroll
        for (int st = 0; st < 5; st++) {
          A0[st] = Pc[lo16 * S + 4 * st + g];
          A1[st] = Pc[(16 + (lane & 3)) * S + 4 * st + g];
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
          const bool keep = catT[t] == c;
          if (__ballot(keep) == 0) continue;  // wave-uniform
          const double *xr = td + (16 * t + lo16) * kRow + g;
          f64x4 u0 = {0.0, 0.0, 0.0, 0.0};
          double u1 = 0.0;
#pragma unroll
          for (int st = 0; st < 5; st++) {
            const double b = xr[4 * st];
            u0 = __builtin_amdgcn_mfma_f64_16x16x4f64(A0[st], b, u0, 0, 0, 0);
            u1 = __builtin_amdgcn_mfma_f64_4x4x4f64(A1[st], b, u1, 0, 0, 0);
          }
          fn(t, keep, u0, u1);
        }
        todo &= ~__ballot(cat == c);
      }
    };

    if constexpr (T1) {
      copy_rows(prot_code(tip1[ld]));
    } else {
      if constexpr (!kPf) psr_prot_tile_fetch<double>(x1, wbase, n, lane, pf);
      psr_prot_tile_put<double>(pf, lane, tile);
    }
    psr_prot_wave_sync();
    if constexpr (kPf && !T1) {  // the next tile's loads, in flight under the products
      if constexpr (!T2) psr_prot_tile_fetch<double>(x2, wbase, n, lane, pf);
      else if (next < n) psr_prot_tile_fetch<double>(x1, next, n, lane, pf);
    }
    side(left, [&](int t, bool keep, const f64x4 &u0, double u1) {
#pragma unroll
      for (int r = 0; r < 4; r++) P0[t][r] = keep ? u0[r] : P0[t][r];
      P1[t] = keep ? u1 : P1[t];
    });
    psr_prot_wave_sync();  // every lane is done reading child 1: the tile takes child 2
    if constexpr (T2) {
      copy_rows(prot_code(tip2[ld]));
    } else {
      if constexpr (!kPf) psr_prot_tile_fetch<double>(x2, wbase, n, lane, pf);
      psr_prot_tile_put<double>(pf, lane, tile);
    }
    psr_prot_wave_sync();
    if constexpr (kPf && !T2) {
      if (next < n) psr_prot_tile_fetch<double>(T1 ? x2 : x1, next, n, lane, pf);
    }
    side(right, [&](int t, bool keep, const f64x4 &u0, double u1) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const double p = P0[t][r] * u0[r];  // umpL[k] * umpR[k]
        P0[t][r] = keep ? p : P0[t][r];
      }
      const double p1 = P1[t] * u1;
      P1[t] = keep ? p1 : P1[t];
    });
    psr_prot_wave_sync();  // every lane is done reading child 2: the tile takes X3

    // back-transform: lane holds X3[site 16 t + lo16][l = 4 g + r] and [l = 16 + g]
    unsigned long long small_sites = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      f64x4 X0 = {0.0, 0.0, 0.0, 0.0};
      double X1 = 0.0;
#pragma unroll
      for (int st = 0; st < 5; st++) {
        const double b = st < 4 ? P0[t][st & 3] : P1[t];
        X0 = __builtin_amdgcn_mfma_f64_16x16x4f64(AE[0][st], b, X0, 0, 0, 0);
        X1 = __builtin_amdgcn_mfma_f64_4x4x4f64(AE[1][st], b, X1, 0, 0, 0);
      }
      const bool small = (__builtin_fabs(X0[0]) < m) && (__builtin_fabs(X0[1]) < m) &&
                         (__builtin_fabs(X0[2]) < m) && (__builtin_fabs(X0[3]) < m) && (__builtin_fabs(X1) < m);
      const unsigned long long b = __ballot(small);
      // site lo16 of sub-tile t scales iff its 4 lanes agree
      const unsigned long long s16 = b & (b >> 16) & (b >> 32) & (b >> 48) & 0xFFFFull;
      small_sites |= s16 << (16 * t);
      if ((s16 >> lo16) & 1ull) {  // exact: power-of-two scaling
        X0 = X0 * Num<double>::two32();
        X1 = X1 * Num<double>::two32();
      }
      double *o = tw + (16 * t + lo16) * kRow;
      *reinterpret_cast<f64x2 *>(o + 4 * g) = f64x2{X0[0], X0[1]};
      *reinterpret_cast<f64x2 *>(o + 4 * g + 2) = f64x2{X0[2], X0[3]};
      o[16 + g] = X1;
    }
    if (in) {
      const bool sc = (small_sites >> lane) & 1ull;
      if (scaler) scaler[site] = (uint8_t)sc;
      if (kSum) acc += sc ? (long long)wgt_at(wgt, site, ws) : 0ll;
    }
    psr_prot_wave_sync();
    psr_prot_tile_store<double>(x3, wbase, n, lane, tile);
    psr_prot_wave_sync();  // the tile is the next trip's
  }
  if constexpr (kSum) block_ticket_sum(acc, ws, scaler_sum);
}

// Up to kMaxBatch nodes per launch, node = blockIdx.y, sharing EV, n, wgt and
// rate_cat; T1 / T2, kSum and the ticket regions as plf_psr_prot_kernel.
template <bool kSum, bool T1, bool T2>
__global__ void __launch_bounds__(kBlock, kPsrProtMfmaMinWaves)
plf_psr_prot_mfma_kernel(const NodeBatch nodes, const double *__restrict__ EV,
                         const uint8_t *__restrict__ rate_cat, int ncat, const int32_t *__restrict__ wgt,
                         int64_t n, unsigned long long *ws, const double *__restrict__ tipvec) {
  const NodeDesc &d = nodes.d[blockIdx.y];
  psr_prot_mfma_body<kSum, T1, T2>(d.x1, d.x2, static_cast<double *>(d.x3), EV,
                                   static_cast<const double *>(d.left), static_cast<const double *>(d.right),
                                   rate_cat, ncat, wgt, d.scaler, n, ws + (size_t)blockIdx.y * kWsWords,
                                   d.scaler_sum, tipvec);
}

}  // namespace dev
}  // namespace plfx
