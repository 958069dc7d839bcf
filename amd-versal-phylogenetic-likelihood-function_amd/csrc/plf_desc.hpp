// plf_desc.hpp -- the host-side descriptors the batched and fused launchers
// of plf_kernels.hpp take, with their limits.  No HIP header: trav_lower.cpp
// fills them on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

namespace plfx {

// Batched nodes (<= kMaxBatch per launch) sharing EV, n, wgt.
// tips: 0 dense children; 1 x1 of every node is a tip (uint8 state codes);
// 2 x1 and x2 are tips.
struct NodeDescH {
  const void *x1, *x2;
  void *x3;
  const void *left, *right;
  uint8_t *scaler;
  int64_t *scaler_sum;
};
constexpr int kMaxBatch = 32;

// Batched PSR sum tables (plf_psr.hpp PsrEdgeDesc; <= kMaxBatch per launch,
// all with the same kind of side 1): out = x1 * x2, x1 a dense CLV or the
// uint8 codes of a coded side.
struct PsrEdgeDescH {
  const void *x1, *x2;
  void *out;
};

// One tip of a tiling launch of the PSR rate scan (plf_psr.hpp PsrTileDesc; <=
// kMaxBatch per launch): dst[g * n + i] = src[i] for every candidate g of a group.
struct PsrTileDescH {
  const uint8_t *src;
  uint8_t *dst;
};

// Tip/tip protein nodes from their 576-combination tables (plf_prot.hpp
// prot_tiptip_gather_kernel): x3 / scaler / sum of each node gathered by code pair.
struct ProtGatherDescH {
  const uint8_t *c1, *c2;
  void *x3;
  uint8_t *scaler;
  int64_t *scaler_sum;
  const void *tab;
  const uint8_t *tsc;
};
constexpr int kProtCombos = 24 * 24;
// One node's slot in its stream's tip/tip tables: a 576 x 80 table (sized for
// f64) followed by 576 scaler bytes, padded.
constexpr size_t kTtTabBytes = (size_t)kProtCombos * 80 * sizeof(double);
constexpr size_t kTtScBytes = 1024;

// Protein nodes (f64, f32; FMA or exact) whose two children are tip/tip nodes held in
// combination tables (plf_prot.hpp ProtTabDesc), batched as above.
struct ProtTabDescH {
  const void *tab1, *tab2;
  const uint8_t *c1a, *c1b, *c2a, *c2b;
  void *x3;
  const void *left, *right;
  uint8_t *scaler;
  int64_t *scaler_sum;
};

// Fused level pairs (plf_dna.hpp TripleDesc); <= kMaxTriples per launch.
struct TripleDescH {
  const void *a1, *a2, *b1, *b2;
  void *xa, *xb, *xp;
  const double *la, *ra, *lb, *rb, *lp, *rp;
  uint8_t *sa, *sb, *sp;
  int64_t *ssa, *ssb, *ssp;
};
constexpr int kMaxTriples = 10;

// A fused sibling pair (plf_psr_branch.hpp BranchPairDesc): op (v, c1, c2)
// with W(v) dense.  c1 / c2: the children, coded child first (the uint8
// codes of a coded child); p1 / p2 their matrices; w1 / w2 the outer CLVs
// (NULL for a coded child: never written), t1 / t2 the tables, ss1 / ss2 the
// weighted scaler sums of W(c1) / W(c2) (NULL: not wanted).
struct BranchPairDescH {
  const void *wv, *c1, *c2;
  const void *pup, *p1, *p2;
  void *w1, *w2, *t1, *t2;
  int64_t *ss1, *ss2;
};
constexpr int kMaxPairs = 16;  // 16 * 96 B of descriptors; two ticket regions each

// One op of the counters' pass (plf_psr_branch.hpp BranchScaleDesc): w1 / w2
// the ops that wrote its children (-1: a tip), up the edge of its parent slot
// in the op that reads it (-1: the root op).
struct BranchScaleDescH {
  int32_t w1, w2, up;
};
constexpr int kScaleChunk = 256;  // ops per launch of the counters' kernel: 3 KB of descriptors

// Fused three-level subtrees (plf_dna.hpp SeptetDesc); <= kMaxSeptets per launch.
struct SeptetDescH {
  const void *g[8];
  void *x[7];
  const void *mat[14];
  uint8_t *sc[7];
  int64_t *ss[7];
};
constexpr int kMaxSeptets = 8;

// Fused complete subtree of depth 4..6 (plf_dna.hpp DeepDesc: 2^depth leaves,
// 2^depth - 1 nodes in heap order by level), one per launch.
struct DeepDescH {
  const void *g[64];
  void *x[63];
  const void *mat[126];
  uint8_t *sc[63];
  int64_t *ss[63];
};
constexpr int kDeepNodes = 63;

}  // namespace plfx
