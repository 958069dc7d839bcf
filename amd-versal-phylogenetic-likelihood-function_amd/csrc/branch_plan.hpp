// branch_plan.hpp -- plfx.h section 13: from a post-order op list that
// plfx_traverse_psr_ex has run to the outer CLVs W(c) of every child c, the
// sum table of every branch and the scaler count of every branch.  One planner
// and one lowering, plain C++: device pointers are stored and compared, never
// followed (tests/branch_lower_main.cpp drives it on the CPU).
//
// Edge e = 2 * j + s is the branch of op j to its child s (0 = child1).  The
// pre-order level of an op is its depth from the root op (the last op, level
// 0).  The children of the ops of level L >= 1 get their W in stage L, from
// W(v) of the op's own parent slot v, made in stage L - 1; stage 0 is the root
// edge's table alone (W(a) = slot b, W(b) = slot a, nothing copied).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/plfx.h"
#include "plf_desc.hpp"
#include "psr_edge_lower.hpp"
#include "psr_lower.hpp"

namespace plfx {

enum BranchLaunchKind {
  kBranchPairs,   // pairs[first, first + count): count <= kMaxPairs, tips = coded children of each op
  kBranchNodes,   // nodes[first, first + count): unfused W nodes of one kind of children (tips as PsrLaunch)
  kBranchTables,  // edges[first, first + count): sum tables, tips = side 1 is coded
  kBranchSub,     // scale[first, first + count): subtree sums, ops ascending
  kBranchScale,   // scale[first, first + count): outer sums and edge_scale, ops descending
};

struct BranchLaunch {
  int kind, level, tips, first, count;
};

// The workspace: slabs of `slab` bytes (a CLV rounded up to 256 B) -- the outer
// CLVs of the 2 * (nops - 1) non-root edges, then the 2 * nops - 1 tables --
// and the counters: int64 wsum[2 * nops], sub[nops], outer[2 * nops].
struct BranchLayout {
  size_t slab, w_off, tab_off, cnt_off, bytes;
};

struct BranchPlan {
  BranchLayout lay{};
  int nlev = 0;
  std::vector<int> level;       // per op: depth from the root op
  std::vector<int> up_edge;     // per op: the edge of its parent slot in the op that reads it, -1 for the root op
  std::vector<const void *> pup;  // per op: the matrix of its parent slot's branch (NULL for the root op)
  std::vector<const void *> wv;   // per op: W of its parent slot (dense CLV or codes; NULL for the root op)
  std::vector<unsigned char> wv_coded, fused;  // per op
  std::vector<void *> w, tab;   // per edge: the outer CLV's slab (NULL for the root op's edges) and the table
  std::vector<int64_t *> wsum;  // per edge: the W's scaler sum (NULL for the root op's edges)
  std::vector<BranchLaunch> items;
  std::vector<BranchPairDescH> pairs;
  std::vector<NodeDescH> nodes;
  std::vector<PsrEdgeDescH> edges;
  std::vector<BranchScaleDescH> scale;
  int64_t *sub = nullptr, *outer = nullptr;  // the counters' regions
  void clear();
  int launches() const { return (int)items.size(); }
};

// What a plfx_branch_sumtables_psr call hands over.
struct BranchCall {
  int dtype, states, flags;
  const plfx_trav_op *ops;
  int nops;
  void *const *clv;
  const uint8_t *const *tips;  // may be NULL
  int nslots;
  const void *pmats;
  int npmats;
  const void *root_pmat, *EV;
  int64_t n;
  const uint8_t *rate_cat;
  int ncat;
  const int64_t *scaler_sums;
  const void *tipvec;
  void *workspace;
  size_t workspace_bytes;
  const int64_t *edge_scale;  // NULL: no counters' pass, no W sums
};

// PLFX_OK and *lay, or PLFX_ERR_INVALID (dtype, states, nops < 1, n < 0).
int branch_layout(int dtype, int states, int nops, int64_t n, BranchLayout *lay);

// The plan of a call: the tree rules, the call's and every node's checks, the
// slab of every W and table and the launch list.  n == 0 checks the tree and
// the call and leaves an empty launch list with the tables' pointers set.
// Returns PLFX_OK, or PLFX_ERR_INVALID with *err set and *out cleared: nothing
// of a refused call is launched.
int plan_branches(const BranchCall &call, BranchPlan *out, std::string *err);

}  // namespace plfx
