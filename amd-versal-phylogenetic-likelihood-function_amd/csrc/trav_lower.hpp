// trav_lower.hpp -- from a batch of nodes, or a traversal plan and the call's
// arrays, to the flat list of kernel launches the C ABI issues: node checks,
// descriptors, launch groups and the protein tip/tip table path.  Plain C++:
// device pointers are stored and compared, never followed
// (tests/trav_lower_main.cpp drives it on the CPU).
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "../../include/plfx.h"
#include "plf_desc.hpp"
#include "trav_plan.hpp"

namespace plfx {

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return na > 0 && nb > 0 && pa < pb + nb && pb < pa + na;
}

// bytes of one CLV: n sites * 4 categories * states * element size
inline size_t clv_bytes_of(int dtype, int states, int64_t n) {
  return (size_t)(n > 0 ? n : 0) * 4 * states * (dtype == PLFX_F32 ? 4 : 8);
}

// One kernel launch each, in issue order; kLaunchProtTipTip is a launch pair.
enum LaunchKind {
  kLaunchDeep,        // deeps[first]: one fused subtree of `depth` levels
  kLaunchSeptets,     // septets[first, first + count)
  kLaunchTriples,     // triples[first, first + count)
  kLaunchDnaBatch,    // nodes[first, first + count)
  kLaunchProtNode,    // nodes[first]: one protein node with the whole GPU
  kLaunchProtBatch,   // nodes[first, first + count)
  kLaunchProtTipTip,  // combs[first, ..): the nodes' combination tables, then gathers[first, ..)
  kLaunchProtTab,     // tabs[first, first + count): children staged from the tip/tip tables
};

struct LaunchItem {
  int kind;   // LaunchKind
  int level;  // of the traversal (0 for a plain batch)
  int tips;   // tip children of every node (leaf op) of the item, tip child first
  int depth;  // kLaunchDeep: 4..6, else 0
  int first, count;
};

struct LaunchList {
  std::vector<LaunchItem> items;
  std::vector<NodeDescH> nodes, combs;
  std::vector<ProtGatherDescH> gathers;
  std::vector<ProtTabDescH> tabs;
  std::vector<TripleDescH> triples;
  std::vector<SeptetDescH> septets;
  std::vector<DeepDescH> deeps;
  void clear();          // keeps the capacity: a context lowers every call into one list
  int launches() const;  // kernel launches: plfx_traverse_schedule's entry 6
};

// What every node of a call shares.  tt, tt_codes: the stream's tip/tip
// tables (kMaxBatch slots of kTtTabBytes + kTtScBytes) and the context's two
// constant 576-code arrays (the second 1024 bytes after the first); needed
// when states == 20 and some node has two tip children, else unused.
struct LowerCall {
  int dtype, states;
  int64_t n;
  char *tt;
  const uint8_t *tt_codes;
};

// `count` > 0 nodes of one kind (tips = number of tip children, tip child
// first; a tip child is a uint8 code array with no alignment rule), n > 0,
// as *out in launches of kMaxBatch: DNA launch j of L takes nodes j,
// j + L, ...; protein in consecutive chunks, one node alone as
// kLaunchProtNode, tip/tip nodes through the tables.  ids (may be NULL) names
// the nodes in messages (the op indices in a traversal).  Returns PLFX_OK, or
// PLFX_ERR_INVALID with *err set and *out cleared.
int lower_batch(const LowerCall &call, const plfx_node *nodes, int count, int tips, const int *ids,
                LaunchList *out, std::string *err);

// The arrays of a traversal call (plfx_traverse_tips).
struct TravArrays {
  const plfx_trav_op *ops;
  int nops;
  void *const *clv;
  const uint8_t *const *tips;  // may be NULL
  const void *pmats;
  uint8_t *const *scalers;  // may be NULL
  int64_t *scaler_sums;     // may be NULL
};

// A node whose x1 / x2 name the uint8 codes of a coded child (t1 / t2).
struct OpNode {
  plfx_node nd;
  bool t1, t2;
};

// Op j of a traversal as a node, children as the op names them; mat_bytes: of
// one matrix (ncat * S * S values).
inline OpNode op_node(const TravArrays &t, size_t mat_bytes, int j) {
  const plfx_trav_op &o = t.ops[j];
  const char *pmats = static_cast<const char *>(t.pmats);
  const bool t1 = t.tips && t.tips[o.child1], t2 = t.tips && t.tips[o.child2];
  return OpNode{{t1 ? (const void *)t.tips[o.child1] : t.clv[o.child1],
                 t2 ? (const void *)t.tips[o.child2] : t.clv[o.child2], t.clv[o.parent],
                 pmats + (size_t)(2 * o.pmat) * mat_bytes, pmats + (size_t)(2 * o.pmat + 1) * mat_bytes,
                 t.scalers ? t.scalers[j] : nullptr, t.scaler_sums ? t.scaler_sums + j : nullptr},
                t1, t2};
}

// Coded child first: dense/tip runs as tip/dense, (x1, left) swapped with
// (x2, right).  Only u1[k] * u2[k] crosses the sides, so the bits are the same.
inline OpNode tip_first(OpNode o) {
  if (!o.t1 && o.t2) {
    std::swap(o.nd.x1, o.nd.x2);
    std::swap(o.nd.left, o.nd.right);
    std::swap(o.t1, o.t2);
  }
  return o;
}

inline NodeDescH node_desc(const plfx_node &d) {
  return NodeDescH{d.x1, d.x2, d.x3, d.left, d.right, d.scaler, d.scaler_sum};
}

// The level pair of leaf ops F, G and their parent op P, F the writer of P's child 1.
inline TripleDescH triple_desc(const plfx_node &F, const plfx_node &G, const plfx_node &P) {
  return TripleDescH{F.x1, F.x2, G.x1, G.x2, F.x3, G.x3, P.x3, (const double *)F.left, (const double *)F.right,
                     (const double *)G.left, (const double *)G.right, (const double *)P.left, (const double *)P.right,
                     F.scaler, G.scaler, P.scaler, F.scaler_sum, G.scaler_sum, P.scaler_sum};
}

// true when lower_traversal will use call.tt: protein with a tip/tip op
bool traversal_uses_tables(const TravArrays &t, int states);

// The whole traversal, n > 0: level by level, the level's deep passes first,
// then by number of tip children its septets, triples and unfused ops (these
// through lower_batch).  A protein op whose two children are tip/tip nodes of
// the level before, still in the tables of that level's last launch group,
// becomes a kLaunchProtTab node.  *out is replaced; refusals as lower_batch.
int lower_traversal(const TravPlan &plan, const TravArrays &t, const LowerCall &call, LaunchList *out,
                    std::string *err);

}  // namespace plfx
