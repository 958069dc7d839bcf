// psr_lower.hpp -- from the nodes of a plfx_plf_psr_dev call, or a traversal
// plan (trav_plan.hpp) and the arrays of a plfx_traverse_psr call, to the list
// of kernel launches the C ABI issues: the call's, every node's and every
// fused group's checks, the descriptors, and the split into launches of one
// kind of children.  Plain C++: device pointers are stored and compared, never
// followed (tests/psr_lower_main.cpp and tests/psr_trav_lower_main.cpp drive
// it on the CPU).
#pragma once
#include <string>
#include <vector>

#include "../../include/plfx.h"
#include "plf_desc.hpp"
#include "trav_lower.hpp"  // TravArrays
#include "trav_plan.hpp"

namespace plfx {

// What the nodes of a call share.  states: 4 (plfx.h section 11) or 20
// (section 11b): values per site of a CLV, and states * states per category
// of a matrix.  flags: 0, or PLFX_FMA (section 11d) -- the lowered list does
// not depend on it, only the launcher the executor picks for 20 states.
struct PsrCall {
  int dtype;
  int64_t n;
  int ncat;
  const void *EV;
  const uint8_t *rate_cat;
  int states = 4;
  int flags = 0;
};

enum PsrLaunchKind {
  kPsrNodes,    // nodes[first, first + count): count <= kMaxBatch
  kPsrTriples,  // triples[first, first + count): count <= kMaxTriples
};

// One kernel launch.  Nodes: all with the same kind of children -- tips bit 0:
// child 1 is coded, bit 1: child 2.  Triples: tips = the number of coded
// children of each leaf op (0, 1, 2), coded child first.  A coded child's
// descriptor pointer names its uint8 codes.
struct PsrLaunch {
  int kind;   // PsrLaunchKind
  int level;  // of the traversal (0 for a plain batch)
  int tips;
  int first, count;
};

struct PsrLaunchList {
  std::vector<PsrLaunch> items;
  std::vector<NodeDescH> nodes;
  std::vector<TripleDescH> triples;
  void clear() {  // keeps the capacity: a context lowers every call into one list
    items.clear();
    nodes.clear();
    triples.clear();
  }
  int launches() const { return (int)items.size(); }  // plfx_traverse_schedule's entry 6
};

// bytes of one PSR CLV: n sites * states * element size
inline size_t psr_clv_bytes(int dtype, int64_t n, int states = 4) {
  return (size_t)(n > 0 ? n : 0) * (size_t)states * (dtype == PLFX_F32 ? 4 : 8);
}

// The launches of `count` nodes, in issue order: the kinds dense/dense,
// tip/dense, dense/tip, tip/tip one after the other, each kind's nodes in the
// caller's order in consecutive chunks of kMaxBatch.  n == 0 gives an empty
// list (nothing runs; the caller zeroes the sums) after the call-level checks
// alone, as the Gamma entry points do.  Returns PLFX_OK, or PLFX_ERR_INVALID
// with *err set and *out empty: nothing of a refused call is launched.
int lower_psr(const PsrCall &call, const plfx_psr_node *nodes, int count, PsrLaunchList *out, std::string *err);

// The whole traversal, level by level.  Within a level: its triples by tip
// kind 0, 1, 2 in launches of at most kMaxTriples, then its unfused ops by
// kind of children as lower_psr.  Op j's matrices are pmats + (2 * pmat) *
// ncat * states^2 and + (2 * pmat + 1) * ncat * states^2 values.  With 20
// states there is no fused kernel: the plan's level pairs are ignored, every
// op is lowered unfused and no kPsrTriples item is emitted.  A triple's leaf
// ops are stored coded child first (tip_first); P's children keep the order op
// P names them in.  Checks, all before the list holds anything: the call's
// (n == 0 gives an empty list here), every op's section-11 node checks, and
// per triple that none of its three outputs shares a byte with another of
// them or with one of its four leaves.  Refusals as lower_psr.
int lower_psr_traversal(const TravPlan &plan, const TravArrays &t, const PsrCall &call, PsrLaunchList *out,
                        std::string *err);

}  // namespace plfx
