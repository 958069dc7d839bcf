// psr_trav_lower.hpp -- from a traversal plan (trav_plan.hpp) and the arrays
// of a plfx_traverse_psr call to the list of kernel launches the C ABI issues:
// the call's, every op's and every fused group's checks, the descriptors, and
// per level the fused level pairs followed by the unfused ops.  Plain C++:
// device pointers are stored and compared, never followed
// (tests/psr_trav_lower_main.cpp drives it on the CPU).
#pragma once
#include <string>
#include <vector>

#include "../../include/plfx.h"
#include "plf_desc.hpp"
#include "psr_lower.hpp"   // PsrCall, psr_clv_bytes
#include "trav_lower.hpp"  // TravArrays, aligned16, overlap
#include "trav_plan.hpp"

namespace plfx {

enum PsrTravKind {
  kPsrTravTriples,  // triples[first, first + count): count <= kMaxTriples
  kPsrTravNodes,    // nodes[first, first + count): count <= kMaxBatch
};

// One kernel launch.  Triples: tips = the number of coded children of each
// leaf op (0, 1, 2), coded child first.  Nodes: tips bit 0 / 1 = child 1 / 2
// of every node is coded, as PsrLaunch.  A coded child's descriptor pointer
// names its uint8 codes.
struct PsrTravItem {
  int kind;   // PsrTravKind
  int level;  // of the traversal
  int tips;
  int first, count;
};

struct PsrTravList {
  std::vector<PsrTravItem> items;
  std::vector<NodeDescH> nodes;
  std::vector<TripleDescH> triples;
  void clear() {  // keeps the capacity: a context lowers every call into one list
    items.clear();
    nodes.clear();
    triples.clear();
  }
  int launches() const { return (int)items.size(); }  // plfx_traverse_schedule's entry 6
};

// The whole traversal, level by level.  Within a level: its triples by tip
// kind 0, 1, 2 in launches of at most kMaxTriples, then its unfused ops by
// kind of children (dense/dense, tip/dense, dense/tip, tip/tip), each kind in
// list order in consecutive chunks of kMaxBatch.  Op j's matrices are pmats +
// (2 * pmat) * ncat * 16 and + (2 * pmat + 1) * ncat * 16 values.  A triple's
// leaf ops are stored coded child first ((x1, left) swapped with (x2, right)
// where child 2 alone is coded: only u1[k] * u2[k] crosses the sides, so the
// bits are the same); P's children keep the order op P names them in.
// Checks, all before the list holds anything: the call's (dtype, ncat, n >= 0,
// then -- n == 0 gives an empty list here -- EV, rate_cat, pmats, clv), every
// op's section-11 node checks, and per triple that none of its three outputs
// shares a byte with another of them or with one of its four leaves.  Returns
// PLFX_OK, or PLFX_ERR_INVALID with *err set and *out empty.
int lower_psr_traversal(const TravPlan &plan, const TravArrays &t, const PsrCall &call, PsrTravList *out,
                        std::string *err);

}  // namespace plfx
