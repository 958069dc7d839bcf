// trav_plan.hpp -- the traversal scheduler of plfx_traverse_tips: dependency
// levels of a post-order op list and the greedy choice of fused groups.
// Plain C++: no GPU, no context, no pointers to CLVs; only the op list and
// which slots are tips (tests/trav_plan_main.cpp drives it on the CPU).
#pragma once
#include <string>
#include <vector>

#include "../../include/plfx.h"

namespace plfx {

// kind k counts into TravPlan::counts[k] (plfx_traverse_schedule's entries)
enum TravKind { kTravDeep6 = 0, kTravDeep5, kTravDeep4, kTravSeptet, kTravTriple };

struct TravGroup {
  int level;  // the level of its lowest ops: the group is issued there
  int kind;   // TravKind; a deep group's depth is 6 - kind
  int tips;   // deep: 0 dense leaves, 2 every leaf a tip; septet / triple: the
              // number of tip children of each of its leaf ops
  // deep: the 2^D - 1 ops in DeepDesc heap order by level (ops[i] of level k
  // reads what ops[2i], ops[2i+1] of level k-1 wrote); septet: a0..a3, b0,
  // b1, r (a[2i], a[2i+1] wrote b[i]'s child1, child2; b0, b1 wrote r's);
  // triple: a, b, p (a, b wrote p's child1, child2)
  std::vector<int> ops;
};

struct TravPlan {
  int nlev = 0;
  std::vector<int> level;         // per op
  std::vector<char> fused;        // per op: member of a group
  std::vector<TravGroup> groups;  // in selection order: deeps (6, 5, 4), septets, triples
  int counts[6] = {};             // deep6, deep5, deep4, septets, triples, unfused ops
};

// Levels: op j runs one level after the last write of its children (RAW) and
// after the last write and the last read of its parent slot (WAW, WAR).
// Groups (states 4 only): fuse >= 3 complete subtrees of depth 6, 5, 4;
// >= 2 three-level septets; >= 1 level-pair triples; each pass scans the ops
// in index order and takes what is still unfused.  slot_is_tip: nslots flags,
// NULL = no tips.  Returns PLFX_OK, or PLFX_ERR_INVALID with *err set.
int plan_traversal(const plfx_trav_op *ops, int nops, int nslots, int npmats,
                   const unsigned char *slot_is_tip, int states, int fuse, TravPlan *out,
                   std::string *err);

}  // namespace plfx
