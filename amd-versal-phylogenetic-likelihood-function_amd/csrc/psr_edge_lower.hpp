// psr_edge_lower.hpp -- from the edges of a plfx_edge_sumtable_psr_batch call
// to the list of kernel launches the C ABI issues: the call's and every edge's
// checks, the check that no table of the call shares a byte with another
// table or with an input, the descriptors, and the split into launches of one
// kind of side 1.  Plain C++ as psr_lower.hpp: device pointers are stored and
// compared, never followed (tests/psr_edge_lower_main.cpp drives it on the
// CPU).
#pragma once
#include <string>
#include <vector>

#include "../../include/plfx.h"
#include "plf_desc.hpp"

namespace plfx {

// One kernel launch: edges[first, first + count), count <= kMaxBatch, all with
// a dense side 1 (tip = 0) or all with a coded one (tip = 1: the descriptor's
// x1 names the uint8 codes).
struct PsrEdgeLaunch {
  int tip;
  int first, count;
};

struct PsrEdgeLaunchList {
  std::vector<PsrEdgeLaunch> items;
  std::vector<PsrEdgeDescH> edges;
  void clear() {  // keeps the capacity: a context lowers every call into one list
    items.clear();
    edges.clear();
  }
  int launches() const { return (int)items.size(); }
};

// The launches of `nedges` sum tables, in issue order: the edges with a dense
// side 1, then those with a coded one, each kind in the caller's order in
// consecutive chunks of kMaxBatch.  Checks, all before the list holds
// anything: the call's (dtype, n >= 0, nedges >= 1, edges; n == 0 gives an
// empty list after these alone), per edge the rules of plfx_edge_sumtable_psr
// (exactly one of tip1 / x1, x2 and sumtab, 16-byte alignment of the dense
// sides and the table, tipvec with a coded side, a table apart from its own
// inputs), and across the call that no table shares a byte with another
// edge's table or with any edge's input -- one sort of the byte intervals and
// one sweep.  Inputs may repeat.  Returns PLFX_OK, or PLFX_ERR_INVALID with
// *err set and *out empty: nothing of a refused call is launched.
// states: 4, or 20 for plfx_edge_sumtable_psr_batch_gen's protein tables -- a
// CLV and a table are n * states values, which is what the overlap checks
// span; any other count is refused like a bad dtype.
int lower_psr_edges(int dtype, int64_t n, const void *tipvec, const plfx_psr_edge *edges, int nedges,
                    PsrEdgeLaunchList *out, std::string *err, int states = 4);

}  // namespace plfx
