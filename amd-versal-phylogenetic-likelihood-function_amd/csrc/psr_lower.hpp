// psr_lower.hpp -- from the nodes of a plfx_plf_psr_dev call to the list of
// kernel launches the C ABI issues: the call's and every node's checks, the
// descriptors, and the split into launches of one kind of children and at
// most kMaxBatch nodes.  Plain C++: device pointers are stored and compared,
// never followed (tests/psr_lower_main.cpp drives it on the CPU).
#pragma once
#include <string>
#include <vector>

#include "../../include/plfx.h"
#include "plf_desc.hpp"

namespace plfx {

// What the nodes of a call share.
struct PsrCall {
  int dtype;
  int64_t n;
  int ncat;
  const void *EV;
  const uint8_t *rate_cat;
};

// One kernel launch: nodes[first, first + count), count <= kMaxBatch, all with
// the same kind of children -- tips bit 0: child 1 is coded, bit 1: child 2
// (a coded child's descriptor pointer names its uint8 codes).
struct PsrLaunch {
  int tips;
  int first, count;
};

struct PsrLaunchList {
  std::vector<PsrLaunch> items;
  std::vector<NodeDescH> nodes;
  void clear() {  // keeps the capacity: a context lowers every call into one list
    items.clear();
    nodes.clear();
  }
};

// bytes of one PSR CLV: n sites * 4 states * element size
inline size_t psr_clv_bytes(int dtype, int64_t n) {
  return (size_t)(n > 0 ? n : 0) * 4 * (dtype == PLFX_F32 ? 4 : 8);
}

// The launches of `count` nodes, in issue order: the kinds dense/dense,
// tip/dense, dense/tip, tip/tip one after the other, each kind's nodes in the
// caller's order in consecutive chunks of kMaxBatch.  n == 0 gives an empty
// list (nothing runs; the caller zeroes the sums) after the call-level checks
// alone, as the Gamma entry points do.  Returns PLFX_OK, or PLFX_ERR_INVALID
// with *err set and *out empty: nothing of a refused call is launched.
int lower_psr(const PsrCall &call, const plfx_psr_node *nodes, int count, PsrLaunchList *out, std::string *err);

}  // namespace plfx
