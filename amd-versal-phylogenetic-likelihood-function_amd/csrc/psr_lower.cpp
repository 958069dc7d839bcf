// psr_lower.cpp -- see psr_lower.hpp.
#include "psr_lower.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "trav_lower.hpp"  // aligned16, overlap

namespace plfx {
namespace {

int refuse(PsrLaunchList *out, std::string *err, const char *what, int node = -1) {
  out->clear();
  if (err) {
    char buf[160];
    if (node >= 0) std::snprintf(buf, sizeof buf, "psr node %d: %s", node, what);
    else std::snprintf(buf, sizeof buf, "psr: %s", what);
    *err = buf;
  }
  return PLFX_ERR_INVALID;
}

}  // namespace

int lower_psr(const PsrCall &call, const plfx_psr_node *nodes, int count, PsrLaunchList *out, std::string *err) {
  out->clear();
  if (call.dtype != PLFX_F32 && call.dtype != PLFX_F64) return refuse(out, err, "bad dtype");
  if (call.ncat < 1 || call.ncat > PLFX_PSR_MAX_CATS) return refuse(out, err, "ncat outside 1..PLFX_PSR_MAX_CATS");
  if (count < 1 || !nodes) return refuse(out, err, "needs count >= 1 nodes");
  if (call.n < 0) return refuse(out, err, "n < 0");
  if (call.n == 0) return PLFX_OK;
  if (!call.EV || !call.rate_cat) return refuse(out, err, "null EV / rate_cat");

  const size_t cb = psr_clv_bytes(call.dtype, call.n), tb = (size_t)call.n;
  for (int i = 0; i < count; i++) {
    const plfx_psr_node &d = nodes[i];
    if ((d.tip1 != nullptr) == (d.x1 != nullptr)) return refuse(out, err, "child 1 needs exactly one of tip / CLV", i);
    if ((d.tip2 != nullptr) == (d.x2 != nullptr)) return refuse(out, err, "child 2 needs exactly one of tip / CLV", i);
    if (!d.x3 || !d.left || !d.right) return refuse(out, err, "null x3 / left / right", i);
    if ((d.x1 && !aligned16(d.x1)) || (d.x2 && !aligned16(d.x2)) || !aligned16(d.x3))
      return refuse(out, err, "CLV pointers must be 16-byte aligned", i);
    if (overlap(d.x3, cb, d.tip1 ? (const void *)d.tip1 : d.x1, d.tip1 ? tb : cb) ||
        overlap(d.x3, cb, d.tip2 ? (const void *)d.tip2 : d.x2, d.tip2 ? tb : cb))
      return refuse(out, err, "x3 may not overlap a child it reads", i);
  }

  out->nodes.reserve((size_t)count);
  for (int tips = 0; tips < 4; tips++) {
    const int first = (int)out->nodes.size();
    for (int i = 0; i < count; i++) {
      const plfx_psr_node &d = nodes[i];
      if (((d.tip1 ? 1 : 0) | (d.tip2 ? 2 : 0)) != tips) continue;
      out->nodes.push_back(NodeDescH{d.tip1 ? (const void *)d.tip1 : d.x1, d.tip2 ? (const void *)d.tip2 : d.x2, d.x3,
                                     d.left, d.right, d.scaler, d.scaler_sum});
    }
    const int end = (int)out->nodes.size();
    for (int f = first; f < end; f += kMaxBatch) out->items.push_back(PsrLaunch{tips, f, std::min(kMaxBatch, end - f)});
  }
  return PLFX_OK;
}

}  // namespace plfx
