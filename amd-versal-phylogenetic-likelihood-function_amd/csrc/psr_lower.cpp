// psr_lower.cpp -- see psr_lower.hpp.
#include "psr_lower.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>

namespace plfx {
namespace {

// how an entry point's refusals begin: a fault of the call, of node / op i
struct Prefix {
  const char *call, *unit;
};
constexpr Prefix kBatch{"psr", "psr node"}, kTrav{"psr traverse", "psr traverse op"};

int refuse(PsrLaunchList *out, std::string *err, const Prefix &who, const char *what, int i = -1) {
  out->clear();
  if (err) {
    char buf[160];
    if (i >= 0) std::snprintf(buf, sizeof buf, "%s %d: %s", who.unit, i, what);
    else std::snprintf(buf, sizeof buf, "%s: %s", who.call, what);
    *err = buf;
  }
  return PLFX_ERR_INVALID;
}

// What both entry points check of the call, in the order its faults are
// reported: dtype, ncat, n >= 0, the entry point's own arguments (`own`: their
// fault or NULL) and, unless nothing is to run (*run = false: n == 0 or
// `none`), EV and rate_cat.  Returns the fault or NULL.
const char *check_call(const PsrCall &c, const char *own, bool none, bool *run) {
  *run = false;
  if (c.dtype != PLFX_F32 && c.dtype != PLFX_F64) return "bad dtype";
  if (c.states != 4 && c.states != 20) return "states must be 4 or 20";
  if (c.ncat < 1 || c.ncat > PLFX_PSR_MAX_CATS) return "ncat outside 1..PLFX_PSR_MAX_CATS";
  if (c.n < 0) return "n < 0";
  if (own) return own;
  if (c.n == 0 || none) return nullptr;
  if (!c.EV || !c.rate_cat) return "null EV / rate_cat";
  *run = true;
  return nullptr;
}

// One node of plfx.h section 11, x1 / x2 naming the codes of a coded child
// (t1 / t2): cb bytes of a CLV, n code bytes.  Returns the fault or NULL.
const char *check_node(const plfx_node &d, bool t1, bool t2, size_t cb, size_t n) {
  if (!d.x1 || !d.x2 || !d.x3 || !d.left || !d.right) return "null CLV / tip / matrix pointer";
  if ((!t1 && !aligned16(d.x1)) || (!t2 && !aligned16(d.x2)) || !aligned16(d.x3))
    return "CLV pointers must be 16-byte aligned";
  if (overlap(d.x3, cb, d.x1, t1 ? n : cb) || overlap(d.x3, cb, d.x2, t2 ? n : cb))
    return "the parent may not overlap a child it reads";
  return nullptr;
}

// nb[k]: the nodes of `level` whose children are of kind k, in launches of kMaxBatch
void add_nodes(PsrLaunchList *out, int level, const std::vector<NodeDescH> (&nb)[4]) {
  for (int k = 0; k < 4; k++) {
    const int first = (int)out->nodes.size(), count = (int)nb[k].size();
    out->nodes.insert(out->nodes.end(), nb[k].begin(), nb[k].end());
    for (int i = 0; i < count; i += kMaxBatch)
      out->items.push_back(PsrLaunch{kPsrNodes, level, k, first + i, std::min(kMaxBatch, count - i)});
  }
}

}  // namespace

int lower_psr(const PsrCall &call, const plfx_psr_node *nodes, int count, PsrLaunchList *out, std::string *err) {
  out->clear();
  bool run;
  if (const char *f = check_call(call, count < 1 || !nodes ? "needs count >= 1 nodes" : nullptr, false, &run))
    return refuse(out, err, kBatch, f);
  if (!run) return PLFX_OK;

  const size_t cb = psr_clv_bytes(call.dtype, call.n, call.states);
  std::vector<NodeDescH> nb[4];
  for (int i = 0; i < count; i++) {
    const plfx_psr_node &d = nodes[i];
    if ((d.tip1 != nullptr) == (d.x1 != nullptr)) return refuse(out, err, kBatch, "child 1 needs exactly one of tip / CLV", i);
    if ((d.tip2 != nullptr) == (d.x2 != nullptr)) return refuse(out, err, kBatch, "child 2 needs exactly one of tip / CLV", i);
    const bool t1 = d.tip1 != nullptr, t2 = d.tip2 != nullptr;
    const plfx_node nd{t1 ? (const void *)d.tip1 : d.x1, t2 ? (const void *)d.tip2 : d.x2, d.x3, d.left, d.right,
                       d.scaler, d.scaler_sum};
    if (const char *f = check_node(nd, t1, t2, cb, (size_t)call.n)) return refuse(out, err, kBatch, f, i);
    nb[(t1 ? 1 : 0) | (t2 ? 2 : 0)].push_back(node_desc(nd));
  }
  add_nodes(out, 0, nb);
  return PLFX_OK;
}

int lower_psr_traversal(const TravPlan &plan, const TravArrays &t, const PsrCall &call, PsrLaunchList *out,
                        std::string *err) {
  out->clear();
  bool run;
  if (const char *f = check_call(call, t.nops < 0 || (t.nops > 0 && !t.ops) ? "null ops" : nullptr, t.nops == 0, &run))
    return refuse(out, err, kTrav, f);
  if (!run) return PLFX_OK;
  if (!t.pmats || !t.clv) return refuse(out, err, kTrav, "null pmats / clv");
  if ((int)plan.level.size() != t.nops || (int)plan.fused.size() != t.nops)
    return refuse(out, err, kTrav, "the plan is not this op list's");

  const size_t cb = psr_clv_bytes(call.dtype, call.n, call.states), tb = (size_t)call.n;
  const size_t mat_bytes = (size_t)call.ncat * call.states * call.states * (call.dtype == PLFX_F32 ? 4 : 8);
  const bool pairs = call.states == 4;  // the fused level pair exists for 4 states only
  for (int j = 0; j < t.nops; j++) {
    const OpNode d = op_node(t, mat_bytes, j);
    if (const char *f = check_node(d.nd, d.t1, d.t2, cb, tb)) return refuse(out, err, kTrav, f, j);
  }
  // every triple: three outputs written and four leaves read by one launch
  for (const TravGroup &g : plan.groups) {
    if (!pairs) break;
    if (g.kind != kTravTriple || g.ops.size() != 3 || g.tips < 0 || g.tips > 2)
      return refuse(out, err, kTrav, "the plan holds a fused group other than a level pair");
    const OpNode A = op_node(t, mat_bytes, g.ops[0]), B = op_node(t, mat_bytes, g.ops[1]);
    const void *outs[3] = {A.nd.x3, B.nd.x3, t.clv[t.ops[g.ops[2]].parent]};
    const std::pair<const void *, size_t> leaves[4] = {{A.nd.x1, A.t1 ? tb : cb}, {A.nd.x2, A.t2 ? tb : cb},
                                                       {B.nd.x1, B.t1 ? tb : cb}, {B.nd.x2, B.t2 ? tb : cb}};
    for (int i = 0; i < 3; i++) {
      for (int k = i + 1; k < 3; k++)
        if (overlap(outs[i], cb, outs[k], cb))
          return refuse(out, err, kTrav, "two outputs of a fused level pair overlap", g.ops[2]);
      for (const auto &lf : leaves)
        if (overlap(outs[i], cb, lf.first, lf.second))
          return refuse(out, err, kTrav, "an output of a fused level pair overlaps one of its leaves", g.ops[2]);
    }
  }

  std::vector<TripleDescH> tb3[3];
  std::vector<NodeDescH> nb[4];
  for (int lv = 0; lv < plan.nlev; lv++) {
    for (auto &v : tb3) v.clear();
    for (auto &v : nb) v.clear();
    for (const TravGroup &g : plan.groups) {
      if (!pairs || g.level != lv) continue;
      const int a = g.ops[0], b = g.ops[1], p = g.ops[2];
      const plfx_node A = tip_first(op_node(t, mat_bytes, a)).nd, B = tip_first(op_node(t, mat_bytes, b)).nd;
      // P's children as op P names them: child1 = A's slot or B's slot
      const bool a_first = t.ops[p].child1 == t.ops[a].parent;
      tb3[g.tips].push_back(triple_desc(a_first ? A : B, a_first ? B : A, op_node(t, mat_bytes, p).nd));
    }
    for (int j = 0; j < t.nops; j++) {
      if (plan.level[j] != lv || (pairs && plan.fused[j])) continue;
      const OpNode d = op_node(t, mat_bytes, j);
      nb[(d.t1 ? 1 : 0) | (d.t2 ? 2 : 0)].push_back(node_desc(d.nd));
    }
    for (int k = 0; k < 3; k++) {
      const int first = (int)out->triples.size(), count = (int)tb3[k].size();
      out->triples.insert(out->triples.end(), tb3[k].begin(), tb3[k].end());
      for (int i = 0; i < count; i += kMaxTriples)
        out->items.push_back(PsrLaunch{kPsrTriples, lv, k, first + i, std::min(kMaxTriples, count - i)});
    }
    add_nodes(out, lv, nb);
  }
  return PLFX_OK;
}

}  // namespace plfx
