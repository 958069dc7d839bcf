// psr_trav_lower.cpp -- see psr_trav_lower.hpp.
#include "psr_trav_lower.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>

namespace plfx {
namespace {

int refuse(PsrTravList *out, std::string *err, const char *what, int op = -1) {
  out->clear();
  if (err) {
    char buf[160];
    if (op >= 0) std::snprintf(buf, sizeof buf, "psr traverse op %d: %s", op, what);
    else std::snprintf(buf, sizeof buf, "psr traverse: %s", what);
    *err = buf;
  }
  return PLFX_ERR_INVALID;
}

// Op j as a node: x1 / x2 name the codes of a coded child (t1 / t2).
struct OpNode {
  const void *x1, *x2;
  void *x3;
  const void *left, *right;
  uint8_t *scaler;
  int64_t *scaler_sum;
  bool t1, t2;
};

OpNode op_node(const TravArrays &t, size_t mat_bytes, int j) {
  const plfx_trav_op &o = t.ops[j];
  const char *pmats = static_cast<const char *>(t.pmats);
  const bool t1 = t.tips && t.tips[o.child1], t2 = t.tips && t.tips[o.child2];
  return OpNode{t1 ? (const void *)t.tips[o.child1] : t.clv[o.child1],
                t2 ? (const void *)t.tips[o.child2] : t.clv[o.child2],
                t.clv[o.parent],
                pmats + (size_t)(2 * o.pmat) * mat_bytes,
                pmats + (size_t)(2 * o.pmat + 1) * mat_bytes,
                t.scalers ? t.scalers[j] : nullptr,
                t.scaler_sums ? t.scaler_sums + j : nullptr,
                t1,
                t2};
}

// a triple's leaf op, coded child first
OpNode tip_first(OpNode nd) {
  if (!nd.t1 && nd.t2) {
    std::swap(nd.x1, nd.x2);
    std::swap(nd.left, nd.right);
    std::swap(nd.t1, nd.t2);
  }
  return nd;
}

}  // namespace

int lower_psr_traversal(const TravPlan &plan, const TravArrays &t, const PsrCall &call, PsrTravList *out,
                        std::string *err) {
  out->clear();
  if (call.dtype != PLFX_F32 && call.dtype != PLFX_F64) return refuse(out, err, "bad dtype");
  if (call.ncat < 1 || call.ncat > PLFX_PSR_MAX_CATS) return refuse(out, err, "ncat outside 1..PLFX_PSR_MAX_CATS");
  if (call.n < 0) return refuse(out, err, "n < 0");
  if (t.nops < 0 || (t.nops > 0 && !t.ops)) return refuse(out, err, "null ops");
  if (call.n == 0 || t.nops == 0) return PLFX_OK;
  if (!call.EV || !call.rate_cat || !t.pmats || !t.clv) return refuse(out, err, "null EV / rate_cat / pmats / clv");
  if ((int)plan.level.size() != t.nops || (int)plan.fused.size() != t.nops)
    return refuse(out, err, "the plan is not this op list's");

  // every op's node checks (plfx.h section 11)
  const size_t cb = psr_clv_bytes(call.dtype, call.n), tb = (size_t)call.n;
  const size_t mat_bytes = (size_t)call.ncat * 16 * (call.dtype == PLFX_F32 ? 4 : 8);
  for (int j = 0; j < t.nops; j++) {
    const OpNode d = op_node(t, mat_bytes, j);
    if (!d.x1 || !d.x2 || !d.x3) return refuse(out, err, "null CLV of a slot that is not a tip", j);
    if ((!d.t1 && !aligned16(d.x1)) || (!d.t2 && !aligned16(d.x2)) || !aligned16(d.x3))
      return refuse(out, err, "CLV pointers must be 16-byte aligned", j);
    if (overlap(d.x3, cb, d.x1, d.t1 ? tb : cb) || overlap(d.x3, cb, d.x2, d.t2 ? tb : cb))
      return refuse(out, err, "the parent may not overlap a child it reads", j);
  }
  // every triple: three outputs written and four leaves read by one launch
  for (const TravGroup &g : plan.groups) {
    if (g.kind != kTravTriple || g.ops.size() != 3 || g.tips < 0 || g.tips > 2)
      return refuse(out, err, "the plan holds a fused group other than a level pair");
    const OpNode A = op_node(t, mat_bytes, g.ops[0]), B = op_node(t, mat_bytes, g.ops[1]);
    const void *outs[3] = {A.x3, B.x3, t.clv[t.ops[g.ops[2]].parent]};
    const std::pair<const void *, size_t> leaves[4] = {
        {A.x1, A.t1 ? tb : cb}, {A.x2, A.t2 ? tb : cb}, {B.x1, B.t1 ? tb : cb}, {B.x2, B.t2 ? tb : cb}};
    for (int i = 0; i < 3; i++) {
      for (int k = i + 1; k < 3; k++)
        if (overlap(outs[i], cb, outs[k], cb))
          return refuse(out, err, "two outputs of a fused level pair overlap", g.ops[2]);
      for (const auto &lf : leaves)
        if (overlap(outs[i], cb, lf.first, lf.second))
          return refuse(out, err, "an output of a fused level pair overlaps one of its leaves", g.ops[2]);
    }
  }

  std::vector<TripleDescH> tb3[3];
  std::vector<NodeDescH> nb[4];
  for (int lv = 0; lv < plan.nlev; lv++) {
    for (auto &v : tb3) v.clear();
    for (auto &v : nb) v.clear();
    for (const TravGroup &g : plan.groups) {
      if (g.level != lv) continue;
      const int a = g.ops[0], b = g.ops[1], p = g.ops[2];
      const OpNode A = tip_first(op_node(t, mat_bytes, a)), B = tip_first(op_node(t, mat_bytes, b));
      const OpNode P = op_node(t, mat_bytes, p);
      // P's children as op P names them: child1 = A's slot or B's slot
      const bool a_first = t.ops[p].child1 == t.ops[a].parent;
      const OpNode &F = a_first ? A : B, &G = a_first ? B : A;
      tb3[g.tips].push_back(TripleDescH{
          F.x1, F.x2, G.x1, G.x2, F.x3, G.x3, P.x3, (const double *)F.left, (const double *)F.right,
          (const double *)G.left, (const double *)G.right, (const double *)P.left, (const double *)P.right,
          F.scaler, G.scaler, P.scaler, F.scaler_sum, G.scaler_sum, P.scaler_sum});
    }
    for (int j = 0; j < t.nops; j++) {
      if (plan.level[j] != lv || plan.fused[j]) continue;
      const OpNode d = op_node(t, mat_bytes, j);
      nb[(d.t1 ? 1 : 0) | (d.t2 ? 2 : 0)].push_back(NodeDescH{d.x1, d.x2, d.x3, d.left, d.right, d.scaler, d.scaler_sum});
    }
    for (int k = 0; k < 3; k++) {
      const int first = (int)out->triples.size(), count = (int)tb3[k].size();
      out->triples.insert(out->triples.end(), tb3[k].begin(), tb3[k].end());
      for (int i = 0; i < count; i += kMaxTriples)
        out->items.push_back(PsrTravItem{kPsrTravTriples, lv, k, first + i, std::min(kMaxTriples, count - i)});
    }
    for (int k = 0; k < 4; k++) {
      const int first = (int)out->nodes.size(), count = (int)nb[k].size();
      out->nodes.insert(out->nodes.end(), nb[k].begin(), nb[k].end());
      for (int i = 0; i < count; i += kMaxBatch)
        out->items.push_back(PsrTravItem{kPsrTravNodes, lv, k, first + i, std::min(kMaxBatch, count - i)});
    }
  }
  return PLFX_OK;
}

}  // namespace plfx
