// trav_lower.cpp -- see trav_lower.hpp.
#include "trav_lower.hpp"

#include <algorithm>
#include <cstdio>

namespace plfx {
namespace {

int invalid(std::string *err, int i, const char *what) {
  char buf[128];
  snprintf(buf, sizeof buf, "node %d: %s", i, what);
  if (err) *err = buf;
  return PLFX_ERR_INVALID;
}

// One node of a kind (tips = number of tip children, tip child first); i
// names it in the message (the op index in a traversal).  The parent may not
// share a byte with either child (a CLV is clv_bytes, a tip child n code
// bytes): every site's children are read by other blocks than the one
// writing that site's parent.
int check_node(const plfx_node &d, int tips, int64_t n, int i, size_t clv_bytes, std::string *err) {
  if (n <= 0) return PLFX_OK;
  if (!d.x1 || !d.x2 || !d.x3 || !d.left || !d.right) return invalid(err, i, "null CLV/tip/matrix pointer");
  if ((tips < 1 && !aligned16(d.x1)) || (tips < 2 && !aligned16(d.x2)) || !aligned16(d.x3))
    return invalid(err, i, "CLV pointers must be 16-byte aligned");
  const size_t b1 = tips >= 1 ? (size_t)n : clv_bytes, b2 = tips >= 2 ? (size_t)n : clv_bytes;
  if (overlap(d.x3, clv_bytes, d.x1, b1) || overlap(d.x3, clv_bytes, d.x2, b2))
    return invalid(err, i, "x3 may not overlap a child");
  return PLFX_OK;
}

void add(LaunchList *out, int kind, int level, int tips, int depth, size_t first, int count) {
  out->items.push_back(LaunchItem{kind, level, tips, depth, (int)first, count});
}

// A tip/tip protein node whose values sit in its stream's combination tables
// after its launch pair: its CLV (x3), its table and its two tip-code arrays.
struct TabRef {
  const void *x3;
  const void *tab;
  const uint8_t *ca, *cb;
};

// lower_batch after the checks, appending to *out.  *tabs (may be NULL)
// receives the tip/tip protein nodes whose tables are still in the stream's
// workspace afterwards (the last launch group's).
void batch(const LowerCall &call, const plfx_node *nodes, int count, int tips, int level, LaunchList *out,
           std::vector<TabRef> *tabs) {
  if (call.states == 20 && tips == 2) {
    // both children coded tips: the node's 576 code pairs through its own
    // kernel, then x3 / scaler / sum gathered by code pair (a write stream;
    // the direct kernel is compute-bound: 77 us f64, 95 us f32 per 2^18 sites)
    const uint8_t *cc1 = call.tt_codes, *cc2 = cc1 + 1024;
    for (int j = 0; j < count; j += kMaxBatch) {
      const int c = std::min(count - j, kMaxBatch);
      if (tabs) tabs->clear();  // this group's tables stay until the next group overwrites them
      add(out, kLaunchProtTipTip, level, tips, 0, out->combs.size(), c);
      for (int i = 0; i < c; i++) {
        const plfx_node &d = nodes[j + i];
        char *tab = call.tt + (size_t)i * (kTtTabBytes + kTtScBytes);
        uint8_t *tsc = reinterpret_cast<uint8_t *>(tab + kTtTabBytes);
        const uint8_t *c1 = static_cast<const uint8_t *>(d.x1), *c2 = static_cast<const uint8_t *>(d.x2);
        out->combs.push_back(NodeDescH{cc1, cc2, tab, d.left, d.right, tsc, nullptr});
        out->gathers.push_back(ProtGatherDescH{c1, c2, d.x3, d.scaler, d.scaler_sum, tab, tsc});
        if (tabs) tabs->push_back(TabRef{d.x3, tab, c1, c2});
      }
    }
    return;
  }
  if (call.states == 20) {
    // protein: one node alone is one full-GPU launch (plf_prot.hpp); more go
    // up to kMaxBatch per launch, node = blockIdx.y, each node with the full
    // resident grid so the nodes' blocks follow each other through the
    // co-resident slots (the next node's blocks fill the CUs the previous
    // node's last trips leave idle).  64-taxon tree at 2^18 sites per sweep
    // vs one launch per node: f64 FMA 5.67 -> 5.38 ms, f64 exact 8.45 ->
    // 8.02 ms, f32 FMA 2.94 -> 2.66 ms; splitting the resident grid over the
    // nodes (the DNA batches' rule) gains only 1-3 % (tools/prot_batch_ab.py@f9b3af3,
    // profiles/r03_protein_batch_ab.log).
    for (int j = 0; j < count; j += kMaxBatch)
      add(out, count == 1 ? kLaunchProtNode : kLaunchProtBatch, level, tips, 0, out->nodes.size() + j,
          std::min(count - j, kMaxBatch));
    for (int i = 0; i < count; i++) out->nodes.push_back(node_desc(nodes[i]));
    return;
  }
  // More than kMaxBatch nodes: launch j takes nodes j, j + L, j + 2L, ... (L
  // launches), so every launch mixes nodes from across the caller's list.
  // Consecutive nodes are usually consecutive allocations, and a launch made of
  // 32 neighbouring allocations of 128 MiB ran up to 15 % slower than a mixed
  // one while each of its nodes alone ran at the same speed (nodes512 at N = 1:
  // launches of 2.09-2.48 ms consecutive, 2.10-2.12 ms interleaved;
  // tools/probes/nodes_groups.py, nodes_sched.py, HISTORY.md section 5).
  const int L = (count + kMaxBatch - 1) / kMaxBatch;
  for (int j = 0; j < L; j++) {
    const size_t first = out->nodes.size();
    for (int i = j; i < count; i += L) out->nodes.push_back(node_desc(nodes[i]));
    add(out, kLaunchDnaBatch, level, tips, 0, first, (int)(out->nodes.size() - first));
  }
}

int checked_batch(const LowerCall &call, const plfx_node *nodes, int count, int tips, const int *ids, int level,
                  LaunchList *out, std::vector<TabRef> *tabs, std::string *err) {
  const size_t cb = clv_bytes_of(call.dtype, call.states, call.n);
  for (int i = 0; i < count; i++) {
    const int rc = check_node(nodes[i], tips, call.n, ids ? ids[i] : i, cb, err);
    if (rc != PLFX_OK) return rc;
  }
  batch(call, nodes, count, tips, level, out, tabs);
  return PLFX_OK;
}

// The ops of a traversal call as node descriptors.
struct TravNodes {
  const TravArrays &t;
  size_t mat_bytes;  // of one matrix (C*S*S values)
  // the node descriptor of op j, tip child first (dense/tip runs as tip/dense:
  // the product u1*u2 commutes exactly); *kind = number of tip children
  plfx_node node(int j, int *kind) const {
    const OpNode o = tip_first(op_node(t, mat_bytes, j));
    *kind = o.t1 + o.t2;
    return o.nd;
  }
};

// The descriptor of a fused pass (DeepDescH, SeptetDescH) over the ops ids[0..count),
// each checked as a node; the first `leaves` of them are the leaf ops, whose
// children are the pass's inputs g.  A septet's leaf ops come tip child first
// (node()); a deep pass's leaves are all dense or all tips, so there child1,
// child2 stay as the op names them.
template <typename Desc>
int fill_fused(const TravNodes &tn, const int *ids, int count, int leaves, int64_t n, size_t clv_bytes, Desc *d,
               std::string *err) {
  for (int q = 0; q < count; q++) {
    int kq;
    const plfx_node nd = tn.node(ids[q], &kq);
    const int rc = check_node(nd, kq, n, ids[q], clv_bytes, err);
    if (rc != PLFX_OK) return rc;
    if (q < leaves) {
      d->g[2 * q] = nd.x1;
      d->g[2 * q + 1] = nd.x2;
    }
    d->x[q] = nd.x3;
    d->mat[2 * q] = nd.left;
    d->mat[2 * q + 1] = nd.right;
    d->sc[q] = nd.scaler;
    d->ss[q] = nd.scaler_sum;
  }
  return PLFX_OK;
}

int lower_levels(const TravPlan &plan, const TravArrays &t, const LowerCall &call, LaunchList *out,
                 std::string *err) {
  const int64_t n = call.n;
  const size_t cb = clv_bytes_of(call.dtype, call.states, n);
  const TravNodes tn{t, (size_t)call.states * call.states * 4 * (call.dtype == PLFX_F32 ? 4 : 8)};
  std::vector<plfx_node> batch_nodes[3];  // the level's unfused ops by number of tip children
  std::vector<int> bop[3];                // the op index of each
  std::vector<TripleDescH> tb[3];
  std::vector<SeptetDescH> sb[3];
  // protein: the previous level's tip/tip nodes still in their
  // combination tables; a node of this level whose two children are among them
  // stages its child tiles from the tables (plf_prot.hpp kTab) instead of
  // reading the children's CLVs back from HBM.  Only for the next level: later
  // levels may overwrite the tables or the children's slots.
  std::vector<TabRef> prev_tabs, cur_tabs;
  const bool tab_mode = call.states == 20;
  for (int lv = 0; lv < plan.nlev; lv++) {
    for (int k = 0; k < 3; k++) {
      batch_nodes[k].clear();
      bop[k].clear();
      tb[k].clear();
      sb[k].clear();
    }
    // plan.groups holds the deep passes, then the septets, then the triples
    for (const TravGroup &g : plan.groups) {
      if (g.level != lv) continue;
      if (g.kind == kTravSeptet) {
        SeptetDescH d{};
        const int rc = fill_fused(tn, g.ops.data(), 7, 4, n, cb, &d, err);
        if (rc != PLFX_OK) return rc;
        sb[g.tips].push_back(d);
      } else if (g.kind == kTravTriple) {
        const int a = g.ops[0], b = g.ops[1], p = g.ops[2];
        int ka, kb, kp;
        const plfx_node A = tn.node(a, &ka), B = tn.node(b, &kb), P = tn.node(p, &kp);
        for (int rc : {check_node(A, ka, n, a, cb, err), check_node(B, kb, n, b, cb, err),
                       check_node(P, kp, n, p, cb, err)})
          if (rc != PLFX_OK) return rc;
        // P's children as op P names them: child1 = A's slot or B's slot
        const bool a_first = t.ops[p].child1 == t.ops[a].parent;
        const plfx_node &F = a_first ? A : B, &G = a_first ? B : A;
        tb[g.tips].push_back(triple_desc(F, G, P));
      } else {  // a deep pass: one launch each, ahead of the level's other work
        const int D = 6 - g.kind;
        add(out, kLaunchDeep, lv, g.tips, D, out->deeps.size(), 1);
        out->deeps.emplace_back();
        const int rc = fill_fused(tn, g.ops.data(), (1 << D) - 1, 1 << (D - 1), n, cb, &out->deeps.back(), err);
        if (rc != PLFX_OK) return rc;
      }
    }
    for (int j = 0; j < t.nops; j++) {
      if (plan.level[j] != lv || plan.fused[j]) continue;
      int kind;
      const plfx_node nd = tn.node(j, &kind);
      batch_nodes[kind].push_back(nd);
      bop[kind].push_back(j);
    }
    for (int k = 0; k < 3; k++) {
      for (size_t i = 0; i < sb[k].size(); i += kMaxSeptets)
        add(out, kLaunchSeptets, lv, k, 0, out->septets.size() + i,
            (int)std::min<size_t>(kMaxSeptets, sb[k].size() - i));
      out->septets.insert(out->septets.end(), sb[k].begin(), sb[k].end());
      for (size_t i = 0; i < tb[k].size(); i += kMaxTriples)
        add(out, kLaunchTriples, lv, k, 0, out->triples.size() + i,
            (int)std::min<size_t>(kMaxTriples, tb[k].size() - i));
      out->triples.insert(out->triples.end(), tb[k].begin(), tb[k].end());
      if (k == 0 && tab_mode && !prev_tabs.empty() && !batch_nodes[0].empty()) {
        auto find = [&](const void *x) -> const TabRef * {
          for (const TabRef &r : prev_tabs)
            if (r.x3 == x) return &r;
          return nullptr;
        };
        std::vector<plfx_node> rest;
        std::vector<int> rest_op;
        const size_t first = out->tabs.size();
        for (size_t q = 0; q < batch_nodes[0].size(); q++) {
          const plfx_node &nd = batch_nodes[0][q];
          const TabRef *a = find(nd.x1), *b = find(nd.x2);
          if (!a || !b) {
            rest.push_back(nd);
            rest_op.push_back(bop[0][q]);
            continue;
          }
          // these nodes do not go through checked_batch: checked here
          const int rc = check_node(nd, 0, n, bop[0][q], cb, err);
          if (rc != PLFX_OK) return rc;
          out->tabs.push_back(ProtTabDescH{a->tab, b->tab, a->ca, a->cb, b->ca, b->cb, nd.x3, nd.left, nd.right,
                                           nd.scaler, nd.scaler_sum});
        }
        for (size_t i = first; i < out->tabs.size(); i += kMaxBatch)
          add(out, kLaunchProtTab, lv, 0, 0, i, (int)std::min<size_t>(kMaxBatch, out->tabs.size() - i));
        batch_nodes[0].swap(rest);
        bop[0].swap(rest_op);
      }
      if (batch_nodes[k].empty()) continue;
      const int rc = checked_batch(call, batch_nodes[k].data(), (int)batch_nodes[k].size(), k, bop[k].data(), lv,
                                   out, k == 2 && tab_mode ? &cur_tabs : nullptr, err);
      if (rc != PLFX_OK) return rc;
    }
    prev_tabs.swap(cur_tabs);
    cur_tabs.clear();
  }
  return PLFX_OK;
}

}  // namespace

void LaunchList::clear() {
  items.clear();
  nodes.clear();
  combs.clear();
  gathers.clear();
  tabs.clear();
  triples.clear();
  septets.clear();
  deeps.clear();
}

int LaunchList::launches() const {
  int c = 0;
  for (const LaunchItem &it : items) c += it.kind == kLaunchProtTipTip ? 2 : 1;
  return c;
}

int lower_batch(const LowerCall &call, const plfx_node *nodes, int count, int tips, const int *ids,
                LaunchList *out, std::string *err) {
  out->clear();
  const int rc = checked_batch(call, nodes, count, tips, ids, 0, out, nullptr, err);
  if (rc != PLFX_OK) out->clear();
  return rc;
}

bool traversal_uses_tables(const TravArrays &t, int states) {
  if (states != 20 || !t.tips) return false;
  for (int j = 0; j < t.nops; j++)
    if (t.tips[t.ops[j].child1] && t.tips[t.ops[j].child2]) return true;
  return false;
}

int lower_traversal(const TravPlan &plan, const TravArrays &t, const LowerCall &call, LaunchList *out,
                    std::string *err) {
  out->clear();
  const int rc = lower_levels(plan, t, call, out, err);
  if (rc != PLFX_OK) out->clear();
  return rc;
}

}  // namespace plfx
