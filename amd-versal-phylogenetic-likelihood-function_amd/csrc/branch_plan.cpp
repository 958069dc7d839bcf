// branch_plan.cpp -- see branch_plan.hpp.
#include "branch_plan.hpp"

#include <algorithm>
#include <cstdio>

#include "trav_lower.hpp"  // aligned16, overlap

namespace plfx {
namespace {

int refuse(BranchPlan *out, std::string *err, const char *what, int op = -1) {
  out->clear();
  if (err) {
    char buf[200];
    if (op >= 0) std::snprintf(buf, sizeof buf, "psr branches op %d: %s", op, what);
    else std::snprintf(buf, sizeof buf, "psr branches: %s", what);
    *err = buf;
  }
  return PLFX_ERR_INVALID;
}

size_t align256(size_t b) { return (b + 255u) & ~(size_t)255u; }

}  // namespace

void BranchPlan::clear() {
  lay = BranchLayout{};
  nlev = 0;
  level.clear();
  up_edge.clear();
  pup.clear();
  wv.clear();
  wv_coded.clear();
  fused.clear();
  w.clear();
  tab.clear();
  wsum.clear();
  items.clear();
  pairs.clear();
  nodes.clear();
  edges.clear();
  scale.clear();
  sub = outer = nullptr;
}

int branch_layout(int dtype, int states, int nops, int64_t n, BranchLayout *lay) {
  if ((dtype != PLFX_F32 && dtype != PLFX_F64) || (states != 4 && states != 20) || nops < 1 || n < 0 || !lay)
    return PLFX_ERR_INVALID;
  lay->slab = align256(psr_clv_bytes(dtype, n, states));
  lay->w_off = 0;
  lay->tab_off = 2 * (size_t)(nops - 1) * lay->slab;
  lay->cnt_off = lay->tab_off + (2 * (size_t)nops - 1) * lay->slab;
  lay->bytes = lay->cnt_off + align256(5 * (size_t)nops * sizeof(int64_t));
  return PLFX_OK;
}

int plan_branches(const BranchCall &c, BranchPlan *out, std::string *err) {
  out->clear();
  // ---- the call ----
  if (c.dtype != PLFX_F32 && c.dtype != PLFX_F64) return refuse(out, err, "bad dtype");
  if (c.states != 4 && c.states != 20) return refuse(out, err, "states must be 4 or 20");
  if (c.flags & ~(PLFX_FMA | PLFX_BRANCH_NOFUSE)) return refuse(out, err, "bad flags");
  if (c.ncat < 1 || c.ncat > PLFX_PSR_MAX_CATS) return refuse(out, err, "ncat outside 1..PLFX_PSR_MAX_CATS");
  if (c.n < 0) return refuse(out, err, "n < 0");
  if (c.nops < 1 || !c.ops) return refuse(out, err, "needs nops >= 1 ops");
  if (c.nslots < 1 || c.npmats < 1) return refuse(out, err, "needs nslots >= 1 and npmats >= 1");

  // ---- the tree: one rooted binary tree in post-order, the last op its root ----
  const int nops = c.nops, root = nops - 1;
  auto coded = [&](int slot) { return c.tips && c.tips[slot] != nullptr; };
  std::vector<int> writer((size_t)c.nslots, -1), reader((size_t)c.nslots, -1), side((size_t)c.nslots, 0);
  for (int j = 0; j < nops; j++) {
    const plfx_trav_op &o = c.ops[j];
    const int ch[2] = {o.child1, o.child2};
    if (o.parent < 0 || o.parent >= c.nslots || ch[0] < 0 || ch[0] >= c.nslots || ch[1] < 0 || ch[1] >= c.nslots)
      return refuse(out, err, "slot out of range", j);
    if (o.pmat < 0 || o.pmat >= c.npmats) return refuse(out, err, "pmat out of range", j);
    if (o.parent == ch[0] || o.parent == ch[1] || ch[0] == ch[1])
      return refuse(out, err, "an op names one slot twice", j);
    if (coded(o.parent)) return refuse(out, err, "a tip slot may not be a parent", j);
    if (writer[(size_t)o.parent] >= 0) return refuse(out, err, "the parent slot is written twice", j);
    if (reader[(size_t)o.parent] >= 0) return refuse(out, err, "the parent slot was read by an earlier op", j);
    for (int s = 0; s < 2; s++) {
      if (reader[(size_t)ch[s]] >= 0) return refuse(out, err, "a child slot is read twice: not a tree", j);
      reader[(size_t)ch[s]] = j;
      side[(size_t)ch[s]] = s;
    }
    writer[(size_t)o.parent] = j;
  }
  for (int j = 0; j < root; j++)
    if (reader[(size_t)c.ops[j].parent] < 0)
      return refuse(out, err, "the parent slot is never read: a forest (the last op must be the root op)", j);
  const plfx_trav_op &ro = c.ops[root];
  if (coded(ro.child1) && coded(ro.child2))
    return refuse(out, err, "the root op's two children may not both be coded tips", root);

  // ---- the workspace ----
  BranchLayout lay;
  if (branch_layout(c.dtype, c.states, nops, c.n, &lay) != PLFX_OK) return refuse(out, err, "bad layout arguments");
  if (!c.workspace) return refuse(out, err, "null workspace");
  if (reinterpret_cast<uintptr_t>(c.workspace) & 255u) return refuse(out, err, "the workspace must be 256-byte aligned");
  if (c.workspace_bytes < lay.bytes) return refuse(out, err, "the workspace is too short");
  if (c.edge_scale && !c.scaler_sums) return refuse(out, err, "edge_scale needs scaler_sums");
  if (c.edge_scale && overlap(c.workspace, lay.bytes, c.edge_scale, 2 * (size_t)nops * sizeof(int64_t)))
    return refuse(out, err, "edge_scale shares a byte with the workspace");
  const bool run = c.n > 0;
  const size_t cb = psr_clv_bytes(c.dtype, c.n, c.states), tb = (size_t)c.n;
  if (run) {
    if (!c.EV || !c.rate_cat) return refuse(out, err, "null EV / rate_cat");
    if (!c.pmats || !c.clv || !c.root_pmat) return refuse(out, err, "null pmats / clv / root_pmat");
    for (int j = 0; j < nops; j++) {
      const int sl[3] = {c.ops[j].child1, c.ops[j].child2, c.ops[j].parent};
      for (int s = 0; s < 3; s++) {
        const bool t = s < 2 && coded(sl[s]);
        const void *p = t ? (const void *)c.tips[sl[s]] : c.clv[sl[s]];
        if (t && !c.tipvec)
          return refuse(out, err, "a coded tip needs tipvec (the default 0/1 table is not in eigen coordinates)", j);
        if (!p) return refuse(out, err, "null CLV of a slot that is no coded tip", j);
        if (!t && !aligned16(p)) return refuse(out, err, "CLV pointers must be 16-byte aligned", j);
        if (overlap(c.workspace, lay.bytes, p, t ? tb : cb))
          return refuse(out, err, "a slot shares a byte with the workspace", j);
      }
    }
  }

  // ---- levels, Pup, W(v), slabs ----
  BranchPlan &pl = *out;
  pl.lay = lay;
  char *ws = static_cast<char *>(c.workspace);
  int64_t *cnt = reinterpret_cast<int64_t *>(ws + lay.cnt_off);
  pl.sub = cnt + 2 * (size_t)nops;
  pl.outer = cnt + 3 * (size_t)nops;
  pl.level.assign((size_t)nops, 0);
  pl.up_edge.assign((size_t)nops, -1);
  pl.pup.assign((size_t)nops, nullptr);
  pl.wv.assign((size_t)nops, nullptr);
  pl.wv_coded.assign((size_t)nops, 0);
  pl.fused.assign((size_t)nops, 0);
  pl.w.assign(2 * (size_t)nops, nullptr);
  pl.tab.assign(2 * (size_t)nops, nullptr);
  pl.wsum.assign(2 * (size_t)nops, nullptr);
  const size_t mat_bytes = (size_t)c.ncat * c.states * c.states * (c.dtype == PLFX_F32 ? 4 : 8);
  const char *pmats = static_cast<const char *>(c.pmats);
  for (int e = 0; e < 2 * nops; e++) {
    const bool re = e >= 2 * root;  // the root op's two branches are one edge: one table, no W of their own
    pl.tab[(size_t)e] = ws + lay.tab_off + (size_t)(re ? 2 * root : e) * lay.slab;
    if (!re) {
      pl.w[(size_t)e] = ws + lay.w_off + (size_t)e * lay.slab;
      if (c.edge_scale) pl.wsum[(size_t)e] = cnt + e;
    }
  }
  const bool fuse_ok = c.states == 4 && !(c.flags & PLFX_BRANCH_NOFUSE);
  for (int j = root - 1; j >= 0; j--) {  // post-order: the reader of op j's parent comes after j
    const int v = c.ops[j].parent, r = reader[(size_t)v], s = side[(size_t)v];
    pl.level[(size_t)j] = pl.level[(size_t)r] + 1;
    pl.nlev = std::max(pl.nlev, pl.level[(size_t)j]);
    pl.up_edge[(size_t)j] = 2 * r + s;
    if (r == root) {  // W(v) is the root op's other child itself, across the joined root branch
      const int sib = s ? ro.child1 : ro.child2;
      pl.wv_coded[(size_t)j] = coded(sib);
      if (run) pl.wv[(size_t)j] = coded(sib) ? (const void *)c.tips[sib] : c.clv[sib];
      pl.pup[(size_t)j] = c.root_pmat;
    } else {
      pl.wv[(size_t)j] = pl.w[(size_t)(2 * r + s)];
      pl.pup[(size_t)j] = pmats + (size_t)(2 * c.ops[r].pmat + s) * mat_bytes;
    }
    pl.fused[(size_t)j] = fuse_ok && !pl.wv_coded[(size_t)j];
  }
  pl.nlev += 1;
  if (!run) return PLFX_OK;

  // ---- the launch list, stage by stage ----
  const PsrCall pc{c.dtype, c.n, c.ncat, c.EV, c.rate_cat, c.states, c.states == 20 ? (c.flags & PLFX_FMA) : 0};
  PsrLaunchList nl;
  PsrEdgeLaunchList el;
  std::vector<plfx_psr_node> nd;
  std::vector<plfx_psr_edge> ed;
  std::vector<BranchPairDescH> pb[3];
  std::string sub_err;
  auto slot_ptr = [&](int slot) { return coded(slot) ? (const void *)c.tips[slot] : (const void *)c.clv[slot]; };
  for (int lv = 0; lv < pl.nlev; lv++) {
    nd.clear();
    ed.clear();
    for (auto &v : pb) v.clear();
    if (lv == 0) {  // the root edge: x_a * x_b, a coded child as side 1
      const int a = coded(ro.child2) ? ro.child2 : ro.child1, b = a == ro.child1 ? ro.child2 : ro.child1;
      ed.push_back(plfx_psr_edge{coded(a) ? c.tips[a] : nullptr, coded(a) ? nullptr : c.clv[a], c.clv[b],
                                 pl.tab[(size_t)(2 * root)]});
    }
    for (int j = 0; j < root && lv > 0; j++) {
      if (pl.level[(size_t)j] != lv) continue;
      const plfx_trav_op &o = c.ops[j];
      const int ch[2] = {o.child1, o.child2};
      const void *mat[2] = {pmats + (size_t)(2 * o.pmat) * mat_bytes, pmats + (size_t)(2 * o.pmat + 1) * mat_bytes};
      if (pl.fused[(size_t)j]) {
        const int f = (!coded(ch[0]) && coded(ch[1])) ? 1 : 0, g = 1 - f;  // coded child first
        const int ef = 2 * j + f, eg = 2 * j + g;
        pb[(coded(ch[0]) ? 1 : 0) + (coded(ch[1]) ? 1 : 0)].push_back(BranchPairDescH{
            pl.wv[(size_t)j], slot_ptr(ch[f]), slot_ptr(ch[g]), pl.pup[(size_t)j], mat[f], mat[g],
            coded(ch[f]) ? nullptr : pl.w[(size_t)ef], coded(ch[g]) ? nullptr : pl.w[(size_t)eg], pl.tab[(size_t)ef],
            pl.tab[(size_t)eg], pl.wsum[(size_t)ef], pl.wsum[(size_t)eg]});
        continue;
      }
      const bool wc = pl.wv_coded[(size_t)j] != 0;
      for (int s = 0; s < 2; s++) {  // W(child s): x1 = W(v) across Pup, x2 = the sibling across its own matrix
        const int e = 2 * j + s, sib = ch[1 - s];
        nd.push_back(plfx_psr_node{wc ? (const uint8_t *)pl.wv[(size_t)j] : nullptr, wc ? nullptr : pl.wv[(size_t)j],
                                   coded(sib) ? c.tips[sib] : nullptr, coded(sib) ? nullptr : c.clv[sib],
                                   pl.w[(size_t)e], pl.pup[(size_t)j], mat[1 - s], nullptr, pl.wsum[(size_t)e]});
        ed.push_back(plfx_psr_edge{coded(ch[s]) ? c.tips[ch[s]] : nullptr, coded(ch[s]) ? nullptr : c.clv[ch[s]],
                                   pl.w[(size_t)e], pl.tab[(size_t)e]});
      }
    }
    for (int k = 0; k < 3; k++) {
      const int first = (int)pl.pairs.size(), count = (int)pb[k].size();
      pl.pairs.insert(pl.pairs.end(), pb[k].begin(), pb[k].end());
      for (int i = 0; i < count; i += kMaxPairs)
        pl.items.push_back(BranchLaunch{kBranchPairs, lv, k, first + i, std::min(kMaxPairs, count - i)});
    }
    if (!nd.empty()) {
      if (lower_psr(pc, nd.data(), (int)nd.size(), &nl, &sub_err) != PLFX_OK) return refuse(out, err, sub_err.c_str());
      const int base = (int)pl.nodes.size();
      pl.nodes.insert(pl.nodes.end(), nl.nodes.begin(), nl.nodes.end());
      for (const PsrLaunch &it : nl.items)
        pl.items.push_back(BranchLaunch{kBranchNodes, lv, it.tips, base + it.first, it.count});
    }
    if (!ed.empty()) {
      if (lower_psr_edges(c.dtype, c.n, c.tipvec, ed.data(), (int)ed.size(), &el, &sub_err, c.states) != PLFX_OK)
        return refuse(out, err, sub_err.c_str());
      const int base = (int)pl.edges.size();
      pl.edges.insert(pl.edges.end(), el.edges.begin(), el.edges.end());
      for (const PsrEdgeLaunch &it : el.items)
        pl.items.push_back(BranchLaunch{kBranchTables, lv, it.tip, base + it.first, it.count});
    }
  }

  // ---- the counters: subtree sums up the list, outer sums and edge_scale down it ----
  if (c.edge_scale) {
    for (int j = 0; j < nops; j++)
      pl.scale.push_back(BranchScaleDescH{writer[(size_t)c.ops[j].child1], writer[(size_t)c.ops[j].child2],
                                          pl.up_edge[(size_t)j]});
    const int chunks = (nops + kScaleChunk - 1) / kScaleChunk;
    for (int k = 0; k < chunks; k++)
      pl.items.push_back(BranchLaunch{kBranchSub, pl.nlev, 0, k * kScaleChunk, std::min(kScaleChunk, nops - k * kScaleChunk)});
    for (int k = chunks - 1; k >= 0; k--)
      pl.items.push_back(BranchLaunch{kBranchScale, pl.nlev, 0, k * kScaleChunk, std::min(kScaleChunk, nops - k * kScaleChunk)});
  }
  return PLFX_OK;
}

}  // namespace plfx
