// trav_plan.cpp -- see trav_plan.hpp.
#include "trav_plan.hpp"

#include <algorithm>
#include <cstdio>

namespace plfx {
namespace {

struct Planner {
  const plfx_trav_op *ops;
  int nops;
  const unsigned char *slot_is_tip;
  TravPlan &plan;
  // pdep: the level op j's parent slot is free from (WAR/WAW); w1, w2: the
  // last writers of its children (-1: never written)
  std::vector<int> pdep, w1, w2;
  std::vector<int> &level;
  std::vector<char> &used;

  Planner(const plfx_trav_op *o, int n, const unsigned char *tip, TravPlan &p)
      : ops(o), nops(n), slot_is_tip(tip), plan(p), pdep(n, 0), w1(n, -1), w2(n, -1),
        level(p.level), used(p.fused) {}

  bool is_tip(int sl) const { return slot_is_tip && slot_is_tip[sl]; }
  int tip_children(int j) const { return (is_tip(ops[j].child1) ? 1 : 0) + (is_tip(ops[j].child2) ? 1 : 0); }

  void add(int lv, int kind, int tips, std::vector<int> members) {
    for (int j : members) used[j] = 1;
    plan.counts[kind]++;
    plan.groups.push_back(TravGroup{lv, kind, tips, std::move(members)});
  }

  // r roots a complete subtree of depth D over levels L..L+D-1, every op
  // unfused and its own slot free by L; its ops are appended to lv[0..D-1]
  // children left to right before parents
  bool complete(int r, int D, int L, std::vector<int> *lv) const {
    if (r < 0 || used[r] || level[r] != L + D - 1 || pdep[r] > L) return false;
    if (D > 1 && (w1[r] < 0 || w2[r] < 0 || w1[r] == w2[r] || !complete(w1[r], D - 1, L, lv) ||
                  !complete(w2[r], D - 1, L, lv)))
      return false;
    lv[D - 1].push_back(r);
    return true;
  }

  // p's writers x, y, both at level L and p one above, all three unfused
  bool fusible_pair(int p, int L, int &x, int &y) const {
    x = w1[p];
    y = w2[p];
    return x >= 0 && y >= 0 && x != y && !used[x] && !used[y] && !used[p] && level[x] == L &&
           level[y] == L && level[p] == L + 1;
  }

  // Fused deep subtrees (plf_dna.hpp DeepDesc): a complete binary subtree of
  // depth D (2^D - 1 ops on consecutive levels L..L+D-1), every op's own slot
  // free by L (pdep <= L), all leaves dense or all leaves tips.
  void deeps(int D) {
    for (int r = 0; r < nops; r++) {
      if (level[r] < D - 1 || used[r]) continue;
      std::vector<int> lv[6];
      if (!complete(r, D, level[r] - (D - 1), lv)) continue;
      // every leaf dense, or every leaf a tip (the coded-leaf pass's
      // tables); mixed leaves stay with the three-level passes
      bool dense = true, coded = true;
      for (int j : lv[0]) {
        const bool t1 = is_tip(ops[j].child1), t2 = is_tip(ops[j].child2);
        dense = dense && !t1 && !t2;
        coded = coded && t1 && t2;
      }
      // nor may a deep pass take the top of a subtree whose lower levels are
      // still unfused (over coded leaves: the septets below it would become
      // level pairs and move more bytes in all)
      for (int j : lv[0])
        for (int wr : {w1[j], w2[j]})
          if (wr >= 0 && !used[wr] && level[wr] == level[r] - D) dense = coded = false;
      if (!dense && !coded) continue;
      std::vector<int> members;
      for (int k = 0; k < D; k++) members.insert(members.end(), lv[k].begin(), lv[k].end());
      add(level[r] - (D - 1), 6 - D, coded ? 2 : 0, std::move(members));
    }
  }

  // Fused three-level subtrees (plf_dna.hpp SeptetDesc): root R two levels
  // above four ops A of one tip kind, through the two ops B that R's children
  // were last written by; R's and the B's slots free by level L.
  void septets() {
    for (int r = 0; r < nops; r++) {
      int a[4], b[2];
      const int L = level[r] - 2;
      if (L < 0 || used[r] || pdep[r] > L) continue;
      if (!fusible_pair(r, L + 1, b[0], b[1])) continue;
      if (pdep[b[0]] > L || pdep[b[1]] > L) continue;
      if (!fusible_pair(b[0], L, a[0], a[1]) || !fusible_pair(b[1], L, a[2], a[3])) continue;
      const int k = tip_children(a[0]);
      if (tip_children(a[1]) != k || tip_children(a[2]) != k || tip_children(a[3]) != k) continue;
      add(L, kTravSeptet, k, {a[0], a[1], a[2], a[3], b[0], b[1], r});
    }
  }

  // Fused level pairs (plf_dna.hpp TripleDesc): op P whose two children were
  // last written by ops A, B of the level just below it, with the same tip
  // kind, and whose own slot is free by then (pdep <= level of A).
  void triples() {
    for (int p = 0; p < nops; p++) {
      const int a = w1[p], b = w2[p];
      if (a < 0 || b < 0 || a == b || used[a] || used[b] || used[p]) continue;
      const int L = level[a];
      if (level[b] != L || level[p] != L + 1 || pdep[p] > L) continue;
      if (tip_children(a) != tip_children(b)) continue;
      add(L, kTravTriple, tip_children(a), {a, b, p});
    }
  }
};

int invalid(std::string *err, const char *fmt, int j) {
  char buf[128];
  snprintf(buf, sizeof buf, fmt, j);
  if (err) *err = buf;
  return PLFX_ERR_INVALID;
}

}  // namespace

int plan_traversal(const plfx_trav_op *ops, int nops, int nslots, int npmats,
                   const unsigned char *slot_is_tip, int states, int fuse, TravPlan *out,
                   std::string *err) {
  *out = TravPlan{};
  if (nops <= 0) return PLFX_OK;
  out->level.assign(nops, 0);
  out->fused.assign(nops, 0);
  Planner pl(ops, nops, slot_is_tip, *out);
  // dependency levels: RAW on children (cdep), WAR/WAW on the parent slot (pd)
  std::vector<int> slot_write(nslots > 0 ? nslots : 0, -1), slot_read(slot_write), last_writer(slot_write);
  for (int j = 0; j < nops; j++) {
    const plfx_trav_op &o = ops[j];
    if (o.parent < 0 || o.parent >= nslots || o.child1 < 0 || o.child1 >= nslots || o.child2 < 0 ||
        o.child2 >= nslots || o.pmat < 0 || o.pmat >= npmats)
      return invalid(err, "op %d: slot/pmat index out of range", j);
    if (o.parent == o.child1 || o.parent == o.child2)
      return invalid(err, "op %d: parent slot aliases a child", j);
    if (pl.is_tip(o.parent)) return invalid(err, "op %d: parent slot is a tip", j);
    int cdep = 0, pd = 0;
    for (int sl : {o.child1, o.child2})
      if (slot_write[sl] >= 0) cdep = std::max(cdep, slot_write[sl] + 1);
    if (slot_write[o.parent] >= 0) pd = std::max(pd, slot_write[o.parent] + 1);
    if (slot_read[o.parent] >= 0) pd = std::max(pd, slot_read[o.parent] + 1);
    const int lv = std::max(cdep, pd);
    out->level[j] = lv;
    pl.pdep[j] = pd;
    pl.w1[j] = last_writer[o.child1];
    pl.w2[j] = last_writer[o.child2];
    slot_write[o.parent] = lv;
    last_writer[o.parent] = j;
    for (int sl : {o.child1, o.child2}) slot_read[sl] = std::max(slot_read[sl], lv);
    out->nlev = std::max(out->nlev, lv + 1);
  }
  if (states == 4) {
    if (fuse >= 3)
      for (int D = 6; D >= 4; D--) pl.deeps(D);  // deepest first
    if (fuse >= 2) pl.septets();
    if (fuse >= 1) pl.triples();
  }
  for (int j = 0; j < nops; j++) out->counts[5] += out->fused[j] ? 0 : 1;
  return PLFX_OK;
}

}  // namespace plfx
