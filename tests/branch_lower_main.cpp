// branch_lower_main.cpp -- the planner and lowering of a
// plfx_branch_sumtables_psr call (csrc/branch_plan.cpp: the tree rules, the
// pre-order levels, each op's Pup and W(v), the slab of every W and table and
// the launch list) as a stand-alone program for tests/test_branch_lower.py
// (built with ASan + UBSan).  Every pointer is a made-up address that is never
// followed:
//   dense CLV of slot i   0x100000 + i * 0x10000
//   tip codes of slot i   0x40000000 + i * 64 + 1 (odd: no alignment rule)
//   tipvec 0x80000000, pmats 0x90000000, root_pmat 0xA0000000, EV 0xB0000000,
//   rate_cat 0xC0000000, scaler_sums 0xD0000000, edge_scale 0xD8000000,
//   workspace 0x10000000 of exactly the layout's bytes
//
// stdin, any number of cases:
//   case dtype states flags n ncat nops nslots npmats nover
//     nops lines "parent child1 child2 pmat", nslots kinds (0 nothing, 1 dense
//     CLV, 2 coded tip), then nover lines "FIELD INDEX HEX" replacing a value:
//     clv / tip (slot INDEX), ws wsbytes tipvec root_pmat edge_scale
//     scaler_sums ops (the call's; ops: 0 = NULL)
// stdout per case:
//   layout SLAB W_OFF TAB_OFF CNT_OFF BYTES NLEV
//   op J LEVEL UP_EDGE PUP WV WV_CODED FUSED          per op
//   edge E W TAB WSUM                                  per edge
//   item KIND LEVEL TIPS COUNT, then COUNT lines
//     p wv c1 c2 pup p1 p2 w1 w2 t1 t2 ss1 ss2 | n x1 x2 x3 left right sum | e x1 x2 out | s w1 w2 up
//   end
// or, for a refusal: "error CODE items pairs nodes edges scale text", then "end".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../amd-versal-phylogenetic-likelihood-function_amd/csrc/branch_plan.hpp"

namespace {

template <typename T>
T *at(unsigned long long a) {
  return reinterpret_cast<T *>(static_cast<uintptr_t>(a));
}

unsigned long long hex(const void *p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }

}  // namespace

int main() {
  char word[32];
  plfx::BranchPlan plan;  // one plan for every case, as a context keeps one
  while (scanf("%31s", word) == 1) {
    if (strcmp(word, "case")) return 2;
    int dtype, states, flags, ncat, nops, nslots, npmats, nover;
    long long n;
    if (scanf("%d %d %d %lld %d %d %d %d %d", &dtype, &states, &flags, &n, &ncat, &nops, &nslots, &npmats, &nover) != 9)
      return 2;
    std::vector<plfx_trav_op> ops((size_t)(nops > 0 ? nops : 0));
    for (auto &o : ops)
      if (scanf("%d %d %d %d", &o.parent, &o.child1, &o.child2, &o.pmat) != 4) return 2;
    std::vector<void *> clv((size_t)(nslots > 0 ? nslots : 0), nullptr);
    std::vector<const uint8_t *> tips((size_t)(nslots > 0 ? nslots : 0), nullptr);
    for (int i = 0; i < nslots; i++) {
      int kind;
      if (scanf("%d", &kind) != 1) return 2;
      if (kind == 1) clv[(size_t)i] = at<void>(0x100000ull + 0x10000ull * i);
      if (kind == 2) tips[(size_t)i] = at<const uint8_t>(0x40000000ull + 64ull * i + 1);
    }
    plfx::BranchLayout lay{};
    (void)plfx::branch_layout(dtype, states, nops, n, &lay);
    plfx::BranchCall call{dtype, states, flags, ops.data(), nops, clv.data(), tips.data(), nslots,
                          at<const void>(0x90000000ull), npmats, at<const void>(0xA0000000ull),
                          at<const void>(0xB0000000ull), n, at<const uint8_t>(0xC0000000ull), ncat,
                          at<const int64_t>(0xD0000000ull), at<const void>(0x80000000ull), at<void>(0x10000000ull),
                          lay.bytes, at<const int64_t>(0xD8000000ull)};
    for (int k = 0; k < nover; k++) {
      int i;
      unsigned long long a;
      if (scanf("%31s %d %llx", word, &i, &a) != 3) return 2;
      if (!strcmp(word, "clv")) clv.at((size_t)i) = at<void>(a);
      else if (!strcmp(word, "tip")) tips.at((size_t)i) = at<const uint8_t>(a);
      else if (!strcmp(word, "ws")) call.workspace = at<void>(a);
      else if (!strcmp(word, "wsbytes")) call.workspace_bytes = (size_t)a;
      else if (!strcmp(word, "tipvec")) call.tipvec = at<const void>(a);
      else if (!strcmp(word, "root_pmat")) call.root_pmat = at<const void>(a);
      else if (!strcmp(word, "edge_scale")) call.edge_scale = at<const int64_t>(a);
      else if (!strcmp(word, "scaler_sums")) call.scaler_sums = at<const int64_t>(a);
      else if (!strcmp(word, "ops")) call.ops = a ? at<const plfx_trav_op>(a) : nullptr;
      else return 2;
    }
    std::string err;
    const int rc = plfx::plan_branches(call, &plan, &err);
    if (rc != PLFX_OK) {
      printf("error %d %zu %zu %zu %zu %zu %s\n", rc, plan.items.size(), plan.pairs.size(), plan.nodes.size(),
             plan.edges.size(), plan.scale.size(), err.c_str());
      printf("end\n");
      continue;
    }
    printf("layout %zu %zu %zu %zu %zu %d\n", plan.lay.slab, plan.lay.w_off, plan.lay.tab_off, plan.lay.cnt_off,
           plan.lay.bytes, plan.nlev);
    for (int j = 0; j < nops; j++)
      printf("op %d %d %d %llx %llx %d %d\n", j, plan.level.at((size_t)j), plan.up_edge.at((size_t)j),
             hex(plan.pup.at((size_t)j)), hex(plan.wv.at((size_t)j)), (int)plan.wv_coded.at((size_t)j),
             (int)plan.fused.at((size_t)j));
    for (int e = 0; e < 2 * nops; e++)
      printf("edge %d %llx %llx %llx\n", e, hex(plan.w.at((size_t)e)), hex(plan.tab.at((size_t)e)),
             hex(plan.wsum.at((size_t)e)));
    for (const plfx::BranchLaunch &it : plan.items) {
      printf("item %d %d %d %d\n", it.kind, it.level, it.tips, it.count);
      for (int i = it.first; i < it.first + it.count; i++) {
        if (it.kind == plfx::kBranchPairs) {
          const plfx::BranchPairDescH &d = plan.pairs.at((size_t)i);
          printf("p %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx\n", hex(d.wv), hex(d.c1), hex(d.c2),
                 hex(d.pup), hex(d.p1), hex(d.p2), hex(d.w1), hex(d.w2), hex(d.t1), hex(d.t2), hex(d.ss1), hex(d.ss2));
        } else if (it.kind == plfx::kBranchNodes) {
          const plfx::NodeDescH &d = plan.nodes.at((size_t)i);
          printf("n %llx %llx %llx %llx %llx %llx\n", hex(d.x1), hex(d.x2), hex(d.x3), hex(d.left), hex(d.right),
                 hex(d.scaler_sum));
        } else if (it.kind == plfx::kBranchTables) {
          const plfx::PsrEdgeDescH &d = plan.edges.at((size_t)i);
          printf("e %llx %llx %llx\n", hex(d.x1), hex(d.x2), hex(d.out));
        } else {
          const plfx::BranchScaleDescH &d = plan.scale.at((size_t)i);
          printf("s %d %d %d\n", d.w1, d.w2, d.up);
        }
      }
    }
    printf("end\n");
  }
  return 0;
}
