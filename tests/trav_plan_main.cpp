// trav_plan_main.cpp -- the traversal planner (csrc/trav_plan.cpp) as a
// stand-alone program for tests/test_trav_plan.py (built with ASan + UBSan).
//
// stdin, any number of cases:
//   nops nslots npmats states fuse
//   nslots tip flags (0/1)
//   nops lines "parent child1 child2 pmat"
// stdout per case:
//   counts deep6 deep5 deep4 septets triples unfused
//   levels NLEV l l ...               (the level of every op)
//   group KIND TIPS LEVEL op op ...   (KIND deep6|deep5|deep4|septet|triple)
//   end
// or, for a refused op list: "error CODE text", then "end".
// The order the launches are issued in is csrc/trav_lower.cpp's
// (tests/trav_lower_main.cpp).
#include <cstdio>
#include <string>
#include <vector>

#include "../amd-versal-phylogenetic-likelihood-function_amd/csrc/trav_plan.hpp"

int main() {
  static const char *const kKind[] = {"deep6", "deep5", "deep4", "septet", "triple"};
  int nops, nslots, npmats, states, fuse;
  while (scanf("%d %d %d %d %d", &nops, &nslots, &npmats, &states, &fuse) == 5) {
    if (nops < 0 || nslots < 0) return 2;
    std::vector<unsigned char> tip(nslots);
    for (int i = 0; i < nslots; i++) {
      int t;
      if (scanf("%d", &t) != 1) return 2;
      tip[i] = t != 0;
    }
    std::vector<plfx_trav_op> ops(nops);
    for (plfx_trav_op &o : ops)
      if (scanf("%d %d %d %d", &o.parent, &o.child1, &o.child2, &o.pmat) != 4) return 2;
    plfx::TravPlan plan;
    std::string err;
    const int rc = plfx::plan_traversal(ops.data(), nops, nslots, npmats, tip.data(), states, fuse,
                                        &plan, &err);
    if (rc != PLFX_OK) {
      printf("error %d %s\nend\n", rc, err.c_str());
      continue;
    }
    printf("counts");
    for (int c : plan.counts) printf(" %d", c);
    printf("\n");
    printf("levels %d", plan.nlev);
    for (int lv : plan.level) printf(" %d", lv);
    printf("\n");
    for (const plfx::TravGroup &g : plan.groups) {
      printf("group %s %d %d", kKind[g.kind], g.tips, g.level);
      for (int j : g.ops) printf(" %d", j);
      printf("\n");
    }
    printf("end\n");
  }
  return 0;
}
