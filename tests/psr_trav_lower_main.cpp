// psr_trav_lower_main.cpp -- the planning and lowering of a plfx_traverse_psr
// call (csrc/trav_plan.cpp with states 4 and fuse <= 1, then
// csrc/psr_lower.cpp: checks, descriptors, per level the fused level
// pairs and the unfused ops) as a stand-alone program for
// tests/test_psr_trav_lower.py (built with ASan + UBSan).  Every pointer is a
// made-up address that is never followed:
//   CLV of slot s        0x100000 + s * clv_bytes
//   tip codes of slot s  0x40000000 + s * 64 + 1 (odd: no alignment rule)
//   pmats                0x50000000
//   scaler bytes of op j 0x60000000 + j * 64,  scaler_sums 0x70000000
//   EV 0x80000000, rate_cat 0x90000001
//
// stdin, any number of cases:
//   case dtype n ncat fuse nslots npmats nops nover
//     nslots flags (1: the slot is a coded tip), nops lines "parent child1
//     child2 pmat", then nover lines "FIELD INDEX HEXADDR" replacing an
//     address -- FIELD one of clv tip (slot's), sc (op's), EV cat pmats sums
//     clvs scs (call's; clvs / scs 0: the array itself is NULL)
// stdout per case:
//   plan TRIPLES UNFUSED LEVELS
//   item t LEVEL TIPS COUNT  then COUNT lines "t" + the 19 TripleDescH fields (hex)
//   item n LEVEL TIPS COUNT  then COUNT lines "n x1 x2 x3 left right scaler sum"
//   end
// or, for a refusal: "error CODE items-left triples-left nodes-left text", then "end".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../amd-versal-phylogenetic-likelihood-function_amd/csrc/psr_lower.hpp"

namespace {

template <typename T>
T *at(unsigned long long a) {
  return reinterpret_cast<T *>(static_cast<uintptr_t>(a));
}

unsigned long long hex(const void *p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }

}  // namespace

int main() {
  char word[32];
  plfx::PsrLaunchList list;  // one list for every case, as a context keeps one
  while (scanf("%31s", word) == 1) {
    if (strcmp(word, "case")) return 2;
    int dtype, ncat, fuse, nslots, npmats, nops, nover;
    long long n;
    if (scanf("%d %lld %d %d %d %d %d %d", &dtype, &n, &ncat, &fuse, &nslots, &npmats, &nops, &nover) != 8) return 2;
    const unsigned long long cb = (unsigned long long)(n > 0 ? n : 0) * 4 * (dtype == PLFX_F32 ? 4 : 8);
    std::vector<unsigned char> is_tip((size_t)nslots);
    std::vector<void *> clv((size_t)nslots);
    std::vector<const uint8_t *> tips((size_t)nslots);
    bool any_tip = false;
    for (int s = 0; s < nslots; s++) {
      int f;
      if (scanf("%d", &f) != 1) return 2;
      is_tip[(size_t)s] = f != 0;
      any_tip |= f != 0;
      clv[(size_t)s] = f ? nullptr : at<void>(0x100000ull + (unsigned long long)s * cb);
      tips[(size_t)s] = f ? at<const uint8_t>(0x40000000ull + 64ull * s + 1) : nullptr;
    }
    std::vector<plfx_trav_op> ops((size_t)nops);
    std::vector<uint8_t *> scalers((size_t)nops);
    for (int j = 0; j < nops; j++) {
      plfx_trav_op &o = ops[(size_t)j];
      if (scanf("%d %d %d %d", &o.parent, &o.child1, &o.child2, &o.pmat) != 4) return 2;
      scalers[(size_t)j] = at<uint8_t>(0x60000000ull + 64ull * j);
    }
    plfx::PsrCall call{dtype, n, ncat, at<const void>(0x80000000ull), at<const uint8_t>(0x90000001ull)};
    plfx::TravArrays arr{ops.data(), nops, clv.data(), any_tip ? tips.data() : nullptr, at<const void>(0x50000000ull),
                         scalers.data(), at<int64_t>(0x70000000ull)};
    for (int j = 0; j < nover; j++) {
      int i;
      unsigned long long a;
      if (scanf("%31s %d %llx", word, &i, &a) != 3) return 2;
      if (!strcmp(word, "EV")) call.EV = at<const void>(a);
      else if (!strcmp(word, "cat")) call.rate_cat = at<const uint8_t>(a);
      else if (!strcmp(word, "pmats")) arr.pmats = at<const void>(a);
      else if (!strcmp(word, "sums")) arr.scaler_sums = at<int64_t>(a);
      else if (!strcmp(word, "clvs")) arr.clv = a ? at<void *const>(a) : nullptr;
      else if (!strcmp(word, "scs")) arr.scalers = a ? at<uint8_t *const>(a) : nullptr;
      else if (!strcmp(word, "clv")) clv.at((size_t)i) = at<void>(a);
      else if (!strcmp(word, "tip")) tips.at((size_t)i) = at<const uint8_t>(a);
      else if (!strcmp(word, "sc")) scalers.at((size_t)i) = at<uint8_t>(a);
      else return 2;
    }
    plfx::TravPlan plan;
    std::string err;
    // the planner sees the slots' tip flags as the C ABI forms them: tips[s] != NULL
    std::vector<unsigned char> mask;
    if (arr.tips)
      for (int s = 0; s < nslots; s++) mask.push_back(tips[(size_t)s] != nullptr);
    int rc = plfx::plan_traversal(ops.data(), nops, nslots, npmats, mask.empty() ? nullptr : mask.data(), 4,
                                  fuse < 1 ? fuse : 1, &plan, &err);
    if (rc == PLFX_OK) rc = plfx::lower_psr_traversal(plan, arr, call, &list, &err);
    else list.clear();
    if (rc != PLFX_OK) {
      printf("error %d %zu %zu %zu %s\n", rc, list.items.size(), list.triples.size(), list.nodes.size(), err.c_str());
    } else {
      printf("plan %d %d %d\n", plan.counts[plfx::kTravTriple], plan.counts[5], plan.nlev);
      for (const plfx::PsrLaunch &it : list.items) {
        const bool tr = it.kind == plfx::kPsrTriples;
        printf("item %c %d %d %d\n", tr ? 't' : 'n', it.level, it.tips, it.count);
        for (int i = it.first; i < it.first + it.count; i++) {
          if (tr) {
            const plfx::TripleDescH &d = list.triples.at((size_t)i);
            printf("t %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx\n",
                   hex(d.a1), hex(d.a2), hex(d.b1), hex(d.b2), hex(d.xa), hex(d.xb), hex(d.xp), hex(d.la), hex(d.ra),
                   hex(d.lb), hex(d.rb), hex(d.lp), hex(d.rp), hex(d.sa), hex(d.sb), hex(d.sp), hex(d.ssa), hex(d.ssb),
                   hex(d.ssp));
          } else {
            const plfx::NodeDescH &d = list.nodes.at((size_t)i);
            printf("n %llx %llx %llx %llx %llx %llx %llx\n", hex(d.x1), hex(d.x2), hex(d.x3), hex(d.left),
                   hex(d.right), hex(d.scaler), hex(d.scaler_sum));
          }
        }
      }
    }
    printf("end\n");
  }
  return 0;
}
