// psr_prot_edge_lower_main.cpp -- the lowering of a
// plfx_edge_sumtable_psr_batch_gen call (csrc/psr_edge_lower.cpp with a state
// count: a CLV and a table are n * states values) as a stand-alone program for
// tests/test_psr_prot_edge_lower.py (built with ASan + UBSan).  Every pointer
// is a made-up address that is never followed; with clv_bytes = n * states *
// element size:
//   dense CLVs of edge i  0x100000 + (3i, 3i+1, 3i+2) * clv_bytes: x1, x2, sumtab
//   tip codes of edge i   0x40000000 + i * 64 + 1 (odd: no alignment rule)
//   tipvec                0x80000000
//
// stdin, any number of cases:
//   case dtype states n nedges nover
//     nedges kinds (0 dense side 1, 1 coded side 1), then nover lines
//     "FIELD EDGE HEXADDR" replacing an address -- FIELD one of tip1 x1 x2
//     sumtab (edge's), tipvec edges (call's; edges: 0 = NULL)
// stdout per case:
//   item TIP COUNT     then COUNT lines "e x1 x2 sumtab" (hex)
//   end
// or, for a refusal: "error CODE items-left edges-left text", then "end".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../amd-versal-phylogenetic-likelihood-function_amd/csrc/psr_edge_lower.hpp"

namespace {

template <typename T>
T *at(unsigned long long a) {
  return reinterpret_cast<T *>(static_cast<uintptr_t>(a));
}

unsigned long long hex(const void *p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }

}  // namespace

int main() {
  char word[32];
  plfx::PsrEdgeLaunchList list;  // one list for every case, as a context keeps one
  while (scanf("%31s", word) == 1) {
    if (strcmp(word, "case")) return 2;
    int dtype, states, nedges, nover;
    long long n;
    if (scanf("%d %d %lld %d %d", &dtype, &states, &n, &nedges, &nover) != 5) return 2;
    const unsigned long long cb =
        (unsigned long long)(n > 0 ? n : 0) * (unsigned long long)(states > 0 ? states : 0) * (dtype == PLFX_F32 ? 4 : 8);
    std::vector<plfx_psr_edge> edges((size_t)(nedges > 0 ? nedges : 0));
    for (int i = 0; i < nedges; i++) {
      int kind;
      if (scanf("%d", &kind) != 1) return 2;
      plfx_psr_edge &d = edges[(size_t)i];
      d = plfx_psr_edge{};
      if (kind) d.tip1 = at<const uint8_t>(0x40000000ull + 64ull * i + 1);
      else d.x1 = at<const void>(0x100000ull + (3ull * i) * cb);
      d.x2 = at<const void>(0x100000ull + (3ull * i + 1) * cb);
      d.sumtab = at<void>(0x100000ull + (3ull * i + 2) * cb);
    }
    const void *tipvec = at<const void>(0x80000000ull);
    const plfx_psr_edge *ep = edges.data();
    for (int j = 0; j < nover; j++) {
      int i;
      unsigned long long a;
      if (scanf("%31s %d %llx", word, &i, &a) != 3) return 2;
      if (!strcmp(word, "tipvec")) tipvec = at<const void>(a);
      else if (!strcmp(word, "edges")) ep = a ? at<const plfx_psr_edge>(a) : nullptr;
      else {
        plfx_psr_edge &d = edges.at((size_t)i);
        if (!strcmp(word, "tip1")) d.tip1 = at<const uint8_t>(a);
        else if (!strcmp(word, "x1")) d.x1 = at<const void>(a);
        else if (!strcmp(word, "x2")) d.x2 = at<const void>(a);
        else if (!strcmp(word, "sumtab")) d.sumtab = at<void>(a);
        else return 2;
      }
    }
    std::string err;
    const int rc = plfx::lower_psr_edges(dtype, n, tipvec, ep, nedges, &list, &err, states);
    if (rc != PLFX_OK) {
      printf("error %d %zu %zu %s\n", rc, list.items.size(), list.edges.size(), err.c_str());
    } else {
      for (const plfx::PsrEdgeLaunch &it : list.items) {
        printf("item %d %d\n", it.tip, it.count);
        for (int i = it.first; i < it.first + it.count; i++) {
          const plfx::PsrEdgeDescH &d = list.edges.at((size_t)i);
          printf("e %llx %llx %llx\n", hex(d.x1), hex(d.x2), hex(d.out));
        }
      }
    }
    printf("end\n");
  }
  return 0;
}
