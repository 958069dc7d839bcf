// psr_prot_scan_lower_main.cpp -- the lowering of a plfx_psr_rate_scan_gen call
// (csrc/psr_scan_lower.cpp with a state count: plfx.h section 12b) as a
// stand-alone program for tests/test_psr_prot_scan_lower.py (built with ASan +
// UBSan).  psr_scan_lower_main.cpp with one more number per case; every
// pointer is a made-up address that is never followed:
//   tip codes of slot s  0x40000000 + s * 64 + 1
//   blen 0x50000000, eigen 0x51000000, EV 0x52000000, tipvec 0x53000000,
//   cand_rates 0x54000000, best_idx 0x55000000, best_lnl 0x56000000,
//   all_lnl 0x57000000, out_lnl 0x58000000
//
// stdin, any number of cases:
//   case states dtype n ncand group fuse nslots npmats nops WSADDR(hex) WSBYTES nover
//     states 0: the trailing `states` of psr_scan_layout and PsrScanCall is
//     left out (what section 12's entry points pass), else it is given;
//     WSBYTES -1: exactly what the size query reports for `states`, -2: one
//     byte less, -4: what the query reports for 4 states;
//     nslots flags (1: the slot is a coded tip), nops lines "parent child1
//     child2 pmat", then nover lines "FIELD HEXADDR" replacing an address --
//     FIELD one of blen eigen EV tipvec cand best_idx best_lnl tips ops
// stdout per case:
//   layout clv0 clv_stride tip0 row sc0 cat0 pm0 end QUERY
//   misc cat pmats root scalers sc_stride            (hex addresses, stride decimal)
//   tile src dst                                     per tiled tip
//   pass k0 gc tail                                  per pass
//   list full|tail, then per launch "item n|t LEVEL TIPS COUNT" and COUNT lines
//     "n x1 x2 x3 left right scaler sum" or "t" + the 19 TripleDescH fields
//   end
// or, for a refusal: "error CODE passes tiles full-items tail-items text", then "end".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../amd-versal-phylogenetic-likelihood-function_amd/csrc/psr_scan_lower.hpp"

namespace {

template <typename T>
T *at(unsigned long long a) {
  return reinterpret_cast<T *>(static_cast<uintptr_t>(a));
}

unsigned long long hex(const void *p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }

void print_list(const char *name, const plfx::PsrLaunchList &l) {
  printf("list %s\n", name);
  for (const plfx::PsrLaunch &it : l.items) {
    const bool tr = it.kind == plfx::kPsrTriples;
    printf("item %c %d %d %d\n", tr ? 't' : 'n', it.level, it.tips, it.count);
    for (int i = it.first; i < it.first + it.count; i++) {
      if (tr) {
        const plfx::TripleDescH &d = l.triples.at((size_t)i);
        const void *f[19] = {d.a1, d.a2, d.b1, d.b2, d.xa, d.xb, d.xp, d.la,  d.ra, d.lb,
                             d.rb, d.lp, d.rp, d.sa, d.sb, d.sp, d.ssa, d.ssb, d.ssp};
        printf("t");
        for (const void *p : f) printf(" %llx", hex(p));
        printf("\n");
      } else {
        const plfx::NodeDescH &d = l.nodes.at((size_t)i);
        printf("n %llx %llx %llx %llx %llx %llx %llx\n", hex(d.x1), hex(d.x2), hex(d.x3), hex(d.left), hex(d.right),
               hex(d.scaler), hex(d.scaler_sum));
      }
    }
  }
}

}  // namespace

int main() {
  char word[32];
  plfx::PsrScanPlan plan;  // one plan for every case, as a context keeps one
  while (scanf("%31s", word) == 1) {
    if (strcmp(word, "case")) return 2;
    int states, dtype, ncand, group, fuse, nslots, npmats, nops, nover;
    long long n, wsbytes;
    unsigned long long wsaddr;
    if (scanf("%d %d %lld %d %d %d %d %d %d %llx %lld %d", &states, &dtype, &n, &ncand, &group, &fuse, &nslots, &npmats,
              &nops, &wsaddr, &wsbytes, &nover) != 12)
      return 2;
    std::vector<const uint8_t *> tips((size_t)(nslots > 0 ? nslots : 0));
    int ntips = 0;
    for (int s = 0; s < nslots; s++) {
      int f;
      if (scanf("%d", &f) != 1) return 2;
      ntips += f != 0;
      tips[(size_t)s] = f ? at<const uint8_t>(0x40000000ull + 64ull * s + 1) : nullptr;
    }
    std::vector<plfx_trav_op> ops((size_t)(nops > 0 ? nops : 0));
    for (int j = 0; j < nops; j++) {
      plfx_trav_op &o = ops[(size_t)j];
      if (scanf("%d %d %d %d", &o.parent, &o.child1, &o.child2, &o.pmat) != 4) return 2;
    }
    size_t query = 0, query4 = 0;
    plfx::PsrScanLayout ql{};
    const int qrc = states ? plfx::psr_scan_layout(dtype, nops, ntips, npmats, n, group, &ql, states)
                           : plfx::psr_scan_layout(dtype, nops, ntips, npmats, n, group, &ql);
    if (qrc == PLFX_OK) query = ql.end;
    if (plfx::psr_scan_layout(dtype, nops, ntips, npmats, n, group, &ql, 4) == PLFX_OK) query4 = ql.end;
    plfx::PsrScanCall c{dtype,
                        ops.data(),
                        nops,
                        tips.data(),
                        nslots,
                        at<const double>(0x50000000ull),
                        npmats,
                        at<const double>(0x51000000ull),
                        at<const void>(0x52000000ull),
                        at<const void>(0x53000000ull),
                        at<const double>(0x54000000ull),
                        ncand,
                        group,
                        n,
                        at<void>(wsaddr),
                        wsbytes == -1   ? query
                        : wsbytes == -2 ? query - 1
                        : wsbytes == -4 ? query4
                                        : (size_t)wsbytes,
                        at<int32_t>(0x55000000ull),
                        at<double>(0x56000000ull),
                        at<double>(0x57000000ull),
                        at<double>(0x58000000ull),
                        fuse};
    if (states) c.states = states;
    for (int j = 0; j < nover; j++) {
      unsigned long long a;
      if (scanf("%31s %llx", word, &a) != 2) return 2;
      if (!strcmp(word, "blen")) c.blen = at<const double>(a);
      else if (!strcmp(word, "eigen")) c.eigen = at<const double>(a);
      else if (!strcmp(word, "EV")) c.EV = at<const void>(a);
      else if (!strcmp(word, "tipvec")) c.tipvec = at<const void>(a);
      else if (!strcmp(word, "cand")) c.cand_rates = at<const double>(a);
      else if (!strcmp(word, "best_idx")) c.best_idx = at<int32_t>(a);
      else if (!strcmp(word, "best_lnl")) c.best_lnl = at<double>(a);
      else if (!strcmp(word, "tips")) c.tips = a ? at<const uint8_t *const>(a) : nullptr;
      else if (!strcmp(word, "ops")) c.ops = a ? at<const plfx_trav_op>(a) : nullptr;
      else return 2;
    }
    std::string err;
    const int rc = plfx::lower_psr_scan(c, &plan, &err);
    if (rc != PLFX_OK) {
      printf("error %d %zu %zu %zu %zu %s\n", rc, plan.passes.size(), plan.tiles.size(), plan.full.items.size(),
             plan.tail.items.size(), err.c_str());
    } else {
      const plfx::PsrScanLayout &l = plan.lay;
      printf("layout %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", l.clv0, l.clv_stride, l.tip0, l.row, l.sc0, l.cat0, l.pm0,
             l.end, query);
      printf("misc %llx %llx %llx %llx %lld\n", hex(plan.cat), hex(plan.pmats), hex(plan.root), hex(plan.scalers),
             (long long)plan.sc_stride);
      for (const plfx::PsrTileDescH &t : plan.tiles) printf("tile %llx %llx\n", hex(t.src), hex(t.dst));
      for (const plfx::PsrScanPass &p : plan.passes) printf("pass %d %d %d\n", p.k0, p.gc, (int)p.tail);
      print_list("full", plan.full);
      print_list("tail", plan.tail);
    }
    printf("end\n");
  }
  return 0;
}
