// psr_edge_lower.cpp -- see psr_edge_lower.hpp.
#include "psr_edge_lower.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "psr_lower.hpp"  // psr_clv_bytes; aligned16, overlap (trav_lower.hpp)

namespace plfx {
namespace {

int refuse(PsrEdgeLaunchList *out, std::string *err, const char *what, int i = -1) {
  out->clear();
  if (err) {
    char buf[160];
    if (i >= 0) std::snprintf(buf, sizeof buf, "psr sumtable edge %d: %s", i, what);
    else std::snprintf(buf, sizeof buf, "psr sumtable batch: %s", what);
    *err = buf;
  }
  return PLFX_ERR_INVALID;
}

// the bytes [lo, hi) edge `edge` writes (table) or reads
struct Span {
  uintptr_t lo, hi;
  int edge;
  bool table;
};

}  // namespace

int lower_psr_edges(int dtype, int64_t n, const void *tipvec, const plfx_psr_edge *edges, int nedges,
                    PsrEdgeLaunchList *out, std::string *err, int states) {
  out->clear();
  if (dtype != PLFX_F32 && dtype != PLFX_F64) return refuse(out, err, "bad dtype");
  if (states != 4 && states != 20) return refuse(out, err, "states not built (4, 20)");
  if (n < 0) return refuse(out, err, "n < 0");
  if (nedges < 1 || !edges) return refuse(out, err, "needs nedges >= 1 edges");
  if (n == 0) return PLFX_OK;

  const size_t cb = psr_clv_bytes(dtype, n, states), tb = (size_t)n;
  for (int i = 0; i < nedges; i++) {
    const plfx_psr_edge &d = edges[i];
    if ((d.tip1 != nullptr) == (d.x1 != nullptr)) return refuse(out, err, "side 1 needs exactly one of tip / CLV", i);
    if (!d.x2 || !d.sumtab) return refuse(out, err, "null CLV / sum table pointer", i);
    if ((d.x1 && !aligned16(d.x1)) || !aligned16(d.x2) || !aligned16(d.sumtab))
      return refuse(out, err, "CLV pointers must be 16-byte aligned", i);
    if (d.tip1 && !tipvec)
      return refuse(out, err, "a coded side needs tipvec (the default 0/1 table is not in eigen coordinates)", i);
    if (overlap(d.sumtab, cb, d.tip1 ? (const void *)d.tip1 : d.x1, d.tip1 ? tb : cb) ||
        overlap(d.sumtab, cb, d.x2, cb))
      return refuse(out, err, "sumtab may not overlap x1/x2", i);
  }

  // Across the call: sorted by their first byte, a span overlaps an earlier
  // one exactly if it begins before the furthest end seen so far.  Tables are
  // held against tables and inputs, inputs against tables only.
  std::vector<Span> spans;
  spans.reserve(3 * (size_t)nedges);
  auto add = [&](const void *p, size_t bytes, int edge, bool table) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    spans.push_back(Span{lo, lo + bytes, edge, table});
  };
  for (int i = 0; i < nedges; i++) {
    const plfx_psr_edge &d = edges[i];
    add(d.sumtab, cb, i, true);
    if (d.tip1) add(d.tip1, tb, i, false);
    else add(d.x1, cb, i, false);
    add(d.x2, cb, i, false);
  }
  std::sort(spans.begin(), spans.end(), [](const Span &a, const Span &b) {
    return a.lo != b.lo ? a.lo < b.lo : (a.edge != b.edge ? a.edge < b.edge : a.table && !b.table);
  });
  uintptr_t table_end = 0, input_end = 0;  // the furthest ends so far; no span begins at address 0
  for (const Span &sp : spans) {
    if (sp.lo < table_end)
      return refuse(out, err, sp.table ? "the table shares a byte with another table of the call"
                                       : "an input shares a byte with a table of the call", sp.edge);
    if (sp.table && sp.lo < input_end)
      return refuse(out, err, "the table shares a byte with an input of the call", sp.edge);
    if (sp.table) table_end = std::max(table_end, sp.hi);
    else input_end = std::max(input_end, sp.hi);
  }

  for (int tip = 0; tip < 2; tip++) {
    const int first = (int)out->edges.size();
    for (int i = 0; i < nedges; i++) {
      const plfx_psr_edge &d = edges[i];
      if ((d.tip1 != nullptr) == (tip != 0))
        out->edges.push_back(PsrEdgeDescH{tip ? (const void *)d.tip1 : d.x1, d.x2, d.sumtab});
    }
    const int count = (int)out->edges.size() - first;
    for (int i = 0; i < count; i += kMaxBatch)
      out->items.push_back(PsrEdgeLaunch{tip, first + i, std::min(kMaxBatch, count - i)});
  }
  return PLFX_OK;
}

}  // namespace plfx
