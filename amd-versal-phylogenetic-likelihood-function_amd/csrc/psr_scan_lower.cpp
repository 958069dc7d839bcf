// psr_scan_lower.cpp -- see psr_scan_lower.hpp.
#include "psr_scan_lower.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>

namespace plfx {
namespace {

size_t up(size_t v) { return (v + kPsrScanAlign - 1) / kPsrScanAlign * kPsrScanAlign; }

int refuse(PsrScanPlan *out, std::string *err, int code, const char *what, int i = -1) {
  out->clear();
  if (err) {
    char buf[200];
    if (i >= 0) std::snprintf(buf, sizeof buf, "psr rate scan op %d: %s", i, what);
    else std::snprintf(buf, sizeof buf, "psr rate scan: %s", what);
    *err = buf;
  }
  return code;
}

}  // namespace

void PsrScanPlan::clear() {
  lay = PsrScanLayout{};
  tiles.clear();
  passes.clear();
  full.clear();
  tail.clear();
  trav = TravPlan{};
  cat = nullptr;
  pmats = nullptr;
  root = nullptr;
  scalers = nullptr;
  sc_stride = 0;
  clv.clear();
  wtips.clear();
  sc_rows.clear();
}

int psr_scan_layout(int dtype, int nops, int ntips, int npmats, int64_t n, int group, PsrScanLayout *out,
                    int states) {
  if ((dtype != PLFX_F32 && dtype != PLFX_F64) || nops < 0 || ntips < 0 || npmats < 0 || n < 0 || group < 1 ||
      group > PLFX_PSR_MAX_CATS || !out || (states != 4 && states != 20))
    return PLFX_ERR_INVALID;
  const size_t es = dtype == PLFX_F32 ? 4 : 8, vn = (size_t)group * (size_t)n, S = (size_t)states;
  PsrScanLayout l{};
  l.clv_stride = up(vn * S * es);
  l.row = up(vn);
  l.clv0 = 0;
  l.tip0 = l.clv0 + (size_t)nops * l.clv_stride;
  l.sc0 = l.tip0 + (size_t)ntips * l.row;
  l.cat0 = l.sc0 + (size_t)nops * l.row;
  l.pm0 = l.cat0 + l.row;
  l.end = l.pm0 + up((size_t)2 * (size_t)npmats * (size_t)group * S * S * es);
  *out = l;
  return PLFX_OK;
}

int lower_psr_scan(const PsrScanCall &c, PsrScanPlan *out, std::string *err) {
  out->clear();
  const int inv = PLFX_ERR_INVALID;
  if (c.dtype != PLFX_F32 && c.dtype != PLFX_F64) return refuse(out, err, inv, "bad dtype");
  if (c.states != 4 && c.states != 20) return refuse(out, err, inv, "states must be 4 or 20");
  if (c.n < 0) return refuse(out, err, inv, "n < 0");
  if (c.nops < 1 || !c.ops) return refuse(out, err, inv, "needs nops >= 1 ops");
  if (c.ncand < 1 || c.ncand > PLFX_PSR_SCAN_MAX_RATES)
    return refuse(out, err, inv, "ncand outside 1..PLFX_PSR_SCAN_MAX_RATES");
  if (c.group < 1 || c.group > PLFX_PSR_MAX_CATS) return refuse(out, err, inv, "group outside 1..PLFX_PSR_MAX_CATS");
  if (c.nslots < 1 || c.npmats < 1) return refuse(out, err, inv, "needs nslots >= 1 and npmats >= 1");
  if (!c.blen || !c.eigen || !c.EV || !c.cand_rates) return refuse(out, err, inv, "null blen / eigen / EV / cand_rates");
  if (!c.tipvec) return refuse(out, err, inv, "tipvec is required (the default 0/1 table is not in eigen coordinates)");
  if (!c.best_idx || !c.best_lnl) return refuse(out, err, inv, "null best_idx / best_lnl");

  // the op list's own checks and its levels / level pairs
  std::vector<unsigned char> mask;
  if (c.tips)
    for (int s = 0; s < c.nslots; s++) mask.push_back(c.tips[s] != nullptr);
  std::string perr;
  // 20 states: no level pair is built, whatever the context's switch says
  const int fuse = c.states == 4 ? std::min(std::max(c.fuse, 0), 1) : 0;
  if (plan_traversal(c.ops, c.nops, c.nslots, c.npmats, mask.empty() ? nullptr : mask.data(), c.states, fuse,
                     &out->trav, &perr) != PLFX_OK)
    return refuse(out, err, inv, perr.c_str());
  // every slot that is read holds a coded tip or what an earlier op wrote
  std::vector<int> first_write((size_t)c.nslots, -1);
  for (int j = c.nops - 1; j >= 0; j--) first_write[(size_t)c.ops[j].parent] = j;
  for (int j = 0; j < c.nops; j++)
    for (const int s : {c.ops[j].child1, c.ops[j].child2}) {
      if (!mask.empty() && mask[(size_t)s]) continue;
      if (first_write[(size_t)s] < 0)
        return refuse(out, err, PLFX_ERR_UNSUPPORTED, "a leaf that is not a coded tip (dense leaves are not built)", j);
      if (first_write[(size_t)s] >= j) return refuse(out, err, inv, "reads a slot no earlier op wrote", j);
    }
  if (c.n == 0) return PLFX_OK;

  int ntips = 0;
  for (const unsigned char m : mask) ntips += m;
  PsrScanLayout lay{};
  if (psr_scan_layout(c.dtype, c.nops, ntips, c.npmats, c.n, c.group, &lay, c.states) != PLFX_OK)
    return refuse(out, err, inv, "bad sizes");
  if (!c.workspace || (reinterpret_cast<uintptr_t>(c.workspace) % kPsrScanAlign) != 0)
    return refuse(out, err, inv, "the workspace must be non-NULL and 256-byte aligned");
  if (c.workspace_bytes < lay.end)
    return refuse(out, err, inv, "the workspace is smaller than plfx_psr_rate_scan_workspace reports");

  char *const ws = static_cast<char *>(c.workspace);
  out->lay = lay;
  out->cat = reinterpret_cast<uint8_t *>(ws + lay.cat0);
  out->pmats = ws + lay.pm0;
  out->scalers = reinterpret_cast<const uint8_t *>(ws + lay.sc0);
  out->sc_stride = (int64_t)lay.row;
  out->clv.assign((size_t)c.nslots, nullptr);
  out->wtips.assign((size_t)c.nslots, nullptr);
  out->sc_rows.assign((size_t)c.nops, nullptr);
  int nclv = 0, ntile = 0;
  for (int j = 0; j < c.nops; j++) {
    void *&slot = out->clv[(size_t)c.ops[j].parent];
    if (!slot) slot = ws + lay.clv0 + (size_t)nclv++ * lay.clv_stride;
    out->sc_rows[(size_t)j] = reinterpret_cast<uint8_t *>(ws + lay.sc0 + (size_t)j * lay.row);
  }
  for (int s = 0; s < c.nslots; s++) {
    if (mask.empty() || !mask[(size_t)s]) continue;
    uint8_t *dst = reinterpret_cast<uint8_t *>(ws + lay.tip0 + (size_t)ntile++ * lay.row);
    out->wtips[(size_t)s] = dst;
    out->tiles.push_back(PsrTileDescH{c.tips[s], dst});
  }
  out->root = out->clv[(size_t)c.ops[c.nops - 1].parent];

  const int tail_gc = c.ncand % c.group;
  for (int k0 = 0; k0 < c.ncand; k0 += c.group) {
    const int gc = std::min(c.group, c.ncand - k0);
    out->passes.push_back(PsrScanPass{k0, gc, gc < c.group});
  }
  const TravArrays arr{c.ops, c.nops, out->clv.data(), out->wtips.data(), out->pmats, out->sc_rows.data(), nullptr};
  std::string lerr;
  if (c.ncand >= c.group &&
      lower_psr_traversal(out->trav, arr, PsrCall{c.dtype, (int64_t)c.group * c.n, c.group, c.EV, out->cat, c.states},
                          &out->full, &lerr) != PLFX_OK)
    return refuse(out, err, inv, lerr.c_str());
  if (tail_gc &&
      lower_psr_traversal(out->trav, arr, PsrCall{c.dtype, (int64_t)tail_gc * c.n, tail_gc, c.EV, out->cat, c.states},
                          &out->tail, &lerr) != PLFX_OK)
    return refuse(out, err, inv, lerr.c_str());
  return PLFX_OK;
}

}  // namespace plfx
