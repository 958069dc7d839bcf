// psr_prot_fma_lower_main.cpp -- PsrCall::flags and PsrScanCall::flags
// (plfx.h section 11d) do not change what a call lowers to: the launch list
// of a batch, of a traversal and of a rate scan is the same for flags 0 and
// PLFX_FMA -- only the executor's launcher differs.  A stand-alone program for
// tests/test_psr_prot_fma_abi.py (built with ASan + UBSan); every pointer is a
// made-up address that is never followed (the layout of
// psr_prot_lower_main.cpp and psr_prot_scan_lower_main.cpp).
//
// No input.  stdout: per case "same NAME items nodes" when the two lists agree
// field by field (and hold something), else "differ NAME" and exit status 1.
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

bool same_lists(const plfx::PsrLaunchList &a, const plfx::PsrLaunchList &b) {
  if (a.items.size() != b.items.size() || a.nodes.size() != b.nodes.size() || a.triples.size() != b.triples.size())
    return false;
  for (size_t i = 0; i < a.items.size(); i++) {
    const plfx::PsrLaunch &x = a.items[i], &y = b.items[i];
    if (x.kind != y.kind || x.level != y.level || x.tips != y.tips || x.first != y.first || x.count != y.count)
      return false;
  }
  for (size_t i = 0; i < a.nodes.size(); i++) {
    const plfx::NodeDescH &x = a.nodes[i], &y = b.nodes[i];
    if (x.x1 != y.x1 || x.x2 != y.x2 || x.x3 != y.x3 || x.left != y.left || x.right != y.right ||
        x.scaler != y.scaler || x.scaler_sum != y.scaler_sum)
      return false;
  }
  return true;
}

int verdict(const char *name, bool ok, const plfx::PsrLaunchList &l) {
  if (ok && !l.items.empty()) {
    printf("same %s %zu %zu\n", name, l.items.size(), l.nodes.size());
    return 0;
  }
  printf("differ %s\n", name);
  return 1;
}

constexpr int kStates = 20, kNcat = 25;
constexpr long long kN = 33;
constexpr unsigned long long kCb = kN * kStates * 8;

plfx::PsrCall call_with(int flags) {
  plfx::PsrCall c{PLFX_F64, kN, kNcat, at<const void>(0x80000000ull), at<const uint8_t>(0x90000001ull), kStates};
  c.flags = flags;
  return c;
}

// a balanced tree over 8 coded tips: slots 0..7 tips, 8..14 inner nodes
std::vector<plfx_trav_op> balanced8() {
  std::vector<plfx_trav_op> ops;
  int level[8] = {0, 1, 2, 3, 4, 5, 6, 7}, width = 8, next = 8;
  while (width > 1) {
    for (int i = 0; i < width; i += 2) {
      ops.push_back(plfx_trav_op{next, level[i], level[i + 1], (int)ops.size()});
      level[i / 2] = next++;
    }
    width /= 2;
  }
  return ops;
}

}  // namespace

int main() {
  int bad = 0;
  std::string err;
  // a batch of 70 nodes, the four kinds of children in turn
  {
    std::vector<plfx_psr_node> nodes(70);
    for (int i = 0; i < 70; i++) {
      plfx_psr_node &d = nodes[(size_t)i];
      d = plfx_psr_node{};
      const int kind = i % 4;
      if (kind & 1) d.tip1 = at<const uint8_t>(0x40000000ull + (2ull * i) * 64 + 1);
      else d.x1 = at<const void>(0x100000ull + (3ull * i) * kCb);
      if (kind & 2) d.tip2 = at<const uint8_t>(0x40000000ull + (2ull * i + 1) * 64 + 1);
      else d.x2 = at<const void>(0x100000ull + (3ull * i + 1) * kCb);
      d.x3 = at<void>(0x100000ull + (3ull * i + 2) * kCb);
      d.left = at<const void>(0x50000000ull + (2ull * i) * 102400);
      d.right = at<const void>(0x50000000ull + (2ull * i + 1) * 102400);
      d.scaler = at<uint8_t>(0x60000000ull + 64ull * i);
      d.scaler_sum = at<int64_t>(0x70000000ull + 8ull * i);
    }
    plfx::PsrLaunchList exact, fma;
    const int r0 = plfx::lower_psr(call_with(0), nodes.data(), 70, &exact, &err);
    const int r1 = plfx::lower_psr(call_with(PLFX_FMA), nodes.data(), 70, &fma, &err);
    bad |= verdict("batch", r0 == PLFX_OK && r1 == PLFX_OK && same_lists(exact, fma), fma);
  }
  // a traversal and a rate scan of the balanced tree
  const std::vector<plfx_trav_op> ops = balanced8();
  const int nops = (int)ops.size(), nslots = 15;
  std::vector<void *> clv((size_t)nslots);
  std::vector<const uint8_t *> tips((size_t)nslots);
  std::vector<unsigned char> mask((size_t)nslots);
  for (int s = 0; s < nslots; s++) {
    const bool tip = s < 8;
    clv[(size_t)s] = tip ? nullptr : at<void>(0x100000ull + (unsigned long long)s * kCb);
    tips[(size_t)s] = tip ? at<const uint8_t>(0x40000000ull + 64ull * s + 1) : nullptr;
    mask[(size_t)s] = tip;
  }
  {
    std::vector<uint8_t *> scalers((size_t)nops);
    for (int j = 0; j < nops; j++) scalers[(size_t)j] = at<uint8_t>(0x60000000ull + 64ull * j);
    plfx::TravArrays arr{ops.data(),           nops, clv.data(), tips.data(), at<const void>(0x50000000ull),
                         scalers.data(), at<int64_t>(0x70000000ull)};
    plfx::TravPlan plan;
    int rc = plfx::plan_traversal(ops.data(), nops, nslots, nops, mask.data(), kStates, 0, &plan, &err);
    plfx::PsrLaunchList exact, fma;
    if (rc == PLFX_OK) rc = plfx::lower_psr_traversal(plan, arr, call_with(0), &exact, &err);
    if (rc == PLFX_OK) rc = plfx::lower_psr_traversal(plan, arr, call_with(PLFX_FMA), &fma, &err);
    bad |= verdict("traversal", rc == PLFX_OK && same_lists(exact, fma), fma);
  }
  {
    const int ncand = 7, group = 3;  // two full passes and a tail of one candidate
    plfx::PsrScanLayout lay{};
    int rc = plfx::psr_scan_layout(PLFX_F64, nops, 8, nops, kN, group, &lay, kStates);
    plfx::PsrScanCall c{PLFX_F64,
                        ops.data(),
                        nops,
                        tips.data(),
                        nslots,
                        at<const double>(0x50000000ull),
                        nops,
                        at<const double>(0x51000000ull),
                        at<const void>(0x52000000ull),
                        at<const void>(0x53000000ull),
                        at<const double>(0x54000000ull),
                        ncand,
                        group,
                        kN,
                        at<void>(0x10000000ull),
                        lay.end,
                        at<int32_t>(0x55000000ull),
                        at<double>(0x56000000ull),
                        at<double>(0x57000000ull),
                        at<double>(0x58000000ull),
                        0,
                        kStates};
    plfx::PsrScanPlan exact, fma;
    if (rc == PLFX_OK) rc = plfx::lower_psr_scan(c, &exact, &err);
    c.flags = PLFX_FMA;
    if (rc == PLFX_OK) rc = plfx::lower_psr_scan(c, &fma, &err);
    bool ok = rc == PLFX_OK && exact.passes.size() == fma.passes.size() && exact.tiles.size() == fma.tiles.size() &&
              !memcmp(&exact.lay, &fma.lay, sizeof exact.lay) && exact.cat == fma.cat && exact.pmats == fma.pmats &&
              exact.root == fma.root && exact.scalers == fma.scalers && exact.sc_stride == fma.sc_stride;
    for (size_t p = 0; ok && p < exact.passes.size(); p++)
      ok = exact.passes[p].k0 == fma.passes[p].k0 && exact.passes[p].gc == fma.passes[p].gc &&
           exact.passes[p].tail == fma.passes[p].tail;
    ok = ok && fma.passes.size() == 3 && fma.passes.back().tail;
    bad |= verdict("scan full", ok && same_lists(exact.full, fma.full), fma.full);
    bad |= verdict("scan tail", ok && same_lists(exact.tail, fma.tail), fma.tail);
  }
  if (bad) fprintf(stderr, "last lowering message: %s\n", err.c_str());
  return bad;
}
