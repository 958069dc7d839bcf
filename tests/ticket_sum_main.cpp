// ticket_sum_main.cpp -- the cross-block scaler sum of the kernels
// (csrc/plf_dna.hpp ticket_publish) replayed on plain int64 words with the
// arithmetic of csrc/ticket_sum.hpp, for tests/test_ticket_sum.py (built there
// with the sanitizers).  Within a launch only the arrival order per word
// matters, so a launch is a permutation of its G blocks; a block does what
// ticket_publish does, in its order: fetch-add on its slot, decode, store 0,
// fetch-add on top, decode, write out, store 0.
//
// Commands (whitespace-separated tokens):
//   decode
//        -> "decode A S got" for arrival counts A and running sums S at and
//           next to both ends of the exact range
//   sweep G seed nshuffles
//        -> per block-total pattern one line
//           "case G pattern runs bad slot_max slot_min top_max top_min total"
//           over the orders ascending, descending, alternating and nshuffles
//           seeded shuffles.  bad counts the runs in which anything but this
//           held: the slots' arrivals sum to G, exactly one block wrote out,
//           the value equals the total formed in __int128, every word is zero
//           afterwards.  slot_/top_ max/min: the extreme running sums a slot
//           word and the top word held (count removed), over all runs.
//   past G
//        -> "past writers dirty": one ascending run with 2^40 on block 0 and
//           nothing elsewhere (one past the contract)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../amd-versal-phylogenetic-likelihood-function_amd/csrc/ticket_sum.hpp"

namespace {

using namespace plfx::dev;

constexpr long long kBound = (1ll << 40) - 1;  // the largest sum |partial| of the contract

struct Rng {
  uint64_t x;
  uint64_t next() {  // splitmix64
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

struct Launch {
  long long G;
  std::vector<long long> ws;  // slot s at ws[s], top at ws[kSlots]
  int writers = 0;
  long long out = 0;
  long long slot_max = 0, slot_min = 0, top_max = 0, top_min = 0;

  explicit Launch(long long G) : G(G), ws(kSlots + 1, 0) {}

  long long fetch_add(int w, long long v, long long &mx, long long &mn) {
    const long long old = ws[w];
    ws[w] = old + v;
    // the running sum the word now holds: the count is the adds so far, known here
    adds[w]++;
    const long long S = ws[w] - adds[w] * kTick;
    mx = std::max(mx, S);
    mn = std::min(mn, S);
    return old;
  }

  // ticket_publish of block b with block total tot
  void block(long long b, long long tot) {
    const long long slot = ticket_slot<unsigned>((unsigned)b);
    const long long nslots = ticket_nslots(G);
    const long long arrivals = ticket_arrivals(G, slot);
    const long long old = fetch_add((int)slot, ticket_add(tot), slot_max, slot_min);
    if (decode_count(old) != arrivals - 1) return;
    const long long slot_sum = ticket_sum_of(old, tot, arrivals);
    ws[slot] = 0;
    adds[slot] = 0;
    const long long told = fetch_add(kSlots, ticket_add(slot_sum), top_max, top_min);
    if (decode_count(told) != nslots - 1) return;
    out = ticket_sum_of(told, slot_sum, nslots);
    writers++;
    ws[kSlots] = 0;
    adds[kSlots] = 0;
  }

  bool clean() const {
    return std::all_of(ws.begin(), ws.end(), [](long long w) { return w == 0; });
  }

  long long adds[kSlots + 1] = {};
};

const char *const kPatterns[] = {"zero",     "one_first", "one_last", "slot_pos", "slot_neg", "last_slot_neg",
                                 "spread_pos", "spread_neg", "cancel",   "random"};

// spread `total` (>= 0) over the blocks idx, the remainder on the first
void spread(std::vector<long long> &p, const std::vector<long long> &idx, long long total, long long sign) {
  const long long q = total / (long long)idx.size();
  for (long long b : idx) p[b] = sign * q;
  p[idx[0]] += sign * (total - q * (long long)idx.size());
}

std::vector<long long> pattern(const std::string &name, long long G, Rng &r) {
  std::vector<long long> p(G, 0), all(G), s0, sl;
  for (long long b = 0; b < G; b++) all[b] = b;
  for (long long b = 0; b < G; b += kSlots) s0.push_back(b);
  for (long long b = (G - 1) % kSlots; b < G; b += kSlots) sl.push_back(b);
  if (name == "zero") return p;
  if (name == "one_first") p[0] = kBound;
  else if (name == "one_last") p[G - 1] = -kBound;
  else if (name == "slot_pos") spread(p, s0, kBound, 1);          // slot 0 and top reach +kBound
  else if (name == "slot_neg") spread(p, s0, kBound, -1);         // ... -kBound
  else if (name == "last_slot_neg") spread(p, sl, kBound, -1);    // the slot of the last block
  else if (name == "spread_pos") spread(p, all, kBound, 1);       // top alone reaches +kBound
  else if (name == "spread_neg") spread(p, all, kBound, -1);
  else if (name == "cancel") {                                    // + on the first half, - on the second
    if (G == 1) return p;
    std::vector<long long> lo(all.begin(), all.begin() + G / 2), hi(all.begin() + G / 2, all.end());
    spread(p, lo, kBound / 2, 1);
    spread(p, hi, kBound - kBound / 2, -1);
  } else {                                                        // random signs and sizes, sum |p| = kBound
    long long left = kBound;
    for (long long b = 0; b < G; b++) {
      const long long m = b == G - 1 ? left : (long long)(r.next() % (uint64_t)(left / 2 + 1));
      p[b] = (r.next() & 1) ? m : -m;
      left -= m;
    }
    std::swap(p[G - 1], p[r.next() % (uint64_t)G]);
  }
  return p;
}

std::vector<long long> order(int kind, long long G, Rng &r) {
  std::vector<long long> o(G);
  for (long long i = 0; i < G; i++) o[i] = i;
  if (kind == 1) std::reverse(o.begin(), o.end());
  else if (kind == 2)  // 0, G-1, 1, G-2, ...
    for (long long i = 0; i < G; i++) o[i] = i % 2 ? G - 1 - i / 2 : i / 2;
  else if (kind >= 3)
    for (long long i = G - 1; i > 0; i--) std::swap(o[i], o[r.next() % (uint64_t)(i + 1)]);
  return o;
}

}  // namespace

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "decode") {
      const long long H = 1ll << 40;
      for (long long A : {0ll, 1ll, 2ll, 31ll, 32ll, 127ll, 128ll, 4096ll, 1ll << 20})
        for (long long S : {-H - 1, -H, -H + 1, -1ll, 0ll, 1ll, H - 2, H - 1, H})
          std::printf("decode %lld %lld %lld\n", A, S, decode_count(A * kTick + S));
    } else if (cmd == "sweep") {
      long long G;
      uint64_t seed;
      int nshuffles;
      if (!(std::cin >> G >> seed >> nshuffles) || G < 1 || nshuffles < 0) return 2;
      long long arrivals = 0;
      for (long long s = 0; s < ticket_nslots(G); s++) arrivals += ticket_arrivals(G, s);
      Rng r{seed};
      for (const char *name : kPatterns) {
        const std::vector<long long> p = pattern(name, G, r);
        __int128 exact = 0, mag = 0;
        for (long long v : p) {
          exact += v;
          mag += v < 0 ? -(__int128)v : v;
        }
        if (mag != 0 && mag != kBound && !(G == 1 && std::string(name) == "cancel")) return 3;
        long long runs = 0, bad = 0, smax = 0, smin = 0, tmax = 0, tmin = 0;
        for (int k = 0; k < 3 + nshuffles; k++) {
          const std::vector<long long> o = order(k, G, r);
          Launch L(G);
          for (long long b : o) L.block(b, p[b]);
          runs++;
          bad += !(arrivals == G && L.writers == 1 && (__int128)L.out == exact && L.clean());
          smax = std::max(smax, L.slot_max);
          smin = std::min(smin, L.slot_min);
          tmax = std::max(tmax, L.top_max);
          tmin = std::min(tmin, L.top_min);
        }
        std::printf("case %lld %s %lld %lld %lld %lld %lld %lld %lld\n", G, name, runs, bad, smax, smin, tmax, tmin,
                    (long long)exact);
      }
    } else if (cmd == "past") {
      long long G;
      if (!(std::cin >> G) || G < 1) return 2;
      Launch L(G);
      for (long long b = 0; b < G; b++) L.block(b, b == 0 ? kBound + 1 : 0);
      std::printf("past %d %d\n", L.writers, (int)!L.clean());
    } else {
      return 2;
    }
  }
  return 0;
}
