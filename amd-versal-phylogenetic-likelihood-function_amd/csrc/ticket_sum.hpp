// ticket_sum.hpp -- the arithmetic of the cross-block sum that ends every
// kernel with a scaler_sum (plf_dna.hpp ticket_publish holds the atomics and
// states the protocol), as plain inline functions shared by the device code
// and a host model (tests/ticket_sum_main.cpp): the packed word, the count
// decode, which slot a block adds to, how many arrivals a slot and top
// expect, and the sums the last arrivals read back.  The count-only election
// of plf_lnl.hpp lnl_finish takes its geometry from here too.  Integer + - /
// % >> only.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef PLFX_HD
#define PLFX_HD __host__ __device__
#endif
#else
#ifndef PLFX_HD
#define PLFX_HD
#endif
#endif

namespace plfx {
namespace dev {

constexpr int kSlots = 32;
constexpr long long kTick = 1ll << 41;

// Every add carries its own arrival count: word += kTick + partial, so after
// A arrivals word = A*kTick + S with S the running sum of the partials.  The
// count decodes exactly, decode_count(word) == A, iff -2^40 <= S <= 2^40 - 1;
// at S = 2^40 it reads A + 1 and at S = -2^40 - 1 it reads A - 1.  Any running
// sum of a launch is bounded by sum |wgt|, hence the contract sum |wgt| < 2^40
// (plfx.h).
PLFX_HD inline long long decode_count(long long word) {
  return (word + (kTick >> 1)) >> 41;  // floor((word + kTick/2) / kTick)
}

// ---- geometry: G blocks over min(G, kSlots) slots ----
// the slot block b adds to
template <typename I>
PLFX_HD inline I ticket_slot(I block) {
  return block % kSlots;
}
// the slots in use = the arrivals top expects
template <typename I>
PLFX_HD inline I ticket_nslots(I G) {
  return G < kSlots ? G : (I)kSlots;
}
// the blocks b < G with b % kSlots == slot (slot < min(G, kSlots))
template <typename I>
PLFX_HD inline I ticket_arrivals(I G, I slot) {
  return (G - slot + kSlots - 1) / kSlots;
}

// ---- what one add contributes, and what the last arrival reads back ----
PLFX_HD inline long long ticket_add(long long partial) { return kTick + partial; }
// the sum of all `count` partials added to a word, from the value `old` the
// last fetch-add returned and that add's own partial (slot: count = arrivals;
// top: count = nslots, and the result is the launch's total)
PLFX_HD inline long long ticket_sum_of(long long old, long long partial, long long count) {
  return old + kTick + partial - count * kTick;
}

}  // namespace dev
}  // namespace plfx
