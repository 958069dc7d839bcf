"""The cross-block scaler sum at its weight bound, on the CPU.

Every kernel with a scaler_sum ends in ticket_publish (csrc/plf_dna.hpp): a
count and a signed partial sum packed into one 64-bit word, the count decoded
by rounding.  Its arithmetic lives in csrc/ticket_sum.hpp, which the
stand-alone program tests/ticket_sum_main.cpp (plain g++, ASan + UBSan)
replays over int64 words: a launch is a permutation of its G blocks, each
doing ticket_publish's steps in order.  Block totals carry
sum |partial| = 2^40 - 1, the most the contract of plfx.h allows, placed so
that a slot word and the top word hold running sums of +(2^40 - 1) and
-(2^40 - 1).  Asserted per run: the slots' arrivals sum to G, exactly one
block writes the output, the value is the exact total (__int128), every word
is zero afterwards; UBSan reports no signed overflow.  The decode is exact for
a running sum S with -2^40 <= S <= 2^40 - 1 and off by one at S = 2^40 and at
S = -2^40 - 1."""
import os
import subprocess
from pathlib import Path

import pytest

from test_sanitizers import SAN

ROOT = Path(__file__).resolve().parents[1]
BOUND = 2**40 - 1
GRIDS = [1, 2, 31, 32, 33, 63, 64, 65, 1000, 2047, 2048, 4096]
SHUFFLES = 200
PATTERNS = ["zero", "one_first", "one_last", "slot_pos", "slot_neg", "last_slot_neg", "spread_pos", "spread_neg",
            "cancel", "random"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ticket_sum") / "ticket_sum_main"
    subprocess.run(["g++", "-std=c++17", *SAN, str(ROOT / "tests" / "ticket_sum_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=300)

    def run(text):
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=300,
                           # verify_asan_link_order=0: tolerate a preloaded library ahead of the ASan runtime
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0",
                                    UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        return [ln.split() for ln in r.stdout.splitlines()]

    return run


def test_decode_is_exact_on_the_stated_range_and_off_by_one_next_to_it(program):
    rows = [tuple(map(int, r[1:])) for r in program("decode\n") if r[0] == "decode"]
    sums = {S for _, S, _ in rows}
    assert {-2**40 - 1, -2**40, 2**40 - 1, 2**40} <= sums and len(rows) == 9 * 9
    for A, S, got in rows:
        if -2**40 <= S <= 2**40 - 1:
            assert got == A, (A, S, got)
        elif S == 2**40:
            assert got == A + 1, (A, S, got)
        else:
            assert S == -2**40 - 1 and got == A - 1, (A, S, got)


@pytest.mark.parametrize("G", GRIDS)
def test_every_order_elects_one_writer_with_the_exact_total(program, G):
    rows = [r for r in program(f"sweep {G} {20261021 + G} {SHUFFLES}\n") if r[0] == "case"]
    assert [r[2] for r in rows] == PATTERNS
    for r in rows:
        name = r[2]
        g, runs, bad, smax, smin, tmax, tmin, total = map(int, [r[1]] + r[3:])
        print(name, runs, bad, smax, smin, tmax, tmin, total)
        assert g == G and runs == 3 + SHUFFLES
        assert bad == 0, r
        # the running sums the words held, by construction of the patterns
        if name == "zero":
            assert (smax, smin, tmax, tmin, total) == (0, 0, 0, 0, 0)
        if name in ("one_first", "slot_pos"):
            assert smax == BOUND and tmax == BOUND and total == BOUND
        if name in ("one_last", "slot_neg", "last_slot_neg"):
            assert smin == -BOUND and tmin == -BOUND and total == -BOUND
        if name == "spread_pos":
            assert tmax == BOUND and total == BOUND and smin == 0
        if name == "spread_neg":
            assert tmin == -BOUND and total == -BOUND and smax == 0
        if name == "cancel" and G > 1:
            assert total == -1   # 2^39 - 1 up, 2^39 down
            # block 0 (+) arrives first on its slot in ascending order, block G-1 (-) in descending
            assert smax > 0 and smin < 0
        assert -BOUND <= smin and smax <= BOUND and -BOUND <= tmin and tmax <= BOUND


def test_one_past_the_bound_elects_nobody(program):
    """2^40 in one block of a slot with two arrivals: the second arrival
    decodes a count of 2 where it expects 1, returns, and no block writes.
    (Why the GPU tests stay inside the contract.)"""
    assert program("past 33\n") == [["past", "0", "1"]]
