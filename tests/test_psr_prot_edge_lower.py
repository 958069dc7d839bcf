"""The lowering of a plfx_edge_sumtable_psr_batch_gen call with 20 states
(csrc/psr_edge_lower.cpp: the state count sets the bytes of a CLV and of a
table, and with them every overlap interval) on the CPU, as the stand-alone
program tests/psr_prot_edge_lower_main.cpp under ASan + UBSan.  Nothing is
loaded into Python.  Pointers are made-up addresses (the layout is
psr_prot_edge_lower_main.cpp's); n = 33 sites."""
import os
import subprocess
from pathlib import Path

import pytest

from test_sanitizers import SAN

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "amd-versal-phylogenetic-likelihood-function_amd" / "csrc"
ERR_INVALID = -1  # PLFX_ERR_INVALID
F32, F64 = 0, 1
S = 20
N = 33
CLV, TIP, TIPVEC = 0x100000, 0x40000000, 0x80000000
MAX_BATCH = 32


def clv_bytes(dtype, states=S, n=N):
    return n * states * (4 if dtype == F32 else 8)


@pytest.fixture(scope="module")
def lower(tmp_path_factory):
    exe = tmp_path_factory.mktemp("psr_prot_edge_lower") / "psr_prot_edge_lower_main"
    subprocess.run(["g++", "-std=c++17", *SAN, "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "psr_prot_edge_lower_main.cpp"), str(CSRC / "psr_edge_lower.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True, timeout=300)

    def run(cases):
        """cases: (dtype, states, n, kinds, overrides) with kinds 0 (dense side
        1) or 1 (coded) per edge and overrides = [(field, edge, address)] ->
        one dict per case: {"error": (code, items left, edges left, text)} or
        {"items": [(tip, count, [edge rows of 3 addresses])]}."""
        text = []
        for dtype, states, n, kinds, over in cases:
            text.append(f"case {dtype} {states} {n} {len(kinds)} {len(over)}")
            text.append(" ".join(map(str, kinds)))
            text += [f"{f} {i} {a:x}" for f, i, a in over]
        r = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=300,
                           # verify_asan_link_order=0: tolerate a preloaded library ahead of the ASan runtime
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0",
                                    UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        out, cur = [], {"items": []}
        for ln in r.stdout.splitlines():
            w = ln.split()
            if w[0] == "error":
                cur = {"error": (int(w[1]), int(w[2]), int(w[3]), ln.split(" ", 4)[4])}
            elif w[0] == "item":
                cur["items"].append((int(w[1]), int(w[2]), []))
            elif w[0] == "e":
                cur["items"][-1][2].append([int(x, 16) for x in w[1:]])
            elif w[0] == "end":
                out.append(cur)
                cur = {"items": []}
        assert len(out) == len(cases)
        return out

    return run


def expected_row(i, kind, dtype, states=S):
    cb = clv_bytes(dtype, states)
    return [TIP + 64 * i + 1 if kind else CLV + 3 * i * cb, CLV + (3 * i + 1) * cb, CLV + (3 * i + 2) * cb]


@pytest.mark.parametrize("dtype", [F32, F64])
def test_split_by_kind_and_by_32(lower, dtype):
    kinds = [((7 * i + i // 3) % 4) & 1 for i in range(150)]
    assert 40 < sum(kinds) < 110
    cases = [(dtype, S, N, [k] * count, []) for k in (0, 1) for count in (1, 32, 33, 65)] + [(dtype, S, N, kinds, [])]
    res = lower(cases)
    j = 0
    for k in (0, 1):
        for count, launches in ((1, [1]), (32, [32]), (33, [32, 1]), (65, [32, 32, 1])):
            r = res[j]
            j += 1
            assert [(t, c) for t, c, _ in r["items"]] == [(k, c) for c in launches]
            rows = [row for _, _, rs in r["items"] for row in rs]
            assert rows == [expected_row(i, k, dtype) for i in range(count)]  # every edge once, in the caller's order
    seen = []
    for tip, count, rows in res[-1]["items"]:
        assert 1 <= count <= MAX_BATCH and len(rows) == count
        seen += [(tip, r) for r in rows]
    want = [(k, expected_row(i, k, dtype)) for k in (0, 1) for i in range(150) if kinds[i] == k]
    assert seen == want  # dense kind first, each kind in the caller's order, every edge exactly once
    per_kind = [sum(1 for t, _, _ in res[-1]["items"] if t == k) for k in (0, 1)]
    assert per_kind == [-(-kinds.count(k) // MAX_BATCH) for k in (0, 1)]


def refusals(dtype):
    """Every refusal of plfx_edge_sumtable_psr, and the cross-edge ones, with 20-state extents."""
    cb = clv_bytes(dtype)
    tab0 = CLV + 2 * cb  # the table of edge 0
    return [
        ("both tip and CLV", [0], [("tip1", 0, TIP + 1)]),
        ("neither tip nor CLV", [0], [("x1", 0, 0)]),
        ("neither, coded", [1], [("tip1", 0, 0)]),
        ("null x2", [0], [("x2", 0, 0)]),
        ("null sumtab", [1], [("sumtab", 0, 0)]),
        ("x1 misaligned", [0], [("x1", 0, CLV + 8)]),
        ("x2 misaligned", [0], [("x2", 0, CLV + cb + 4)]),
        ("sumtab misaligned", [0], [("sumtab", 0, tab0 + 8)]),
        ("coded side without tipvec", [0, 1], [("tipvec", 0, 0)]),
        ("table over its own x1", [0], [("sumtab", 0, CLV)]),
        ("table shares its own x1's last 16 bytes", [0], [("sumtab", 0, CLV + cb - 16)]),
        ("table over its own x2", [0], [("x2", 0, tab0)]),
        ("table over its own codes", [1], [("tip1", 0, tab0 + 5)]),
        ("table over another edge's table", [0, 0], [("sumtab", 1, tab0)]),
        ("table shares another table's last 16 bytes", [0, 1], [("sumtab", 1, tab0 + cb - 16)]),
        ("table shares another edge's x1's last 16 bytes", [0, 0], [("sumtab", 0, CLV + 3 * cb + cb - 16)]),
        ("table shares another edge's x2's last 16 bytes", [1, 0], [("sumtab", 1, CLV + cb + cb - 16)]),
        ("another edge's input begins inside a table", [0, 0], [("x2", 1, tab0 + 16)]),
        ("the same table twice", [0, 1, 0], [("sumtab", 2, tab0)]),
        ("null edges", [0], [("edges", 0, 0)]),
    ]


@pytest.mark.parametrize("dtype", [F32, F64])
def test_refusals_leave_an_empty_list(lower, dtype):
    cb = clv_bytes(dtype)
    bad = refusals(dtype)
    cases = [(dtype, S, N, kinds, over) for _, kinds, over in bad]
    # the last edge of a second launch is the bad one: nothing of the call may stay
    cases += [(dtype, S, N, [0] * 40, [("sumtab", 39, 0)]),
              (dtype, S, N, [0] * 40, [("sumtab", 39, CLV + 5 * cb)]),  # over edge 1's table
              (dtype, S, N, [1] * 40, [("x2", 39, CLV + 38 * 3 * cb + 8)])]
    cases += [(dtype, S, -1, [0], []), (2, S, N, [0], []), (-1, S, N, [0], []), (dtype, S, N, [], []),
              (dtype, 5, N, [0], []), (dtype, 0, N, [0], [])]  # a state count that is not built
    good = (dtype, S, N, [0, 1, 0], [])
    res = lower([good] + cases + [good])
    for r in (res[0], res[-1]):  # the list is reused: a refusal leaves nothing behind for the next call
        assert [(t, c) for t, c, _ in r["items"]] == [(0, 2), (1, 1)]
        assert [row for _, _, rs in r["items"] for row in rs] == [expected_row(i, k, dtype)
                                                                  for i, k in ((0, 0), (2, 0), (1, 1))]
    names = [b[0] for b in bad] + ["late"] * 3 + ["n < 0", "dtype 2", "dtype -1", "nedges 0", "states 5", "states 0"]
    assert len(names) == len(res) - 2
    for what, r in zip(names, res[1:-1]):
        assert "error" in r, what
        code, items, edges, text = r["error"]
        assert (code, items, edges) == (ERR_INVALID, 0, 0), (what, text)
        assert text.startswith("psr"), what


@pytest.mark.parametrize("dtype", [F32, F64])
def test_apart_at_four_states_is_shared_at_twenty(lower, dtype):
    """Buffers laid out n * 4 values apart: fine for section 11's tables, one
    byte into each other for tables of n * 20 values."""
    cb4, cb20 = clv_bytes(dtype, 4), clv_bytes(dtype, 20)
    base = 0x2000000
    # edge 0's inputs far away and its table alone at base; edge 1's table n * 4 values behind that table's start
    lone = [("x1", 0, 0x4000000), ("x2", 0, 0x4000000 + cb20), ("sumtab", 0, base)]
    two_tables = lone + [("x1", 1, 0x3000000), ("x2", 1, 0x3000000 + cb20), ("sumtab", 1, base + cb4)]
    # ... or edge 1 reads its x2 there
    table_and_input = lone + [("x1", 1, 0x3000000), ("x2", 1, base + cb4), ("sumtab", 1, 0x5000000)]
    # ... the same reached from the other side: the input ends one CLV of 4 states before the table starts
    input_then_table = lone + [("x1", 1, 0x3000000), ("x2", 1, base - cb4), ("sumtab", 1, 0x5000000)]
    own = [("x1", 0, base), ("x2", 0, base + cb4), ("sumtab", 0, base + 2 * cb4)]  # a table over its own inputs at 20
    res = lower([(dtype, 4, N, [0, 0], two_tables), (dtype, 20, N, [0, 0], two_tables),
                 (dtype, 4, N, [0, 0], table_and_input), (dtype, 20, N, [0, 0], table_and_input),
                 (dtype, 4, N, [0, 0], input_then_table), (dtype, 20, N, [0, 0], input_then_table),
                 (dtype, 4, N, [0], own), (dtype, 20, N, [0], own)])
    for r4, r20, word in ((res[0], res[1], "another table"), (res[2], res[3], "input"), (res[4], res[5], "input"),
                          (res[6], res[7], "overlap")):
        assert sum(c for _, c, _ in r4["items"]) in (1, 2), r4  # states 4: accepted
        code, items, edges, text = r20["error"]
        assert (code, items, edges) == (ERR_INVALID, 0, 0) and word in text, text
    # exactly apart at 20 states passes: the last byte of one is the byte before the other
    touch = [("x1", 0, base), ("x2", 0, base + cb20), ("sumtab", 0, base + 2 * cb20),
             ("x1", 1, base + 3 * cb20), ("x2", 1, base + cb20), ("sumtab", 1, base + 4 * cb20)]
    (ok,) = lower([(dtype, 20, N, [0, 0], touch)])
    assert [(t, c) for t, c, _ in ok["items"]] == [(0, 2)]


def test_repeated_inputs_coded_alignment_and_n0(lower):
    cb = clv_bytes(F64)
    shared = [("x1", 1, CLV), ("x2", 2, CLV), ("x2", 1, CLV + cb), ("x2", 3, CLV + cb), ("tip1", 4, TIP + 64 * 3 + 1)]
    res = lower([(F64, S, N, [0, 0, 0, 1, 1], shared),                      # one CLV is an end of three branches
                 (F32, S, N, [1, 1], [("tip1", 0, TIP + 3), ("tip1", 1, TIP + 3)]),  # odd code addresses, one tip twice
                 # n == 0: the call-level checks alone -- nothing of the edges is looked at
                 (F32, S, 0, [0, 1], [("sumtab", 0, 0), ("x2", 1, 8), ("tipvec", 0, 0)]),
                 (F32, S, 0, [], []),                                        # ... and they still run
                 (F32, S, 0, [0], [("edges", 0, 0)]),
                 (F32, 5, 0, [0], [])])
    rows = [expected_row(i, k, F64) for i, k in enumerate([0, 0, 0, 1, 1])]
    rows[1][0], rows[2][1], rows[1][1], rows[3][1], rows[4][0] = CLV, CLV, CLV + cb, CLV + cb, TIP + 64 * 3 + 1
    assert res[0]["items"] == [(0, 3, rows[:3]), (1, 2, rows[3:])]
    assert res[1]["items"] == [(1, 2, [[TIP + 3] + expected_row(i, 1, F32)[1:] for i in (0, 1)])]
    assert res[2] == {"items": []}
    for r in res[3:]:
        assert r["error"][:3] == (ERR_INVALID, 0, 0)
