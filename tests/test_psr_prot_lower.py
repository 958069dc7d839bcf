"""The lowering of plfx_plf_psr_dev_gen and plfx_traverse_psr_gen calls with 20
states (csrc/psr_lower.cpp: PsrCall::states sets the CLV bytes, the matrix
stride of 400 values per category and the overlap intervals; no fused level
pair is ever emitted) on the CPU, as the stand-alone program
tests/psr_prot_lower_main.cpp under ASan + UBSan.  Pointers are made-up
addresses (the layout is psr_prot_lower_main.cpp's); n = 33 sites."""
import os
import subprocess
from pathlib import Path

import pytest

import psr_trees as T
from test_sanitizers import SAN

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "amd-versal-phylogenetic-likelihood-function_amd" / "csrc"
ERR_INVALID = -1  # PLFX_ERR_INVALID
F32, F64 = 0, 1
N = 33
CLV, TIP, PM, SC, SS = 0x100000, 0x40000000, 0x50000000, 0x60000000, 0x70000000
MAT = 102400  # bytes between the made-up matrices of a batch: 32 * 400 * 8
MAX_BATCH = 32


def es(dtype):
    return 4 if dtype == F32 else 8


def clv_bytes(dtype, states=20, n=N):
    return n * states * es(dtype)


@pytest.fixture(scope="module")
def lower(tmp_path_factory):
    exe = tmp_path_factory.mktemp("psr_prot_lower") / "psr_prot_lower_main"
    subprocess.run(["g++", "-std=c++17", *SAN, "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "psr_prot_lower_main.cpp"), str(CSRC / "psr_lower.cpp"),
                    str(CSRC / "trav_plan.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=300)

    def run(cases):
        """cases: ("batch", dtype, states, n, ncat, kinds, overrides) or
        ("trav", dtype, states, n, ncat, pstates, fuse, tree, npmats,
        overrides) -> one dict per case: {"error": (code, items left, triples
        left, nodes left, text)} or {"plan": (pairs, unfused, levels) or None,
        "items": [(kind, level, tips, count, [node rows of 7 addresses])]}."""
        text = []
        for c in cases:
            if c[0] == "batch":
                _, dtype, states, n, ncat, kinds, over = c
                text.append(f"batch {dtype} {states} {n} {ncat} {len(kinds)} {len(over)}")
                text.append(" ".join(map(str, kinds)))
            else:
                _, dtype, states, n, ncat, pstates, fuse, (ops, nslots, flags), npmats, over = c
                text.append(f"trav {dtype} {states} {n} {ncat} {pstates} {fuse} {nslots} {npmats} {len(ops)} {len(over)}")
                text.append(" ".join(str(int(f)) for f in flags))
                text += [" ".join(map(str, op)) for op in ops]
            text += [f"{f} {i} {a:x}" for f, i, a in over]
        r = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=300,
                           # verify_asan_link_order=0: tolerate a preloaded library ahead of the ASan runtime
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0",
                                    UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        out, cur = [], {"plan": None, "items": []}
        for ln in r.stdout.splitlines():
            w = ln.split()
            if w[0] == "plan":
                cur["plan"] = tuple(map(int, w[1:]))
            elif w[0] == "error":
                cur = {"error": (int(w[1]), int(w[2]), int(w[3]), int(w[4]), ln.split(" ", 5)[5])}
            elif w[0] == "item":
                cur["items"].append((w[1], int(w[2]), int(w[3]), int(w[4]), []))
            elif w[0] == "n":
                cur["items"][-1][4].append([int(x, 16) for x in w[1:]])
            elif w[0] == "end":
                out.append(cur)
                cur = {"plan": None, "items": []}
        assert len(out) == len(cases)
        return out

    return run


def expected_row(i, kind, dtype, states=20):
    cb = clv_bytes(dtype, states)
    return [TIP + 2 * i * 64 + 1 if kind & 1 else CLV + 3 * i * cb,
            TIP + (2 * i + 1) * 64 + 1 if kind & 2 else CLV + (3 * i + 1) * cb, CLV + (3 * i + 2) * cb,
            PM + 2 * i * MAT, PM + (2 * i + 1) * MAT, SC + 64 * i, SS + 8 * i]


@pytest.mark.parametrize("count,launches", [(1, [1]), (32, [32]), (33, [32, 1]), (70, [32, 32, 6])])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_chunks_of_at_most_32_nodes(lower, count, launches, dtype):
    for kind in range(4):
        (res,) = lower([("batch", dtype, 20, N, 25, [kind] * count, [])])
        assert [(k, t, c) for k, _, t, c, _ in res["items"]] == [("n", kind, c) for c in launches]
        assert all(len(rs) == c <= MAX_BATCH for _, _, _, c, rs in res["items"])
        rows = [r for it in res["items"] for r in it[4]]
        assert rows == [expected_row(i, kind, dtype) for i in range(count)]  # every node once, in the caller's order


def test_mixed_kinds_are_grouped_in_order(lower):
    kinds = [(7 * i + i // 3) % 4 for i in range(70)]
    (res,) = lower([("batch", F64, 20, N, 4, kinds, [])])
    seen = [(t, r) for _, _, t, c, rows in res["items"] for r in rows]
    assert seen == [(k, expected_row(i, k, F64)) for k in range(4) for i in range(70) if kinds[i] == k]
    per_kind = [sum(1 for it in res["items"] if it[2] == k) for k in range(4)]
    assert per_kind == [-(-kinds.count(k) // MAX_BATCH) for k in range(4)]


@pytest.mark.parametrize("dtype", [F32, F64])
def test_overlap_uses_twenty_values_per_site(lower, dtype):
    """The parent's interval is n * 20 values: one byte into a child is
    refused, exactly after (or before) it accepted -- where the 4-state size
    would have decided the other way."""
    cb20, cb4 = clv_bytes(dtype, 20), clv_bytes(dtype, 4)
    x1, x3 = CLV, CLV + 2 * cb20  # node 0's dense child 1 and its parent, as the program places them
    ok = lambda st, kinds, over: ("batch", dtype, st, N, 25, kinds, over)  # noqa: E731
    res = lower([
        # a coded child (N bytes, no alignment rule) whose first byte is the parent's last
        ok(20, [1], [("tip1", 0, x3 + cb20 - 1)]),
        ok(20, [1], [("tip1", 0, x3 + cb20)]),          # the first byte after the parent
        ok(20, [2], [("tip2", 0, x3 - N + 1)]),         # the child's last byte is the parent's first
        ok(20, [2], [("tip2", 0, x3 - N)]),
        # a dense child: the parent begins in its last 16 bytes / exactly after it
        ok(20, [0], [("x2", 0, x1 + 4 * cb20), ("x3", 0, x1 + cb20 - 16)]),  # (child 2 out of the way)
        ok(20, [0], [("x2", 0, x1 + 4 * cb20), ("x3", 0, x1 + cb20)]),
        # the same addresses under 4 states: the 4-state intervals decide the other way
        ok(4, [1], [("x3", 0, x3), ("tip1", 0, x3 + cb20 - 1)]),   # far past a 4-state parent
        ok(4, [1], [("x3", 0, x3), ("tip1", 0, x3 + cb4 - 1)]),    # its last byte
        ok(4, [1], [("x3", 0, x3), ("tip1", 0, x3 + cb4)]),
        ok(20, [1], [("tip1", 0, x3 + cb4)]),                      # accepted by 4-state sizes, inside a 20-state parent
        ok(4, [0], [("x1", 0, x1), ("x2", 0, x1 + 4 * cb20), ("x3", 0, x1 + cb4)]),    # after a 4-state child
        ok(20, [0], [("x1", 0, x1), ("x2", 0, x1 + 4 * cb20), ("x3", 0, x1 + cb4)]),   # inside a 20-state child
    ])
    want = [False, True, False, True, False, True, True, False, True, False, True, False]
    for i, (r, accepted) in enumerate(zip(res, want)):
        assert ("error" not in r) == accepted, (i, r)
        if not accepted:
            assert r["error"][:4] == (ERR_INVALID, 0, 0, 0) and "overlap" in r["error"][4], (i, r)


def test_refusals_leave_an_empty_list(lower):
    cb = clv_bytes(F64)
    x3 = CLV + 2 * cb
    bad = [
        ("both tip and CLV, child 1", [0], [("tip1", 0, TIP + 1)]),
        ("neither, child 2", [1], [("x2", 0, 0)]),
        ("parent over child 1", [0], [("x1", 0, x3)]),
        ("parent over a coded child", [1], [("tip1", 0, x3 + 5)]),
        ("x1 misaligned", [0], [("x1", 0, CLV + 8)]),
        ("x3 misaligned", [0], [("x3", 0, x3 + 8)]),
        ("null x3", [0], [("x3", 0, 0)]),
        ("null left", [3], [("left", 0, 0)]),
        ("null right", [0], [("right", 0, 0)]),
    ]
    cases = [("batch", F64, 20, N, 25, kinds, over) for _, kinds, over in bad]
    # the last node of a third launch is the bad one: nothing of the call may stay
    cases += [("batch", F64, 20, N, 25, [0] * 70, [("x3", 69, 0)])]
    cases += [("batch", F64, 20, N, 0, [0], []), ("batch", F64, 20, N, 33, [0], []), ("batch", F64, 20, -1, 4, [0], []),
              ("batch", 2, 20, N, 4, [0], []), ("batch", F64, 20, N, 4, [], []), ("batch", F64, 5, N, 4, [0], []),
              ("batch", F64, 0, N, 4, [0], [])]
    good = ("batch", F64, 20, N, 25, [0, 3, 1], [])
    res = lower([good] + cases + [good])
    for r in (res[0], res[-1]):  # the list is reused: a refusal leaves nothing behind for the next call
        assert [(t, c) for _, _, t, c, _ in r["items"]] == [(0, 1), (1, 1), (3, 1)]
    names = [b[0] for b in bad] + ["late", "ncat 0", "ncat 33", "n < 0", "dtype", "count 0", "states 5", "states 0"]
    for what, r in zip(names, res[1:-1]):
        assert "error" in r, what
        code, items, triples, nodes, text = r["error"]
        assert (code, items, triples, nodes) == (ERR_INVALID, 0, 0, 0), (what, text)
        assert text.startswith("psr"), what
    (empty,) = lower([("batch", F32, 20, 0, 1, [0, 3], [("x3", 0, 0)])])  # n == 0: call-level checks only
    assert empty == {"plan": None, "items": []}


@pytest.mark.parametrize("dtype", [F32, F64])
def test_traversal_matrices_sit_at_a_400_value_stride(lower, dtype):
    ncat = 25
    tree = T.caterpillar(6, True)
    ops, nslots, flags = tree
    (res,) = lower([("trav", dtype, 20, N, ncat, 20, 0, tree, len(ops), [])])
    assert res["plan"] == (0, len(ops), len(ops))  # a caterpillar: one op per level
    cb, mb = clv_bytes(dtype), ncat * 400 * es(dtype)
    addr = lambda s: TIP + 64 * s + 1 if flags[s] else CLV + s * cb  # noqa: E731
    rows = {}
    for kind, lv, tips, count, rs in res["items"]:
        assert kind == "n" and count == 1
        rows[lv] = (tips, rs[0])
    for j, (p, a, b, pm) in enumerate(ops):
        tips, r = rows[j]
        assert tips == (int(flags[a]) | 2 * int(flags[b]))
        assert r == [addr(a), addr(b), addr(p), PM + 2 * pm * mb, PM + (2 * pm + 1) * mb, SC + 64 * j, SS + 8 * j], j


@pytest.mark.parametrize("coded", [False, True])
def test_no_level_pair_even_when_the_plan_holds_some(lower, coded):
    """A plan made with 4 states and fuse 1 holds level pairs; lowered with 20
    states every op goes out unfused, by level and kind of children; the same
    plan lowered with 4 states does fuse (the program would show it)."""
    tree = T.forest(12, 4, coded)  # 12 trees of 4 leaves: 24 ops on level 0, 12 on level 1
    ops, nslots, flags = tree
    res = lower([("trav", F64, 20, N, 25, 4, 1, tree, len(ops), []),
                 ("trav", F64, 4, N, 25, 4, 1, tree, len(ops), []),
                 ("trav", F64, 20, N, 25, 20, 1, tree, len(ops), [])])
    assert res[0]["plan"] == res[1]["plan"] == (12, 0, 2)
    assert res[2]["plan"] == (0, 36, 2)  # the planner itself fuses nothing for 20 states
    assert any(it[0] == "t" for it in res[1]["items"])
    kind0 = 3 if coded else 0
    for r in (res[0], res[2]):
        assert [(k, lv, t, c) for k, lv, t, c, _ in r["items"]] == [("n", 0, kind0, 24), ("n", 1, 0, 12)]
        assert sorted(row[2] for it in r["items"] for row in it[4]) == sorted(
            CLV + p * clv_bytes(F64) for p, _, _, _ in ops)  # every op's parent once


def test_a_refused_traversal_leaves_an_empty_list(lower):
    tree = T.balanced(8, True)
    ops, nslots, flags = tree
    cb = clv_bytes(F64)
    root, inner = ops[-1][0], ops[-1][1]
    res = lower([("trav", F64, 20, N, 25, 20, 0, tree, len(ops), []),
                 ("trav", F64, 20, N, 25, 20, 0, tree, len(ops), [("clv", root, CLV + inner * cb + cb - 16)]),
                 ("trav", F64, 20, N, 25, 20, 0, tree, len(ops), [("clv", root, CLV + inner * cb + 8)]),
                 ("trav", F64, 20, N, 33, 20, 0, tree, len(ops), []),
                 ("trav", F64, 7, N, 25, 20, 0, tree, len(ops), []),
                 ("trav", F64, 20, N, 25, 20, 0, tree, len(ops), [])])
    for r in (res[0], res[-1]):
        assert [(k, lv, t, c) for k, lv, t, c, _ in r["items"]] == [("n", 0, 3, 4), ("n", 1, 0, 2), ("n", 2, 0, 1)]
    for r in res[1:-1]:
        assert r["error"][:4] == (ERR_INVALID, 0, 0, 0), r
        assert r["error"][4].startswith("psr traverse")
