"""GPU tests of plfx_traverse_psr (plfx.h section 11): a whole post-order op
list under per-site rate categories in one call, with fused level pairs
(plf_psr_triple_kernel) where the schedule finds them.  Level pairs are formed
under PLFX_FUSE >= 1 only (unset means unfused for PSR), so
the tests run on contexts created with PLFX_FUSE=1 unless they say otherwise.

The expectation is tests/psr_ref.py's `node` (pinned to the oracle by
tests/test_psr_ref.py), composed op by op in list order on expanded tips.
Everything is compared bit for bit: every inner slot, every scaler byte, every
scaler sum.  Every output buffer sits between guard elements that must not
change.  Each tree's expected schedule (level pairs, unfused ops, launches) is
asserted, so a schedule that silently does not fuse fails; the expected
figures are tests/psr_trees.py's restatement of the planner's rule, which
tests/test_psr_trav_lower.py pins to the planner on the CPU."""
import functools

import numpy as np
import pytest

import plfx
import psr_ref
import psr_trees as T
import scale_cases as SC
from test_gpu_psr import bits, dev, np_dtype, placed_case, same, tdtype

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 4099)
GUARD = 64  # elements: 256 / 512 bytes of values, 64 scaler bytes, on either side


@pytest.fixture(scope="module")
def fctx():
    """A context that fuses level pairs: PLFX_FUSE=1 is read when the context is
    created (unset, a PSR traversal runs every op unfused)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PLFX_FUSE", "1")
        c = plfx.Context(0, lazy_tables=True)
    yield c
    c.close()


# ---- cases ----

def tip_table(rng, dt):
    tv = rng.random((16, 4)) * 0.95 + 0.05
    tv[8:] *= 1e-6  # two coded children scale where both codes are >= 8
    return tv.astype(dt).reshape(-1)


def compose(case, tipvec="own"):
    """The ops one after another in list order through psr_ref.node: per op
    (x3, scaler bytes, weighted sum, sum with wgt NULL)."""
    dt = case["dt"]
    tv = case["tipvec"] if isinstance(tipvec, str) else tipvec
    vals = {s: (psr_ref.expand_tips(x, dt, tv) if case["flags"][s] else x) for s, x in case["inputs"].items()}
    out = []
    for j, (p, a, b, pm) in enumerate(case["ops"]):
        M = case["ncat"] * 16
        left, right = case["pmats"][2 * pm * M:(2 * pm + 1) * M], case["pmats"][(2 * pm + 1) * M:(2 * pm + 2) * M]
        x3, sc, inc = psr_ref.node(vals[a], vals[b], case["EV"], left, right, case["cat"], case["ncat"], case["wgt"])
        vals[p] = x3
        out.append((x3, sc, inc, int(sc.sum())))
    return out


@functools.lru_cache(maxsize=None)
def tree_case(dt, name, n, ncat, seed=0):
    """Inputs of a traversal and its reference.  The matrices are scaled so
    that values shrink by a few orders of magnitude per level: the rescale
    fires at the small sites of the first level and nearly everywhere a few
    levels up, and nothing overflows in a deep tree."""
    dt = np.dtype(dt).type
    tree = TREES[name]() if isinstance(name, str) else name
    ops, nslots, flags = tree
    rng = np.random.default_rng(7919 * n + 31 * ncat + len(ops) + seed)
    cat = rng.integers(0, ncat, n).astype(np.uint8)
    cat[3::7] = np.resize(np.array([ncat, ncat + 1, 200, 255], np.uint8), cat[3::7].size)  # clamped to ncat - 1
    c = dict(dt=dt, n=n, ncat=ncat, ops=[tuple(map(int, o)) for o in ops], nslots=nslots, flags=flags,
             EV=((rng.random(16) - 0.25) * 0.4).astype(dt), pmats=rng.random(2 * len(ops) * ncat * 16).astype(dt),
             cat=cat, wgt=rng.integers(1, 6, n).astype(np.int32), tipvec=tip_table(rng, dt), inputs={})
    written = {o[0] for o in ops}
    for s in range(nslots):
        if s in written:
            continue
        if flags[s]:
            codes = rng.integers(0, 256, n).astype(np.uint8)  # ambiguity sets, junk upper nibbles
            codes[:4] = np.array([0x03, 0xF5, 0x1E, 0x2F], np.uint8)[:min(n, 4)]
            c["inputs"][s] = codes
        else:
            x = rng.random(4 * n)
            x.reshape(n, 4)[::4] *= 1e-12
            c["inputs"][s] = x.astype(dt)
    c["ref"] = compose(c)
    if n >= 64:  # both outcomes of the rescale decision occur
        allsc = np.concatenate([r[1] for r in c["ref"]])
        assert 0 < allsc.sum() < allsc.size
    return c


TREES = {
    "4 coded": lambda: T.balanced(4, True),
    "8 dense": lambda: T.balanced(8, False),
    "mixed": lambda: T.mixed(False),
    "mixed, p swapped": lambda: T.mixed(True),
    "caterpillar": lambda: T.caterpillar(6, True),
    "11 x 4 coded": lambda: T.forest(11, 4, True),
    "random 24": lambda: T.random_tree(24, True, 13),
    "8 dense, shuffled": lambda: (lambda t: (T.shuffled_within_levels(t[0], 3), t[1], t[2]))(T.balanced(8, False)),
    "11 x 4 coded, shuffled": lambda: (lambda t: (T.shuffled_within_levels(t[0], 4), t[1], t[2]))(T.forest(11, 4, True)),
    "random 24, shuffled": lambda: (lambda t: (T.shuffled_within_levels(t[0], 5), t[1], t[2]))(T.random_tree(24, True, 13)),
}
# level pairs, unfused ops, launches
SCHEDULES = {"4 coded": (1, 0, 1), "8 dense": (2, 1, 2), "mixed": (1, 0, 1), "mixed, p swapped": (1, 0, 1),
             "caterpillar": (0, 5, 5), "11 x 4 coded": (11, 0, 2), "8 dense, shuffled": (2, 1, 2),
             "11 x 4 coded, shuffled": (11, 0, 2)}


def schedule_of(name):
    tree = TREES[name]()
    want = T.expected_schedule(tree)
    assert SCHEDULES.get(name, want) == want
    if name.startswith("random"):
        assert want[0] >= 3 and want[1] >= 3  # the random tree has both kinds of work
    return want


def guarded(n, fill, dtype):
    """A buffer of n elements between two guards: (whole, the n elements)."""
    import torch

    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def run(c, case, wgt=True, scalers=True, sums=True, tipvec="own", stream=None, no_scaler=(), keep=None):
    """The traversal through Context.traverse_psr.  Returns a dict of the
    output buffers; `keep` (a former result) reuses its buffers."""
    import torch

    n, nops, td = case["n"], len(case["ops"]), tdtype(case["dt"])
    if keep is None:
        o = dict(clv=[None] * case["nslots"], whole={}, tips=[None] * case["nslots"], sc=[], sc_whole=[])
        for s in range(case["nslots"]):
            if s in case["inputs"]:
                if case["flags"][s]:
                    o["tips"][s] = dev(case["inputs"][s])
                else:
                    o["clv"][s] = dev(case["inputs"][s])
            else:
                o["whole"][s], o["clv"][s] = guarded(4 * n, -7.0, td)
        for j in range(nops):
            w, v = guarded(n, 9, torch.uint8)
            o["sc_whole"].append(w)
            o["sc"].append(None if (not scalers or j in no_scaler) else v)
        o["ss_whole"], o["ss"] = guarded(nops, -5, torch.int64)
        o["dev"] = {k: dev(case[k]) for k in ("pmats", "EV", "cat", "wgt")}
        o["dev"]["tipvec"] = dev(case["tipvec"] if isinstance(tipvec, str) else tipvec) if tipvec is not None else None
    else:
        o = keep
    d = o["dev"]
    has_tips = any(case["flags"])
    c.traverse_psr(np.array(case["ops"], np.int32).reshape(-1, 4), o["clv"], d["pmats"], d["EV"], n, d["cat"],
                   case["ncat"], wgt=d["wgt"] if wgt else None, scalers=o["sc"] if scalers else None,
                   scaler_sums=o["ss"] if sums else None, stream=stream, tips=o["tips"] if has_tips else None,
                   tipvec=d["tipvec"] if has_tips else None)
    return o


def check(case, o, ref=None, wgt=True, scalers=True, sums=True, no_scaler=(), what=""):
    import torch

    torch.cuda.synchronize()
    n = case["n"]
    ref = case["ref"] if ref is None else ref
    for j, (p, _, _, _) in enumerate(case["ops"]):
        x3, esc, einc, eunit = ref[j]
        got = o["whole"][p].cpu().numpy()
        assert same(got[GUARD:GUARD + 4 * n], x3), (what, "op", j)
        assert np.all(got[:GUARD] == -7.0) and np.all(got[GUARD + 4 * n:] == -7.0), (what, "guard of op", j)
        gsc = o["sc_whole"][j].cpu().numpy()
        if scalers and j not in no_scaler:
            assert np.array_equal(gsc[GUARD:GUARD + n], esc), (what, "scaler bytes of op", j)
            assert np.all(gsc[:GUARD] == 9) and np.all(gsc[GUARD + n:] == 9), (what, "scaler guard of op", j)
        else:
            assert np.all(gsc == 9), (what, "scaler bytes of op", j, "were not asked for")
    gss = o["ss_whole"].cpu().numpy()
    nops = len(case["ops"])
    if sums:
        assert gss[GUARD:GUARD + nops].tolist() == [r[2] if wgt else r[3] for r in ref], what
        assert np.all(gss[:GUARD] == -5) and np.all(gss[GUARD + nops:] == -5), what
    else:
        assert np.all(gss == -5), what


def assert_schedule(c, want):
    s = c.last_schedule()
    assert [s[k] for k in ("deep6", "deep5", "deep4", "septets")] == [0, 0, 0, 0]
    assert (s["triples"], s["unfused"], s["launches"]) == tuple(want), s


# ---- shapes, trees, categories ----

@pytest.mark.parametrize("name", ["4 coded", "8 dense", "mixed"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_shapes_are_bit_exact(fctx, dt, name):
    """Fewer sites than one wave, a wave edge, and a partial trip behind a full
    block of U sites per lane, for the three kinds of level pair."""
    want = schedule_of(name)
    for n in SIZES:
        case = tree_case(np_dtype(dt), name, n, 25)
        check(case, run(fctx, case), what=(name, n))
        assert_schedule(fctx, want)


@pytest.mark.parametrize("name", list(TREES))
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_trees_and_their_schedules(fctx, dt, name):
    n = 65 if name.startswith("11 x 4") else 257
    case = tree_case(np_dtype(dt), name, n, 25)
    check(case, run(fctx, case), what=name)
    assert_schedule(fctx, schedule_of(name))


@pytest.mark.parametrize("ncat", [1, 25, 32])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_category_counts_and_the_clamp(fctx, dt, ncat):
    for name in ("4 coded", "8 dense", "mixed, p swapped", "caterpillar"):
        case = tree_case(np_dtype(dt), name, 257, ncat)
        assert (case["cat"] >= ncat).sum() >= 4  # bytes past ncat are present
        check(case, run(fctx, case), what=(name, ncat))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_optional_arguments_and_tip_tables(fctx, dt):
    dt = np_dtype(dt)
    for name in ("random 24", "8 dense"):
        case = tree_case(dt, name, 257, 25)
        check(case, run(fctx, case, wgt=False), wgt=False, what=(name, "wgt NULL"))
        check(case, run(fctx, case, scalers=False), scalers=False, what=(name, "scalers NULL"))
        check(case, run(fctx, case, sums=False), sums=False, what=(name, "scaler_sums NULL"))
        some = tuple(range(0, len(case["ops"]), 2))  # one of a level pair's three, and unfused ops
        check(case, run(fctx, case, no_scaler=some), no_scaler=some, what=(name, "single scalers NULL"))
    case = tree_case(dt, "random 24", 257, 25)
    check(case, run(fctx, case, tipvec=None), ref=compose(case, tipvec=None), what="default tip table")
    custom = np.random.default_rng(5).random(64).astype(dt)
    check(case, run(fctx, case, tipvec=custom), ref=compose(case, tipvec=custom), what="custom tip table")
    case = tree_case(dt, "mixed", 65, 4)
    check(case, run(fctx, case, tipvec=None), ref=compose(case, tipvec=None), what="default tip table, one coded child")


def test_fuse_0_runs_every_op_unfused(monkeypatch):
    monkeypatch.setenv("PLFX_FUSE", "0")
    with plfx.Context(0, lazy_tables=True) as c:
        for dt in (np.float64, np.float32):
            for name in ("random 24", "8 dense", "mixed"):
                case = tree_case(dt, name, 257, 25)
                check(case, run(c, case), what=(name, "PLFX_FUSE=0"))
                tree = TREES[name]()
                want = T.expected_schedule(tree, fuse=False)
                assert want[:2] == (0, len(tree[0]))
                assert_schedule(c, want)
    monkeypatch.delenv("PLFX_FUSE")  # unset: unfused too (level pairs lose at 2^14 sites)
    with plfx.Context(0, lazy_tables=True) as c:
        case = tree_case(np.float64, "8 dense", 257, 25)
        check(case, run(c, case), what="PLFX_FUSE unset")
        assert_schedule(c, (0, 7, 3))
    monkeypatch.setenv("PLFX_FUSE", "2")  # anything >= 1 means level pairs
    with plfx.Context(0, lazy_tables=True) as c:
        case = tree_case(np.float64, "8 dense", 257, 25)
        check(case, run(c, case), what="PLFX_FUSE=2")
        assert_schedule(c, (2, 1, 2))


def test_one_block_walks_every_site(monkeypatch):
    """PLFX_MAX_BLOCKS=1: one block per level pair makes all the trips and is its own last block."""
    monkeypatch.setenv("PLFX_MAX_BLOCKS", "1")
    monkeypatch.setenv("PLFX_FUSE", "1")
    with plfx.Context(0, lazy_tables=True) as c:
        for dt in (np.float64, np.float32):
            for name in ("4 coded", "8 dense", "mixed"):
                case = tree_case(dt, name, 4099, 25)
                check(case, run(c, case), what=(dt, name))
                assert_schedule(c, schedule_of(name))


# ---- the rescale decision ----

def triple_case(dt, a, b, pl, pr, EV, cat, ncat, wgt):
    """ops (4; 0, 1) (5; 2, 3) (6; 4, 5) over four dense inputs."""
    dt = np.dtype(dt).type
    c = dict(dt=dt, n=cat.size, ncat=ncat, ops=[(4, 0, 1, 0), (5, 2, 3, 1), (6, 4, 5, 2)], nslots=7, flags=[False] * 7,
             EV=EV, pmats=np.concatenate([a["left"], a["right"], b["left"], b["right"], pl, pr]).astype(dt), cat=cat,
             wgt=wgt, tipvec=np.zeros(64, dt), inputs={0: a["x1"], 1: a["x2"], 2: b["x1"], 3: b["x2"]})
    c["ref"] = compose(c)
    return c


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_rescale_decision_of_a_and_b_position_by_position(fctx, dt):
    """a and b are test_gpu_psr's placed node (one value at 2^-32, just under it
    or at minus the threshold decides the site, at each of the four positions
    and at every lane); they rescale at half their sites, alone and together, and p
    consumes the rescaled values."""
    dt = np_dtype(dt)
    a, b = placed_case(dt, 0), placed_case(dt, 1)
    assert np.array_equal(a["cat"], b["cat"]) and same(a["EV"], b["EV"])
    case = triple_case(dt, a, b, a["left"], a["right"], a["EV"], a["cat"], a["ncat"], a["wgt"])
    for j, d in enumerate((a, b)):  # the composition meets the closed form of the placed node
        assert same(case["ref"][j][0], d["exp"]) and np.array_equal(case["ref"][j][1], d["sc"])
        for pos in range(4):
            assert np.unique(np.flatnonzero(d["hot"] == pos) % 64).size == 64
    sa, sb, sp = (case["ref"][j][1].astype(bool) for j in range(3))
    assert (sa & sb).any() and (sa & ~sb).any() and (~sa & sb).any() and (~sa & ~sb).any()
    assert sp.any() and (~sp & (sa | sb)).any()  # p decides on its own, also over rescaled children
    check(case, run(fctx, case), what="a, b placed")
    assert_schedule(fctx, (1, 0, 1))


@pytest.mark.parametrize("rot", range(4))
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_rescale_decision_of_p_position_by_position(fctx, dt, rot):
    """a and b pass their first child through (identity matrices and EV, second
    child all ones) with values far above the threshold, and p's left matrices
    are permutations times 2^-F: p is the placed node.  Over the four `rot`
    the deciding value visits each of the four positions at every lane and at
    each of the U sites of a lane's trip (n = 4 * 256 + 37 >= 256 U + 1)."""
    dt = np_dtype(dt)
    F = dt(2.0) ** (1010 if dt == np.float64 else 110)
    ncat = 6
    n = 4 * 256 + SC.TAIL
    thr, below, sub = SC.consts(dt)
    i = np.arange(n)
    hot = (i // 256 + i % 256 + rot) % 4
    kind = (7 * i + i // 64 + rot) % 6
    P = np.full((n, 4), below, dt)
    P[kind == SC.NEGUNDER] *= np.array([1, -1, 1, -1], dt)
    P[kind == SC.ZERO] = sub
    P[i, hot] = np.array([thr, -thr, below, -below, 0.0, np.nan], dt)[kind]
    cat = ((3 * i + i // 7) % ncat).astype(np.uint8)
    perms = [SC.perm(4, 1 + c) for c in range(ncat)]
    A = np.empty((n, 4), dt)
    for c in range(ncat):  # p[k] = A[perm_c[k]] * 2^-F
        m = cat == c
        A[np.ix_(m, perms[c])] = P[m] * F  # exact: a power of two, no overflow
    ident = SC.perm_matrix(4, dt, [np.arange(4)] * ncat)
    a = dict(x1=A.reshape(-1), x2=np.ones(4 * n, dt), left=ident, right=ident)
    b = dict(x1=np.ones(4 * n, dt), x2=np.ones(4 * n, dt), left=ident, right=ident)
    pl = SC.perm_matrix(4, dt, perms, [dt(1) / F] * ncat)
    case = triple_case(dt, a, b, pl, ident, SC.perm_matrix(4, dt, [np.arange(4)]), cat, ncat,
                       (1 + i % 5).astype(np.int32))
    ok = kind != SC.NAN
    ra, rb, rp = case["ref"][:3]
    assert same(ra[0].reshape(n, 4)[ok], A[ok]) and not ra[1].any() and not rb[1].any()  # passed through, unscaled
    finite = A[ok]
    assert np.abs(finite[finite != 0]).min() >= 2.0 ** -20  # far above 2^-32
    exp = P.copy()
    sc = np.array(SC.SCALES)[kind]
    exp[sc] = (exp[sc].astype(np.float64) * SC.TWO32).astype(dt)
    exp[kind == SC.NAN] = np.nan
    assert same(rp[0], exp.reshape(-1)) and np.array_equal(rp[1], sc.astype(np.uint8))  # p is the placed node
    for pos in range(4):
        assert {int(k) for k in kind[hot == pos]} == set(range(6))
    check(case, run(fctx, case), what=("p placed", rot))
    assert_schedule(fctx, (1, 0, 1))


# ---- against the node path, capture, refusals ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_traversal_equals_level_by_level_node_batches(ctx, fctx, dt):
    import torch

    dt = np_dtype(dt)
    for name in ("random 24", "8 dense, shuffled"):
        case = tree_case(dt, name, 257, 25)
        o = run(fctx, case)
        torch.cuda.synchronize()
        n, M, d = case["n"], 25 * 16, o["dev"]
        clv = [None if t is None else t.clone() for t in o["clv"]]
        lv = T.levels(case["ops"])
        sc = [torch.full((n,), 9, dtype=torch.uint8, device="cuda") for _ in case["ops"]]
        ss = torch.full((len(case["ops"]),), -5, dtype=torch.int64, device="cuda")
        for s in o["whole"]:
            clv[s].fill_(-7.0)
        for level in range(max(lv) + 1):
            nodes = []
            for j, (p, a, b, pm) in enumerate(case["ops"]):
                if lv[j] != level:
                    continue
                nd = dict(x3=clv[p], left=d["pmats"][2 * pm * M:(2 * pm + 1) * M],
                          right=d["pmats"][(2 * pm + 1) * M:(2 * pm + 2) * M], scaler=sc[j], scaler_sum=ss[j:j + 1])
                for side, s in ((1, a), (2, b)):
                    nd[f"tip{side}" if case["flags"][s] else f"x{side}"] = o["tips"][s] if case["flags"][s] else clv[s]
                nodes.append(nd)
            ctx.plf_psr(nodes, d["EV"], n, d["cat"], 25, wgt=d["wgt"], tipvec=d["tipvec"] if any(case["flags"]) else None)
        torch.cuda.synchronize()
        for j, (p, _, _, _) in enumerate(case["ops"]):
            assert np.array_equal(bits(o["clv"][p].cpu().numpy()), bits(clv[p].cpu().numpy())), (name, j)
            assert np.array_equal(o["sc"][j].cpu().numpy(), sc[j].cpu().numpy()), (name, j)
        assert np.array_equal(o["ss"].cpu().numpy(), ss.cpu().numpy()), name


def test_captured_traversal_replays_to_the_eager_bits(monkeypatch):
    """Captured on a stream whose first use is the capture, replayed twice with the outputs cleared."""
    import torch

    monkeypatch.setenv("PLFX_FUSE", "1")
    case = tree_case(np.float64, "random 24", 257, 25)
    with plfx.Context(0, lazy_tables=True) as c:
        o = run(c, case)
        check(case, o, what="eager")
        want = schedule_of("random 24")
        cold = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cold):
            run(c, case, stream=cold, keep=o)
        assert_schedule(c, want)
        for _ in range(2):
            for t in list(o["whole"].values()):
                t[GUARD:GUARD + 4 * case["n"]].zero_()
            for t in o["sc_whole"]:
                t[GUARD:GUARD + case["n"]].zero_()
            o["ss"].fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            check(case, o, what="replay")
        del g
        torch.cuda.synchronize()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_argument_errors_enqueue_nothing_and_leave_the_context_usable(monkeypatch):
    import torch

    monkeypatch.setenv("PLFX_FUSE", "1")
    n, ncat, dt = 65, 4, np.float64
    case = tree_case(dt, "8 dense", n, ncat)
    mixed = tree_case(dt, "mixed", n, ncat)
    C = plfx.C
    with plfx.Context(0, lazy_tables=True) as c:
        L, h = c._L, c.h
        o = run(c, case)
        check(case, o, what="before")
        for t in o["whole"].values():
            t.fill_(-7.0)
        o["ss"].fill_(-5)
        torch.cuda.synchronize()
        d = o["dev"]
        p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        big = torch.full((4 * n * 3 + 8,), -7.0, dtype=torch.float64, device="cuda")

        def call(ops=case["ops"], clv=None, over=None, tips=None, nslots=15, pmats=d["pmats"], npmats=7, EV=d["EV"],
                 n_=n, cat=d["cat"], ncat_=ncat, dtype=plfx.F64, null_clv=False, null_ops=False, nops=None, sums=o["ss"]):
            ptrs = [p(t) for t in (o["clv"] if clv is None else clv)]
            for s, t in (over or {}).items():
                ptrs[s] = p(t)
            top = (plfx.TravOp * len(ops))(*[plfx.TravOp(*map(int, r)) for r in ops])
            slots = (C.c_void_p * len(ptrs))(*ptrs)
            tp = None if tips is None else (C.c_void_p * len(tips))(*[p(t) for t in tips])
            return L.plfx_traverse_psr(h, dtype, None if null_ops else top, len(ops) if nops is None else nops,
                                       None if null_clv else slots, tp, nslots, p(pmats), npmats, p(EV), n_, p(cat), ncat_,
                                       None, None, p(sums), None, None)

        INV = plfx.ERR_INVALID
        # ops (8;0,1) (9;2,3) (10;8,9) (11;4,5) (12;6,7) (13;11,12) (14;10,13)
        assert call(ncat_=0) == INV and call(ncat_=33) == INV
        assert b"ncat" in L.plfx_last_error(h)
        assert call(n_=-1) == INV and call(dtype=2) == INV and call(nops=-1) == INV
        assert call(EV=None) == INV and call(cat=None) == INV and call(pmats=None) == INV
        assert call(null_clv=True) == INV and call(null_ops=True) == INV
        assert call(npmats=6) == INV                                  # the planner's checks: pmat out of range
        assert call(nslots=14) == INV                                 # slot out of range
        assert call(ops=[(8, 0, 8, 0)]) == INV                        # a parent that is its own child
        assert call(over={5: None}) == INV and call(over={12: None}) == INV   # null CLV of an input / a parent slot
        assert call(over={3: big[1:]}) == INV and call(over={14: big[1:]}) == INV  # misaligned
        assert call(over={8: o["clv"][0]}) == INV                     # a parent over child 1
        assert call(over={9: o["clv"][3][4 * n - 2:]}) == INV         # sharing child 2's last 16 bytes
        assert call(over={10: o["clv"][0]}) == INV                    # p over a leaf of a
        assert call(over={10: o["clv"][3][4 * n - 2:]}) == INV        # p over 16 bytes of a leaf of b
        assert call(over={8: o["clv"][3]}) == INV                     # a over a leaf of b
        assert call(over={9: o["clv"][8]}) == INV                     # a and b: distinct slots, one buffer
        assert b"level pair" in L.plfx_last_error(h)
        assert call(over={14: o["clv"][13]}) == INV                   # the last op, unfused, over its child
        # a tip slot as a parent; a coded child under its parent
        om = run(c, mixed)
        torch.cuda.synchronize()
        mt = [None if t is None else t for t in om["tips"]]
        assert call(ops=[(4, 0, 2, 0), (1, 3, 2, 1)], clv=om["clv"], tips=mt, nslots=7, npmats=3) == INV
        codes_in_clv = list(mt)
        codes_in_clv[0] = om["clv"][4].view(torch.uint8)[5:]
        assert call(ops=mixed["ops"], clv=om["clv"], tips=codes_in_clv, nslots=7, npmats=3, sums=None) == INV
        cap = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cap):
            rc = call(ncat_=33)
        assert rc == INV
        del g
        torch.cuda.synchronize()
        for t in o["whole"].values():
            assert np.all(t.cpu().numpy() == -7.0)                    # nothing ran
        assert np.all(o["ss_whole"].cpu().numpy() == -5)
        assert c.last_schedule()["launches"] == 0
        # n == 0 and nops == 0 launch nothing and zero the sums
        assert call(n_=0) == plfx.OK
        torch.cuda.synchronize()
        assert o["ss"].cpu().numpy().tolist() == [0] * 7 and np.all(o["ss_whole"].cpu().numpy()[:GUARD] == -5)
        s = c.last_schedule()
        assert (s["triples"], s["unfused"], s["launches"]) == (2, 1, 0)
        o["ss"].fill_(-5)
        assert call(ops=[], nops=0) == plfx.OK
        torch.cuda.synchronize()
        assert np.all(o["ss_whole"].cpu().numpy() == -5)
        for t in o["whole"].values():
            assert np.all(t.cpu().numpy() == -7.0)
        with pytest.raises(plfx.PlfxError) as ei:                     # protein: not built
            c.traverse_psr(np.array(case["ops"], np.int32), o["clv"], d["pmats"], d["EV"], n, d["cat"], ncat, states=20)
        assert ei.value.code == plfx.ERR_UNSUPPORTED
        # and the context still works
        check(case, run(c, case, keep=o), what="after")
        assert_schedule(c, (2, 1, 2))
