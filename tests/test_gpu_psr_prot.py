"""GPU tests of plfx.h section 11b, protein per-site rate categories: the node
(plfx_plf_psr_dev_gen: dense and coded children, batches, the category loop
under every pattern of categories within a wave, the clamp, the rescale
decision position by position), the traversal (plfx_traverse_psr_gen) and the
root lnL (plfx_root_lnl_psr_gen).

The reference is tests/psr_prot_ref.py, the numpy restatement that
tests/test_psr_prot_ref.py pins to oracle.plf_generic(20, 1, ...) per category
on the CPU.  Node results are compared bit for bit: values, scaler bytes and
the weighted scaler sum.  The root lnL is compared with oracle.root_lnl(20, 1,
...) at the bar tests/test_gpu_psr.py applies to plfx_root_lnl_psr (LNL_RTOL
relatively, per-site log L at LNL_RTOL * max(1, |log L|)).  The last test runs
the whole pipeline against tests/felsenstein_ref.py, which shares nothing with
the library, under the tolerance rule of tests/test_gpu_likelihood_ref.py."""
import functools

import numpy as np
import pytest

import felsenstein_ref as F
import plfx
import psr_prot_ref as R
import psr_trees as T
from test_felsenstein_ref import F32_LNL_CAP
from test_gpu_psr import bits, dev, np_dtype, same, tdtype

pytestmark = pytest.mark.gpu

S = 20
LNL_RTOL = 1e-10
LOG_MINLIK = R.LOG_MINLIK
SIZES = (1, 63, 64, 65, 255, 256, 257)
NCATS = (1, 25, 32)
KINDS = ("dense/dense", "tip/dense", "dense/tip", "tip/tip")
GUARD = 64
BLOCK_SITES = 256  # sites of a block's trip: four waves of 64


# ---- the node ----

def make_node(dt, n, ncat, kind, seed=0, cat=None, default_table=False):
    """Inputs of one node and its reference (x3, scaler bytes, weighted sum).
    Every fourth site of a dense child carries 1e-14, and the rows 12.. of the
    tip table 1e-8 (two coded children scale where both codes are >= 12), so
    the rescale fires on a share of the sites."""
    dt = np.dtype(dt).type
    rng = np.random.default_rng(1000 * n + 10 * ncat + kind + seed)
    t1, t2 = bool(kind & 1), bool(kind & 2)
    d = dict(n=n, ncat=ncat, kind=kind, EV=(rng.random(S * S) - 0.25).astype(dt),
             left=rng.random(S * S * ncat).astype(dt), right=rng.random(S * S * ncat).astype(dt),
             cat=rng.integers(0, ncat, n).astype(np.uint8) if cat is None else np.asarray(cat, np.uint8),
             wgt=rng.integers(1, 6, n).astype(np.int32))
    tv = rng.random((R.CODES, S)) * 0.95 + 0.05
    tv[12:] *= 1e-8
    d["tipvec"] = None if default_table else tv.astype(dt).reshape(-1)
    dense = [None, None]
    for side, tip in enumerate((t1, t2)):
        if tip:
            codes = rng.integers(0, 30, n).astype(np.uint8)  # the rows of the table, and codes past it
            if n >= 32:  # every row, then 24 and 255, which read row 23
                codes[3:29] = list(range(24)) + [24, 255]
            elif n >= 4:
                codes[:4] = [23, 24, 255, 0]
            d[f"tip{side + 1}"] = codes
            dense[side] = R.expand_tips(codes, dt, d["tipvec"])
        else:
            x = rng.random(S * n)
            if side == 0 or t1:  # one dense child carries the small sites
                x.reshape(n, S)[::4] *= 1e-14
            d[f"x{side + 1}"] = dense[side] = x.astype(dt)
    d["dense"] = dense
    d["ref"] = R.node(dense[0], dense[1], d["EV"], d["left"], d["right"], d["cat"], ncat, d["wgt"])
    d["ref_unit"] = int(d["ref"][1].sum())  # the sum with wgt NULL
    return d


node_case = functools.lru_cache(maxsize=None)(make_node)


def run_node(c, d, dt, wgt=True, scaler=True, scaler_sum=True, cat=None, stream=None, dense=False):
    """One node through Context.plf_psr_gen: (x3 buffer with its guard, scaler
    bytes, sum).  dense: the coded children expanded on the host."""
    import torch

    n = d["n"]
    buf = torch.full((S * n + GUARD,), -7.0, dtype=tdtype(dt), device="cuda")
    sc = torch.full((n + GUARD,), 9, dtype=torch.uint8, device="cuda") if scaler else None
    ss = torch.full((1,), -5, dtype=torch.int64, device="cuda") if scaler_sum else None
    nd = dict(x3=buf, left=dev(d["left"]), right=dev(d["right"]), scaler=sc, scaler_sum=ss)
    if dense:
        nd.update(x1=dev(d["dense"][0]), x2=dev(d["dense"][1]))
    else:
        for k in ("x1", "x2", "tip1", "tip2"):
            if k in d:
                nd[k] = dev(d[k])
    tv = None if (d["tipvec"] is None or dense) else dev(d["tipvec"])
    c.plf_psr_gen(S, nd, dev(d["EV"]), n, dev(d["cat"] if cat is None else cat), d["ncat"],
                  wgt=dev(d["wgt"]) if wgt else None, tipvec=tv, stream=stream)
    return buf, sc, ss


def check_node(d, buf, sc, ss, wgt=True, what=""):
    import torch

    torch.cuda.synchronize()
    n = d["n"]
    x3, esc, einc = d["ref"]
    got = buf.cpu().numpy()
    assert same(got[:S * n], x3), what
    assert np.all(got[S * n:] == -7.0), what  # nothing written past the CLV
    if sc is not None:
        gsc = sc.cpu().numpy()
        assert np.array_equal(gsc[:n], esc) and np.all(gsc[n:] == 9), what
    if ss is not None:
        assert int(ss.item()) == (einc if wgt else d["ref_unit"]), what


NULLS = (dict(wgt=False), dict(scaler=False), dict(scaler_sum=False))


@pytest.mark.parametrize("kind", range(4), ids=KINDS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_node_is_bit_exact_at_the_tile_edges(ctx, dt, kind):
    dt = np_dtype(dt)
    j = scaled = 0
    for n in SIZES:
        for ncat in NCATS:
            d = node_case(dt, n, ncat, kind)
            scaled += d["ref_unit"]
            check_node(d, *run_node(ctx, d, dt), what=(n, ncat, "all outputs"))
            null = NULLS[j % 3]  # wgt, scaler, scaler_sum NULL in turn
            j += 1
            check_node(d, *run_node(ctx, d, dt, **null), wgt=null.get("wgt", True), what=(n, ncat, null))
    total = 3 * sum(SIZES)
    assert total // 8 <= scaled <= total - total // 8  # both outcomes of the rescale on a good share of the sites


def category_patterns(n, ncat):
    rng = np.random.default_rng(7)
    runs = np.repeat(np.arange(8) % ncat, [1, 7, 64, 100, 3, 60, 21, 1])  # boundaries inside the waves
    assert runs.size == n
    return {"one category": np.full(n, ncat - 1), "sorted runs": np.sort(runs), "runs, unsorted": runs,
            "i % 32": np.arange(n) % 32, "random": rng.integers(0, ncat, n)}


@pytest.mark.parametrize("kind", [0, 1, 3], ids=["dense/dense", "tip/dense", "tip/tip"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_category_patterns_within_a_wave(ctx, dt, kind):
    dt = np_dtype(dt)
    n, ncat = 257, 32
    for name, cat in category_patterns(n, ncat).items():
        d = make_node(dt, n, ncat, kind, seed=5, cat=cat)
        check_node(d, *run_node(ctx, d, dt), what=name)


@pytest.mark.parametrize("kind", [0, 3], ids=["dense/dense", "tip/tip"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_categories_past_ncat_are_the_last(ctx, dt, kind):
    dt = np_dtype(dt)
    for ncat in (1, 4, 25):
        d = node_case(dt, 257, ncat, kind)
        hi = d["cat"].copy()
        last = np.flatnonzero(hi == ncat - 1)
        assert last.size >= 4
        hi[last] = np.resize(np.array([ncat, ncat - 1, 200, 255], np.uint8), last.size)  # mixed with ncat - 1 itself
        check_node(d, *run_node(ctx, d, dt, cat=hi), what=ncat)


def test_one_block_walks_every_site(monkeypatch):
    """PLFX_MAX_BLOCKS=1: one block per node makes all three trips (two whole
    tiles of 256 sites and one site) and is its own last block."""
    monkeypatch.setenv("PLFX_MAX_BLOCKS", "1")
    with plfx.Context(0, lazy_tables=True) as c:
        for dt in (np.float64, np.float32):
            for kind in range(4):
                d = node_case(dt, 2 * BLOCK_SITES + 1, 25, kind)
                check_node(d, *run_node(c, d, dt), what=(dt, kind))


@pytest.mark.parametrize("default_table", [False, True], ids=["custom table", "default table"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_coded_children_equal_the_dense_call_on_their_expansion(ctx, dt, default_table):
    import torch

    dt = np_dtype(dt)
    n = 131
    for kind in (1, 2, 3):
        d = make_node(dt, n, 25, kind, seed=9, default_table=default_table)
        for s in (1, 2):
            if f"tip{s}" in d:  # every row of the table, 24 and 255 (which read row 23)
                assert set(range(24)) | {24, 255} <= set(d[f"tip{s}"].tolist())
        coded = run_node(ctx, d, dt)
        check_node(d, *coded, what=(kind, "coded"))
        expanded = run_node(ctx, d, dt, dense=True)
        check_node(d, *expanded, what=(kind, "expanded"))
        torch.cuda.synchronize()
        assert same(coded[0].cpu().numpy(), expanded[0].cpu().numpy())


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batch_of_33_mixed_nodes_equals_one_node_calls(ctx, dt):
    """33 nodes with distinct matrices, the four kinds of children in turn (one
    launch per kind; a second batch of 33 dense/dense nodes crosses the
    32-node launch boundary), some without scaler bytes or a sum."""
    import torch

    dt = np_dtype(dt)
    n, ncat, count = 257, 25, 33
    for mode in ("mixed", "dense"):
        cases = [node_case(dt, n, ncat, i % 4 if mode == "mixed" else 0, 100 + i) for i in range(count)]
        cat, wgt, EV, tv = (dev(cases[0][k]) for k in ("cat", "wgt", "EV", "tipvec"))
        nodes = []
        for i, d in enumerate(cases):
            nd = dict(x3=torch.full((S * n + GUARD,), -7.0, dtype=tdtype(dt), device="cuda"), left=dev(d["left"]),
                      right=dev(d["right"]),
                      scaler=None if i % 7 == 3 else torch.full((n,), 9, dtype=torch.uint8, device="cuda"),
                      scaler_sum=None if i % 5 == 4 else torch.full((1,), -5, dtype=torch.int64, device="cuda"))
            for k in ("x1", "x2", "tip1", "tip2"):
                if k in d:
                    nd[k] = dev(d[k])
            nodes.append(nd)
        ctx.plf_psr_gen(S, nodes, EV, n, cat, ncat, wgt=wgt, tipvec=tv)
        torch.cuda.synchronize()
        for i, (d, nd) in enumerate(zip(cases, nodes)):
            one = dict(nd, x3=torch.full((S * n + GUARD,), -7.0, dtype=tdtype(dt), device="cuda"),
                       scaler=torch.full((n,), 9, dtype=torch.uint8, device="cuda"),
                       scaler_sum=torch.full((1,), -5, dtype=torch.int64, device="cuda"))
            ctx.plf_psr_gen(S, one, EV, n, cat, ncat, wgt=wgt, tipvec=tv)
            torch.cuda.synchronize()
            assert same(nd["x3"].cpu().numpy(), one["x3"].cpu().numpy()), i
            if nd["scaler"] is not None:
                assert np.array_equal(nd["scaler"].cpu().numpy(), one["scaler"].cpu().numpy()), i
            if nd["scaler_sum"] is not None:
                assert int(nd["scaler_sum"].item()) == int(one["scaler_sum"].item()), i
            # and the one-node call is the reference (the shared EV / cat / wgt / table are node 0's)
            x = [R.expand_tips(d[f"tip{s}"], dt, cases[0]["tipvec"]) if f"tip{s}" in d else d[f"x{s}"] for s in (1, 2)]
            x3, esc, einc = R.node(x[0], x[1], cases[0]["EV"], d["left"], d["right"], cases[0]["cat"], ncat,
                                   cases[0]["wgt"])
            assert same(one["x3"].cpu().numpy()[:S * n], x3), i
            assert np.array_equal(one["scaler"].cpu().numpy(), esc) and int(one["scaler_sum"].item()) == einc, i


def test_no_sites_zero_the_sums_and_launch_nothing(ctx):
    import torch

    dt = np.float64
    cases = [node_case(dt, 65, 25, k) for k in (0, 3)]
    nodes = []
    for d in cases:
        nd = dict(x3=torch.full((S * 65,), -7.0, dtype=tdtype(dt), device="cuda"), left=dev(d["left"]),
                  right=dev(d["right"]), scaler=torch.full((65,), 9, dtype=torch.uint8, device="cuda"),
                  scaler_sum=torch.full((1,), -5, dtype=torch.int64, device="cuda"))
        nd.update({k: dev(d[k]) for k in ("x1", "x2", "tip1", "tip2") if k in d})
        nodes.append(nd)
    nodes[1]["scaler_sum"] = None
    ctx.plf_psr_gen(S, nodes, dev(cases[0]["EV"]), 0, dev(cases[0]["cat"]), 25, wgt=dev(cases[0]["wgt"]))
    torch.cuda.synchronize()
    assert int(nodes[0]["scaler_sum"].item()) == 0
    for nd in nodes:
        assert np.all(nd["x3"].cpu().numpy() == -7.0) and np.all(nd["scaler"].cpu().numpy() == 9)


def scale_case(dt, carrier):
    """60 sites whose deciding value -- exactly 2^-32, the value just under it,
    -2^-32 -- visits each of the 20 positions among values far below the
    threshold; then four sites with every value below it and a NaN site.  The
    matrices and EV are permutation matrices (one per category) and the other
    child is all ones, so a parent value is one value of the carrier.  Weights
    positive, zero, negative and the int32 extremes (their absolute sum stays
    far inside the 2^40 contract)."""
    dt = np.dtype(dt).type
    thr = dt(2.0 ** -32)
    under = np.nextafter(thr, dt(0))
    far = dt(2.0 ** -60)
    ncat, n = 3, 65
    P = np.full((n, S), far, dt)
    for i in range(60):
        P[i, i % S] = (thr, under, -thr)[i // S]
    P[60] = under
    P[61] = -under
    P[62] = far
    P[63] = dt(0.0)
    P[64, 7] = np.nan
    must = np.zeros(n, bool)
    must[20:40] = True
    must[60:64] = True
    cat = ((3 * np.arange(n) + np.arange(n) // 7) % ncat).astype(np.uint8)
    i32 = np.iinfo(np.int32)
    wgt = np.resize(np.array([3, 0, -2, i32.max, i32.min, 1, -1], np.int32), n)
    perms = [(3 * np.arange(S) + 1 + c) % S for c in range(ncat)]
    mats = np.zeros((ncat, S, S), dt)
    for c, p in enumerate(perms):
        mats[c, np.arange(S), p] = 1
    ev = (7 * np.arange(S) + 3) % S
    EV = np.zeros((S, S), dt)
    EV[np.arange(S), ev] = 1
    x = np.empty((n, S), dt)
    for c, p in enumerate(perms):  # x3[ev[k]] = x[perm_c[k]]
        m = cat == c
        x[np.ix_(m, p)] = P[np.ix_(m, ev)]
    ones = np.ones(S * n, dt)
    other = np.ascontiguousarray(np.tile(np.eye(S, dtype=dt), (ncat, 1, 1)).reshape(-1))
    d = dict(n=n, ncat=ncat, kind=0, EV=EV.reshape(-1), cat=cat, wgt=wgt, tipvec=None, must=must)
    xs = np.ascontiguousarray(x.reshape(-1))
    if carrier == 1:
        d.update(x1=xs, x2=ones, left=mats.reshape(-1), right=other)
    else:
        d.update(x1=ones, x2=xs, left=other, right=mats.reshape(-1))
    d["dense"] = [d["x1"], d["x2"]]
    d["ref"] = R.node(d["x1"], d["x2"], d["EV"], d["left"], d["right"], cat, ncat, wgt)
    d["ref_unit"] = int(d["ref"][1].sum())
    return d


@pytest.mark.parametrize("carrier", [1, 2])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_rescale_decision_position_by_position(ctx, dt, carrier):
    dt = np_dtype(dt)
    d = scale_case(dt, carrier)
    assert np.array_equal(d["ref"][1], d["must"].astype(np.uint8))  # the restatement decides as the construction says
    assert np.isnan(d["ref"][0].reshape(-1, S)[64]).all()            # 0 * NaN in every chain of the site
    assert d["ref"][2] == int(d["wgt"].astype(np.int64)[d["must"]].sum())
    check_node(d, *run_node(ctx, d, dt), what="weighted")
    check_node(d, *run_node(ctx, d, dt, wgt=False), wgt=False, what="unit weights")


# ---- the traversal ----

TREES = {"balanced 8": lambda: T.balanced(8, True), "caterpillar 6": lambda: T.caterpillar(6, True)}


def tree_problem(dt, name, n=65, ncat=25):
    dt = np.dtype(dt).type
    ops, nslots, flags = TREES[name]()
    ops = [tuple(map(int, o)) for o in ops]
    rng = np.random.default_rng(len(ops) + n)
    tv = rng.random((R.CODES, S)) * 0.95 + 0.05
    tv[12:] *= 1e-8
    return dict(ops=ops, nslots=nslots, flags=flags, n=n, ncat=ncat, EV=(rng.random(S * S) - 0.25).astype(dt),
                pmats=(rng.random(2 * len(ops) * ncat * S * S) * 0.2).astype(dt),
                cat=rng.integers(0, ncat + 3, n).astype(np.uint8), wgt=rng.integers(1, 6, n).astype(np.int32),
                tipvec=tv.astype(dt).reshape(-1), codes={s: rng.integers(0, 30, n).astype(np.uint8)
                                                         for s in range(nslots) if flags[s]})


def run_tree(c, p, dt, n=None):
    import torch

    full = p["n"]  # the tensors keep the problem's size when the call is for fewer sites
    n = full if n is None else n
    clv = [None if p["flags"][s] else torch.full((S * full + GUARD,), -7.0, dtype=tdtype(dt), device="cuda")
           for s in range(p["nslots"])]
    tips = [dev(p["codes"][s]) if p["flags"][s] else None for s in range(p["nslots"])]
    scalers = [torch.full((full,), 9, dtype=torch.uint8, device="cuda") for _ in p["ops"]]
    sums = torch.full((len(p["ops"]),), -5, dtype=torch.int64, device="cuda")
    c.traverse_psr_gen(S, np.array(p["ops"], np.int32), clv, dev(p["pmats"]), dev(p["EV"]), n, dev(p["cat"]),
                       p["ncat"], wgt=dev(p["wgt"]), scalers=scalers, scaler_sums=sums, tips=tips,
                       tipvec=dev(p["tipvec"]))
    torch.cuda.synchronize()
    return clv, scalers, sums


@pytest.fixture(scope="module")
def fctx():
    """A context created with PLFX_FUSE=1: it would fuse the level pairs of a DNA traversal."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PLFX_FUSE", "1")
        c = plfx.Context(0, lazy_tables=True)
    yield c
    c.close()


@pytest.mark.parametrize("fused_ctx", [False, True], ids=["PLFX_FUSE unset", "PLFX_FUSE=1"])
@pytest.mark.parametrize("name", sorted(TREES))
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_traversal_equals_the_ops_one_by_one(ctx, fctx, dt, name, fused_ctx):
    import torch

    dt = np_dtype(dt)
    c = fctx if fused_ctx else ctx
    p = tree_problem(dt, name)
    n, ncat, M = p["n"], p["ncat"], p["ncat"] * S * S
    clv, scalers, sums = run_tree(c, p, dt)
    sched = c.last_schedule()
    assert [sched[k] for k in ("deep6", "deep5", "deep4", "septets", "triples")] == [0] * 5
    assert sched["unfused"] == len(p["ops"])
    assert sched["launches"] == T.expected_schedule(TREES[name](), fuse=False)[2]
    EV, cat, wgt, tv, pm = (dev(p[k]) for k in ("EV", "cat", "wgt", "tipvec", "pmats"))
    one = {s: t for s, t in enumerate(clv)}
    vals = {s: R.expand_tips(c_, dt, p["tipvec"]) for s, c_ in p["codes"].items()}
    total = 0
    for j, (par, a, b, m) in enumerate(p["ops"]):
        nd = dict(x3=torch.full((S * n + GUARD,), -7.0, dtype=tdtype(dt), device="cuda"),
                  left=pm[2 * m * M:(2 * m + 1) * M], right=pm[(2 * m + 1) * M:(2 * m + 2) * M],
                  scaler=torch.full((n,), 9, dtype=torch.uint8, device="cuda"),
                  scaler_sum=torch.full((1,), -5, dtype=torch.int64, device="cuda"))
        for side, s in ((1, a), (2, b)):
            if p["flags"][s]:
                nd[f"tip{side}"] = dev(p["codes"][s])
            else:
                nd[f"x{side}"] = one[s]
        c.plf_psr_gen(S, nd, EV, n, cat, ncat, wgt=wgt, tipvec=tv)
        torch.cuda.synchronize()
        one[par] = nd["x3"]
        assert same(clv[par].cpu().numpy(), nd["x3"].cpu().numpy()), j
        assert np.array_equal(scalers[j].cpu().numpy(), nd["scaler"].cpu().numpy()), j
        assert int(sums[j].item()) == int(nd["scaler_sum"].item()), j
        # and the op is the reference's
        vals[par], esc, einc = R.node(vals[a], vals[b], p["EV"], p["pmats"][2 * m * M:(2 * m + 1) * M],
                                      p["pmats"][(2 * m + 1) * M:(2 * m + 2) * M], p["cat"], ncat, p["wgt"])
        assert same(nd["x3"].cpu().numpy()[:S * n], vals[par]), j
        assert np.array_equal(nd["scaler"].cpu().numpy(), esc) and int(nd["scaler_sum"].item()) == einc, j
        total += einc
    assert total > 0  # the rescale fired somewhere in the tree


def test_traversal_of_no_sites_zeroes_the_sums(ctx):
    p = tree_problem(np.float64, "balanced 8")
    clv, scalers, sums = run_tree(ctx, p, np.float64, n=0)
    assert sums.cpu().numpy().tolist() == [0] * len(p["ops"])
    assert ctx.last_schedule()["launches"] == 0
    assert all(np.all(t.cpu().numpy() == -7.0) for t in clv if t is not None)


# ---- the root lnL ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_root_lnl_matches_the_oracle(ctx, oracle, dt):
    import torch

    dt = np_dtype(dt)
    freq = np.random.default_rng(2).dirichlet(np.ones(S))
    sums = np.array([3, 0, 5], np.int64)
    for n in (0, 1, 65, 257, 1031):
        rng = np.random.default_rng(n)
        x = (rng.random(S * n) * 0.95 + 0.05).astype(dt)
        wgt = rng.integers(0, 4, n).astype(np.int32)
        for full in (False, True):
            kw = dict(freq=dev(freq), wgt=dev(wgt), scaler_sums=dev(sums)) if full else {}
            outs = []
            for _ in range(2):
                out = torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
                site = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
                ctx.root_lnl_psr_gen(S, dev(x), n, out, site_lnl=site, **kw)
                torch.cuda.synchronize()
                outs.append((out.cpu().numpy(), site.cpu().numpy()))
            assert np.array_equal(bits(outs[0][0]), bits(outs[1][0]))  # the reduction order is fixed
            assert np.array_equal(bits(outs[0][1]), bits(outs[1][1]))
            got, site = float(outs[0][0][0]), outs[0][1]
            if n == 0:
                assert got == (8 * LOG_MINLIK if full else 0.0)
                continue
            okw = dict(freq=freq, wgt=wgt, scaler_sums=sums) if full else {}
            ref, ref_site = oracle.root_lnl(S, 1, x, n, catw=np.ones(1), site=True, **okw)
            print(f"n={n} full={full}: lnL {got!r} ref {ref!r} rel {abs(got - ref) / abs(ref):.2e}")
            assert abs(got - ref) <= LNL_RTOL * abs(ref)
            assert np.all(np.abs(site - ref_site) <= LNL_RTOL * np.maximum(1.0, np.abs(ref_site)))
            if not full:  # freq NULL is 1/20 each, and the site_lnl output is optional
                out2 = torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
                ctx.root_lnl_psr_gen(S, dev(x), n, out2, freq=dev(np.full(S, 1.0 / S)))
                torch.cuda.synchronize()
                assert np.array_equal(bits(out2.cpu().numpy()), bits(outs[0][0]))


# ---- states = 4 through the _gen entries ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_four_states_through_the_gen_entries_are_section_11(fctx, dt):
    import torch

    import test_gpu_psr as G

    dt = np_dtype(dt)
    n, ncat = 257, 25
    for kind in range(4):
        d = G.node_case(dt, n, ncat, kind)
        old = G.run_node(fctx, d, dt)
        buf = torch.full((4 * n + G.GUARD,), -7.0, dtype=tdtype(dt), device="cuda")
        sc = torch.full((n + G.GUARD,), 9, dtype=torch.uint8, device="cuda")
        ss = torch.full((1,), -5, dtype=torch.int64, device="cuda")
        nd = dict(x3=buf, left=dev(d["left"]), right=dev(d["right"]), scaler=sc, scaler_sum=ss)
        nd.update({k: dev(d[k]) for k in ("x1", "x2", "tip1", "tip2") if k in d})
        fctx.plf_psr_gen(4, nd, dev(d["EV"]), n, dev(d["cat"]), ncat, wgt=dev(d["wgt"]),
                         tipvec=dev(d["tipvec"]) if kind else None)
        G.check_node(d, buf, sc, ss, what=kind)
        torch.cuda.synchronize()
        assert np.array_equal(bits(buf.cpu().numpy()), bits(old[0].cpu().numpy()))
    # a traversal: the same bits and the same schedule (this context fuses level pairs), then the root lnL
    ops, nslots, flags = T.balanced(8, False)
    rng = np.random.default_rng(11)
    leaves = [dev(rng.random(4 * n).astype(dt)) for _ in range(8)]
    pm, EV, cat = dev((rng.random(2 * len(ops) * ncat * 16) * 0.5).astype(dt)), dev(d["EV"]), dev(d["cat"])
    res = []
    for gen in (False, True):
        clv = leaves + [torch.full((4 * n,), -7.0, dtype=tdtype(dt), device="cuda") for _ in range(nslots - 8)]
        sums = torch.full((len(ops),), -5, dtype=torch.int64, device="cuda")
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        if gen:
            fctx.traverse_psr_gen(4, np.array(ops, np.int32), clv, pm, EV, n, cat, ncat, scaler_sums=sums)
            fctx.root_lnl_psr_gen(4, clv[-1], n, out, scaler_sums=sums)
        else:
            fctx.traverse_psr(np.array(ops, np.int32), clv, pm, EV, n, cat, ncat, scaler_sums=sums)
            fctx.root_lnl_psr(clv[-1], n, out, scaler_sums=sums)
        torch.cuda.synchronize()
        res.append((fctx.last_schedule(), [t.cpu().numpy() for t in clv[8:]], sums.cpu().numpy(), out.cpu().numpy()))
    assert res[0][0] == res[1][0] and res[0][0]["triples"] > 0
    assert all(same(a, b) for a, b in zip(res[0][1], res[1][1]))
    assert np.array_equal(res[0][2], res[1][2]) and same(res[0][3], res[1][3])


# ---- refusals ----

@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_argument_errors_enqueue_nothing_and_leave_the_context_usable():
    import torch

    n, ncat, dt = 65, 4, np.float64
    d = node_case(dt, n, ncat, 0)
    V = S * n
    with plfx.Context(0, lazy_tables=True) as c:
        L, h = c._L, c.h
        big = torch.full((V * 3 + 8,), -7.0, dtype=torch.float64, device="cuda")
        a, b, x3 = big[:V], big[V:2 * V], big[2 * V:3 * V]
        a.copy_(dev(d["x1"]))
        b.copy_(dev(d["x2"]))
        codes = dev(np.full(n, 5, np.uint8))
        EV, left, right, cat = (dev(d[k]) for k in ("EV", "left", "right", "cat"))
        out = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
        sums = torch.full((1,), -5, dtype=torch.int64, device="cuda")
        p = lambda x: None if x is None else x.data_ptr()  # noqa: E731

        def node(tip1=None, x1=a, tip2=None, x2=b, x3_=x3, left_=left, right_=right, n_=n, ncat_=ncat, EV_=EV, cat_=cat,
                 count=1, dtype=plfx.F64, states=S):
            nd = plfx.PsrNode(p(tip1), p(x1), p(tip2), p(x2), p(x3_), p(left_), p(right_), None, p(sums))
            return L.plfx_plf_psr_dev_gen(h, dtype, states, plfx.C.byref(nd), count, p(EV_), n_, p(cat_), ncat_, None,
                                          None, None)

        pmats = torch.cat([left, right])  # the op's (left, right) pair

        def traverse(states=S, clv2=x3, ncat_=ncat, n_=n, pm=pmats, EV_=EV, cat_=cat, parent=2, npmats=1):
            op = plfx.TravOp(parent, 0, 1, 0)
            slots = (plfx.C.c_void_p * 3)(p(a), p(b), p(clv2))
            return L.plfx_traverse_psr_gen(h, plfx.F64, states, plfx.C.byref(op), 1, slots, None, 3, p(pm), npmats,
                                           p(EV_), n_, p(cat_), ncat_, None, None, p(sums), None, None)

        def root(states=S, x=a, n_=n, out_=out, nsums=0, sums_=None):
            return L.plfx_root_lnl_psr_gen(h, plfx.F64, states, p(x), n_, None, None, p(sums_), nsums, p(out_), None,
                                           None)

        INV, UNS = plfx.ERR_INVALID, plfx.ERR_UNSUPPORTED
        for st in (0, 5, 16, 21, 80, -4):  # states outside {4, 20}
            assert node(states=st) == UNS and traverse(states=st) == UNS and root(states=st) == UNS, st
        assert b"states" in L.plfx_last_error(h)
        assert node(tip1=codes) == INV                   # both a tip and a CLV
        assert node(x1=None) == INV                      # neither
        assert node(tip2=codes) == INV
        assert node(x2=None) == INV
        assert node(x1=x3) == INV                        # the parent over child 1
        assert node(x2=x3) == INV
        assert node(x3_=big[2 * V - 2:]) == INV          # sharing 16 bytes with child 2, at the 20-state size
        assert node(x3_=big[V - 2:], x2=big[2 * V:]) == INV  # ... and with child 1
        assert node(x1=big[1:]) == INV                   # misaligned
        assert node(x2=big[V + 1:]) == INV
        assert node(x3_=big[2 * V + 1:]) == INV
        assert node(x3_=None) == INV and node(left_=None) == INV and node(right_=None) == INV
        assert node(EV_=None) == INV and node(cat_=None) == INV
        assert node(n_=-1) == INV and node(count=0) == INV and node(dtype=2) == INV
        assert node(ncat_=0) == INV and node(ncat_=33) == INV
        assert b"ncat" in L.plfx_last_error(h)
        assert traverse(clv2=None) == INV and traverse(clv2=big[2 * V + 1:]) == INV
        assert traverse(clv2=big[2 * V - 2:]) == INV     # the parent shares 16 bytes with child 2
        assert traverse(ncat_=0) == INV and traverse(ncat_=33) == INV and traverse(n_=-1) == INV
        assert traverse(pm=None) == INV and traverse(EV_=None) == INV and traverse(cat_=None) == INV
        assert traverse(parent=0) == INV and traverse(parent=3) == INV and traverse(npmats=0) == INV
        assert root(out_=None) == INV and root(x=big[1:]) == INV and root(n_=-1) == INV and root(x=None) == INV
        assert root(nsums=1) == INV and root(nsums=-1, sums_=sums) == INV
        with pytest.raises(plfx.PlfxError) as ei:
            c.plf_psr_gen(5, dict(x1=a, x2=b, x3=x3, left=left, right=right), EV, n, cat, ncat)
        assert ei.value.code == UNS
        with pytest.raises(plfx.PlfxError) as ei:
            c.root_lnl_psr_gen(80, a, n, out)
        assert ei.value.code == UNS
        with pytest.raises(plfx.PlfxError) as ei:        # a 4-state tensor size for a 20-state call
            c.plf_psr_gen(S, dict(x1=a[:4 * n], x2=b, x3=x3, left=left, right=right), EV, n, cat, ncat)
        assert ei.value.code == INV
        torch.cuda.synchronize()
        assert np.all(x3.cpu().numpy() == -7.0) and out.item() == -7.0 and sums.item() == -5  # nothing ran
        # and the context still works
        assert node() == plfx.OK and traverse() == plfx.OK and root() == plfx.OK
        torch.cuda.synchronize()
        assert same(x3.cpu().numpy(), d["ref"][0]) and sums.item() == d["ref_unit"]


# ---- capture ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_graph_replays_equal_the_eager_run(dt):
    """A batch, a traversal and a root lnL captured in one HIP graph, replayed twice."""
    import torch

    dt = np_dtype(dt)
    n, ncat = 257, 25
    with plfx.Context(0, lazy_tables=True) as c:
        cases = [node_case(dt, n, ncat, i % 4, 100 + i) for i in range(5)]
        cat, wgt, EV, tv = (dev(cases[0][k]) for k in ("cat", "wgt", "EV", "tipvec"))
        nodes = []
        for d in cases:
            nd = dict(x3=torch.zeros(S * n, dtype=tdtype(dt), device="cuda"), left=dev(d["left"]),
                      right=dev(d["right"]), scaler=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                      scaler_sum=torch.zeros(1, dtype=torch.int64, device="cuda"))
            nd.update({k: dev(d[k]) for k in ("x1", "x2", "tip1", "tip2") if k in d})
            nodes.append(nd)
        p = tree_problem(dt, "balanced 8", n=n, ncat=ncat)
        clv = [None if p["flags"][s] else torch.zeros(S * n, dtype=tdtype(dt), device="cuda")
               for s in range(p["nslots"])]
        tips = [dev(p["codes"][s]) if p["flags"][s] else None for s in range(p["nslots"])]
        tsums = torch.zeros(len(p["ops"]), dtype=torch.int64, device="cuda")
        tpm, tEV, tcat, ttv = (dev(p[k]) for k in ("pmats", "EV", "cat", "tipvec"))
        ops = np.array(p["ops"], np.int32)
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        site = torch.zeros(n, dtype=torch.float64, device="cuda")
        outs = ([t for nd in nodes for t in (nd["x3"], nd["scaler"], nd["scaler_sum"])] +
                [t for t in clv if t is not None] + [tsums, out, site])

        def call(stream):
            c.plf_psr_gen(S, nodes, EV, n, cat, ncat, wgt=wgt, tipvec=tv, stream=stream)
            c.traverse_psr_gen(S, ops, clv, tpm, tEV, n, tcat, ncat, wgt=wgt, scaler_sums=tsums, tips=tips, tipvec=ttv,
                               stream=stream)
            # (EV is signed, so a site's sum may be negative and its log NaN: on every run alike)
            c.root_lnl_psr_gen(S, clv[-1], n, out, wgt=wgt, scaler_sums=tsums, site_lnl=site, stream=stream)

        call(None)
        torch.cuda.synchronize()
        first = [t.cpu().numpy().copy() for t in outs]
        assert same(first[0], cases[0]["ref"][0])
        cold = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cold):
            call(cold)
        for _ in range(2):
            for t in outs:
                t.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for t, f in zip(outs, first):
                a = t.cpu().numpy()
                assert same(a, f) if a.dtype.kind == "f" else np.array_equal(a, f)
        del g
        torch.cuda.synchronize()


# ---- end to end against the independent reference ----

@functools.lru_cache(maxsize=None)
def protein_problem(n=40, ncat=7):
    """A random reversible 20-state model on a 6-taxon tree, random amino acids
    with 5 % gaps (code 23) and a few B / Z / X, categories with values past ncat."""
    ops, nslots, flags = T.random_tree(6, True, 5)
    ops = [tuple(map(int, o)) for o in ops]
    rng = np.random.default_rng(77)
    exch = rng.random(S * (S - 1) // 2) * 2 + 0.05
    freqs = rng.random(S) + 0.1
    Q, pi = F.gtr_q(exch, freqs)
    rates = np.geomspace(0.1, 3.0, ncat)
    cat = rng.integers(0, ncat, n).astype(np.uint8)
    cat[3::7] = np.resize(np.array([ncat, ncat + 1, 200, 255], np.uint8), cat[3::7].size)
    codes = {s: rng.integers(0, 20, n).astype(np.uint8) for s in range(6)}
    for k in codes.values():
        k[rng.random(n) < 0.05] = 23
        k[rng.random(n) < 0.05] = rng.integers(20, 23)
    return dict(ops=ops, nslots=nslots, ntips=6, n=n, ncat=ncat, exch=exch, freqs=freqs, Q=Q, pi=pi, rates=rates,
                cat=cat, site_rates=F.site_rates_psr(rates, cat), blen=rng.random(2 * len(ops)) * 0.25 + 0.05,
                wgt=rng.integers(1, 4, n).astype(np.int32), codes=codes)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_pipeline_lnl_against_the_state_space_reference(ctx, dt):
    """model_eigen(20) -> pmatrix(ncat rates, eigen convention) -> traverse_psr_gen
    -> root_lnl_psr_gen against felsenstein_ref's prune / root_lnl; the bars are
    tests/test_gpu_likelihood_ref.py's: f64 LNL_RTOL * |ref|; f32 |rest - ref| +
    LNL_RTOL * |ref| with rest the numpy restatement on the device's own
    matrices, itself first held to F32_LNL_CAP * |ref|."""
    import torch

    dt = np_dtype(dt)
    p = protein_problem()
    n, ncat, ops = p["n"], p["ncat"], p["ops"]
    table = R.tip_table(np.float64)
    clv_ref = F.prune(p["Q"], ops, p["blen"], {s: table[np.minimum(k, 23)] for s, k in p["codes"].items()},
                      p["site_rates"])
    root = ops[-1][0]
    ref = F.root_lnl(clv_ref[root][0], clv_ref[root][1], p["pi"], None, p["wgt"])[0]
    e = plfx.model_eigen(p["exch"], p["freqs"])
    EV = plfx.model_ev(e, S, plfx.PMAT_EIGEN)
    w = plfx.model_root_weights(e, p["freqs"], plfx.PMAT_EIGEN)
    tv = (table @ EV.reshape(S, S)).astype(dt).reshape(-1)  # tv[code][k] = sum_s table[code][s] * Vi[k][s]
    EV = EV.astype(dt)
    M = ncat * S * S
    pm = torch.empty(2 * len(ops) * M, dtype=tdtype(dt), device="cuda")
    ctx.pmatrix(dev(e), dev(p["rates"]), dev(p["blen"]), pm, states=S, convention=plfx.PMAT_EIGEN)
    clv = [None] * 6 + [torch.empty(S * n, dtype=tdtype(dt), device="cuda") for _ in range(p["nslots"] - 6)]
    tips = [dev(p["codes"][s]) for s in range(6)] + [None] * (p["nslots"] - 6)
    sums = torch.full((len(ops),), -1, dtype=torch.int64, device="cuda")
    ctx.traverse_psr_gen(S, np.array(ops, np.int32), clv, pm, dev(EV), n, dev(p["cat"]), ncat, wgt=dev(p["wgt"]),
                         scaler_sums=sums, tips=tips, tipvec=dev(tv))
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    ctx.root_lnl_psr_gen(S, clv[root], n, out, freq=dev(w), wgt=dev(p["wgt"]), scaler_sums=sums)
    torch.cuda.synchronize()
    got = float(out.item())
    # the restatement on what the kernels read
    pmh = pm.cpu().numpy()
    vals = {s: R.expand_tips(k, dt, tv) for s, k in p["codes"].items()}
    rsums = []
    for par, a, b, m in ops:
        vals[par], _, inc = R.node(vals[a], vals[b], EV, pmh[2 * m * M:(2 * m + 1) * M],
                                   pmh[(2 * m + 1) * M:(2 * m + 2) * M], p["cat"], ncat, p["wgt"])
        rsums.append(inc)
    assert sums.cpu().numpy().tolist() == rsums
    rest = R.root_lnl(vals[root], n, freq=w, wgt=p["wgt"], scaler_sums=np.array(rsums))[0]
    err, margin, scale = abs(got - ref), abs(rest - ref), abs(ref)
    print(f"{np.dtype(dt).name}: gpu {got!r} ref {ref!r} |gpu - ref| / scale {err / scale:.2e}, "
          f"|rest - ref| / scale {margin / scale:.2e}")
    if dt == np.float64:
        assert err <= LNL_RTOL * scale
    else:
        assert margin <= F32_LNL_CAP * scale, "the restatement itself misses the cap: change the input"
        assert err <= margin + LNL_RTOL * scale
