"""GPU tests of plfx.h section 11, per-site rate categories (PSR): the DNA
node (dense and coded children, batches, the category clamp, the rescale
decision position by position), the root lnL, the sum table, the three edge
sums and the branch-length optimum.

The reference is tests/psr_ref.py, the numpy restatement that
tests/test_psr_ref.py pins to the oracle on the CPU.  Node results are compared
bit for bit: values, scaler bytes and the weighted scaler sum.  The lnL and the
edge sums are compared at the project's f64 bar (LNL_RTOL, as
tests/test_gpu_edge.py and tests/test_gpu_model.py): lnL relatively, d1 and d2
against the sums of their absolute per-site terms, per-site log L at
1e-10 * max(1, |log L|).

Two tests cross-check against code that predates the feature: a PSR node whose
sites all sit in category c is the category-c slice of the Gamma node
(plfx_plf_dev_f32 / _f64) on the four-fold replicated children, and the edge
lnL of A o B at t is the root lnL of the node update at (0.3 t, 0.7 t)."""
import functools

import numpy as np
import pytest
from scipy.optimize import brentq

import plfx
import psr_ref
import scale_cases as SC

pytestmark = pytest.mark.gpu

LNL_RTOL = 1e-10
LOG_MINLIK = psr_ref.LOG_MINLIK
STARTS = (1e-8, 0.01, 0.1, 1.0, 3.0, 10.0)
SIZES = (1, 63, 64, 65, 257, 4099)
NCATS = (1, 4, 25, 32)
KINDS = ("dense/dense", "tip/dense", "dense/tip", "tip/tip")
GUARD = 64


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(got, exp):
    """Equal bits, NaN by position."""
    nan = np.isnan(exp)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(exp[~nan]))


def np_dtype(dt):
    return np.float64 if dt == "f64" else np.float32


def tdtype(dt):
    import torch

    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


# ---- the node ----

@functools.lru_cache(maxsize=None)
def node_case(dt, n, ncat, kind, seed=0):
    """Inputs of one node and its reference (x3, scaler bytes, weighted sum).
    Every fourth site of a dense child carries 1e-12, and the rows 8..15 of
    the tip-vector table 1e-6 (so two coded children scale where both codes
    are >= 8): the rescale fires on a good share of the sites, checked below."""
    dt = np.dtype(dt).type
    rng = np.random.default_rng(1000 * n + 10 * ncat + kind + seed)
    t1, t2 = bool(kind & 1), bool(kind & 2)
    d = dict(n=n, ncat=ncat, kind=kind, EV=(rng.random(16) - 0.25).astype(dt), left=rng.random(16 * ncat).astype(dt),
             right=rng.random(16 * ncat).astype(dt), cat=rng.integers(0, ncat, n).astype(np.uint8),
             wgt=rng.integers(1, 6, n).astype(np.int32))
    tv = rng.random((16, 4)) * 0.95 + 0.05
    tv[8:] *= 1e-6
    d["tipvec"] = tv.astype(dt).reshape(-1)
    dense = [None, None]
    for side, tip in enumerate((t1, t2)):
        if tip:
            codes = rng.integers(0, 256, n).astype(np.uint8)  # ambiguity sets, junk upper nibbles
            if n >= 4:
                codes[:4] = [0x03, 0xF5, 0x1E, 0x2F]
            d[f"tip{side + 1}"] = codes
            dense[side] = psr_ref.expand_tips(codes, dt, d["tipvec"])
        else:
            x = rng.random(4 * n)
            if side == 0 or t1:  # one dense child carries the small sites
                x.reshape(n, 4)[::4] *= 1e-12
            d[f"x{side + 1}"] = dense[side] = x.astype(dt)
    d["ref"] = psr_ref.node(dense[0], dense[1], d["EV"], d["left"], d["right"], d["cat"], ncat, d["wgt"])
    d["ref_unit"] = int(d["ref"][1].sum())  # the sum with wgt NULL
    if n >= 64:
        ones = int(d["ref"][1].sum())
        assert ones >= n / 8 and n - ones >= n / 8, (n, ncat, kind, ones)
    return d


def run_node(c, d, dt, wgt=True, scaler=True, scaler_sum=True, tipvec=True, cat=None, stream=None):
    """One node through Context.plf_psr: (x3 buffer with its guard, scaler bytes, sum)."""
    import torch

    n = d["n"]
    buf = torch.full((4 * n + GUARD,), -7.0, dtype=tdtype(dt), device="cuda")
    sc = torch.full((n + GUARD,), 9, dtype=torch.uint8, device="cuda") if scaler else None
    ss = torch.full((1,), -5, dtype=torch.int64, device="cuda") if scaler_sum else None
    nd = dict(x3=buf, left=dev(d["left"]), right=dev(d["right"]), scaler=sc, scaler_sum=ss)
    for k in ("x1", "x2", "tip1", "tip2"):
        if k in d:
            nd[k] = dev(d[k])
    has_tip = "tip1" in d or "tip2" in d
    args = dict(EV=dev(d["EV"]), rate_cat=dev(d["cat"] if cat is None else cat), wgt=dev(d["wgt"]) if wgt else None,
                tipvec=dev(d["tipvec"]) if (tipvec and has_tip) else None)
    c.plf_psr(nd, args["EV"], n, args["rate_cat"], d["ncat"], wgt=args["wgt"], tipvec=args["tipvec"], stream=stream)
    return buf, sc, ss


def check_node(d, buf, sc, ss, wgt=True, what=""):
    import torch

    torch.cuda.synchronize()
    n = d["n"]
    x3, esc, einc = d["ref"]
    got = buf.cpu().numpy()
    assert np.array_equal(bits(got[:4 * n]), bits(x3)), what
    assert np.all(got[4 * n:] == -7.0), what  # nothing written past the CLV
    if sc is not None:
        gsc = sc.cpu().numpy()
        assert np.array_equal(gsc[:n], esc) and np.all(gsc[n:] == 9), what
    if ss is not None:
        assert int(ss.item()) == (einc if wgt else d["ref_unit"]), what


NULLS = (dict(wgt=False), dict(scaler=False), dict(scaler_sum=False))


@pytest.mark.parametrize("kind", range(4), ids=KINDS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_node_is_bit_exact(ctx, dt, kind):
    dt = np_dtype(dt)
    j = 0
    for n in SIZES:
        for ncat in NCATS:
            d = node_case(dt, n, ncat, kind)
            check_node(d, *run_node(ctx, d, dt), what=(n, ncat, "all outputs"))
            null = NULLS[j % 3]  # wgt, scaler, scaler_sum NULL in turn
            j += 1
            check_node(d, *run_node(ctx, d, dt, **null), wgt=null.get("wgt", True), what=(n, ncat, null))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_default_tip_table_is_the_indicator(ctx, dt):
    dt = np_dtype(dt)
    for kind in (1, 2, 3):
        d = dict(node_case(dt, 257, 25, kind))
        x = [psr_ref.expand_tips(d[f"tip{s}"], dt) if f"tip{s}" in d else d[f"x{s}"] for s in (1, 2)]
        d["ref"] = psr_ref.node(x[0], x[1], d["EV"], d["left"], d["right"], d["cat"], 25, d["wgt"])
        check_node(d, *run_node(ctx, d, dt, tipvec=False), what=kind)


def test_one_block_walks_every_site(monkeypatch):
    """PLFX_MAX_BLOCKS=1: one block per node makes all the trips and is its own last block."""
    monkeypatch.setenv("PLFX_MAX_BLOCKS", "1")
    with plfx.Context(0, lazy_tables=True) as c:
        for dt in (np.float64, np.float32):
            for kind in (0, 3):
                d = node_case(dt, 4099, 25, kind)
                check_node(d, *run_node(c, d, dt), what=(dt, kind))


@pytest.mark.parametrize("mode", ["dense", "mixed"])
@pytest.mark.parametrize("count", [1, 3, 33])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batch_equals_one_node_calls(ctx, dt, count, mode):
    """33 dense/dense nodes cross the 32-node launch boundary; mixed kinds go out
    as one launch per kind.  Every node equals its own one-node call."""
    import torch

    dt = np_dtype(dt)
    n, ncat = 257, 25
    cases = [node_case(dt, n, ncat, 0 if mode == "dense" else i % 4, seed=100 + i) for i in range(count)]
    cat, wgt, EV, tv = (dev(cases[0][k]) for k in ("cat", "wgt", "EV", "tipvec"))
    nodes = []
    for i, d in enumerate(cases):
        nd = dict(x3=torch.full((4 * n + GUARD,), -7.0, dtype=tdtype(dt), device="cuda"), left=dev(d["left"]),
                  right=dev(d["right"]), scaler=torch.full((n,), 9, dtype=torch.uint8, device="cuda"),
                  scaler_sum=None if i % 5 == 4 else torch.full((1,), -5, dtype=torch.int64, device="cuda"))
        for k in ("x1", "x2", "tip1", "tip2"):
            if k in d:
                nd[k] = dev(d[k])
        nodes.append(nd)
    ctx.plf_psr(nodes, EV, n, cat, ncat, wgt=wgt, tipvec=tv)
    torch.cuda.synchronize()
    for i, (d, nd) in enumerate(zip(cases, nodes)):
        one = dict(nd, x3=torch.full((4 * n + GUARD,), -7.0, dtype=tdtype(dt), device="cuda"),
                   scaler=torch.full((n,), 9, dtype=torch.uint8, device="cuda"),
                   scaler_sum=torch.full((1,), -5, dtype=torch.int64, device="cuda"))
        ctx.plf_psr(one, EV, n, cat, ncat, wgt=wgt, tipvec=tv)
        torch.cuda.synchronize()
        assert np.array_equal(bits(nd["x3"].cpu().numpy()), bits(one["x3"].cpu().numpy())), i
        assert np.array_equal(nd["scaler"].cpu().numpy(), one["scaler"].cpu().numpy()), i
        if nd["scaler_sum"] is not None:
            assert int(nd["scaler_sum"].item()) == int(one["scaler_sum"].item()), i
        # and the one-node call is the reference (the shared cat / wgt are node 0's)
        x = [psr_ref.expand_tips(d[f"tip{s}"], dt, cases[0]["tipvec"]) if f"tip{s}" in d else d[f"x{s}"]
             for s in (1, 2)]
        x3, esc, einc = psr_ref.node(x[0], x[1], cases[0]["EV"], d["left"], d["right"], cases[0]["cat"], ncat,
                                     cases[0]["wgt"])
        assert np.array_equal(bits(one["x3"].cpu().numpy()[:4 * n]), bits(x3)), i
        assert np.array_equal(one["scaler"].cpu().numpy(), esc) and int(one["scaler_sum"].item()) == einc, i


@pytest.mark.parametrize("kind", [0, 3], ids=["dense/dense", "tip/tip"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_categories_past_ncat_are_the_last(ctx, dt, kind):
    dt = np_dtype(dt)
    for ncat in (1, 4, 25):
        d = node_case(dt, 257, ncat, kind)
        hi = d["cat"].copy()
        last = np.flatnonzero(hi == ncat - 1)
        assert last.size >= 4
        hi[last] = np.resize(np.array([ncat, ncat + 1, 200, 255], np.uint8), last.size)
        check_node(d, *run_node(ctx, d, dt, cat=hi), what=ncat)


def placed_case(dt, shift, ncat=6):
    """scale_cases' placed case restated for a site's four values: the tables
    and EV are permutation matrices and x2 is all ones, so each parent value is
    one value of x1; the deciding value visits all 4 positions at every lane
    (n = 4 * 256 + 37)."""
    dt = np.dtype(dt).type
    n = 4 * 256 + SC.TAIL
    thr, below, sub = SC.consts(dt)
    i = np.arange(n)
    hot = (i // 256 + i % 256) % 4
    kind = (7 * i + i // 64 + shift) % 6
    wgt = (1 + i % 5).astype(np.int32)
    P = np.full((n, 4), below, dt)
    P[kind == SC.NEGUNDER] *= np.array([1, -1, 1, -1], dt)
    P[kind == SC.ZERO] = sub
    P[i, hot] = np.array([thr, -thr, below, -below, 0.0, np.nan], dt)[kind]
    cat = ((3 * i + i // 7) % ncat).astype(np.uint8)
    ev = SC.ev_perm(4)
    perms = [SC.perm(4, 1 + c) for c in range(ncat)]
    x1 = np.empty((n, 4), dt)
    for c in range(ncat):  # x3[ev[k]] = x1[perm_c[k]]
        m = cat == c
        x1[np.ix_(m, perms[c])] = P[np.ix_(m, ev)]
    exp = P.copy()
    sc = np.array(SC.SCALES)[kind]
    exp[sc] = (exp[sc].astype(np.float64) * SC.TWO32).astype(dt)
    exp[kind == SC.NAN] = np.nan  # 0 * NaN in every chain of the site
    return dict(n=n, ncat=ncat, x1=x1.reshape(-1), x2=np.ones(4 * n, dt), EV=SC.perm_matrix(4, dt, [ev]),
                left=SC.perm_matrix(4, dt, perms), right=SC.perm_matrix(4, dt, [SC.perm(4, 2 + c) for c in range(ncat)]),
                cat=cat, wgt=wgt, hot=hot, kind=kind, exp=exp.reshape(-1), sc=sc.astype(np.uint8))


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_rescale_decision_position_by_position(ctx, dt, shift):
    import torch

    dt = np_dtype(dt)
    d = placed_case(dt, shift)
    for pos in range(4):  # the deciding value visits every position at every lane, in every kind
        assert np.unique(np.flatnonzero(d["hot"] == pos) % 64).size == 64, pos
        assert {int(k) for k in d["kind"][d["hot"] == pos]} == set(range(6)), pos
    for k in range(6):
        assert np.unique(np.flatnonzero(d["kind"] == k) % 64).size == 64, k
    ref = psr_ref.node(d["x1"], d["x2"], d["EV"], d["left"], d["right"], d["cat"], d["ncat"], d["wgt"])
    assert same(ref[0], d["exp"]) and np.array_equal(ref[1], d["sc"])  # the restatement meets the closed form
    buf, sc, ss = run_node(ctx, d, dt)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert same(got[:4 * d["n"]], d["exp"])
    assert np.array_equal(sc.cpu().numpy()[:d["n"]], d["sc"])
    assert int(ss.item()) == int(d["wgt"][d["sc"] == 1].sum())


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_one_category_is_a_slice_of_the_gamma_node(ctx, dt):
    """ncat = 4 with a Gamma node's tables: all sites in category c give the
    category-c slice of plf_dev on the four-fold replicated children."""
    import torch

    dt = np_dtype(dt)
    n = 257
    rng = np.random.default_rng(12)
    x1, x2 = ((rng.random(4 * n) * 0.5 + 0.05).astype(dt) for _ in range(2))
    EV, left, right = ((rng.random(k) * 0.5 + 0.05).astype(dt) for k in (16, 64, 64))
    rep = lambda x: np.ascontiguousarray(np.repeat(x.reshape(n, 1, 4), 4, axis=1).reshape(-1))  # noqa: E731
    g3 = torch.empty(16 * n, dtype=tdtype(dt), device="cuda")
    gsc = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    ctx.plf_dev(dev(rep(x1)), dev(rep(x2)), g3, dev(EV), dev(left), dev(right), None, gsc, None)
    torch.cuda.synchronize()
    assert not gsc.cpu().numpy().any()
    gamma = g3.cpu().numpy().reshape(n, 4, 4)
    for c in range(4):
        d = dict(n=n, ncat=4, x1=x1, x2=x2, EV=EV, left=left, right=right, cat=np.full(n, c, np.uint8),
                 wgt=np.ones(n, np.int32))
        buf, sc, ss = run_node(ctx, d, dt)
        torch.cuda.synchronize()
        assert not sc.cpu().numpy()[:n].any() and int(ss.item()) == 0
        assert np.array_equal(bits(buf.cpu().numpy()[:4 * n].reshape(n, 4)), bits(np.ascontiguousarray(gamma[:, c]))), c


# ---- the root lnL ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_root_lnl_matches_numpy(ctx, dt):
    import torch

    dt = np_dtype(dt)
    freq = np.array([0.1, 0.2, 0.3, 0.4])
    sums = np.array([3, 0, 5], np.int64)
    for n in (0,) + SIZES:
        rng = np.random.default_rng(n)
        x = (rng.random(4 * n) * 0.95 + 0.05).astype(dt)
        wgt = rng.integers(0, 4, n).astype(np.int32)
        for full in (False, True):
            kw = dict(freq=dev(freq), wgt=dev(wgt), scaler_sums=dev(sums)) if full else {}
            outs = []
            for _ in range(2):
                out = torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
                site = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
                ctx.root_lnl_psr(dev(x), n, out, site_lnl=site, **kw)
                torch.cuda.synchronize()
                outs.append((out.cpu().numpy(), site.cpu().numpy()))
            assert np.array_equal(bits(outs[0][0]), bits(outs[1][0]))  # the reduction order is fixed
            assert np.array_equal(bits(outs[0][1]), bits(outs[1][1]))
            got, site = float(outs[0][0][0]), outs[0][1]
            if n == 0:
                assert got == (8 * LOG_MINLIK if full else 0.0)
                continue
            ref, ref_site = psr_ref.root_lnl(x, n, **(dict(freq=freq, wgt=wgt, scaler_sums=sums) if full else {}))
            print(f"n={n} full={full}: lnL {got!r} ref {ref!r} rel {abs(got - ref) / abs(ref):.2e}")
            assert abs(got - ref) <= LNL_RTOL * abs(ref)
            assert np.all(np.abs(site - ref_site) <= LNL_RTOL * np.maximum(1.0, np.abs(ref_site)))


# ---- one branch ----

NCAT_EDGE = 25


@functools.lru_cache(maxsize=None)
def model():
    rng = np.random.default_rng(104)
    exch = rng.random(6) * 2 + 0.05
    freqs = rng.random(4) + 0.1
    e = plfx.model_eigen(exch, freqs)
    return dict(exch=exch, freqs=freqs, pi=freqs / freqs.sum(), e=e, lam=e[:4], V=e[4:20].reshape(4, 4),
                Vi=e[20:].reshape(4, 4), rates=np.geomspace(0.05, 4.0, NCAT_EDGE),
                tv=plfx.model_tip_vectors(e, plfx.PMAT_EIGEN).reshape(16, 4))


def make_sides(dt, side, n, seed):
    """x1, x2 as (n, 4) arrays of dt -- eigen coordinates of positive vectors --
    the categories, and for a coded side 1 its codes and table."""
    m = model()
    rng = np.random.default_rng(seed)
    eig = lambda y: np.einsum("ks,ns->nk", m["Vi"], y).astype(dt)  # noqa: E731
    x2 = eig(rng.random((n, 4)) * 0.5 + 0.05)
    cat = rng.integers(0, NCAT_EDGE + 3, n).astype(np.uint8)  # a few past ncat: clamped
    if side == "dense":
        return eig(rng.random((n, 4)) * 0.5 + 0.05), x2, cat, None, None
    tv = m["tv"].astype(dt)
    codes = rng.integers(0, 256, n).astype(np.uint8)
    codes = np.where((codes & 15) == 0, codes | 15, codes).astype(np.uint8)  # no empty sets
    return psr_ref.expand_tips(codes, dt, tv).reshape(n, 4), x2, cat, codes, tv


def check_out(got, ref, scale, what):
    for j, name in enumerate(("lnL", "d1", "d2")):
        err = abs(got[j] - ref[j])
        print(f"{what} {name}: got {got[j]!r} ref {ref[j]!r} err/scale {err / scale[j] if scale[j] else err:.2e}")
        assert err <= LNL_RTOL * scale[j], (what, name, got[j], ref[j], scale[j])


def gpu_sumtab(c, dt, x1, x2, codes, tv, n, stream=None):
    import torch

    buf = torch.full((4 * n + GUARD,), -7.0, dtype=tdtype(dt), device="cuda")
    st = buf[:4 * n]
    if codes is None:
        c.edge_sumtable_psr(dev(x2.ravel()), st, n, x1=dev(x1.ravel()), stream=stream)
    else:
        c.edge_sumtable_psr(dev(x2.ravel()), st, n, tip1=dev(codes), tipvec=dev(tv.ravel()), stream=stream)
    return st, buf


@pytest.mark.parametrize("side", ["dense", "tip"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_sumtable_is_bit_exact(ctx, dt, side):
    import torch

    dt = np_dtype(dt)
    for n in SIZES:
        x1, x2, _, codes, tv = make_sides(dt, side, n, seed=n)
        st, buf = gpu_sumtab(ctx, dt, x1, x2, codes, tv, n)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(bits(got[:4 * n]), bits(psr_ref.sumtab(x1, x2).ravel())), n
        assert np.all(got[4 * n:] == -7.0), n


@pytest.mark.parametrize("side", ["dense", "tip"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_derivatives_match_numpy(ctx, dt, side):
    import torch

    dt = np_dtype(dt)
    m = model()
    eig, rates = dev(m["e"]), dev(m["rates"])
    sums = np.array([3, 0, 5], np.int64)
    for n in (0, 1, 63, 64, 65, 257, 4099):
        rng = np.random.default_rng(7 * n)
        x1, x2, cat, codes, tv = make_sides(dt, side, n, seed=1000 + n)
        st = gpu_sumtab(ctx, dt, x1, x2, codes, tv, n)[0] if n else dev(np.zeros(0, dt))
        ref_st = psr_ref.sumtab(x1, x2)
        wgt = rng.integers(0, 4, n).astype(np.int32)
        for t in (1e-8, 0.2, 10.0):
            for full in (False, True):
                kw = dict(wgt=dev(wgt), scaler_sums=dev(sums)) if full else {}
                outs = []
                for _ in range(2):
                    out = torch.full((3,), np.nan, dtype=torch.float64, device="cuda")
                    site = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
                    ctx.edge_derivatives_psr(st, n, eig, rates, dev(cat), dev(np.array([t])), out, site_lnl=site, **kw)
                    torch.cuda.synchronize()
                    outs.append((out.cpu().numpy(), site.cpu().numpy()))
                assert np.array_equal(bits(outs[0][0]), bits(outs[1][0]))
                assert np.array_equal(bits(outs[0][1]), bits(outs[1][1]))
                got, site = outs[0]
                if n == 0:
                    assert got.tolist() == [(8 * LOG_MINLIK if full else 0.0), 0.0, 0.0]
                    continue
                ref, scale, ref_site = psr_ref.edge(ref_st, m["lam"], m["rates"], cat, t, wgt if full else None,
                                                    8 if full else 0)
                check_out(got, ref, scale, f"n={n} t={t} full={full}")
                assert np.all(np.abs(site - ref_site) <= LNL_RTOL * np.maximum(1.0, np.abs(ref_site))), (n, t)


PULLEY_T = 0.5


@pytest.fixture(scope="module")
def pulley(ctx):
    """A four-taxon PSR tree ((t0, t1) A, (t2, t3) B): the CLVs A, B (coded
    tips, eigen convention, f64) and the two paths to the lnL over A - B."""
    import torch

    n, ncat = 1000, NCAT_EDGE
    m = model()
    rng = np.random.default_rng(88)
    cat = rng.integers(0, ncat, n).astype(np.uint8)
    blen = rng.random(4) * 0.25 + 0.05
    P = lambda t: np.stack([(m["V"] * np.exp(m["lam"] * r * t)) @ m["Vi"] for r in m["rates"]])  # noqa: E731

    def evolve(parent, t):
        p = np.clip(P(t)[cat, parent], 0, None)
        p /= p.sum(axis=1, keepdims=True)
        return (rng.random(n)[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, 3)

    a = rng.choice(4, n, p=m["pi"])
    b = evolve(a, PULLEY_T)
    states = [evolve(a, blen[0]), evolve(a, blen[1]), evolve(b, blen[2]), evolve(b, blen[3])]
    codes = [(1 << s).astype(np.uint8) for s in states]
    for c in codes:
        c[rng.random(n) < 0.03] = 15  # a few gaps
    wgt = rng.integers(1, 4, n).astype(np.int32)
    d = dict(n=n, ncat=ncat, m=m, wgt=wgt, cat=cat, eig=dev(m["e"]), rates=dev(m["rates"]), cat_d=dev(cat),
             wgt_d=dev(wgt), EV=dev(plfx.model_ev(m["e"], 4, plfx.PMAT_EIGEN)),
             w=dev(plfx.model_root_weights(m["e"], m["freqs"], plfx.PMAT_EIGEN)), tv=dev(m["tv"].ravel()))
    pm = torch.empty(4 * ncat * 16, dtype=torch.float64, device="cuda")
    ctx.pmatrix(d["eig"], d["rates"], dev(blen), pm, states=4, convention=plfx.PMAT_EIGEN)
    M = ncat * 16
    A, B, root = (torch.empty(4 * n, dtype=torch.float64, device="cuda") for _ in range(3))
    d["sums"] = torch.zeros(2, dtype=torch.int64, device="cuda")
    tips = [dev(c) for c in codes]
    ctx.plf_psr([dict(tip1=tips[0], tip2=tips[1], x3=A, left=pm[:M], right=pm[M:2 * M], scaler_sum=d["sums"][0:1]),
                 dict(tip1=tips[2], tip2=tips[3], x3=B, left=pm[2 * M:3 * M], right=pm[3 * M:], scaler_sum=d["sums"][1:2])],
                d["EV"], n, d["cat_d"], ncat, wgt=d["wgt_d"], tipvec=d["tv"])
    d["A"], d["B"] = A, B
    d["st"] = torch.empty(4 * n, dtype=torch.float64, device="cuda")
    ctx.edge_sumtable_psr(B, d["st"], n, x1=A)
    torch.cuda.synchronize()
    d["ref_st"] = psr_ref.sumtab(A.cpu().numpy(), B.cpu().numpy())

    def node_lnl(t):
        """The PSR node update with P matrices at (0.3 t, 0.7 t), then the root lnL."""
        pr = torch.empty(2 * M, dtype=torch.float64, device="cuda")
        ctx.pmatrix(d["eig"], d["rates"], dev(np.array([0.3 * t, 0.7 * t])), pr, states=4, convention=plfx.PMAT_EIGEN)
        own = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx.plf_psr(dict(x1=A, x2=B, x3=root, left=pr[:M], right=pr[M:], scaler_sum=own), d["EV"], n, d["cat_d"], ncat,
                    wgt=d["wgt_d"])
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        ctx.root_lnl_psr(root, n, out, freq=d["w"], wgt=d["wgt_d"], scaler_sums=torch.cat([d["sums"], own]))
        torch.cuda.synchronize()
        return float(out.item())

    def edge(t):
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        ctx.edge_derivatives_psr(d["st"], n, d["eig"], d["rates"], d["cat_d"], dev(np.array([t])), out, wgt=d["wgt_d"],
                                 scaler_sums=d["sums"])
        torch.cuda.synchronize()
        return out.cpu().numpy()

    d["node_lnl"], d["edge"] = node_lnl, edge
    return d


@pytest.mark.parametrize("t", [0.1, 0.45, 1.5])
def test_pulley_edge_lnl_is_the_node_path(pulley, t):
    got = pulley["edge"](t)
    lnl = pulley["node_lnl"](t)
    print(f"t={t}: edge lnL {got[0]!r} node path {lnl!r} rel {abs(got[0] - lnl) / abs(lnl):.2e}")
    assert abs(got[0] - lnl) <= LNL_RTOL * abs(lnl)


def test_optimize_branch_on_the_pulley(ctx, pulley):
    d = pulley
    m, wgt, cat = d["m"], d["wgt"], d["cat"]
    d1 = lambda t: psr_ref.edge(d["ref_st"], m["lam"], m["rates"], cat, t, wgt)[0][1]  # noqa: E731
    assert d1(1e-8) > 0 > d1(10.0)
    t_ref = brentq(d1, 1e-8, 10.0, xtol=1e-14, rtol=1e-14)
    res = [ctx.optimize_branch_psr(d["st"], d["n"], d["eig"], d["rates"], d["cat_d"], t0, 1e-8, 10.0, 64, wgt=d["wgt_d"])
           for t0 in STARTS]
    for t0, (t, lnl, g1, g2, evals) in zip(STARTS, res):
        print(f"start {t0:g}: t {t!r} (numpy optimum {t_ref!r}) lnL {lnl!r} d1 {g1:.3e} d2 {g2:.3e} evals {evals}")
        assert abs(t - t_ref) <= 1e-6 * t_ref
        assert abs(t - res[0][0]) <= 1e-6 * res[0][0]
        assert 1 <= evals <= 64 and g2 < 0
        ref, scale, _ = psr_ref.edge(d["ref_st"], m["lam"], m["rates"], cat, t, wgt)
        check_out(np.array([lnl, g1, g2]), ref, scale, f"start {t0:g}")


# ---- capture, refusals ----

def test_captured_batch_and_root_lnl_replay_to_the_eager_bits():
    """Three nodes of three kinds and the root lnL of the first, captured on a
    stream whose first use is the capture, replayed with the outputs cleared."""
    import torch

    dt, n, ncat = np.float64, 257, 25
    cases = [node_case(dt, n, ncat, k, seed=100 + k) for k in (0, 1, 3)]
    with plfx.Context(0, lazy_tables=True) as c:
        cat, wgt, EV, tv = (dev(cases[0][k]) for k in ("cat", "wgt", "EV", "tipvec"))
        nodes = []
        for d in cases:
            nd = dict(x3=torch.zeros(4 * n, dtype=torch.float64, device="cuda"), left=dev(d["left"]), right=dev(d["right"]),
                      scaler=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                      scaler_sum=torch.zeros(1, dtype=torch.int64, device="cuda"))
            for k in ("x1", "x2", "tip1", "tip2"):
                if k in d:
                    nd[k] = dev(d[k])
            nodes.append(nd)
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        site = torch.zeros(n, dtype=torch.float64, device="cuda")
        outs = [t for nd in nodes for t in (nd["x3"], nd["scaler"], nd["scaler_sum"])] + [out, site]

        def call(stream):
            c.plf_psr(nodes, EV, n, cat, ncat, wgt=wgt, tipvec=tv, stream=stream)
            # (EV is signed, so a site's sum may be negative and its log NaN: on every run alike)
            c.root_lnl_psr(nodes[0]["x3"], n, out, wgt=wgt, scaler_sums=nodes[0]["scaler_sum"], site_lnl=site,
                           stream=stream)

        call(None)
        torch.cuda.synchronize()
        first = [t.cpu().numpy().copy() for t in outs]
        assert np.array_equal(bits(first[0]), bits(cases[0]["ref"][0]))
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
                assert same(a, f) if a.dtype == np.float64 else np.array_equal(a, f)
        del g
        torch.cuda.synchronize()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_argument_errors_enqueue_nothing_and_leave_the_context_usable():
    import torch

    n, ncat, dt = 65, 4, np.float64
    d = node_case(dt, n, ncat, 0)
    m = model()
    with plfx.Context(0, lazy_tables=True) as c:
        L, h = c._L, c.h
        big = torch.full((4 * n * 3 + 8,), -7.0, dtype=torch.float64, device="cuda")
        a, b, x3 = big[:4 * n], big[4 * n:8 * n], big[8 * n:12 * n]
        a.copy_(dev(d["x1"]))
        b.copy_(dev(d["x2"]))
        codes = dev(np.full(n, 5, np.uint8))
        EV, left, right, cat, tv = (dev(d[k]) for k in ("EV", "left", "right", "cat", "tipvec"))
        eig, rates, t = dev(m["e"]), dev(m["rates"][:ncat]), dev(np.array([0.2]))
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        p = lambda x: None if x is None else x.data_ptr()  # noqa: E731

        def node(tip1=None, x1=a, tip2=None, x2=b, x3_=x3, left_=left, right_=right, n_=n, ncat_=ncat, EV_=EV, cat_=cat,
                 count=1, dtype=plfx.F64):
            nd = plfx.PsrNode(p(tip1), p(x1), p(tip2), p(x2), p(x3_), p(left_), p(right_), None, None)
            return L.plfx_plf_psr_dev(h, dtype, plfx.C.byref(nd), count, p(EV_), n_, p(cat_), ncat_, None, p(tv), None)

        INV = plfx.ERR_INVALID
        assert node(tip1=codes) == INV                   # both a tip and a CLV
        assert node(x1=None) == INV                      # neither
        assert node(tip2=codes) == INV
        assert node(x2=None) == INV
        assert node(x1=x3) == INV                        # the parent over child 1
        assert node(x2=x3) == INV
        assert node(x3_=big[8 * n - 2:]) == INV          # sharing 16 bytes with child 2
        assert node(x1=big[1:]) == INV                   # misaligned
        assert node(x2=big[4 * n + 1:]) == INV
        assert node(x3_=big[8 * n + 1:]) == INV
        assert node(x3_=None) == INV and node(left_=None) == INV and node(right_=None) == INV
        assert node(EV_=None) == INV and node(cat_=None) == INV
        assert node(n_=-1) == INV and node(count=0) == INV and node(dtype=2) == INV
        assert node(ncat_=0) == INV and node(ncat_=33) == INV
        assert b"ncat" in L.plfx_last_error(h)
        torch.cuda.synchronize()
        assert np.all(x3.cpu().numpy() == -7.0)          # nothing ran
        with pytest.raises(plfx.PlfxError) as ei:        # protein: not built
            c.root_lnl_psr(a, n, out, states=20)
        assert ei.value.code == plfx.ERR_UNSUPPORTED
        with pytest.raises(plfx.PlfxError) as ei:
            c.plf_psr(dict(x1=a, x2=b, x3=x3, left=left, right=right), EV, n, cat, ncat, states=20)
        assert ei.value.code == plfx.ERR_UNSUPPORTED

        def sumtable(tip1, x1_, x2_, n_, tipvec, st_):
            return L.plfx_edge_sumtable_psr(h, plfx.F64, p(tip1), p(x1_), p(x2_), n_, p(tipvec), p(st_), None)

        def derivs(st_, n_, ncat_, cat_=cat):
            return L.plfx_edge_derivatives_psr(h, plfx.F64, p(st_), n_, p(eig), p(rates), ncat_, p(cat_), None, p(t),
                                               None, 0, p(out), None, None)

        def optimize(t0, tmin, tmax, ncat_=ncat, stream=None):
            topt = plfx.C.c_double(0.0)
            return L.plfx_edge_optimize_psr(h, plfx.F64, p(x3), n, p(eig), p(rates), ncat_, p(cat), None, t0, tmin, tmax,
                                            64, plfx.C.byref(topt), None, None, stream)

        assert sumtable(codes, a, b, n, tv, x3) == INV
        assert sumtable(None, None, b, n, tv, x3) == INV
        assert sumtable(codes, None, b, n, None, x3) == INV   # a coded side without tipvec
        assert sumtable(None, big[1:], b, n, None, x3) == INV
        assert sumtable(None, a, b, -1, None, x3) == INV
        assert sumtable(None, a, b, n, None, a) == INV
        assert sumtable(None, a, b, n, None, big[8 * n - 2:]) == INV
        assert derivs(x3, n, 0) == INV and derivs(x3, n, 33) == INV
        assert derivs(big[8 * n + 1:], n, ncat) == INV
        assert derivs(x3, -1, ncat) == INV and derivs(x3, n, ncat, cat_=None) == INV
        assert optimize(0.5, 1e-8, 10.0, ncat_=0) == INV
        assert optimize(1e-9, 1e-8, 10.0) == INV and optimize(11.0, 1e-8, 10.0) == INV
        assert optimize(0.5, 0.0, 10.0) == INV and optimize(0.5, 1.0, 0.1) == INV
        assert L.plfx_root_lnl_psr(h, plfx.F64, p(a), n, None, None, None, 0, None, None, None) == INV  # no out
        assert L.plfx_root_lnl_psr(h, plfx.F64, p(big[1:]), n, None, None, None, 0, p(out), None, None) == INV
        cap = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cap):
            rc = optimize(0.5, 1e-8, 10.0, stream=cap.cuda_stream)
        assert rc == INV and b"captur" in L.plfx_last_error(h)
        del g
        torch.cuda.synchronize()
        assert np.all(x3.cpu().numpy() == -7.0)
        # and the context still works
        assert node() == plfx.OK
        torch.cuda.synchronize()
        assert np.array_equal(bits(x3.cpu().numpy()), bits(d["ref"][0]))
