"""GPU tests of plfx.h section 11c, the branch-length half of protein per-site
rate categories: the sum table (plfx_edge_sumtable_psr_gen, one and batched),
the three edge sums (plfx_edge_derivatives_psr_gen) and the two Newton loops
(plfx_edge_optimize_psr_gen on the host, plfx_edge_optimize_psr_dev_gen on the
device), with states = 20 -- and with states = 4, where they must be section
11's calls bit for bit.

The reference is tests/psr_prot_edge_ref.py, which tests/test_psr_prot_edge_ref.py
pins to the state-space reference on the CPU.  Sum tables are compared bit for
bit; the three sums at the project's f64 bar (LNL_RTOL of the scales, as
tests/test_gpu_edge.py), per-site log L at LNL_RTOL * max(1, |log L|).  The
device loop's yardstick is the host loop: the same stepper on sums formed in
the derivative kernel's grid and order, so a one-edge call is equal BIT FOR
BIT.

Inputs follow tests/test_gpu_edge.py's make_sides for S = 20 with one category
per site: dense sides are eigen coordinates of rng.random(...) * 0.5 + 0.05, a
coded side has protein codes that include 20, 22, 24 and 255, some rate_cat
bytes are >= ncat, wgt is in 0..3.  For this recipe (n up to 4099, f32 and f64
tables, rates in 1e-3..8, t in 1e-8..10) every site likelihood is positive,
and the f64 numpy reference agrees with the same formula in long double to
8e-16 of the scales: LNL_RTOL = 1e-10 has five orders of margin over the
reference's own error."""
import functools

import numpy as np
import pytest
from scipy.optimize import brentq

import plfx
import psr_prot_edge_ref as E
import psr_prot_ref as R
import psr_ref
from test_gpu_edge import model as gamma_model
from test_gpu_edge import tip_table
from test_gpu_psr import STARTS, bits, check_out, dev, np_dtype, tdtype
from test_gpu_psr import make_sides as dna_sides
from test_gpu_psr import model as dna_model

pytestmark = pytest.mark.gpu

S = 20
LNL_RTOL = 1e-10
LOG_MINLIK = R.LOG_MINLIK
GUARD = 64
NCAT = 25
TMIN, TMAX, MAX_EVALS = 1e-8, 10.0, 64


def model():
    return gamma_model(S)


def cat_rates(ncat):
    return np.ones(1) if ncat == 1 else np.geomspace(1e-3, 8.0, ncat)


def make_sides(dt, side, n, seed, ncat=NCAT):
    """x1, x2 as (n, 20) arrays of dt -- eigen coordinates of positive
    state-space vectors --, the category bytes (a few past ncat: clamped), and
    for a coded side 1 its codes and table (x1 is then the table's expansion)."""
    import oracle

    m = model()
    rng = np.random.default_rng(seed)
    eig = lambda y: np.einsum("ks,ns->nk", m["Vi"], y).astype(dt)  # noqa: E731
    x2 = eig(rng.random((n, S)) * 0.5 + 0.05)
    cat = rng.integers(0, ncat + 3, n).astype(np.uint8)
    if side == "dense":
        return eig(rng.random((n, S)) * 0.5 + 0.05), x2, cat, None, None
    tv = tip_table(S).astype(dt)
    codes = oracle.random_protein_codes(rng, n, 0.3)
    if n >= 4:
        codes[:4] = [20, 22, 24, 255]  # B, X, and two codes >= 24 (row 23)
    return R.expand_tips(codes, dt, tv).reshape(n, S), x2, cat, codes, tv


def gpu_sumtab(c, dt, x1, x2, codes, tv, n, stream=None):
    """The device sum table (a view of a guarded buffer) and the buffer."""
    import torch

    buf = torch.full((S * n + GUARD,), -7.0, dtype=tdtype(dt), device="cuda")
    st = buf[:S * n]
    # n == 0: an empty tensor's pointer is NULL, and side 1 must still name exactly one of tip / CLV
    side1 = lambda a: dev(a.ravel() if a.size else np.ones(S, a.dtype))  # noqa: E731
    if codes is None:
        c.edge_sumtable_psr_gen(S, dev(x2.ravel()), st, n, x1=side1(x1), stream=stream)
    else:
        c.edge_sumtable_psr_gen(S, dev(x2.ravel()), st, n, tip1=side1(codes), tipvec=dev(tv.ravel()), stream=stream)
    return st, buf


def dev_table(tab, dt):
    """The table on the device; n == 0: unused values, so that the pointer is not NULL."""
    return dev(tab.astype(dt).ravel() if tab.size else np.ones(S, dt))


# ---- 1: the sum table ----

@pytest.mark.parametrize("side", ["dense", "tip"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_sumtable_is_bit_exact(ctx, dt, side):
    import torch

    dt = np_dtype(dt)
    for n in (0, 1, 63, 64, 65, 257, 4099):
        x1, x2, _, codes, tv = make_sides(dt, side, n, seed=n)
        if side == "tip" and n >= 4:
            assert {20, 22, 24, 255} <= set(codes.tolist())
        st, buf = gpu_sumtab(ctx, dt, x1, x2, codes, tv, n)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(bits(got[:S * n]), bits(E.sumtab(x1, x2).ravel())), n
        assert np.all(got[S * n:] == -7.0), n  # nothing written past the table


# ---- 2: batched sum tables ----

def sumtab_edges(dt, n):
    """35 edges, dense and coded side 1 mixed, over a pool of shared inputs:
    [(x1 or None, codes or None, x2)] as numpy arrays, and the coded sides' table."""
    dense = [make_sides(dt, "dense", n, seed=10 * n + k) for k in range(4)]
    tips = [make_sides(dt, "tip", n, seed=10 * n + 5 + k) for k in range(3)]
    pool = [d[0] for d in dense] + [d[1] for d in dense] + [t[1] for t in tips]  # 11 dense CLVs
    edges = []
    for j in range(35):
        x2 = pool[(3 * j + 1) % len(pool)]
        if j % 3 == 1:
            edges.append((None, tips[(j // 3) % 3][3], x2))
        else:
            edges.append((pool[(5 * j) % len(pool)], None, x2))
    return edges, tips[0][4]


@pytest.mark.parametrize("n", [1, 63, 257, 4099])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batched_sumtable_is_bit_exact(ctx, dt, n):
    import torch

    dt = np_dtype(dt)
    edges, tv = sumtab_edges(dt, n)
    assert 10 <= sum(1 for e in edges if e[1] is not None) <= 14
    cache = {}

    def on_dev(a):  # one device tensor per input: shared inputs are shared buffers
        if id(a) not in cache:
            cache[id(a)] = dev(a.ravel())
        return cache[id(a)]

    tvd = dev(tv.ravel())
    stride = S * n + GUARD
    buf = torch.full((35 * stride,), -7.0, dtype=tdtype(dt), device="cuda")
    single = torch.full((35 * stride,), -7.0, dtype=tdtype(dt), device="cuda")
    descs = []
    for j, (x1, codes, x2) in enumerate(edges):
        d = dict(x2=on_dev(x2), sumtab=buf[j * stride:j * stride + S * n])
        d.update(dict(x1=on_dev(x1)) if codes is None else dict(tip1=on_dev(codes)))
        descs.append(d)
        ctx.edge_sumtable_psr_gen(S, d["x2"], single[j * stride:j * stride + S * n], n, x1=d.get("x1"),
                                  tip1=d.get("tip1"), tipvec=tvd)
    ctx.edge_sumtables_psr_gen(S, descs, n, tipvec=tvd)
    torch.cuda.synchronize()
    got, one = buf.cpu().numpy().reshape(35, stride), single.cpu().numpy().reshape(35, stride)
    for j, (x1, codes, x2) in enumerate(edges):
        a = x1 if codes is None else R.expand_tips(codes, dt, tv).reshape(n, S)
        assert np.array_equal(bits(got[j, :S * n]), bits(E.sumtab(a, x2).ravel())), j
    assert np.array_equal(bits(got), bits(one))  # the single calls' tables, and every guard element still -7


# ---- 3: the derivatives ----

def run_deriv(c, st, n, eig, rates, cat, t, site=True, **kw):
    import torch

    out = torch.full((3,), np.nan, dtype=torch.float64, device="cuda")
    sl = torch.full((n,), np.nan, dtype=torch.float64, device="cuda") if site else None
    c.edge_derivatives_psr_gen(S, st, n, eig, rates, cat, dev(np.array([t])), out, site_lnl=sl, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), sl.cpu().numpy() if site else None


@pytest.mark.parametrize("side", ["dense", "tip"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_derivatives_match_numpy(ctx, dt, side):
    dt = np_dtype(dt)
    m = model()
    eig = dev(m["e"])
    sums = np.array([3, 0, 5], np.int64)
    for n in (0, 1, 63, 64, 65, 257, 4099):
        for ncat in (1, 4, 25, 32):
            rates = cat_rates(ncat)
            rng = np.random.default_rng(7 * n + ncat)
            x1, x2, cat, codes, tv = make_sides(dt, side, n, seed=1000 + n + ncat, ncat=ncat)
            if n > 1:
                assert np.any(cat >= ncat)  # the clamp is exercised
            ref_st = E.sumtab(x1, x2)
            # the table under test is the numpy one (test 1 has the kernel's): one upload per shape
            st = dev_table(ref_st, dt)
            wgt = rng.integers(0, 4, n).astype(np.int32)
            catd, ratesd, wgtd, sumsd = dev(cat), dev(rates), dev(wgt), dev(sums)
            for t in (1e-8, 0.2, 10.0):
                for full in (False, True):
                    kw = dict(wgt=wgtd, scaler_sums=sumsd) if full else {}
                    outs = [run_deriv(ctx, st, n, eig, ratesd, catd, t, **kw) for _ in range(2)]
                    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0]))
                    assert np.array_equal(bits(outs[0][1]), bits(outs[1][1]))
                    got, site = outs[0]
                    if n == 0:
                        assert got.tolist() == [(8 * LOG_MINLIK if full else 0.0), 0.0, 0.0]
                        continue
                    ref, scale, ref_site = E.edge(ref_st, m["lam"], rates, cat, t, wgt if full else None,
                                                  8 if full else 0)
                    assert np.all(np.isfinite(ref_site))  # every site likelihood is positive
                    check_out(got, ref, scale, f"n={n} ncat={ncat} t={t} full={full}")
                    assert np.all(np.abs(site - ref_site) <= LNL_RTOL * np.maximum(1.0, np.abs(ref_site))), (n, ncat, t)


# ---- 4: the site order ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_site_order_does_not_change_a_site(ctx, dt):
    dt = np_dtype(dt)
    m = model()
    n = 4099
    x1, x2, cat, _, _ = make_sides(dt, "dense", n, seed=44)
    tab = E.sumtab(x1, x2)
    wgt = np.random.default_rng(4).integers(0, 4, n).astype(np.int32)
    perm = plfx.psr_site_order(cat, NCAT)
    assert not np.array_equal(perm, np.arange(n))
    eig, rates = dev(m["e"]), dev(cat_rates(NCAT))
    for t in (1e-8, 0.2, 10.0):
        a3, a = run_deriv(ctx, dev_table(tab, dt), n, eig, rates, dev(cat), t, wgt=dev(wgt))
        b3, b = run_deriv(ctx, dev_table(tab[perm], dt), n, eig, rates, dev(cat[perm]), t, wgt=dev(wgt[perm]))
        assert np.array_equal(bits(a[perm]), bits(b)), t
        ref, scale, _ = E.edge(tab, m["lam"], cat_rates(NCAT), cat, t, wgt)
        check_out(b3, ref, scale, f"sorted sites, t={t}")  # the totals: another order of the same terms


# ---- 5: against the Gamma protein edge kernel, which predates this ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_one_category_is_the_gamma_kernel_with_four_equal_rates(ctx, dt):
    import torch

    dt = np_dtype(dt)
    m = model()
    n = 257
    rates = cat_rates(NCAT)
    x1, x2, _, _, _ = make_sides(dt, "dense", n, seed=55)
    tab = E.sumtab(x1, x2)
    wgt = np.random.default_rng(5).integers(0, 4, n).astype(np.int32)
    st, st4 = dev_table(tab, dt), dev(np.repeat(tab[:, None, :], 4, axis=1).ravel())
    eig, wgtd = dev(m["e"]), dev(wgt)
    for c in (0, 12, 24, 30):  # 30: clamped to 24
        r = rates[min(c, NCAT - 1)]
        cat = dev(np.full(n, c, np.uint8))
        for t in (1e-8, 0.2, 10.0):
            got, site = run_deriv(ctx, st, n, eig, dev(rates), cat, t, wgt=wgtd)
            out = torch.full((3,), np.nan, dtype=torch.float64, device="cuda")
            gsite = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
            ctx.edge_derivatives(st4, n, eig, dev(np.full(4, r)), dev(np.array([t])), out, wgt=wgtd, site_lnl=gsite,
                                 states=S)
            torch.cuda.synchronize()
            _, scale, _ = E.edge(tab, m["lam"], rates, np.full(n, c, np.uint8), t, wgt)
            check_out(got, out.cpu().numpy(), scale, f"category {c} t={t}")
            gs = gsite.cpu().numpy()
            assert np.all(np.abs(site - gs) <= LNL_RTOL * np.maximum(1.0, np.abs(gs))), (c, t)


# ---- the device loop's helpers ----

def shared(n, seed=1, ncat=NCAT):
    """What the edges of a call share: the model, the category rates, the
    categories (a few clamped) and the weights, on the host and on the device."""
    m = model()
    rates = cat_rates(ncat) if ncat != NCAT else np.geomspace(0.05, 4.0, NCAT)
    rng = np.random.default_rng(seed)
    cat = rng.integers(0, ncat + 3, n).astype(np.uint8)
    wgt = rng.integers(1, 4, n).astype(np.int32)
    return dict(n=n, ncat=ncat, m=m, rates_np=rates, cat_np=cat, wgt_np=wgt, eig=dev(m["e"]), rates=dev(rates),
                cat=dev(cat), wgt=dev(wgt))


@functools.lru_cache(maxsize=None)
def transition(tstar):
    m = model()
    return np.stack([(m["V"] * np.exp(m["lam"] * r * tstar)) @ m["Vi"] for r in np.geomspace(0.05, 4.0, NCAT)])


def pair_table(P, tstar, seed, identical=False):
    """The (n, 20) f64 sum table of two simulated taxa at distance tstar (ncat = NCAT)."""
    m, n = P["m"], P["n"]
    rng = np.random.default_rng(seed)
    sa = rng.choice(S, n, p=m["pi"])
    sb = sa.copy()
    if not identical:
        # (ncat != NCAT: the pair is still simulated at NCAT rates -- any table will do there)
        p = np.clip(transition(tstar)[R.clamp(P["cat_np"], min(P["ncat"], NCAT)), sa], 0, None)
        p /= p.sum(axis=1, keepdims=True)
        sb = (rng.random(n)[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, S - 1)
    return m["Vi"][:, sa].T * m["Vi"][:, sb].T


def ref_d1(P, tab):
    return lambda t: E.edge(tab, P["m"]["lam"], P["rates_np"], P["cat_np"], t, P["wgt_np"])[0][1]


def run_dev(c, P, tables, t0, max_evals=MAX_EVALS, tmin=TMIN, tmax=TMAX, stream=None, sync=True, states=S):
    """optimize_branches_psr_gen over `tables` from the starts t0 (array or
    device tensor): (t_opt, out3 (m, 3), evals) as numpy arrays, or the device tensors."""
    import torch

    m = len(tables)
    t0 = t0 if isinstance(t0, torch.Tensor) else dev(np.asarray(t0, np.float64))
    t_opt = torch.full((m,), np.nan, dtype=torch.float64, device="cuda")
    out3 = torch.full((3 * m,), np.nan, dtype=torch.float64, device="cuda")
    evals = torch.full((m,), -1, dtype=torch.int32, device="cuda")
    c.optimize_branches_psr_gen(states, tables, P["n"], P["eig"], P["rates"], P["cat"], t0, t_opt, tmin, tmax, max_evals,
                                out3=out3, evals=evals, wgt=P["wgt"], stream=stream)
    if not sync:
        return t_opt, out3, evals
    torch.cuda.synchronize()
    return t_opt.cpu().numpy(), out3.cpu().numpy().reshape(m, 3), evals.cpu().numpy()


def run_host(c, P, table, t0, max_evals=MAX_EVALS, tmin=TMIN, tmax=TMAX, states=S):
    t, lnl, d1, d2, ev = c.optimize_branch_psr_gen(states, table, P["n"], P["eig"], P["rates"], P["cat"], t0, tmin, tmax,
                                                   max_evals, wgt=P["wgt"])
    return np.array([t]), np.array([[lnl, d1, d2]]), np.array([ev], np.int32)


def assert_same(got, want, what):
    """(t_opt, out3, evals) equal bit for bit."""
    for name, g, w in zip(("t_opt", "out3", "evals"), got, want):
        if name == "evals":
            assert np.array_equal(g, w), (what, name, g, w)
        else:
            assert np.array_equal(bits(g), bits(w)), (what, name, g.tolist(), w.tolist())


# ---- 6: states 4 through the _gen calls is section 11 ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_four_states_are_section_11_bit_for_bit(ctx, dt):
    import torch

    dt = np_dtype(dt)
    m = dna_model()
    n = 2500
    eig, rates = dev(m["e"]), dev(m["rates"])
    wgt = dev(np.random.default_rng(6).integers(1, 4, n).astype(np.int32))
    for side in ("dense", "tip"):
        x1, x2, cat, codes, tv = dna_sides(dt, side, n, seed=66)
        a, b = (torch.full((4 * n + GUARD,), -7.0, dtype=tdtype(dt), device="cuda") for _ in range(2))
        kw = dict(x1=dev(x1.ravel())) if codes is None else dict(tip1=dev(codes), tipvec=dev(tv.ravel()))
        ctx.edge_sumtable_psr(dev(x2.ravel()), a[:4 * n], n, **kw)
        ctx.edge_sumtable_psr_gen(4, dev(x2.ravel()), b[:4 * n], n, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())), side
        assert np.array_equal(bits(a.cpu().numpy()[:4 * n]), bits(psr_ref.sumtab(x1, x2).ravel())), side
        c = torch.full((4 * n,), -7.0, dtype=tdtype(dt), device="cuda")
        ctx.edge_sumtables_psr_gen(4, [dict(x2=dev(x2.ravel()), sumtab=c, **{k: v for k, v in kw.items() if k != "tipvec"})],
                                   n, tipvec=kw.get("tipvec"))
        torch.cuda.synchronize()
        assert np.array_equal(bits(c.cpu().numpy()), bits(a.cpu().numpy()[:4 * n])), side
        st, catd = a[:4 * n], dev(cat)
        P = dict(n=n, eig=eig, rates=rates, cat=catd, wgt=wgt)
        for t in (1e-8, 0.2, 10.0):
            o4, og = (torch.full((3,), np.nan, dtype=torch.float64, device="cuda") for _ in range(2))
            ctx.edge_derivatives_psr(st, n, eig, rates, catd, dev(np.array([t])), o4, wgt=wgt)
            ctx.edge_derivatives_psr_gen(4, st, n, eig, rates, catd, dev(np.array([t])), og, wgt=wgt)
            torch.cuda.synchronize()
            assert np.array_equal(bits(o4.cpu().numpy()), bits(og.cpu().numpy())), (side, t)
        for t0 in (0.01, 3.0):
            t, lnl, d1, d2, ev = ctx.optimize_branch_psr(st, n, eig, rates, catd, t0, TMIN, TMAX, MAX_EVALS, wgt=wgt)
            want = (np.array([t]), np.array([[lnl, d1, d2]]), np.array([ev], np.int32))
            assert_same(run_host(ctx, P, st, t0, states=4), want, (side, t0, "host"))
            assert_same(run_dev(ctx, P, [st], [t0], states=4), want, (side, t0, "device"))


# ---- 7: the pulley ----

PULLEY_T = 0.5


@pytest.fixture(scope="module")
def pulley(ctx):
    """A four-taxon protein PSR tree ((t0, t1) A, (t2, t3) B): the CLVs A, B
    (coded tips, eigen convention, f64, from plf_psr_gen) and the two paths to
    the lnL over A - B."""
    import torch

    n, ncat = 1000, NCAT
    m = model()
    rates_np = np.geomspace(0.05, 4.0, ncat)
    rng = np.random.default_rng(88)
    cat = rng.integers(0, ncat, n).astype(np.uint8)
    blen = rng.random(4) * 0.25 + 0.05
    P = lambda t: np.stack([(m["V"] * np.exp(m["lam"] * r * t)) @ m["Vi"] for r in rates_np])  # noqa: E731

    def evolve(parent, t):
        p = np.clip(P(t)[cat, parent], 0, None)
        p /= p.sum(axis=1, keepdims=True)
        return (rng.random(n)[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, S - 1)

    a = rng.choice(S, n, p=m["pi"])
    b = evolve(a, PULLEY_T)
    codes = [evolve(a, blen[0]).astype(np.uint8), evolve(a, blen[1]).astype(np.uint8),
             evolve(b, blen[2]).astype(np.uint8), evolve(b, blen[3]).astype(np.uint8)]
    for c in codes:
        c[rng.random(n) < 0.03] = 23  # a few gaps
    wgt = rng.integers(1, 4, n).astype(np.int32)
    d = dict(n=n, ncat=ncat, m=m, wgt=wgt, cat=cat, rates_np=rates_np, eig=dev(m["e"]), rates=dev(rates_np),
             cat_d=dev(cat), wgt_d=dev(wgt), EV=dev(plfx.model_ev(m["e"], S, plfx.PMAT_EIGEN)),
             w=dev(plfx.model_root_weights(m["e"], m["freqs"], plfx.PMAT_EIGEN)), tv=dev(tip_table(S).ravel()))
    M = ncat * S * S
    pm = torch.empty(4 * M, dtype=torch.float64, device="cuda")
    ctx.pmatrix(d["eig"], d["rates"], dev(blen), pm, states=S, convention=plfx.PMAT_EIGEN)
    A, B, root = (torch.empty(S * n, dtype=torch.float64, device="cuda") for _ in range(3))
    d["sums"] = torch.zeros(2, dtype=torch.int64, device="cuda")
    tips = [dev(c) for c in codes]
    ctx.plf_psr_gen(S, [dict(tip1=tips[0], tip2=tips[1], x3=A, left=pm[:M], right=pm[M:2 * M],
                             scaler_sum=d["sums"][0:1]),
                        dict(tip1=tips[2], tip2=tips[3], x3=B, left=pm[2 * M:3 * M], right=pm[3 * M:],
                             scaler_sum=d["sums"][1:2])],
                    d["EV"], n, d["cat_d"], ncat, wgt=d["wgt_d"], tipvec=d["tv"])
    d["A"], d["B"] = A, B
    d["st"] = torch.empty(S * n, dtype=torch.float64, device="cuda")
    ctx.edge_sumtable_psr_gen(S, B, d["st"], n, x1=A)
    torch.cuda.synchronize()
    d["ref_st"] = E.sumtab(A.cpu().numpy(), B.cpu().numpy())
    assert np.array_equal(bits(d["st"].cpu().numpy()), bits(d["ref_st"]))

    def node_lnl(t):
        """The node update with P matrices at (0.3 t, 0.7 t), then the root lnL."""
        pr = torch.empty(2 * M, dtype=torch.float64, device="cuda")
        ctx.pmatrix(d["eig"], d["rates"], dev(np.array([0.3 * t, 0.7 * t])), pr, states=S, convention=plfx.PMAT_EIGEN)
        own = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx.plf_psr_gen(S, dict(x1=A, x2=B, x3=root, left=pr[:M], right=pr[M:], scaler_sum=own), d["EV"], n, d["cat_d"],
                        ncat, wgt=d["wgt_d"])
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        ctx.root_lnl_psr_gen(S, root, n, out, freq=d["w"], wgt=d["wgt_d"], scaler_sums=torch.cat([d["sums"], own]))
        torch.cuda.synchronize()
        return float(out.item())

    def edge(t):
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        ctx.edge_derivatives_psr_gen(S, d["st"], n, d["eig"], d["rates"], d["cat_d"], dev(np.array([t])), out,
                                     wgt=d["wgt_d"], scaler_sums=d["sums"])
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
    m, wgt, cat, rates = d["m"], d["wgt"], d["cat"], d["rates_np"]
    d1 = lambda t: E.edge(d["ref_st"], m["lam"], rates, cat, t, wgt)[0][1]  # noqa: E731
    assert d1(1e-8) > 0 > d1(10.0)
    t_ref = brentq(d1, 1e-8, 10.0, xtol=1e-14, rtol=1e-14)
    res = [ctx.optimize_branch_psr_gen(S, d["st"], d["n"], d["eig"], d["rates"], d["cat_d"], t0, 1e-8, 10.0, 64,
                                       wgt=d["wgt_d"]) for t0 in STARTS]
    for t0, (t, lnl, g1, g2, evals) in zip(STARTS, res):
        print(f"start {t0:g}: t {t!r} (numpy optimum {t_ref!r}) lnL {lnl!r} d1 {g1:.3e} d2 {g2:.3e} evals {evals}")
        assert abs(t - t_ref) <= 1e-6 * t_ref
        assert 1 <= evals <= 64 and g2 < 0
        ref, scale, _ = E.edge(d["ref_st"], m["lam"], rates, cat, t, wgt)
        check_out(np.array([lnl, g1, g2]), ref, scale, f"start {t0:g}")


# ---- 8: the device loop ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_one_edge_equals_the_host_path_bit_for_bit(ctx, dt):
    """n = 65 (one block) and 2500 (ten); at 257 also ncat 1 and 32; n = 0
    walks the host loop's sequence on the sums {0, 0, 0}.  (f32: a table of
    two one-hot ends may cancel to L <= 0 at some sites, so only the bits are
    compared there.)"""
    for n, ncat in ((0, NCAT), (65, NCAT), (2500, NCAT), (257, 1), (257, 32)):
        P = shared(n, seed=3 * n + ncat, ncat=ncat)
        for identical in (False, True):
            tab = pair_table(P, 0.25, seed=7000 + n + ncat, identical=identical)
            st = dev_table(tab, np_dtype(dt))
            for t0 in STARTS:
                got = run_dev(ctx, P, [st], [t0])
                want = run_host(ctx, P, st, t0)
                print(f"{dt} n={n} ncat={ncat} identical={identical} start {t0:g}: t {got[0][0]!r} host {want[0][0]!r} "
                      f"evals {got[2][0]} host {want[2][0]}")
                assert_same(got, want, (n, ncat, identical, t0))


@pytest.mark.parametrize("n", [65, 2500])
def test_batches_equal_singles(ctx, n):
    """5 edges against five one-edge calls, and 35 edges (two launch groups)
    against the same; the optima against brentq on numpy's d1."""
    P = shared(n, seed=2 + n)
    tstars = (0.05, 0.25, 1.5, 5.0)
    tabs_np = [pair_table(P, tstars[j % 4], seed=400 + j, identical=j % 8 == 5) for j in range(35)]
    tables = [dev_table(t, np.float64) for t in tabs_np]
    tables[20] = tables[3]  # one table twice, from different starts
    tabs_np[20] = tabs_np[3]
    t0 = np.geomspace(2e-3, 8.0, 35)
    singles = [run_dev(ctx, P, [tables[j]], [t0[j]]) for j in range(35)]
    five = run_dev(ctx, P, tables[:5], t0[:5])
    all35 = run_dev(ctx, P, tables, t0)
    for j in range(35):
        if j < 5:
            assert_same(tuple(g[j:j + 1] for g in five), singles[j], ("batch of 5", j))
        assert_same(tuple(g[j:j + 1] for g in all35), singles[j], ("batch of 35", j))
    interior = 0
    for j in range(35 if n == 2500 else 0):
        d1 = ref_d1(P, tabs_np[j])
        if d1(TMIN) > 0 > d1(TMAX):
            t_ref = brentq(d1, TMIN, TMAX, xtol=1e-14, rtol=1e-14)
            print(f"edge {j}: t {all35[0][j]!r} brentq {t_ref!r} rel {abs(all35[0][j] - t_ref) / t_ref:.2e} "
                  f"evals {all35[2][j]}")
            assert abs(all35[0][j] - t_ref) <= 1e-6 * t_ref
            interior += 1
    assert n != 2500 or interior >= 20  # most simulated pairs have their optimum inside the interval


@pytest.mark.parametrize("n", [65, 2500])
def test_evaluation_caps(ctx, n):
    P = shared(n, seed=n)
    st = dev_table(pair_table(P, 1.5, seed=n + 1), np.float64)
    got = run_dev(ctx, P, [st], [3.0], max_evals=3)
    assert got[2][0] == 3
    assert_same(got, run_host(ctx, P, st, 3.0, max_evals=3), "cap 3")
    got = run_dev(ctx, P, [st], [3.0], max_evals=1)
    out, _ = run_deriv(ctx, st, n, P["eig"], P["rates"], P["cat"], 3.0, site=False, wgt=P["wgt"])
    assert got[0][0] == 3.0 and got[2][0] == 1
    assert np.array_equal(bits(got[1][0]), bits(out))


@pytest.mark.parametrize("n", [65, 2500])
def test_device_t0_is_clamped_and_chains(ctx, n):
    import torch

    P = shared(n, seed=n)
    st = dev_table(pair_table(P, 0.25, seed=n + 2), np.float64)
    lo, hi = run_dev(ctx, P, [st] * 2, [1e-12, 50.0]), run_dev(ctx, P, [st] * 2, [TMIN, TMAX])
    assert_same(lo, hi, "clamped starts")
    assert_same(tuple(g[0:1] for g in lo), run_host(ctx, P, st, TMIN), "start below tmin")
    assert_same(tuple(g[1:2] for g in lo), run_host(ctx, P, st, TMAX), "start above tmax")
    assert_same(run_dev(ctx, P, [st], [np.nan]), run_host(ctx, P, st, TMIN), "a NaN start")
    # call 1 stops at its cap; call 2 starts where it stopped, with no host in between
    first = run_dev(ctx, P, [st], [3.0], max_evals=3, sync=False)
    second = run_dev(ctx, P, [st], first[0], sync=False)
    torch.cuda.synchronize()
    t1 = float(first[0].cpu().numpy()[0])
    assert t1 != 3.0
    got = (second[0].cpu().numpy(), second[1].cpu().numpy().reshape(1, 3), second[2].cpu().numpy())
    assert_same(got, run_host(ctx, P, st, t1), "chained")


# ---- 9: one block ----

def test_one_block_walks_every_site(monkeypatch):
    """PLFX_MAX_BLOCKS=1: one block per edge makes all ten trips over 2500
    sites and is its own last block."""
    monkeypatch.setenv("PLFX_MAX_BLOCKS", "1")
    n = 2500
    with plfx.Context(0, lazy_tables=True) as c:
        P = shared(n, seed=5)
        tab = pair_table(P, 0.25, seed=55)
        x1, x2, cat, _, _ = make_sides(np.float64, "dense", n, seed=56)
        pos = E.sumtab(x1, x2)  # a table with every site likelihood positive, for the values
        for dt in (np.float64, np.float32):
            for t in (1e-8, 0.2, 10.0):
                got, site = run_deriv(c, dev_table(pos, dt), n, P["eig"], P["rates"], dev(cat), t, wgt=P["wgt"])
                ref, scale, ref_site = E.edge(pos.astype(dt), P["m"]["lam"], P["rates_np"], cat, t, P["wgt_np"])
                check_out(got, ref, scale, f"one block {np.dtype(dt).name} t={t}")
                assert np.all(np.abs(site - ref_site) <= LNL_RTOL * np.maximum(1.0, np.abs(ref_site)))
            st = dev_table(tab, dt)
            for t0 in (0.01, 3.0):
                assert_same(run_dev(c, P, [st], [t0]), run_host(c, P, st, t0), (dt, t0))


# ---- 10: capture ----

def test_captured_chain_replays_to_the_eager_bits():
    """Batched sum tables (one dense, one coded edge) + optimize_branches_psr_gen
    captured on a stream whose first use is the capture; replayed with cleared
    outputs; the workspace is at rest afterwards."""
    import torch

    n, dt = 257, np.float64
    with plfx.Context(0, lazy_tables=True) as c:
        P = shared(n, seed=9)
        m = P["m"]
        x1, x2, _, _, _ = make_sides(dt, "dense", n, seed=91)
        _, y2, _, codes, tv = make_sides(dt, "tip", n, seed=92)
        xa, xb, yb, cd, tvd = dev(x1.ravel()), dev(x2.ravel()), dev(y2.ravel()), dev(codes), dev(tv.ravel())
        st = [torch.zeros(S * n, dtype=torch.float64, device="cuda") for _ in range(2)]
        t0 = dev(np.array([0.1, 3.0]))
        t_opt = torch.zeros(2, dtype=torch.float64, device="cuda")
        out3 = torch.zeros(6, dtype=torch.float64, device="cuda")
        evals = torch.zeros(2, dtype=torch.int32, device="cuda")
        outs = (st[0], st[1], t_opt, out3, evals)

        def call(stream):
            c.edge_sumtables_psr_gen(S, [dict(tip1=cd, x2=yb, sumtab=st[1]), dict(x1=xa, x2=xb, sumtab=st[0])], n,
                                     tipvec=tvd, stream=stream)
            c.optimize_branches_psr_gen(S, st, n, P["eig"], P["rates"], P["cat"], t0, t_opt, TMIN, TMAX, MAX_EVALS,
                                        out3=out3, evals=evals, wgt=P["wgt"], stream=stream)

        def eager(starts):
            t0.copy_(dev(np.array(starts)))
            call(None)
            torch.cuda.synchronize()
            return [t.cpu().numpy().copy() for t in outs]

        want = {s: eager(s) for s in ((0.1, 3.0), (5.0, 1e-3))}
        w = want[(0.1, 3.0)]
        ref_st = [E.sumtab(x1, x2), E.sumtab(R.expand_tips(codes, dt, tv).reshape(n, S), y2)]
        for j in (0, 1):  # the eager tables are numpy's and the eager optimum is the host path's
            assert np.array_equal(bits(w[j]), bits(ref_st[j].ravel()))
            ref = run_host(c, P, st[j], (0.1, 3.0)[j])
            assert_same((w[2][j:j + 1], w[3].reshape(2, 3)[j:j + 1], w[4][j:j + 1]), ref, ("eager", j))
        cold = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        t0.copy_(dev(np.array([0.1, 3.0])))
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=cold):
            call(cold)
        for starts in ((0.1, 3.0), (0.1, 3.0), (5.0, 1e-3)):
            t0.copy_(dev(np.array(starts)))
            for t in outs:
                t.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for t, f in zip(outs, want[starts]):
                got = t.cpu().numpy()
                assert np.array_equal(got, f) if got.dtype == np.int32 else np.array_equal(bits(got), bits(f)), starts
        # the workspace is at rest: another sum-producing call on that stream is correct
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        with torch.cuda.stream(cold):
            c.edge_derivatives_psr_gen(S, st[0], n, P["eig"], P["rates"], P["cat"], dev(np.array([0.3])), out,
                                       wgt=P["wgt"], stream=cold)
        torch.cuda.synchronize()
        ref, scale, _ = E.edge(ref_st[0], m["lam"], P["rates_np"], P["cat_np"], 0.3, P["wgt_np"])
        check_out(out.cpu().numpy(), ref, scale, "after the replays")
        del g
        torch.cuda.synchronize()
        c.release_stream(cold)


# ---- 11: refusals ----

def test_argument_errors_leave_the_context_usable():
    import torch

    n = 65
    P = shared(n, seed=8)
    tab = pair_table(P, 0.25, seed=88)
    with plfx.Context(0, lazy_tables=True) as c:
        L, h, C = c._L, c.h, plfx.C
        big = torch.zeros(S * n + 8, dtype=torch.float64, device="cuda")
        big[:S * n].copy_(dev(tab.ravel()))
        st = big[:S * n]
        t0 = dev(np.array([0.5, 0.5]))
        t_opt = torch.zeros(2, dtype=torch.float64, device="cuda")
        out3 = torch.zeros(6, dtype=torch.float64, device="cuda")
        evals = torch.zeros(2, dtype=torch.int32, device="cuda")
        p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        KEEP = object()
        INV, UNS = plfx.ERR_INVALID, plfx.ERR_UNSUPPORTED

        def opt(tabs=(st.data_ptr(),), nedges=None, t0_=t0, t_opt_=t_opt, tmin=TMIN, tmax=TMAX, max_evals=64,
                ncat=NCAT, out3_=out3, evals_=evals, n_=n, eig=P["eig"], rates=P["rates"], cat=P["cat"],
                dtype=plfx.F64, arr=KEEP, states=S):
            if arr is KEEP:
                arr = (C.c_void_p * max(1, len(tabs)))(*tabs)
            return L.plfx_edge_optimize_psr_dev_gen(h, dtype, states, arr, len(tabs) if nedges is None else nedges, n_,
                                                    p(eig), p(rates), ncat, p(cat), p(P["wgt"]), p(t0_), tmin, tmax,
                                                    max_evals, p(t_opt_), p(out3_), p(evals_), None)

        assert opt(nedges=0) == INV
        assert opt(arr=None) == INV                            # null sumtabs
        assert opt(tabs=(st.data_ptr(), None)) == INV          # a null entry
        assert opt(tabs=(st.data_ptr(), big[1:].data_ptr())) == INV  # a table misaligned by 8 bytes
        assert opt(t0_=None) == INV
        assert opt(t_opt_=None) == INV
        assert opt(tmin=0.0) == INV
        assert opt(tmin=1.0, tmax=0.1) == INV
        assert opt(tmax=float("inf")) == INV
        assert opt(max_evals=0) == INV
        assert opt(max_evals=plfx.EDGE_MAX_EVALS + 1) == INV
        assert b"max_evals" in L.plfx_last_error(h)
        assert opt(ncat=0) == INV and opt(ncat=33) == INV      # INVALID, not UNSUPPORTED
        assert b"ncat" in L.plfx_last_error(h)
        assert opt(n_=-1) == INV and opt(dtype=2) == INV
        assert opt(eig=None) == INV and opt(rates=None) == INV and opt(cat=None) == INV
        assert opt(states=5) == UNS and opt(states=0) == UNS
        assert b"states" in L.plfx_last_error(h)

        # the derivatives and the host loop
        one = torch.zeros(3, dtype=torch.float64, device="cuda")
        tt = dev(np.array([0.5]))

        def der(st_=st, n_=n, eig=P["eig"], rates=P["rates"], ncat=NCAT, cat=P["cat"], t=tt, sums=None, nsums=0,
                out=one, dtype=plfx.F64, states=S):
            return L.plfx_edge_derivatives_psr_gen(h, dtype, states, p(st_), n_, p(eig), p(rates), ncat, p(cat),
                                                   p(P["wgt"]), p(t), p(sums), nsums, p(out), None, None)

        assert der(st_=None) == INV and der(st_=big[1:]) == INV and der(n_=-1) == INV and der(dtype=2) == INV
        assert der(eig=None) == INV and der(rates=None) == INV and der(cat=None) == INV
        assert der(ncat=0) == INV and der(ncat=33) == INV
        assert der(t=None) == INV and der(out=None) == INV
        assert der(nsums=-1) == INV and der(nsums=2) == INV    # a count without the array
        assert der(states=5) == UNS

        def host(st_=st, t0_=0.5, tmin=TMIN, tmax=TMAX, max_evals=64, states=S, topt=KEEP, ncat=NCAT):
            t, o, ev = C.c_double(-1.0), (C.c_double * 3)(), C.c_int(-1)
            rc = L.plfx_edge_optimize_psr_gen(h, plfx.F64, states, p(st_), n, p(P["eig"]), p(P["rates"]), ncat,
                                              p(P["cat"]), p(P["wgt"]), t0_, tmin, tmax, max_evals,
                                              C.byref(t) if topt is KEEP else None, o, C.byref(ev), None)
            return rc, t.value, ev.value

        for kw in (dict(st_=None), dict(st_=big[1:]), dict(t0_=0.0), dict(t0_=20.0), dict(tmin=0.0), dict(max_evals=0),
                   dict(topt=None), dict(ncat=0)):
            assert host(**kw) == (INV, -1.0, -1), kw
        assert host(states=5) == (UNS, -1.0, -1)
        torch.cuda.synchronize()
        assert t_opt.tolist() == [0.0, 0.0] and one.tolist() == [0.0] * 3  # the refused calls launched nothing
        assert opt(out3_=None, evals_=None) == plfx.OK
        torch.cuda.synchronize()
        want = run_host(c, P, st, 0.5)
        assert np.array_equal(bits(t_opt.cpu().numpy()[:1]), bits(want[0]))
        assert out3.tolist() == [0.0] * 6 and evals.tolist() == [0, 0]

        # the sum tables, one and batched
        V = S * n
        pool = torch.full((7 * V + 8,), -7.0, dtype=torch.float64, device="cuda")
        a, b, s0, s1, a2, b2, s2 = (pool[k * V:(k + 1) * V] for k in range(7))
        x1, x2, _, _, _ = make_sides(np.float64, "dense", n, seed=81)
        _, _, _, codes, tv = make_sides(np.float64, "tip", n, seed=82)
        a.copy_(dev(x1.ravel()))
        b.copy_(dev(x2.ravel()))
        a2.copy_(a)
        b2.copy_(b)
        cd, tvd = dev(codes), dev(tv.ravel())

        def tab1(tip1=None, x1_=a, x2_=b, st_=s0, n_=n, tipvec=tvd, dtype=plfx.F64, states=S):
            return L.plfx_edge_sumtable_psr_gen(h, dtype, states, p(tip1), p(x1_), p(x2_), n_, p(tipvec), p(st_), None)

        assert tab1(tip1=cd) == INV and tab1(x1_=None) == INV   # both, neither
        assert tab1(tip1=cd, x1_=None, tipvec=None) == INV      # tip1 without tipvec
        assert tab1(n_=-1) == INV and tab1(dtype=2) == INV
        assert tab1(x2_=None) == INV and tab1(st_=None) == INV
        assert tab1(x1_=pool[1:]) == INV and tab1(x2_=pool[V + 1:]) == INV and tab1(st_=pool[2 * V + 1:]) == INV
        assert tab1(st_=a) == INV and tab1(st_=b) == INV        # the table over its own input
        assert tab1(st_=pool[2 * V - 2:]) == INV                # ... sharing x2's last 16 bytes
        assert tab1(x2_=pool[2 * V - 4 * n:]) == INV           # apart at n * 4 values, not at n * 20
        assert tab1(states=5) == UNS

        def E_(tip1=None, x1_=a, x2_=b, st_=s0):
            return plfx.PsrEdge(p(tip1), p(x1_), p(x2_), p(st_))

        def tabs(*edges, n_=n, tipvec=tvd, dtype=plfx.F64, nedges=None, null=False, states=S):
            arr = (plfx.PsrEdge * max(1, len(edges)))(*edges)
            return L.plfx_edge_sumtable_psr_batch_gen(h, dtype, states, None if null else arr,
                                                      len(edges) if nedges is None else nedges, n_, p(tipvec), None)

        good2 = E_(x1_=a2, x2_=b2, st_=s1)
        assert tabs(E_(), nedges=0) == INV and tabs(E_(), null=True) == INV
        assert tabs(E_(), n_=-1) == INV and tabs(E_(), dtype=2) == INV
        assert tabs(E_(tip1=cd)) == INV and tabs(E_(x1_=None)) == INV
        assert tabs(E_(x2_=None)) == INV and tabs(E_(st_=None)) == INV
        assert tabs(E_(x1_=pool[1:])) == INV and tabs(E_(x2_=pool[V + 1:])) == INV and tabs(E_(st_=pool[2 * V + 1:])) == INV
        assert tabs(good2, E_(tip1=cd, x1_=None), tipvec=None) == INV  # a coded side without tipvec
        assert tabs(E_(st_=a)) == INV and tabs(E_(st_=b)) == INV
        assert tabs(E_(), E_(x1_=a2, x2_=b2, st_=s0)) == INV      # the same table twice
        assert tabs(E_(), E_(x1_=a2, x2_=b2, st_=pool[3 * V - 2:])) == INV  # sharing the other table's last 16 bytes
        assert tabs(E_(), E_(x1_=a2, x2_=b2, st_=pool[2 * V + 4 * n:6 * V])) == INV  # apart at n * 4 values only
        assert tabs(E_(st_=pool[5 * V - 2:]), good2) == INV       # sharing the other edge's x1's last 16 bytes
        assert tabs(good2, E_(tip1=cd, x1_=None, st_=a2)) == INV  # over the other edge's x1
        assert b"psr sumtable" in L.plfx_last_error(h)
        assert tabs(E_(), states=5) == UNS
        torch.cuda.synchronize()
        assert np.all(s0.cpu().numpy() == -7.0) and np.all(s1.cpu().numpy() == -7.0)  # nothing ran
        assert tabs(E_(st_=None), n_=0, tipvec=None) == plfx.OK   # n == 0: the call-level checks alone
        assert tab1(st_=None, x2_=None, n_=0) == plfx.OK
        assert tabs(E_(), good2, E_(tip1=cd, x1_=None, st_=s2)) == plfx.OK
        torch.cuda.synchronize()
        ref = E.sumtab(x1, x2).ravel()
        assert np.array_equal(bits(s0.cpu().numpy()), bits(ref)) and np.array_equal(bits(s1.cpu().numpy()), bits(ref))
        coded = E.sumtab(R.expand_tips(codes, np.float64, tv).reshape(n, S), x2).ravel()
        assert np.array_equal(bits(s2.cpu().numpy()), bits(coded))
        assert np.all(pool[7 * V:].cpu().numpy() == -7.0)

        # the binding: a state count that is not built, tensors too small for 20 states
        with pytest.raises(plfx.PlfxError) as ei:
            c.optimize_branches_psr_gen(5, [st], n, P["eig"], P["rates"], P["cat"], t0, t_opt)
        assert ei.value.code == UNS
        with pytest.raises(plfx.PlfxError) as ei:
            c.edge_derivatives_psr_gen(S, st[:4 * n], n, P["eig"], P["rates"], P["cat"], tt, one)
        assert ei.value.code == INV
        with pytest.raises(plfx.PlfxError) as ei:
            c.edge_sumtables_psr_gen(S, [dict(x1=a, x2=b, sumtab=s0[:4 * n])], n)
        assert ei.value.code == INV
        # the section-11 methods still answer a protein request with UNSUPPORTED
        with pytest.raises(plfx.PlfxError) as ei:
            c.edge_derivatives_psr(st, n, P["eig"], P["rates"], P["cat"], tt, one, states=S)
        assert ei.value.code == UNS
        # and the context still gives the host path's bits
        assert_same(run_dev(c, P, [st], [0.5]), want, "after the refused calls")
