"""GPU tests of plfx_edge_optimize_psr_dev and plfx_edge_sumtable_psr_batch
(plfx.h section 11): the branch-length iteration of plfx_edge_optimize_psr with
the loop kept on the device, for a batch of independent PSR branches, and the
sum tables of a batch of branches in one call -- both asynchronous and
capture-safe.

The yardstick for bits is the host path: the device loop runs the same stepper
(csrc/edge_newton_step.hpp) on sums formed by the derivative kernel's
statements in its grid and order, so a one-edge call's t_opt, out3 and evals
must equal ctx.optimize_branch_psr on the same table from the same start BIT
FOR BIT.  The yardstick for values is tests/psr_ref.py's edge and scipy's
brentq on it; the only tolerances are the existing bars, 1e-6 relative for an
optimum and LNL_RTOL through check_out.

Data: two taxa simulated under test_gpu_psr.py's model() (25 rates): sa ~ pi,
sb evolved from sa at rates[clamp(cat)] * t*, table = Vi[:, sa].T * Vi[:, sb].T.
rate_cat is drawn from 0..27 (a few are clamped), weights from 1..3."""
import numpy as np
import pytest
from scipy.optimize import brentq

import plfx
import psr_ref
from test_gpu_psr import GUARD, NCAT_EDGE, STARTS, bits, check_out, dev, make_sides, model, np_dtype, tdtype
from test_gpu_psr import pulley  # noqa: F401  (the four-taxon fixture)

pytestmark = pytest.mark.gpu

TMIN, TMAX, MAX_EVALS = 1e-8, 10.0, 64


def shared(n, seed=1, ncat=NCAT_EDGE):
    """What the edges of a call share: the model (ncat = 25: model()'s rates),
    the categories and the weights, on the host and on the device."""
    m = model()
    rates = m["rates"] if ncat == NCAT_EDGE else np.geomspace(0.05, 4.0, ncat)
    rng = np.random.default_rng(seed)
    cat = rng.integers(0, 28, n).astype(np.uint8)
    wgt = rng.integers(1, 4, n).astype(np.int32)
    return dict(n=n, ncat=ncat, m=m, rates_np=rates, cat_np=cat, wgt_np=wgt, eig=dev(m["e"]), rates=dev(rates),
                cat=dev(cat), wgt=dev(wgt))


def pair_table(P, tstar, seed, identical=False):
    """The (n, 4) f64 sum table of two simulated taxa at distance tstar."""
    m, n = P["m"], P["n"]
    rng = np.random.default_rng(seed)
    sa = rng.choice(4, n, p=m["pi"])
    sb = sa.copy()
    if not identical:
        pm = np.stack([(m["V"] * np.exp(m["lam"] * r * tstar)) @ m["Vi"] for r in P["rates_np"]])
        p = np.clip(pm[psr_ref.clamp(P["cat_np"], P["ncat"]), sa], 0, None)
        p /= p.sum(axis=1, keepdims=True)
        sb = (rng.random(n)[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, 3)
    return m["Vi"][:, sa].T * m["Vi"][:, sb].T


def dev_table(tab, dt):
    """The table on the device; n == 0: four unused values, so that the pointer is not NULL."""
    return dev(tab.astype(dt).ravel() if tab.size else np.ones(4, dt))


def ref_d1(P, tab):
    return lambda t: psr_ref.edge(tab, P["m"]["lam"], P["rates_np"], P["cat_np"], t, P["wgt_np"])[0][1]


def run_dev(c, P, tables, t0, max_evals=MAX_EVALS, tmin=TMIN, tmax=TMAX, stream=None, sync=True):
    """optimize_branches_psr over `tables` from the starts t0 (array or device
    tensor): (t_opt, out3 (m, 3), evals) as numpy arrays, or the device tensors."""
    import torch

    m = len(tables)
    t0 = t0 if isinstance(t0, torch.Tensor) else dev(np.asarray(t0, np.float64))
    t_opt = torch.full((m,), np.nan, dtype=torch.float64, device="cuda")
    out3 = torch.full((3 * m,), np.nan, dtype=torch.float64, device="cuda")
    evals = torch.full((m,), -1, dtype=torch.int32, device="cuda")
    c.optimize_branches_psr(tables, P["n"], P["eig"], P["rates"], P["cat"], t0, t_opt, tmin, tmax, max_evals,
                            out3=out3, evals=evals, wgt=P["wgt"], stream=stream)
    if not sync:
        return t_opt, out3, evals
    torch.cuda.synchronize()
    return t_opt.cpu().numpy(), out3.cpu().numpy().reshape(m, 3), evals.cpu().numpy()


def run_host(c, P, table, t0, max_evals=MAX_EVALS, tmin=TMIN, tmax=TMAX):
    t, lnl, d1, d2, ev = c.optimize_branch_psr(table, P["n"], P["eig"], P["rates"], P["cat"], t0, tmin, tmax,
                                               max_evals, wgt=P["wgt"])
    return np.array([t]), np.array([[lnl, d1, d2]]), np.array([ev], np.int32)


def assert_same(got, want, what):
    """(t_opt, out3, evals) equal bit for bit."""
    for name, g, w in zip(("t_opt", "out3", "evals"), got, want):
        if name == "evals":
            assert np.array_equal(g, w), (what, name, g, w)
        else:
            assert np.array_equal(bits(g), bits(w)), (what, name, g.tolist(), w.tolist())


# ---- 1, 2: one edge is the host path ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_one_edge_equals_the_host_path_bit_for_bit(ctx, dt):
    """n: 0 (sums {0, 0, 0}), one site, 1023 / 1025 around a block's 256 x 4
    sites per trip, 2500 = three blocks; at 257 also ncat 1 and 32.  (f32: a
    table of two one-hot ends cancels to L <= 0 at some sites near tmin, so
    only the bits are compared there, not the optimum.)

    An identical pair's lnL falls with t, so its optimum is tmin -- in exact
    arithmetic.  model()'s zero eigenvalue is 8.2e-17 after the
    decomposition, and for ONE site in the fastest category (rate 4) the
    other three terms have decayed below that at t = 10: numpy's d1 there is
    +3.2e-16, and the host loop itself, started at tmax, stays there.  The
    seeds below put n = 1's site in category 18; that numpy's d1 is negative
    at every start is asserted before tmin is."""
    cases = [(n, NCAT_EDGE) for n in (0, 1, 65, 1023, 1025, 2500)] + [(257, 1), (257, 32)]
    for n, ncat in cases:
        P = shared(n, seed=3 * n + ncat, ncat=ncat)
        for identical in (False, True):
            tab = pair_table(P, 0.25, seed=7000 + n + ncat, identical=identical)
            st = dev_table(tab, np_dtype(dt))
            if identical and n > 0:
                assert all(ref_d1(P, tab)(t) < 0 for t in STARTS), (n, ncat)
            for t0 in STARTS:
                got = run_dev(ctx, P, [st], [t0])
                want = run_host(ctx, P, st, t0)
                print(f"{dt} n={n} ncat={ncat} identical={identical} start {t0:g}: t {got[0][0]!r} host {want[0][0]!r} "
                      f"evals {got[2][0]} host {want[2][0]}")
                assert_same(got, want, (n, ncat, identical, t0))
                if identical and dt == "f64" and n > 0:
                    assert got[0][0] == TMIN


def test_one_block_walks_every_site(monkeypatch):
    """PLFX_MAX_BLOCKS=1: one block per edge makes all the trips and is its own last block."""
    monkeypatch.setenv("PLFX_MAX_BLOCKS", "1")
    n = 2500
    with plfx.Context(0, lazy_tables=True) as c:
        P = shared(n, seed=5)
        tab = pair_table(P, 0.25, seed=55)
        for dt in (np.float64, np.float32):
            st = dev_table(tab, dt)
            for t0 in (0.01, 3.0):
                assert_same(run_dev(c, P, [st], [t0]), run_host(c, P, st, t0), (dt, t0))


# ---- 3, 4: batches ----

def batch_tables(P):
    """33 f64 tables: t* cycling, every edge with j % 8 == 5 identical, table 3 listed again as 20."""
    tstars = (0.05, 0.25, 1.5, 5.0)
    kinds = [j % 8 == 5 for j in range(33)]
    tabs = [pair_table(P, tstars[j % 4], seed=400 + j, identical=kinds[j]) for j in range(33)]
    tabs[20], kinds[20] = tabs[3], kinds[3]
    return tabs, kinds


def test_batch_equals_singles(ctx):
    """33 f64 edges (two launch groups) of 2500 sites (three blocks each)."""
    P = shared(2500, seed=2)
    tabs_np, kinds = batch_tables(P)
    tables = [dev_table(t, np.float64) for t in tabs_np]
    tables[20] = tables[3]  # one table twice, from different starts
    t0 = np.geomspace(2e-3, 8.0, 33)
    got = run_dev(ctx, P, tables, t0)
    interior = 0
    for j in range(33):
        one = run_dev(ctx, P, [tables[j]], [t0[j]])
        assert_same(tuple(g[j:j + 1] for g in got), one, j)
        d1 = ref_d1(P, tabs_np[j])
        if kinds[j]:
            assert got[0][j] == TMIN
        elif d1(TMIN) > 0 > d1(TMAX):
            t_ref = brentq(d1, TMIN, TMAX, xtol=1e-14, rtol=1e-14)
            print(f"edge {j}: t {got[0][j]!r} brentq {t_ref!r} rel {abs(got[0][j] - t_ref) / t_ref:.2e} "
                  f"evals {got[2][j]}")
            assert abs(got[0][j] - t_ref) <= 1e-6 * t_ref
            interior += 1
    assert interior >= 24  # every simulated pair that is not identical has its optimum inside the interval


def test_a_capped_group(ctx):
    """32 x 128 blocks: with 32 edges an edge's grid is capped at 4096 / 32 =
    128 blocks, below the 129 of the one-edge call at 132 000 sites, so the
    sums are formed in another order than the single call's: values, not
    bits, against numpy -- and run-to-run bits."""
    n = 132_000
    P = shared(n, seed=3)
    tab = pair_table(P, 0.25, seed=33)
    st = dev_table(tab, np.float64)
    t0 = np.geomspace(1e-3, 8.0, 32)
    got = run_dev(ctx, P, [st] * 32, t0)
    again = run_dev(ctx, P, [st] * 32, t0)
    assert_same(got, again, "two runs")
    d1 = ref_d1(P, tab)
    assert d1(TMIN) > 0 > d1(TMAX)
    t_ref = brentq(d1, TMIN, TMAX, xtol=1e-14, rtol=1e-14)
    for j in range(32):
        print(f"edge {j}: t {got[0][j]!r} brentq {t_ref!r} rel {abs(got[0][j] - t_ref) / t_ref:.2e} evals {got[2][j]}")
        assert abs(got[0][j] - t_ref) <= 1e-6 * t_ref
        ref, scale, _ = psr_ref.edge(tab, P["m"]["lam"], P["rates_np"], P["cat_np"], got[0][j], P["wgt_np"])
        check_out(got[1][j], ref, scale, f"edge {j}")


# ---- 5: caps, clamping, chaining ----

@pytest.mark.parametrize("n", [65, 2500])
def test_evaluation_caps(ctx, n):
    import torch

    P = shared(n, seed=n)
    st = dev_table(pair_table(P, 1.5, seed=n + 1), np.float64)
    got = run_dev(ctx, P, [st], [3.0], max_evals=3)
    assert got[2][0] == 3
    assert_same(got, run_host(ctx, P, st, 3.0, max_evals=3), "cap 3")
    got = run_dev(ctx, P, [st], [3.0], max_evals=1)
    out = torch.zeros(3, dtype=torch.float64, device="cuda")
    ctx.edge_derivatives_psr(st, n, P["eig"], P["rates"], P["cat"], dev(np.array([3.0])), out, wgt=P["wgt"])
    torch.cuda.synchronize()
    assert got[0][0] == 3.0 and got[2][0] == 1
    assert np.array_equal(bits(got[1][0]), bits(out.cpu().numpy()))


@pytest.mark.parametrize("n", [65, 2500])
def test_device_t0_is_clamped_and_chains(ctx, n):
    import torch

    P = shared(n, seed=n)
    st = dev_table(pair_table(P, 0.25, seed=n + 2), np.float64)
    lo, hi = run_dev(ctx, P, [st] * 2, [1e-12, 50.0]), run_dev(ctx, P, [st] * 2, [TMIN, TMAX])
    assert_same(lo, hi, "clamped starts")
    assert_same(tuple(g[0:1] for g in lo), run_host(ctx, P, st, TMIN), "start below tmin")
    assert_same(tuple(g[1:2] for g in lo), run_host(ctx, P, st, TMAX), "start above tmax")
    # call 1 stops at its cap; call 2 starts where it stopped, with no host in between
    first = run_dev(ctx, P, [st], [3.0], max_evals=3, sync=False)
    second = run_dev(ctx, P, [st], first[0], sync=False)
    torch.cuda.synchronize()
    t1 = float(first[0].cpu().numpy()[0])
    assert t1 != 3.0
    got = (second[0].cpu().numpy(), second[1].cpu().numpy().reshape(1, 3), second[2].cpu().numpy())
    assert_same(got, run_host(ctx, P, st, t1), "chained")


# ---- 6: the batched sum table ----

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
    stride = 4 * n + GUARD
    buf = torch.full((35 * stride,), -7.0, dtype=tdtype(dt), device="cuda")
    single = torch.full((35 * stride,), -7.0, dtype=tdtype(dt), device="cuda")
    descs = []
    for j, (x1, codes, x2) in enumerate(edges):
        d = dict(x2=on_dev(x2), sumtab=buf[j * stride:j * stride + 4 * n])
        d.update(dict(x1=on_dev(x1)) if codes is None else dict(tip1=on_dev(codes)))
        descs.append(d)
        ctx.edge_sumtable_psr(d["x2"], single[j * stride:j * stride + 4 * n], n, x1=d.get("x1"), tip1=d.get("tip1"),
                              tipvec=tvd)
    ctx.edge_sumtables_psr(descs, n, tipvec=tvd)
    torch.cuda.synchronize()
    got, one = buf.cpu().numpy().reshape(35, stride), single.cpu().numpy().reshape(35, stride)
    for j, (x1, codes, x2) in enumerate(edges):
        a = x1 if codes is None else psr_ref.expand_tips(codes, dt, tv).reshape(n, 4)
        assert np.array_equal(bits(got[j, :4 * n]), bits(psr_ref.sumtab(a, x2).ravel())), j
    assert np.array_equal(bits(got), bits(one))  # the single calls' tables, and every guard element still -7


# ---- 7: capture ----

def test_captured_chain_replays_to_the_eager_bits():
    """Batched sum tables (one dense, one coded edge) + optimize_branches_psr
    captured on a stream whose first use is the capture; the workspace is at
    rest afterwards."""
    import torch

    n, dt = 257, np.float64
    with plfx.Context(0, lazy_tables=True) as c:
        P = shared(n, seed=9)
        m = P["m"]
        x1, x2, _, _, _ = make_sides(dt, "dense", n, seed=91)
        _, y2, _, codes, tv = make_sides(dt, "tip", n, seed=92)
        xa, xb, yb, cd, tvd = dev(x1.ravel()), dev(x2.ravel()), dev(y2.ravel()), dev(codes), dev(tv.ravel())
        st = [torch.zeros(4 * n, dtype=torch.float64, device="cuda") for _ in range(2)]
        t0 = dev(np.array([0.1, 3.0]))
        t_opt = torch.zeros(2, dtype=torch.float64, device="cuda")
        out3 = torch.zeros(6, dtype=torch.float64, device="cuda")
        evals = torch.zeros(2, dtype=torch.int32, device="cuda")
        outs = (st[0], st[1], t_opt, out3, evals)

        def call(stream):
            c.edge_sumtables_psr([dict(tip1=cd, x2=yb, sumtab=st[1]), dict(x1=xa, x2=xb, sumtab=st[0])], n, tipvec=tvd,
                                 stream=stream)
            c.optimize_branches_psr(st, n, P["eig"], P["rates"], P["cat"], t0, t_opt, TMIN, TMAX, MAX_EVALS, out3=out3,
                                    evals=evals, wgt=P["wgt"], stream=stream)

        def eager(starts):
            t0.copy_(dev(np.array(starts)))
            call(None)
            torch.cuda.synchronize()
            return [t.cpu().numpy().copy() for t in outs]

        want = {s: eager(s) for s in ((0.1, 3.0), (5.0, 1e-3))}
        w = want[(0.1, 3.0)]
        ref_st = [psr_ref.sumtab(x1, x2), psr_ref.sumtab(psr_ref.expand_tips(codes, dt, tv).reshape(n, 4), y2)]
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
        for starts in ((0.1, 3.0), (0.1, 3.0), (5.0, 1e-3), (0.1, 3.0)):
            t0.copy_(dev(np.array(starts)))
            for t in outs:
                t.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for t, f in zip(outs, want[starts]):
                got = t.cpu().numpy()
                assert np.array_equal(got, f) if got.dtype == np.int32 else np.array_equal(bits(got), bits(f)), starts
        # the workspace is at rest: the other sum-producing calls on that stream are correct
        x = dev(np.random.default_rng(4).random(4 * n) + 0.05)
        lnl = torch.zeros(1, dtype=torch.float64, device="cuda")
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        with torch.cuda.stream(cold):
            c.root_lnl_psr(x, n, lnl, wgt=P["wgt"], stream=cold)
            c.edge_derivatives_psr(st[0], n, P["eig"], P["rates"], P["cat"], dev(np.array([0.3])), out, wgt=P["wgt"],
                                   stream=cold)
        torch.cuda.synchronize()
        ref_lnl = psr_ref.root_lnl(x.cpu().numpy(), n, wgt=P["wgt_np"])[0]
        assert abs(float(lnl.item()) - ref_lnl) <= 1e-10 * abs(ref_lnl)
        ref, scale, _ = psr_ref.edge(ref_st[0], m["lam"], P["rates_np"], P["cat_np"], 0.3, P["wgt_np"])
        check_out(out.cpu().numpy(), ref, scale, "after the replays")
        del g
        torch.cuda.synchronize()
        c.release_stream(cold)


# ---- 8: refusals ----

def test_argument_errors_leave_the_context_usable():
    import torch

    n = 65
    P = shared(n, seed=8)
    tab = pair_table(P, 0.25, seed=88)
    with plfx.Context(0, lazy_tables=True) as c:
        L, h, C = c._L, c.h, plfx.C
        big = torch.zeros(4 * n + 8, dtype=torch.float64, device="cuda")
        big[:4 * n].copy_(dev(tab.ravel()))
        st = big[:4 * n]
        t0 = dev(np.array([0.5, 0.5]))
        t_opt = torch.zeros(2, dtype=torch.float64, device="cuda")
        out3 = torch.zeros(6, dtype=torch.float64, device="cuda")
        evals = torch.zeros(2, dtype=torch.int32, device="cuda")
        p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        KEEP = object()

        def opt(tabs=(st.data_ptr(),), nedges=None, t0_=t0, t_opt_=t_opt, tmin=TMIN, tmax=TMAX, max_evals=64,
                ncat=NCAT_EDGE, out3_=out3, evals_=evals, n_=n, eig=P["eig"], rates=P["rates"], cat=P["cat"],
                dtype=plfx.F64, arr=KEEP):
            if arr is KEEP:
                arr = (C.c_void_p * max(1, len(tabs)))(*tabs)
            return L.plfx_edge_optimize_psr_dev(h, dtype, arr, len(tabs) if nedges is None else nedges, n_, p(eig),
                                                p(rates), ncat, p(cat), p(P["wgt"]), p(t0_), tmin, tmax, max_evals,
                                                p(t_opt_), p(out3_), p(evals_), None)

        INV = plfx.ERR_INVALID
        assert opt(nedges=0) == INV
        assert opt(arr=None) == INV                            # null sumtabs
        assert opt(tabs=(st.data_ptr(), None)) == INV          # a null entry
        assert opt(tabs=(st.data_ptr(), big[1:].data_ptr())) == INV  # an unaligned table
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
        torch.cuda.synchronize()
        assert t_opt.tolist() == [0.0, 0.0]  # the refused calls launched nothing
        assert opt(out3_=None, evals_=None) == plfx.OK
        torch.cuda.synchronize()
        want = run_host(c, P, st, 0.5)
        assert np.array_equal(bits(t_opt.cpu().numpy()[:1]), bits(want[0]))
        assert out3.tolist() == [0.0] * 6 and evals.tolist() == [0, 0]

        # the batched sum table
        pool = torch.full((7 * 4 * n + 8,), -7.0, dtype=torch.float64, device="cuda")
        a, b, s0, s1, a2, b2, s2 = (pool[k * 4 * n:(k + 1) * 4 * n] for k in range(7))
        x1, x2, _, _, _ = make_sides(np.float64, "dense", n, seed=81)
        _, _, _, codes, tv = make_sides(np.float64, "tip", n, seed=82)
        a.copy_(dev(x1.ravel()))
        b.copy_(dev(x2.ravel()))
        a2.copy_(a)
        b2.copy_(b)
        cd, tvd = dev(codes), dev(tv.ravel())

        def E(tip1=None, x1_=a, x2_=b, st_=s0):
            return plfx.PsrEdge(p(tip1), p(x1_), p(x2_), p(st_))

        def tabs(*edges, n_=n, tipvec=tvd, dtype=plfx.F64, nedges=None, null=False):
            arr = (plfx.PsrEdge * max(1, len(edges)))(*edges)
            return L.plfx_edge_sumtable_psr_batch(h, dtype, None if null else arr, len(edges) if nedges is None else nedges,
                                                  n_, p(tipvec), None)

        good2 = E(x1_=a2, x2_=b2, st_=s1)
        assert tabs(E(), nedges=0) == INV and tabs(E(), null=True) == INV
        assert tabs(E(), n_=-1) == INV and tabs(E(), dtype=2) == INV
        assert tabs(E(tip1=cd)) == INV                         # both a tip and a CLV
        assert tabs(E(x1_=None)) == INV                        # neither
        assert tabs(E(x2_=None)) == INV and tabs(E(st_=None)) == INV
        assert tabs(E(x1_=pool[1:])) == INV and tabs(E(x2_=pool[4 * n + 1:])) == INV  # misaligned
        assert tabs(E(st_=pool[8 * n + 1:])) == INV
        assert tabs(good2, E(tip1=cd, x1_=None), tipvec=None) == INV  # a coded side without tipvec
        assert tabs(E(st_=a)) == INV and tabs(E(st_=b)) == INV   # the table over its own input
        assert tabs(E(st_=pool[8 * n - 2:])) == INV              # ... sharing x2's last 16 bytes
        assert tabs(E(), E(x1_=a2, x2_=b2, st_=s0)) == INV       # the same table twice
        assert tabs(E(), E(x1_=a2, x2_=b2, st_=pool[12 * n - 2:])) == INV  # sharing the other table's last 16 bytes
        assert tabs(E(st_=pool[20 * n - 2:]), good2) == INV      # sharing the other edge's x1's last 16 bytes
        assert tabs(good2, E(tip1=cd, x1_=None, st_=a2)) == INV  # over the other edge's x1
        assert b"psr sumtable" in L.plfx_last_error(h)
        torch.cuda.synchronize()
        assert np.all(s0.cpu().numpy() == -7.0) and np.all(s1.cpu().numpy() == -7.0)  # nothing ran
        assert tabs(E(st_=None), n_=0, tipvec=None) == plfx.OK   # n == 0: the call-level checks alone
        assert tabs(E(), good2, E(tip1=cd, x1_=None, st_=s2)) == plfx.OK
        torch.cuda.synchronize()
        ref = psr_ref.sumtab(x1, x2).ravel()
        assert np.array_equal(bits(s0.cpu().numpy()), bits(ref)) and np.array_equal(bits(s1.cpu().numpy()), bits(ref))
        coded = psr_ref.sumtab(psr_ref.expand_tips(codes, np.float64, tv).reshape(n, 4), x2).ravel()
        assert np.array_equal(bits(s2.cpu().numpy()), bits(coded))
        assert np.all(pool[28 * n:].cpu().numpy() == -7.0)

        with pytest.raises(plfx.PlfxError) as ei:                # protein: not built
            c.optimize_branches_psr([st], n, P["eig"], P["rates"], P["cat"], t0, t_opt, states=20)
        assert ei.value.code == plfx.ERR_UNSUPPORTED
        with pytest.raises(plfx.PlfxError) as ei:
            c.edge_sumtables_psr([dict(x1=a, x2=b, sumtab=s0)], n, states=20)
        assert ei.value.code == plfx.ERR_UNSUPPORTED
        # and the context still gives the host path's bits
        assert_same(run_dev(c, P, [st], [0.5]), want, "after the refused calls")


# ---- 9: the pulley ----

def test_pulley_tables_and_optimum_are_the_host_path(ctx, pulley):  # noqa: F811
    import torch

    d = pulley
    n = d["n"]
    P = dict(n=n, eig=d["eig"], rates=d["rates"], cat=d["cat_d"], wgt=d["wgt_d"])
    st = torch.zeros(4 * n, dtype=torch.float64, device="cuda")
    ctx.edge_sumtables_psr([dict(x1=d["A"], x2=d["B"], sumtab=st)], n)
    torch.cuda.synchronize()
    assert np.array_equal(bits(st.cpu().numpy()), bits(d["st"].cpu().numpy()))
    for t0 in STARTS:
        assert_same(run_dev(ctx, P, [st], [t0]), run_host(ctx, P, d["st"], t0), t0)
