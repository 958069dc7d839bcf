"""GPU tests of plfx_edge_optimize_dev (plfx.h section 10): the branch-length
iteration of plfx_edge_optimize with the loop kept on the device, for a batch
of independent edges, asynchronous and capture-safe.

The yardstick is the host path: the device loop runs the same stepper
(csrc/edge_newton_step.hpp) on sums formed in the same order, so every edge's
t_opt, evals and out3 must equal ctx.optimize_branch on the same table from
the same start BIT FOR BIT -- there is no tolerance in this file except the
optimum's distance from scipy's brentq root of the numpy restatement (1e-6
relative, the bar of the existing optimum tests).

Data: two taxa simulated under GTR + Gamma4 (tests/test_edge_newton.py
two_taxon; for batches, which share one model, the same construction over
tests/test_gpu_edge.py's model)."""
import numpy as np
import pytest
from scipy.optimize import brentq

import plfx
from test_edge_newton import two_taxon
from test_gpu_edge import bits, check_out, dev, model, ref_edge

pytestmark = pytest.mark.gpu

TMIN, TMAX, MAX_EVALS = 1e-8, 10.0, 64
STARTS = (1e-8, 0.01, 0.1, 1.0, 3.0, 10.0)


def np_dtype(dt):
    return np.float64 if dt == "f64" else np.float32


def problem_of(d, dt):
    """A two_taxon() problem on the device: eigen holds only lambda (all that is read)."""
    n, _, S = d["st"].shape
    return dict(S=S, n=n, eig=dev(d["lam"]), rates=dev(d["rates"]), wgt=dev(d["wgt"].astype(np.int32)),
                st=dev(d["st"].astype(dt).ravel()))


def pair_table(S, n, tstar, seed, identical=False):
    """two_taxon's sum table (n, 4, S) over the shared model(S)."""
    m = model(S)
    rng = np.random.default_rng(seed)
    sa = rng.choice(S, n, p=m["pi"])
    cat = rng.integers(0, 4, n)
    sb = sa.copy()
    if not identical:
        for i in range(n):
            row = (m["V"] * np.exp(m["lam"] * m["rates"][cat[i]] * tstar)) @ m["Vi"]
            p = np.clip(row[sa[i]], 0, None)
            sb[i] = rng.choice(S, p=p / p.sum())
    a, b = (np.repeat(m["Vi"][:, s].T[:, None, :], 4, axis=1) for s in (sa, sb))
    return a, b


def shared_problem(S, n, seed=1):
    m = model(S)
    wgt = np.random.default_rng(seed).integers(1, 4, n).astype(np.int32)
    return dict(S=S, n=n, m=m, eig=dev(m["e"]), rates=dev(m["rates"]), wgt=dev(wgt), wgt_np=wgt)


def run_dev(c, P, tables, t0, max_evals=MAX_EVALS, tmin=TMIN, tmax=TMAX, stream=None, sync=True):
    """optimize_branches over `tables` from the starts t0 (array or device
    tensor): (t_opt, out3 (m, 3), evals) as numpy arrays, or the device tensors."""
    import torch

    m = len(tables)
    t0 = t0 if isinstance(t0, torch.Tensor) else dev(np.asarray(t0, np.float64))
    t_opt = torch.full((m,), np.nan, dtype=torch.float64, device="cuda")
    out3 = torch.full((3 * m,), np.nan, dtype=torch.float64, device="cuda")
    evals = torch.full((m,), -1, dtype=torch.int32, device="cuda")
    c.optimize_branches(tables, P["n"], P["eig"], P["rates"], t0, t_opt, tmin, tmax, max_evals, out3=out3,
                        evals=evals, wgt=P["wgt"], states=P["S"], stream=stream)
    if not sync:
        return t_opt, out3, evals
    torch.cuda.synchronize()
    return t_opt.cpu().numpy(), out3.cpu().numpy().reshape(m, 3), evals.cpu().numpy()


def run_host(c, P, table, t0, max_evals=MAX_EVALS, tmin=TMIN, tmax=TMAX):
    t, lnl, d1, d2, ev = c.optimize_branch(table, P["n"], P["eig"], P["rates"], t0, tmin, tmax, max_evals,
                                           wgt=P["wgt"], states=P["S"])
    return np.array([t]), np.array([[lnl, d1, d2]]), np.array([ev], np.int32)


def assert_same(got, want, what):
    """(t_opt, out3, evals) equal bit for bit."""
    for name, g, w in zip(("t_opt", "out3", "evals"), got, want):
        if name == "evals":
            assert np.array_equal(g, w), (what, name, g, w)
        else:
            assert np.array_equal(bits(g), bits(w)), (what, name, g.tolist(), w.tolist())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("S", [4, 20])
def test_one_edge_equals_the_host_path_bit_for_bit(ctx, dt, S):
    for n in (1, 65, 257):
        for identical in (False, True):
            P = problem_of(two_taxon(S, n, 0.25, seed=S * 1000 + n, identical=identical), np_dtype(dt))
            for t0 in STARTS:
                got = run_dev(ctx, P, [P["st"]], [t0])
                want = run_host(ctx, P, P["st"], t0)
                print(f"{dt} S={S} n={n} identical={identical} start {t0:g}: t {got[0][0]!r} host {want[0][0]!r} "
                      f"evals {got[2][0]} host {want[2][0]}")
                assert_same(got, want, (n, identical, t0))
                if identical:
                    assert got[0][0] == TMIN


@pytest.mark.parametrize("S,n", [(4, 65), (20, 257)])
def test_batch_equals_singles(ctx, S, n):
    """33 f64 edges (two launch groups): distinct tables and starts, one table
    repeated, identical sequences among them.  (f64 only: at t near tmin an
    f32 table of two one-hot ends cancels to L <= 0 at sites whose ends
    differ, and the numpy restatement has no root to compare with.)"""
    dt = "f64"
    P = shared_problem(S, n)
    tstars = (0.05, 0.25, 1.5, 5.0)
    tabs_np, kinds = [], []
    for j in range(33):
        identical = j % 8 == 5
        a, b = pair_table(S, n, tstars[j % 4], seed=100 * S + j, identical=identical)
        tabs_np.append((a * b).astype(np_dtype(dt)))
        kinds.append(identical)
    tabs_np[20] = tabs_np[3]  # one table twice, from different starts
    kinds[20] = kinds[3]
    tables = [dev(t.ravel()) for t in tabs_np]
    tables[20] = tables[3]
    t0 = np.geomspace(2e-3, 8.0, 33)
    got = run_dev(ctx, P, tables, t0)
    interior = 0
    for j in range(33):
        one = run_dev(ctx, P, [tables[j]], [t0[j]])
        assert_same(tuple(g[j:j + 1] for g in got), one, j)
        d1 = lambda t: ref_edge(tabs_np[j], P["m"], t, None, P["wgt_np"])[0][1]  # noqa: E731
        if kinds[j]:
            assert got[0][j] == TMIN
        elif d1(TMIN) > 0 > d1(TMAX):
            t_ref = brentq(d1, TMIN, TMAX, xtol=1e-14, rtol=1e-14)
            print(f"edge {j}: t {got[0][j]!r} brentq {t_ref!r} rel {abs(got[0][j] - t_ref) / t_ref:.2e} "
                  f"evals {got[2][j]}")
            assert abs(got[0][j] - t_ref) <= 1e-6 * t_ref
            interior += 1
    assert interior >= 16  # most of the simulated pairs have their optimum inside the interval


def test_evaluation_caps(ctx):
    import torch

    for S, n in ((4, 65), (20, 257)):
        P = problem_of(two_taxon(S, n, 1.5, seed=S * 1000 + n), np.float64)
        got = run_dev(ctx, P, [P["st"]], [3.0], max_evals=3)
        assert got[2][0] == 3
        assert_same(got, run_host(ctx, P, P["st"], 3.0, max_evals=3), "cap 3")
        got = run_dev(ctx, P, [P["st"]], [3.0], max_evals=1)
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        ctx.edge_derivatives(P["st"], n, P["eig"], P["rates"], dev(np.array([3.0])), out, wgt=P["wgt"], states=S)
        torch.cuda.synchronize()
        assert got[0][0] == 3.0 and got[2][0] == 1
        assert np.array_equal(bits(got[1][0]), bits(out.cpu().numpy()))


def test_device_t0_is_clamped_and_chains(ctx):
    import torch

    for S, n in ((4, 65), (20, 257)):
        P = problem_of(two_taxon(S, n, 0.25, seed=S * 1000 + n), np.float64)
        lo, hi = run_dev(ctx, P, [P["st"]] * 2, [1e-12, 50.0]), run_dev(ctx, P, [P["st"]] * 2, [TMIN, TMAX])
        assert_same(lo, hi, "clamped starts")
        assert_same(tuple(g[0:1] for g in lo), run_host(ctx, P, P["st"], TMIN), "start below tmin")
        assert_same(tuple(g[1:2] for g in lo), run_host(ctx, P, P["st"], TMAX), "start above tmax")
        # call 1 stops at its cap; call 2 starts where it stopped, with no host in between
        first = run_dev(ctx, P, [P["st"]], [3.0], max_evals=3, sync=False)
        second = run_dev(ctx, P, [P["st"]], first[0], sync=False)
        torch.cuda.synchronize()
        t1 = float(first[0].cpu().numpy()[0])
        assert t1 != 3.0
        got = (second[0].cpu().numpy(), second[1].cpu().numpy().reshape(1, 3), second[2].cpu().numpy())
        assert_same(got, run_host(ctx, P, P["st"], t1), "chained")


def test_captured_chain_replays_to_the_eager_bits():
    """Sum table + optimize_branches captured on a stream whose first use is
    the capture; the workspace is at rest afterwards."""
    import torch

    for S in (4, 20):
        n = 257
        P = None
        with plfx.Context(0, lazy_tables=True) as c:
            P = shared_problem(S, n, seed=S)
            a, b = pair_table(S, n, 0.25, seed=S)
            other = dev((lambda p: p[0] * p[1])(pair_table(S, n, 1.5, seed=S + 1)).ravel())
            xa, xb = dev(a.ravel()), dev(b.ravel())
            st = torch.zeros(4 * S * n, dtype=torch.float64, device="cuda")
            t0 = dev(np.array([0.1, 3.0]))
            t_opt = torch.zeros(2, dtype=torch.float64, device="cuda")
            out3 = torch.zeros(6, dtype=torch.float64, device="cuda")
            evals = torch.zeros(2, dtype=torch.int32, device="cuda")

            def call(stream):
                c.edge_sumtable(xb, st, n, x1=xa, states=S, stream=stream)
                c.optimize_branches([st, other], n, P["eig"], P["rates"], t0, t_opt, TMIN, TMAX, MAX_EVALS,
                                    out3=out3, evals=evals, wgt=P["wgt"], states=S, stream=stream)

            def eager(starts):
                t0.copy_(dev(np.array(starts)))
                call(None)
                torch.cuda.synchronize()
                return [t.cpu().numpy().copy() for t in (st, t_opt, out3, evals)]

            want = {s: eager(s) for s in ((0.1, 3.0), (5.0, 1e-3))}
            for j in (0, 1):  # and the eager result is the host path's
                ref = run_host(c, P, (st, other)[j], 0.1 if j == 0 else 3.0)
                w = want[(0.1, 3.0)]
                assert_same((w[1][j:j + 1], w[2].reshape(2, 3)[j:j + 1], w[3][j:j + 1]), ref, ("eager", j))
            cold = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            t0.copy_(dev(np.array([0.1, 3.0])))
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=cold):
                call(cold)
            for starts in ((0.1, 3.0), (0.1, 3.0), (5.0, 1e-3), (0.1, 3.0)):
                t0.copy_(dev(np.array(starts)))
                for t in (st, t_opt, out3, evals):
                    t.zero_()
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                for t, f in zip((st, t_opt, out3, evals), want[starts]):
                    got = t.cpu().numpy()
                    assert np.array_equal(got, f) if got.dtype == np.int32 else np.array_equal(bits(got), bits(f)), starts
            # the workspace is at rest: the other sum-producing calls on that stream are correct
            x = dev(np.random.default_rng(S).random(4 * S * n) + 0.05)
            lnl = torch.zeros(1, dtype=torch.float64, device="cuda")
            out = torch.zeros(3, dtype=torch.float64, device="cuda")
            with torch.cuda.stream(cold):
                c.root_lnl(x, n, lnl, wgt=P["wgt"], states=S, stream=cold)
                c.edge_derivatives(st, n, P["eig"], P["rates"], dev(np.array([0.3])), out, wgt=P["wgt"], states=S,
                                   stream=cold)
            torch.cuda.synchronize()
            L = x.cpu().numpy().reshape(n, 4, S).sum(axis=2) @ np.full(4, 0.25) / S
            ref_lnl = np.sum(P["wgt_np"] * np.log(L))
            assert abs(float(lnl.item()) - ref_lnl) <= 1e-10 * abs(ref_lnl)
            ref, scale, _ = ref_edge((a * b), P["m"], 0.3, None, P["wgt_np"])
            check_out(out.cpu().numpy(), ref, scale, f"S={S} after the replays")
            del g
            torch.cuda.synchronize()
            c.release_stream(cold)


def test_argument_errors_leave_the_context_usable():
    import torch

    S, n = 4, 65
    P = problem_of(two_taxon(S, n, 0.25, seed=4065), np.float64)
    with plfx.Context(0, lazy_tables=True) as c:
        L, h, C = c._L, c.h, plfx.C
        big = torch.zeros(16 * n + 8, dtype=torch.float64, device="cuda")
        big[:16 * n].copy_(P["st"])
        st = big[:16 * n]
        t0 = dev(np.array([0.5, 0.5]))
        t_opt = torch.zeros(2, dtype=torch.float64, device="cuda")
        out3 = torch.zeros(6, dtype=torch.float64, device="cuda")
        evals = torch.zeros(2, dtype=torch.int32, device="cuda")
        p = lambda x: None if x is None else x.data_ptr()  # noqa: E731

        def opt(tabs=(st.data_ptr(),), nedges=None, t0_=t0, t_opt_=t_opt, tmin=TMIN, tmax=TMAX, max_evals=64, ncat=4,
                states=S, out3_=out3, evals_=evals):
            arr = (C.c_void_p * max(1, len(tabs)))(*tabs)
            return L.plfx_edge_optimize_dev(h, plfx.F64, states, arr, len(tabs) if nedges is None else nedges, n,
                                            p(P["eig"]), p(P["rates"]), ncat, None, p(P["wgt"]), p(t0_), tmin, tmax,
                                            max_evals, p(t_opt_), p(out3_), p(evals_), None)

        INV, UNS = plfx.ERR_INVALID, plfx.ERR_UNSUPPORTED
        assert opt(nedges=0) == INV
        assert opt(tabs=(st.data_ptr(), None)) == INV          # a null entry
        assert opt(tabs=(st.data_ptr(), big[1:].data_ptr())) == INV  # an unaligned table
        assert opt(t0_=None) == INV
        assert opt(t_opt_=None) == INV
        assert opt(tmin=0.0) == INV
        assert opt(tmin=1.0, tmax=0.1) == INV
        assert opt(max_evals=0) == INV
        assert opt(max_evals=plfx.EDGE_MAX_EVALS + 1) == INV
        assert b"max_evals" in L.plfx_last_error(h)
        assert opt(ncat=3) == UNS
        assert opt(states=5) == UNS
        torch.cuda.synchronize()
        assert t_opt.tolist() == [0.0, 0.0]  # the refused calls launched nothing
        assert opt(out3_=None, evals_=None) == plfx.OK
        torch.cuda.synchronize()
        # and the context still works
        want = run_host(c, P, st, 0.5)
        assert np.array_equal(bits(t_opt.cpu().numpy()[:1]), bits(want[0]))
        assert out3.tolist() == [0.0] * 6 and evals.tolist() == [0, 0]
        assert_same(run_dev(c, P, [st], [0.5]), want, "after the refused calls")
