"""GPU tests of plfx.h section (10): the sum table of a branch's two end CLVs,
the edge log-likelihood with its first two derivatives in the branch length,
and the bracketed-Newton branch-length optimum.

The reference is the numpy restatement below: the same product rounded in the
CLVs' dtype, then f64 arithmetic.  The sum table is compared bit for bit.  The
three sums are compared at the project's f64 bar (LNL_RTOL, as
tests/test_gpu_model.py): lnL relatively, d1 and d2 against the sums of the
absolute per-site terms (d1 is near zero at the optimum, where a relative
bound means nothing).  Per-site log L: 1e-10 * max(1, |log L|) -- the error of
log L is the relative error of L, a few hundred ulp at worst with the
cancellation among the eigen-coordinate terms.

The pulley tests cross-check against code that predates the feature: for the
two children A, B of an 8-taxon tree's root, the edge lnL of A o B at t equals
the root lnL of the node update with P matrices at (0.3 t, 0.7 t)."""
import functools

import numpy as np
import pytest
from scipy.optimize import brentq

import plfx

pytestmark = pytest.mark.gpu

LNL_RTOL = 1e-10
LOG_MINLIK = -22.18070977791824990137  # log(2^-32)
STARTS = (1e-8, 0.01, 0.1, 1.0, 3.0, 10.0)
SIZES = (1, 63, 64, 65, 257)
GRID = [(dt, S, side) for dt in ("f64", "f32") for S in (4, 20) for side in ("dense", "tip")]
CATW = np.array([0.1, 0.2, 0.3, 0.4])


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(maxsize=None)
def model(S):
    rng = np.random.default_rng(100 + S)
    exch = rng.random(S * (S - 1) // 2) * 2 + 0.05
    freqs = rng.random(S) + 0.1
    e = plfx.model_eigen(exch, freqs)
    return dict(S=S, exch=exch, freqs=freqs, pi=freqs / freqs.sum(), e=e, lam=e[:S],
                V=e[S:S + S * S].reshape(S, S), Vi=e[S + S * S:].reshape(S, S),
                rates=plfx.gamma_rates(0.7, 4))


def tip_table(S):
    """The eigen-convention tip-vector table: 16 x 4 (DNA) or 24 x 20 (protein)."""
    import oracle

    m = model(S)
    if S == 4:
        return plfx.model_tip_vectors(m["e"], plfx.PMAT_EIGEN).reshape(16, 4)
    return oracle.protein_tip_table() @ m["Vi"].T


def make_sides(S, dt, side, n, seed):
    """x1, x2 as (n, 4, S) arrays of dt -- eigen coordinates of positive
    state-space vectors, so every site likelihood is positive -- and, for a
    coded side 1, its codes and table (x1 is then the table's expansion)."""
    import oracle

    m = model(S)
    rng = np.random.default_rng(seed)
    eig = lambda y: np.einsum("ks,ncs->nck", m["Vi"], y).astype(dt)  # noqa: E731
    x2 = eig(rng.random((n, 4, S)) * 0.5 + 0.05)
    if side == "dense":
        return eig(rng.random((n, 4, S)) * 0.5 + 0.05), x2, None, None
    tv = tip_table(S).astype(dt)
    if S == 4:
        codes = oracle.random_tip_codes(rng, n, 0.3)
        if n >= 4:
            codes[:4] = [0x03, 0xF5, 0x1E, 0x2F]  # ambiguity codes, junk in the upper nibble
        codes = np.where((codes & 15) == 0, codes | 15, codes).astype(np.uint8)  # no empty sets
        x1 = oracle.expand_tips(codes, dt, tipvec=tv)
    else:
        codes = oracle.random_protein_codes(rng, n, 0.3)
        if n >= 4:
            codes[:4] = [20, 22, 24, 255]  # B, X, and two codes >= 24 (row 23)
        x1 = oracle.expand_protein_tips(codes, dt, tipvec=tv)
    return x1.reshape(n, 4, S), x2, codes, tv


def ref_sumtab(x1, x2):
    assert x1.dtype == x2.dtype
    return x1 * x2  # one multiply, rounded in the dtype


def ref_edge(st, m, t, catw=None, wgt=None, nsc=0):
    """out3, the scales of its tolerances, and log L per site."""
    st = st.astype(np.float64)
    n = st.shape[0]
    cw = np.full(4, 0.25) if catw is None else catw
    w = np.ones(n) if wgt is None else wgt.astype(np.float64)
    x = m["rates"][:, None] * m["lam"][None, :]
    e = np.exp(x * t)
    e1 = e * x
    e2 = e1 * x
    L, L1, L2 = ((st * f[None]).sum(axis=2) @ cw for f in (e, e1, e2))
    r1, r2 = L1 / L, L2 / L
    out = np.array([np.sum(w * np.log(L)) + nsc * LOG_MINLIK, np.sum(w * r1), np.sum(w * (r2 - r1 * r1))])
    scale = np.array([abs(out[0]), np.sum(np.abs(w) * np.abs(r1)), np.sum(np.abs(w) * (np.abs(r2) + r1 * r1))])
    return out, scale, np.log(L)


def check_out(got, ref, scale, what):
    for j, name in enumerate(("lnL", "d1", "d2")):
        err = abs(got[j] - ref[j])
        print(f"{what} {name}: got {got[j]!r} ref {ref[j]!r} err/scale {err / scale[j] if scale[j] else err:.2e}")
        assert err <= LNL_RTOL * scale[j], (what, name, got[j], ref[j], scale[j])


def gpu_sumtab(c, S, dt, x1, x2, codes, tv, n, stream=None):
    """The device sum table (a view of a guarded buffer) and the buffer."""
    import torch

    V = 4 * S
    buf = torch.full((V * n + 64,), -7.0, dtype=torch.float64 if dt == np.float64 else torch.float32,
                     device="cuda")
    st = buf[:V * n]
    if codes is None:
        c.edge_sumtable(dev(x2.ravel()), st, n, x1=dev(x1.ravel()), states=S, stream=stream)
    else:
        c.edge_sumtable(dev(x2.ravel()), st, n, tip1=dev(codes), tipvec=dev(tv.ravel()), states=S, stream=stream)
    return st, buf


def np_dtype(dt):
    return np.float64 if dt == "f64" else np.float32


@pytest.mark.parametrize("dt,S,side", GRID)
def test_sumtable_is_bit_exact(ctx, dt, S, side):
    import torch

    dt = np_dtype(dt)
    for n in SIZES:
        x1, x2, codes, tv = make_sides(S, dt, side, n, seed=n)
        st, buf = gpu_sumtab(ctx, S, dt, x1, x2, codes, tv, n)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(bits(got[:4 * S * n]), bits(ref_sumtab(x1, x2).ravel())), n
        assert np.all(got[4 * S * n:] == -7.0), n  # nothing written past the table


@pytest.mark.parametrize("dt,S,side", GRID)
def test_derivatives_match_numpy(ctx, dt, S, side):
    import torch

    dt = np_dtype(dt)
    m = model(S)
    eig, rates = dev(m["e"]), dev(m["rates"])
    sums = np.array([3, 0, 5], np.int64)
    for n in (0,) + SIZES:
        rng = np.random.default_rng(7 * n + S)
        x1, x2, codes, tv = make_sides(S, dt, side, n, seed=1000 + n)
        if n:
            st, _ = gpu_sumtab(ctx, S, dt, x1, x2, codes, tv, n)
        else:
            st = dev(np.zeros(0, dt))
        ref_st = ref_sumtab(x1, x2)
        wgt = rng.integers(0, 4, n).astype(np.int32)
        for t in (1e-8, 0.2, 10.0):
            for full in (False, True):
                kw = dict(catw=dev(CATW), wgt=dev(wgt), scaler_sums=dev(sums)) if full else {}
                outs = []
                for _ in range(2):
                    out = torch.full((3,), np.nan, dtype=torch.float64, device="cuda")
                    site = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
                    ctx.edge_derivatives(st, n, eig, rates, dev(np.array([t])), out, site_lnl=site, states=S, **kw)
                    torch.cuda.synchronize()
                    outs.append((out.cpu().numpy(), site.cpu().numpy()))
                # two calls, the same bits: the reduction order is fixed
                assert np.array_equal(bits(outs[0][0]), bits(outs[1][0]))
                assert np.array_equal(bits(outs[0][1]), bits(outs[1][1]))
                got, site = outs[0]
                if n == 0:
                    assert got.tolist() == [(8 * LOG_MINLIK if full else 0.0), 0.0, 0.0]
                    continue
                ref, scale, ref_site = ref_edge(ref_st, m, t, CATW if full else None, wgt if full else None,
                                                8 if full else 0)
                check_out(got, ref, scale, f"n={n} t={t} full={full}")
                assert np.all(np.abs(site - ref_site) <= LNL_RTOL * np.maximum(1.0, np.abs(ref_site))), (n, t)


def test_many_trips_per_block(monkeypatch):
    """PLFX_MAX_BLOCKS=1: one block walks all 4099 sites (17 trips of the DNA
    kernel, 65 tiles of the protein one) and is its own last block."""
    import torch

    monkeypatch.setenv("PLFX_MAX_BLOCKS", "1")
    n = 4099
    with plfx.Context(0, lazy_tables=True) as c:
        for S in (4, 20):
            m = model(S)
            for dt in (np.float64, np.float32):
                x1, x2, codes, tv = make_sides(S, dt, "dense", n, seed=S)
                st, buf = gpu_sumtab(c, S, dt, x1, x2, codes, tv, n)
                wgt = np.random.default_rng(S).integers(1, 4, n).astype(np.int32)
                out = torch.zeros(3, dtype=torch.float64, device="cuda")
                site = torch.zeros(n, dtype=torch.float64, device="cuda")
                c.edge_derivatives(st, n, dev(m["e"]), dev(m["rates"]), dev(np.array([0.2])), out, wgt=dev(wgt),
                                   site_lnl=site, states=S)
                torch.cuda.synchronize()
                ref_st = ref_sumtab(x1, x2)
                assert np.array_equal(bits(st.cpu().numpy()), bits(ref_st.ravel()))
                ref, scale, ref_site = ref_edge(ref_st, m, 0.2, None, wgt)
                check_out(out.cpu().numpy(), ref, scale, f"S={S} {np.dtype(dt).name} one block")
                assert np.all(np.abs(site.cpu().numpy() - ref_site) <= LNL_RTOL * np.maximum(1.0, np.abs(ref_site)))


# ---- the pulley: an 8-taxon GTR + Gamma4 tree whose root's children are A, B ----

PULLEY_T = 0.5  # the simulated length of the branch A - B


@pytest.fixture(scope="module")
def pulley(ctx, oracle):
    """The subtrees' CLVs A, B (coded tips, EIGEN convention, f64) and
    everything the two paths to the lnL over the branch A - B need."""
    import torch

    S, n, ntips = 4, 1000, 8
    m = model(S)
    rng = np.random.default_rng(88)
    ops = oracle.balanced_tree_ops(ntips)  # ops 0-3: cherries 8-11; 4, 5: A = 12, B = 13; 6: the root 14
    assert ops[6].tolist() == [14, 12, 13, 6]
    blen = rng.random(12) * 0.25 + 0.05
    # sequences evolved from A: B across the pulley, then down both subtrees
    cat = rng.integers(0, 4, n)
    P = lambda t: np.stack([(m["V"] * np.exp(m["lam"] * r * t)) @ m["Vi"] for r in m["rates"]])  # noqa: E731

    def evolve(parent_states, t):
        p = np.clip(P(t)[cat, parent_states], 0, None)
        p /= p.sum(axis=1, keepdims=True)
        return (rng.random(n)[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, S - 1)

    state = {12: rng.choice(S, n, p=m["pi"])}
    state[13] = evolve(state[12], PULLEY_T)
    for j in (5, 4, 3, 2, 1, 0):
        p, c1, c2, _ = ops[j]
        state[c1], state[c2] = evolve(state[p], blen[2 * j]), evolve(state[p], blen[2 * j + 1])
    codes = [(1 << state[k]).astype(np.uint8) for k in range(ntips)]
    for c in codes:
        c[rng.random(n) < 0.03] = 15  # a few gaps
    wgt = rng.integers(1, 4, n).astype(np.int32)

    d = dict(S=S, n=n, m=m, wgt=wgt, eig=dev(m["e"]), rates=dev(m["rates"]), catw=dev(np.full(4, 0.25)),
             wgt_d=dev(wgt), EV=dev(plfx.model_ev(m["e"], S, plfx.PMAT_EIGEN)),
             w=dev(plfx.model_root_weights(m["e"], m["freqs"], plfx.PMAT_EIGEN)))
    pm = torch.empty(12 * 64, dtype=torch.float64, device="cuda")
    ctx.pmatrix(d["eig"], d["rates"], dev(blen), pm, states=S, convention=plfx.PMAT_EIGEN)
    clv = [None] * ntips + [torch.empty(16 * n, dtype=torch.float64, device="cuda") for _ in range(7)]
    d["sums"] = torch.zeros(6, dtype=torch.int64, device="cuda")
    ctx.traverse(ops[:6], clv, pm, d["EV"], n, d["wgt_d"], None, d["sums"],
                 tips=[dev(c) for c in codes] + [None] * 7,
                 tipvec=dev(plfx.model_tip_vectors(m["e"], plfx.PMAT_EIGEN)))
    d["A"], d["B"], d["root"] = clv[12], clv[13], clv[14]
    d["st"] = torch.empty(16 * n, dtype=torch.float64, device="cuda")
    ctx.edge_sumtable(d["B"], d["st"], n, x1=d["A"], states=S)
    torch.cuda.synchronize()
    d["ref_st"] = ref_sumtab(d["A"].cpu().numpy(), d["B"].cpu().numpy()).reshape(n, 4, S)

    def existing_lnl(t):
        """The path that predates the feature: the root's node update with P
        matrices at (0.3 t, 0.7 t), then the root lnL over all seven scaler sums."""
        pr = torch.empty(2 * 64, dtype=torch.float64, device="cuda")
        ctx.pmatrix(d["eig"], d["rates"], dev(np.array([0.3 * t, 0.7 * t])), pr, states=S,
                    convention=plfx.PMAT_EIGEN)
        own = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx.plf_dev(d["A"], d["B"], d["root"], d["EV"], pr[:64], pr[64:], d["wgt_d"], None, own)
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        ctx.root_lnl(d["root"], n, out, catw=d["catw"], freq=d["w"], wgt=d["wgt_d"],
                     scaler_sums=torch.cat([d["sums"], own]))
        torch.cuda.synchronize()
        return float(out.item())

    def edge(t):
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        ctx.edge_derivatives(d["st"], n, d["eig"], d["rates"], dev(np.array([t])), out, catw=d["catw"],
                             wgt=d["wgt_d"], scaler_sums=d["sums"], states=S)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    d["existing_lnl"], d["edge"] = existing_lnl, edge
    return d


@pytest.mark.parametrize("t", [0.1, 0.45, 1.5])
def test_pulley_lnl_and_slope_match_the_existing_path(pulley, t):
    got = pulley["edge"](t)
    lnl = pulley["existing_lnl"](t)
    print(f"t={t}: edge lnL {got[0]!r} existing {lnl!r} rel {abs(got[0] - lnl) / abs(lnl):.2e}")
    assert abs(got[0] - lnl) <= LNL_RTOL * abs(lnl)
    if t != 0.45:  # away from the optimum, where the slope is large
        # central difference of the existing path; its truncation error is
        # ~ h^2 f'''/(6 f') ~ 1e-6 / 3 for f' ~ 1/t: a step-size bound
        h = 1e-3 * t
        fd = (pulley["existing_lnl"](t + h) - pulley["existing_lnl"](t - h)) / (2 * h)
        print(f"t={t}: d1 {got[1]!r} central difference {fd!r} rel {abs(got[1] - fd) / abs(fd):.2e}")
        assert abs(got[1] - fd) <= 1e-5 * abs(fd)


def test_optimize_branch_on_the_pulley(ctx, pulley):
    d = pulley
    m, wgt = d["m"], d["wgt"]
    d1 = lambda t: ref_edge(d["ref_st"], m, t, None, wgt)[0][1]  # noqa: E731
    assert d1(1e-8) > 0 > d1(10.0)
    t_ref = brentq(d1, 1e-8, 10.0, xtol=1e-14, rtol=1e-14)
    res = [ctx.optimize_branch(d["st"], d["n"], d["eig"], d["rates"], t0, 1e-8, 10.0, 64, catw=d["catw"],
                               wgt=d["wgt_d"], states=d["S"]) for t0 in STARTS]
    for t0, (t, lnl, g1, g2, evals) in zip(STARTS, res):
        print(f"start {t0:g}: t {t!r} (numpy optimum {t_ref!r}) lnL {lnl!r} d1 {g1:.3e} d2 {g2:.3e} evals {evals}")
        assert abs(t - t_ref) <= 1e-6 * t_ref
        assert abs(t - res[0][0]) <= 1e-6 * res[0][0]
        assert 1 <= evals <= 64 and g2 < 0
        # the returned terms are those of the returned t
        ref, scale, _ = ref_edge(d["ref_st"], m, t, None, wgt)
        check_out(np.array([lnl, g1, g2]), ref, scale, f"start {t0:g}")
    t, lnl = res[3][0], res[3][1] + float(d["sums"].sum().item()) * LOG_MINLIK
    for tg in np.geomspace(0.02, 5.0, 9):
        other = d["existing_lnl"](float(tg))
        print(f"grid t={tg:.4f}: existing lnL {other!r} <= {lnl!r}")
        assert other <= lnl + LNL_RTOL * abs(lnl)  # the two paths agree to LNL_RTOL


# the refused optimisation below is tried inside a capture, which then ends empty
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_argument_errors_leave_the_context_usable():
    import torch

    S, n, dt = 4, 65, np.float64
    m = model(S)
    x1, x2, codes, tv = make_sides(S, dt, "tip", n, seed=5)
    with plfx.Context(0, lazy_tables=True) as c:
        L, h = c._L, c.h
        eig, rates, t = dev(m["e"]), dev(m["rates"]), dev(np.array([0.2]))
        big = torch.zeros(16 * n * 3 + 8, dtype=torch.float64, device="cuda")
        a, b, st = big[:16 * n], big[16 * n:32 * n], big[32 * n:48 * n]
        a.copy_(dev(x1.ravel()))
        b.copy_(dev(x2.ravel()))
        cd, tvd = dev(codes), dev(tv.ravel())
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        p = lambda x: None if x is None else x.data_ptr()  # noqa: E731

        def sumtable(tip1, x1_, x2_, n_, tipvec, st_):
            return L.plfx_edge_sumtable(h, plfx.F64, S, p(tip1), p(x1_), p(x2_), n_, p(tipvec), p(st_), None)

        def derivs(st_, n_, rates_, ncat, states=S):
            return L.plfx_edge_derivatives(h, plfx.F64, states, p(st_), n_, p(eig), p(rates_), ncat, None, None,
                                           p(t), None, 0, p(out), None, None)

        def optimize(t0, tmin, tmax, ncat=4, stream=None):
            topt = plfx.C.c_double(0.0)
            return L.plfx_edge_optimize(h, plfx.F64, S, p(st), n, p(eig), p(rates), ncat, None, None, t0, tmin,
                                        tmax, 64, plfx.C.byref(topt), None, None, stream)

        INV, UNS = plfx.ERR_INVALID, plfx.ERR_UNSUPPORTED
        assert sumtable(cd, a, b, n, tvd, st) == INV        # both a tip and a CLV on side 1
        assert sumtable(None, None, b, n, tvd, st) == INV   # neither
        assert sumtable(cd, None, b, n, None, st) == INV    # a coded side without tipvec
        assert sumtable(None, big[1:], b, n, None, st) == INV   # x1 not 16-byte aligned
        assert sumtable(None, a, big[1:], n, None, st) == INV   # x2
        assert sumtable(None, a, b, n, None, big[32 * n + 1:]) == INV  # sumtab
        assert sumtable(None, a, b, -1, None, st) == INV
        assert sumtable(None, a, b, n, None, a) == INV      # the table over x1
        assert sumtable(None, a, b, n, None, b) == INV      # over x2
        assert sumtable(None, a, b, n, None, big[32 * n - 2:]) == INV  # sharing 16 bytes with x2
        assert sumtable(None, a, b, n, None, st) == plfx.OK
        assert derivs(st, n, rates, 3) == UNS
        assert derivs(st, n, rates, 5) == UNS
        assert derivs(st, n, rates, 4, states=5) == UNS
        assert derivs(big[32 * n + 1:], n, rates, 4) == INV
        assert derivs(st, -1, rates, 4) == INV
        assert b"ncat" in L.plfx_last_error(h) or b"n < 0" in L.plfx_last_error(h)
        assert optimize(0.5, 1e-8, 10.0, ncat=3) == UNS
        assert optimize(1e-9, 1e-8, 10.0) == INV   # t0 < tmin
        assert optimize(11.0, 1e-8, 10.0) == INV   # t0 > tmax
        assert optimize(0.5, 0.0, 10.0) == INV     # tmin = 0
        assert optimize(0.5, 1.0, 0.1) == INV
        cap = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cap):
            rc = optimize(0.5, 1e-8, 10.0, stream=cap.cuda_stream)
        assert rc == INV and b"captur" in L.plfx_last_error(h)
        del g
        torch.cuda.synchronize()
        # and the context still works
        assert derivs(st, n, rates, 4) == plfx.OK
        torch.cuda.synchronize()
        ref, scale, _ = ref_edge(ref_sumtab(x1, x2), m, 0.2)
        assert np.array_equal(bits(st.cpu().numpy()), bits(ref_sumtab(x1, x2).ravel()))
        check_out(out.cpu().numpy(), ref, scale, "after the refused calls")
        assert optimize(0.5, 1e-8, 10.0) == plfx.OK


def test_captured_graph_replays_to_the_same_bits():
    """Sum table + derivatives captured on a stream whose first use is the
    capture (a pool entry), replayed with the outputs cleared."""
    import torch

    for S in (4, 20):
        n, dt = 257, np.float64
        m = model(S)
        x1, x2, codes, tv = make_sides(S, dt, "tip", n, seed=9)
        with plfx.Context(0, lazy_tables=True) as c:
            args = [dev(x2.ravel()), dev(codes), dev(tv.ravel()), dev(m["e"]), dev(m["rates"]), dev(np.array([0.3])),
                    dev(np.random.default_rng(S).integers(1, 4, n).astype(np.int32))]
            st = torch.zeros(4 * S * n, dtype=torch.float64, device="cuda")
            out = torch.zeros(3, dtype=torch.float64, device="cuda")
            site = torch.zeros(n, dtype=torch.float64, device="cuda")

            def call(stream):
                c.edge_sumtable(args[0], st, n, tip1=args[1], tipvec=args[2], states=S, stream=stream)
                c.edge_derivatives(st, n, args[3], args[4], args[5], out, wgt=args[6], site_lnl=site, states=S,
                                   stream=stream)

            call(None)
            torch.cuda.synchronize()
            first = [t.cpu().numpy().copy() for t in (st, out, site)]
            ref, scale, _ = ref_edge(ref_sumtab(x1, x2), m, 0.3, None, args[6].cpu().numpy())
            check_out(first[1], ref, scale, f"S={S} eager")
            cold = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=cold):
                call(cold)
            for _ in range(3):
                for t in (st, out, site):
                    t.zero_()
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                for t, f in zip((st, out, site), first):
                    assert np.array_equal(bits(t.cpu().numpy()), bits(f))
            del g
            torch.cuda.synchronize()
