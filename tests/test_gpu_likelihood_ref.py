"""GPU tests of whole likelihood pipelines against tests/felsenstein_ref.py, a
state-space reference that shares nothing with the library (no eigen
decomposition: scipy.linalg.expm, derivatives through r Q P and r^2 Q^2 P,
scaling as a separate log term; tests/test_felsenstein_ref.py checks it against
closed forms on the CPU).  The other GPU tests pin every kernel bit for bit to
a numpy restatement of its own arithmetic; these check that the pieces, put
together the way plfx.h and the wrappers document -- model_eigen -> pmatrix ->
traverse_psr -> root_lnl_psr, sum table -> edge derivatives -> optimum --
compute the likelihood the model defines.

Tolerance rule, used throughout.  ref: the reference's value; rest: the numpy
restatement's value on the inputs the device kernels read (the device's own P
matrices, the library's EV and tip table, in the dtype), computed here on the
CPU; scale: the quantity's scale (|ref| for the lnL, the sums of the absolute
per-site terms for d1 and d2, as tests/test_gpu_edge.py).
  f64: |gpu - ref| <= LNL_RTOL * scale, the project's bar.
  f32: |gpu - ref| <= |rest - ref| + LNL_RTOL * scale: the GPU's CLVs and sum
       tables are the restatement's bits and its f64 sums are held to LNL_RTOL
       of the restatement's, so this follows from the existing bars.  So that
       the f32 bound cannot grow until it hides a failure, |rest - ref| is first
       held to 1e-5 * scale (lnL) and 1e-2 * scale (d1, d2).
Every test prints the deviations it measured."""
import functools

import numpy as np
import pytest
from scipy.optimize import brentq

import felsenstein_ref as F
import plfx
import psr_ref
import psr_trees as T
import test_gpu_edge as GE
from test_felsenstein_ref import (EDGE_T, F32_D_CAP, F32_LNL_CAP, TREES, jc69_pair, psr_problem, psr_rates,
                                  psr_reference, reference_edge, restate, restated_edge, restated_lnl)
from test_gpu_psr import dev, np_dtype, tdtype

pytestmark = pytest.mark.gpu

LNL_RTOL = 1e-10
LOG_MINLIK = psr_ref.LOG_MINLIK
TMIN, TMAX = 1e-8, 10.0


@pytest.fixture(scope="module")
def fctx():
    """A context that fuses the level pairs of a PSR traversal (PLFX_FUSE=1 is
    read when the context is created)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PLFX_FUSE", "1")
        c = plfx.Context(0, lazy_tables=True)
    yield c
    c.close()


def within(got, ref, rest, scale, dt, cap, what):
    """The tolerance rule for one quantity."""
    err, margin = abs(got - ref), abs(rest - ref)
    s = scale if scale else 1.0
    print(f"{what}: gpu {got!r} ref {ref!r} |gpu - ref| / scale {err / s:.2e}, |rest - ref| / scale {margin / s:.2e}")
    if np.dtype(dt) == np.float64:
        assert err <= LNL_RTOL * scale, what
    else:
        assert margin <= cap * scale, (what, "the restatement itself misses the cap: change the input")
        assert err <= margin + LNL_RTOL * scale, what


def one_ulp_f32(a, b):
    """a (f32) is within one f32 ulp of the f64 array b cast to f32."""
    b = b.astype(np.float32)
    return np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64))


# ---- pmatrix at the category counts PSR uses ----

@functools.lru_cache(maxsize=None)
def pmat_model(S):
    rng = np.random.default_rng(300 + S)
    exch = rng.random(S * (S - 1) // 2) * 2 + 0.05
    freqs = rng.random(S) + 0.1
    Q, pi = F.gtr_q(exch, freqs)
    return exch, freqs, Q, pi, plfx.model_eigen(exch, freqs)


@pytest.mark.parametrize("conv", [plfx.PMAT_STATE, plfx.PMAT_EIGEN], ids=["state", "eigen"])
@pytest.mark.parametrize("ncat", [1, 7, 25, 32])
@pytest.mark.parametrize("S", [4, 20])
def test_pmatrix_category_counts_vs_expm(ctx, S, ncat, conv):
    """out[b][c] for ncat rates from 1e-3 to 8 is expm(Q r_c t_b) (STATE), or
    composes with the library's EV to it (EIGEN: the eigenvector basis drops
    out), and the f32 output is the f64 output cast: bit for bit (EIGEN), within
    one f32 ulp (STATE, whose S-term sum the two instantiations may round
    differently)."""
    import torch

    exch, freqs, Q, pi, e = pmat_model(S)
    rates = np.ones(1) if ncat == 1 else np.geomspace(1e-3, 8.0, ncat)
    blen = np.array([0.0, 1e-8, 0.1, 2.0, 10.0])
    out = {}
    for td in (torch.float64, torch.float32):
        out[td] = torch.full((blen.size * ncat * S * S + 64,), -7.0, dtype=td, device="cuda")
        ctx.pmatrix(dev(e), dev(rates), dev(blen), out[td][:blen.size * ncat * S * S], states=S, convention=conv)
    torch.cuda.synchronize()
    g64, g32 = (out[td].cpu().numpy() for td in (torch.float64, torch.float32))
    assert np.all(g64[-64:] == -7.0) and np.all(g32[-64:] == -7.0)  # nothing written past the last matrix
    g64, g32 = g64[:-64], g32[:-64]
    got = g64.reshape(blen.size, ncat, S, S)
    if conv == plfx.PMAT_EIGEN:
        ev = plfx.model_ev(e, S, plfx.PMAT_EIGEN).reshape(S, S)
        got = np.einsum("bckl,ml->bckm", got, ev)
    worst = 0.0
    for b, t in enumerate(blen):
        for c, r in enumerate(rates):
            worst = max(worst, np.abs(got[b, c] - F.transition(Q, r, t)).max())
    print(f"S={S} ncat={ncat} conv={conv}: largest |P - expm| {worst:.2e}")
    assert worst < 1e-12
    if conv == plfx.PMAT_EIGEN:
        assert np.array_equal(g32.view(np.uint32), g64.astype(np.float32).view(np.uint32))
    else:
        assert one_ulp_f32(g32, g64)


# ---- the PSR pipeline ----

def device_psr(c, p, dt, coded=True, nops=None):
    """model_eigen -> pmatrix(EIGEN) -> traverse_psr over the first nops ops of
    the problem p: the device tensors, and on the host what the kernels read."""
    import torch

    td = tdtype(dt)
    ops = p["ops"][:nops]
    n, ncat, ntips = p["n"], p["ncat"], p["ntips"]
    e = plfx.model_eigen(p["exch"], p["freqs"])
    d = dict(e=e, eig=dev(e), rates=dev(p["rates"]), cat=dev(p["cat"]), wgt=dev(p["wgt"]),
             w=plfx.model_root_weights(e, p["freqs"], plfx.PMAT_EIGEN))
    pm = torch.empty(2 * len(p["ops"]) * ncat * 16, dtype=td, device="cuda")
    c.pmatrix(d["eig"], d["rates"], dev(p["blen"]), pm, states=4, convention=plfx.PMAT_EIGEN)
    EV = plfx.model_ev(e, 4, plfx.PMAT_EIGEN).astype(dt)
    tv = plfx.model_tip_vectors(e, plfx.PMAT_EIGEN).astype(dt)
    clv = [torch.empty(4 * n, dtype=td, device="cuda") for _ in range(p["nslots"])]
    tips = None
    if coded:
        tips = [dev(p["codes"][s]) for s in range(ntips)] + [None] * (p["nslots"] - ntips)
        clv[:ntips] = [None] * ntips
    else:
        clv[:ntips] = [dev(psr_ref.expand_tips(p["codes"][s], dt, tv)) for s in range(ntips)]
    sums = torch.full((len(ops),), -1, dtype=torch.int64, device="cuda")
    c.traverse_psr(np.array(ops, np.int32).reshape(-1, 4), clv, pm, dev(EV), n, d["cat"], ncat, wgt=d["wgt"],
                   scaler_sums=sums, tips=tips, tipvec=dev(tv) if coded else None)
    torch.cuda.synchronize()
    d.update(clv=clv, tips=tips, sums=sums, pm=pm.cpu().numpy(), EV=EV, tv=tv, tvd=dev(tv))
    return d


PIPELINE = [  # dtype, ncat, tree, n, coded tips, fused context
    ("f32", 7, "caterpillar 48", 257, True, True),
    ("f64", 32, "caterpillar 48", 65, True, False),
    ("f64", 7, "caterpillar 48", 65, False, True),
    ("f64", 1, "balanced 16", 257, False, True),
    ("f32", 32, "balanced 16", 65, True, False),
    ("f64", 7, "random 24", 257, True, True),
    ("f32", 1, "random 24", 65, False, False),
    ("f32", 32, "random 24", 257, True, True),
]


@pytest.mark.parametrize("dt,ncat,tree,n,coded,fused", PIPELINE)
def test_psr_pipeline_lnl(ctx, fctx, dt, ncat, tree, n, coded, fused):
    """Random tip codes with 5 % gaps, rate_cat with values past ncat: the root
    lnL of the device pipeline is the reference's prune + root_lnl."""
    import torch

    dt = np_dtype(dt)
    c = fctx if fused else ctx
    p = psr_problem(tree, n, ncat)
    assert (p["cat"] >= ncat).sum() >= 4  # the clamp is exercised
    _, ref = psr_reference(tree, n, ncat)
    d = device_psr(c, p, dt, coded)
    if fused:
        assert c.last_schedule()["triples"] == T.expected_schedule(TREES[tree]())[0]
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    root = p["ops"][-1][0]
    c.root_lnl_psr(d["clv"][root], n, out, freq=dev(d["w"]), wgt=d["wgt"], scaler_sums=d["sums"])
    torch.cuda.synchronize()
    vals, scs, sums = restate(p, dt, d["pm"], d["EV"], d["tv"])
    assert d["sums"].cpu().numpy().tolist() == sums  # the premise of the f32 bound: the restatement's scaling
    per_site = np.sum(scs, axis=0)
    print(f"rescales per site {per_site.min()}..{per_site.max()}, scaler sums total {sum(sums)}")
    assert sum(sums) > 0
    if tree == "caterpillar 48":
        assert per_site.max() >= 4
    within(float(out.item()), ref, restated_lnl(p, vals, sums, d["w"]), abs(ref), dt, F32_LNL_CAP,
           f"{tree} n={n} ncat={ncat} {np.dtype(dt).name} coded={coded} fused={fused} lnL")


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ncat", [1, 25])
@pytest.mark.parametrize("tree", ["balanced 16", "random 24"])
def test_psr_root_branch_derivatives_and_optimum(fctx, tree, ncat, dt):
    """Sequences simulated down the tree with the root's children 0.5 apart.  A,
    B: the root's children from traverse_psr over all ops but the last; lnL
    (with the scaler sums), d1, d2 of the branch between them against the
    reference's edge, and both optimisers against brentq on the reference's d1."""
    import torch

    dt = np_dtype(dt)
    n = 257
    p = psr_problem(tree, n, ncat, 0, True)
    clv, _ = psr_reference(tree, n, ncat, 0, True)
    nops = len(p["ops"])
    d = device_psr(fctx, p, dt, True, nops - 1)
    _, a, b, _ = p["ops"][-1]
    side = lambda s: d["clv"][s] if s >= p["ntips"] else dev(psr_ref.expand_tips(p["codes"][s], dt, d["tv"]))  # noqa: E731
    st = torch.empty(4 * n, dtype=tdtype(dt), device="cuda")
    fctx.edge_sumtables_psr([dict(x1=side(a), x2=side(b), sumtab=st)], n)
    vals, _, sums = restate(p, dt, d["pm"], d["EV"], d["tv"], nops - 1)
    assert d["sums"].cpu().numpy().tolist() == sums
    lam = d["e"][:4]
    name = f"{tree} ncat={ncat} {np.dtype(dt).name}"
    for t in EDGE_T:
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        fctx.edge_derivatives_psr(st, n, d["eig"], d["rates"], d["cat"], dev(np.array([t])), out, wgt=d["wgt"],
                                  scaler_sums=d["sums"])
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        ref, scale = reference_edge(p, clv, t)
        rest = restated_edge(p, vals, sums, lam, t)
        for j, (q, cap) in enumerate((("lnL", F32_LNL_CAP), ("d1", F32_D_CAP), ("d2", F32_D_CAP))):
            within(got[j], ref[j], rest[j], scale[j], dt, cap, f"{name} t={t} {q}")
    d1 = lambda t: reference_edge(p, clv, t)[0][1]  # noqa: E731
    assert d1(TMIN) > 0 > d1(TMAX)
    t_ref = brentq(d1, TMIN, TMAX, xtol=1e-14, rtol=1e-14)
    for t0 in (0.01, 3.0):
        t_opt = torch.zeros(1, dtype=torch.float64, device="cuda")
        fctx.optimize_branches_psr([st], n, d["eig"], d["rates"], d["cat"], dev(np.array([t0])), t_opt, TMIN, TMAX, 64,
                                   wgt=d["wgt"])
        torch.cuda.synchronize()
        host = fctx.optimize_branch_psr(st, n, d["eig"], d["rates"], d["cat"], t0, TMIN, TMAX, 64, wgt=d["wgt"])[0]
        td = float(t_opt.item())
        print(f"{name} start {t0:g}: device loop {td!r} host loop {host!r} brentq on the reference {t_ref!r} "
              f"rel {abs(td - t_ref) / t_ref:.2e} {abs(host - t_ref) / t_ref:.2e}")
        assert abs(td - t_ref) <= 1e-6 * t_ref
        assert abs(host - t_ref) <= 1e-6 * t_ref


def test_psr_jc69_distance_closed_form(ctx):
    """Two coded tips under JC69, one category of rate 1: both optimisers
    return the Jukes-Cantor distance -3/4 ln(1 - 4p/3) of the share p of
    differing sites, and tmin for identical sequences."""
    import torch

    _, _, xa, xb, ns, nd = jc69_pair(n=257, nd=41, seed=2)
    n = ns + nd
    e = plfx.model_eigen(np.ones(6), np.full(4, 0.25))
    tv = plfx.model_tip_vectors(e, plfx.PMAT_EIGEN)
    ca, cb = ((1 << x.argmax(axis=1)).astype(np.uint8) for x in (xa, xb))
    eig, rates, cat = dev(e), dev(np.ones(1)), dev(np.zeros(n, np.uint8))
    want = -0.75 * np.log(1 - 4 * (nd / n) / 3)
    for other, expect in ((cb, want), (ca, TMIN)):
        st = torch.empty(4 * n, dtype=torch.float64, device="cuda")
        ctx.edge_sumtable_psr(dev(psr_ref.expand_tips(other, np.float64, tv)), st, n, tip1=dev(ca), tipvec=dev(tv))
        for t0 in (0.01, 1.0):
            t_opt = torch.zeros(1, dtype=torch.float64, device="cuda")
            ctx.optimize_branches_psr([st], n, eig, rates, cat, dev(np.array([t0])), t_opt, TMIN, TMAX, 64)
            torch.cuda.synchronize()
            host = ctx.optimize_branch_psr(st, n, eig, rates, cat, t0, TMIN, TMAX, 64)[0]
            print(f"start {t0:g}: device loop {float(t_opt.item())!r} host loop {host!r} closed form {expect!r}")
            for got in (float(t_opt.item()), host):
                assert got == TMIN if expect == TMIN else abs(got - expect) <= 1e-6 * expect


# ---- the Gamma edge kernels ----

def state_space_sides(S, dt, side, n, seed):
    """Positive state-space vectors y1, y2 (n, 4, S) and what the device gets:
    x = Vi . y in dt, or for a coded side 1 its codes and the eigen tip table
    (y1 is then the 0/1 table's expansion, x1 the eigen table's)."""
    import oracle

    m = GE.model(S)
    rng = np.random.default_rng(seed)
    eig = lambda y: np.einsum("ks,ncs->nck", m["Vi"], y).astype(dt)  # noqa: E731
    y2 = rng.random((n, 4, S)) * 0.5 + 0.05
    if side == "dense":
        y1 = rng.random((n, 4, S)) * 0.5 + 0.05
        return y1, y2, eig(y1), eig(y2), None, None
    tv = GE.tip_table(S).astype(dt)
    if S == 4:
        codes = oracle.random_tip_codes(rng, n, 0.3)
        codes = np.where((codes & 15) == 0, codes | 15, codes).astype(np.uint8)  # no empty sets
        y1, x1 = oracle.expand_tips(codes, np.float64), oracle.expand_tips(codes, dt, tipvec=tv)
    else:
        codes = oracle.random_protein_codes(rng, n, 0.3)
        y1, x1 = oracle.expand_protein_tips(codes, np.float64), oracle.expand_protein_tips(codes, dt, tipvec=tv)
    return y1.reshape(n, 4, S), y2, x1.reshape(n, 4, S), eig(y2), codes, tv


@pytest.mark.parametrize("side", ["dense", "coded"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("S", [4, 20])
def test_gamma_edge_derivatives_state_space(ctx, S, dt, side):
    """edge_derivatives on Vi . y1, Vi . y2 against the reference's edge on y1,
    y2 themselves: non-uniform category weights, site weights 0 to 3."""
    import torch

    dt = np_dtype(dt)
    n = 257
    m = GE.model(S)
    Q, pi = F.gtr_q(m["exch"], m["freqs"])
    y1, y2, x1, x2, codes, tv = state_space_sides(S, dt, side, n, seed=40 + S)
    wgt = np.random.default_rng(S).integers(0, 4, n).astype(np.int32)
    st, _ = GE.gpu_sumtab(ctx, S, dt, x1, x2, codes, tv, n)
    rest_st = GE.ref_sumtab(x1, x2)
    sr = F.site_rates_gamma(m["rates"], n)
    for t in (1e-8, 0.2, 10.0):
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        ctx.edge_derivatives(st, n, dev(m["e"]), dev(m["rates"]), dev(np.array([t])), out, catw=dev(GE.CATW),
                             wgt=dev(wgt), states=S)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        ref, scale, _ = F.edge(y1, 0.0, y2, 0.0, Q, pi, sr, GE.CATW, t, wgt)
        rest = GE.ref_edge(rest_st, m, t, GE.CATW, wgt)[0]
        for j, (q, cap) in enumerate((("lnL", F32_LNL_CAP), ("d1", F32_D_CAP), ("d2", F32_D_CAP))):
            within(got[j], ref[j], rest[j], scale[j], dt, cap, f"S={S} {np.dtype(dt).name} {side} t={t} {q}")


@pytest.mark.parametrize("S", [4, 20])
def test_gamma_optimum_state_space(ctx, S):
    """Four taxa simulated under the Gamma model with the two cherries 0.5
    apart; the cherries' CLVs come from the reference's prune.  The device loop
    returns the root of the reference's d1."""
    import torch

    n = 257
    m = GE.model(S)
    Q, pi = F.gtr_q(m["exch"], m["freqs"])
    rng = np.random.default_rng(70 + S)
    ops = [(4, 0, 1, 0), (5, 2, 3, 1), (6, 4, 5, 2)]
    blen = rng.random(6) * 0.25 + 0.05
    states = F.simulate(Q, pi, ops, blen, m["rates"][rng.integers(0, 4, n)], rng, 0.5)
    sr = F.site_rates_gamma(m["rates"], n)
    clv = F.prune(Q, ops[:2], blen, {s: np.eye(S)[states[s]] for s in range(4)}, sr)
    wgt = rng.integers(1, 4, n).astype(np.int32)
    d1 = lambda t: F.edge(clv[4][0], clv[4][1], clv[5][0], clv[5][1], Q, pi, sr, None, t, wgt)[0][1]  # noqa: E731
    assert d1(TMIN) > 0 > d1(TMAX)
    t_ref = brentq(d1, TMIN, TMAX, xtol=1e-14, rtol=1e-14)
    x1, x2 = (np.einsum("ks,ncs->nck", m["Vi"], clv[s][0]) for s in (4, 5))
    st, _ = GE.gpu_sumtab(ctx, S, np.float64, x1, x2, None, None, n)
    for t0 in (0.01, 3.0):
        t_opt = torch.zeros(1, dtype=torch.float64, device="cuda")
        ctx.optimize_branches([st], n, dev(m["e"]), dev(m["rates"]), dev(np.array([t0])), t_opt, TMIN, TMAX, 64,
                              wgt=dev(wgt), states=S)
        torch.cuda.synchronize()
        got = float(t_opt.item())
        print(f"S={S} start {t0:g}: device loop {got!r} brentq on the reference {t_ref!r} rel {abs(got - t_ref) / t_ref:.2e}")
        assert abs(got - t_ref) <= 1e-6 * t_ref


# ---- the placement of the root ----

def test_gamma_root_placement_invariance(ctx):
    """One 8-taxon unrooted tree rooted on two of its edges: traverse +
    root_lnl (GTR + Gamma4, f64, coded tips, eigen convention) agree within
    LNL_RTOL and with the reference; the same for traverse_psr + root_lnl_psr."""
    import torch

    n, ntips, ncat = 257, 8, 7
    rng = np.random.default_rng(8)
    tops = [tuple(map(int, o)) for o in T.random_tree(ntips, True, 5)[0]]
    edges = F.unroot(tops, rng.random(2 * len(tops)) * 0.3 + 0.02)
    exch, freqs = np.array([1.2, 3.9, 0.8, 1.1, 4.6, 1.0]), np.array([0.31, 0.19, 0.22, 0.28])
    Q, pi = F.gtr_q(exch, freqs)
    e = plfx.model_eigen(exch, freqs)
    eig, EV = dev(e), dev(plfx.model_ev(e, 4, plfx.PMAT_EIGEN))
    tv = dev(plfx.model_tip_vectors(e, plfx.PMAT_EIGEN))
    w = dev(plfx.model_root_weights(e, freqs, plfx.PMAT_EIGEN))
    codes = [(1 << rng.integers(0, 4, n)).astype(np.uint8) for _ in range(ntips)]
    for cd in codes:
        cd[rng.random(n) < 0.05] = 15
    wgt = rng.integers(1, 4, n).astype(np.int32)
    cat = rng.integers(0, ncat + 2, n).astype(np.uint8)
    grates, prates = plfx.gamma_rates(0.6, 4), psr_rates(ncat)
    tips_ref = {s: F.tip_states(cd) for s, cd in enumerate(codes)}
    tips = [dev(cd) for cd in codes] + [None] * (ntips - 1)
    got = {"gamma": [], "psr": []}
    ref = {"gamma": [], "psr": []}
    for k, frac in ((0, 0.5), (7, 0.3)):
        ops, blen = F.root_on_edge(edges, ntips, k, frac)
        nops = len(ops)
        opsa = np.array(ops, np.int32)
        for kind, V, rates, sr in (("gamma", 16, grates, F.site_rates_gamma(grates, n)),
                                   ("psr", 4, prates, F.site_rates_psr(prates, cat))):
            pm = torch.empty(2 * nops * rates.size * 16, dtype=torch.float64, device="cuda")
            ctx.pmatrix(eig, dev(rates), dev(blen), pm, states=4, convention=plfx.PMAT_EIGEN)
            clv = [None] * ntips + [torch.empty(V * n, dtype=torch.float64, device="cuda") for _ in range(nops)]
            sums = torch.zeros(nops, dtype=torch.int64, device="cuda")
            out = torch.zeros(1, dtype=torch.float64, device="cuda")
            if kind == "gamma":
                ctx.traverse(opsa, clv, pm, EV, n, dev(wgt), None, sums, tips=tips, tipvec=tv)
                ctx.root_lnl(clv[-1], n, out, freq=w, wgt=dev(wgt), scaler_sums=sums)
            else:
                ctx.traverse_psr(opsa, clv, pm, EV, n, dev(cat), ncat, wgt=dev(wgt), scaler_sums=sums, tips=tips, tipvec=tv)
                ctx.root_lnl_psr(clv[-1], n, out, freq=w, wgt=dev(wgt), scaler_sums=sums)
            torch.cuda.synchronize()
            got[kind].append(float(out.item()))
            r = F.prune(Q, ops, blen, tips_ref, sr)[ops[-1][0]]
            ref[kind].append(F.root_lnl(r[0], r[1], pi, None, wgt)[0])
    for kind in ("gamma", "psr"):
        g, r = got[kind], ref[kind]
        print(f"{kind}: rootings {g[0]!r} {g[1]!r} (rel {abs(g[0] - g[1]) / abs(g[0]):.2e}); reference {r[0]!r} {r[1]!r}; "
              f"|gpu - ref| / |ref| {abs(g[0] - r[0]) / abs(r[0]):.2e} {abs(g[1] - r[1]) / abs(r[1]):.2e}")
        assert abs(r[0] - r[1]) <= 1e-12 * abs(r[0])
        assert abs(g[0] - g[1]) <= LNL_RTOL * abs(g[0])
        assert abs(g[0] - r[0]) <= LNL_RTOL * abs(r[0]) and abs(g[1] - r[1]) <= LNL_RTOL * abs(r[1])
