"""CPU tests of tests/felsenstein_ref.py, the state-space reference the GPU
tests of tests/test_gpu_likelihood_ref.py compare against, and of the margin
those tests rest on.

The reference against things known without it: the JC69 closed forms on two
taxa, the invariance of the lnL under the placement of the root (reversibility
and the pulley principle), and its d1, d2 against central differences of its
own lnL.

The numpy restatements (tests/psr_ref.py: node, root_lnl, sumtab, edge -- what
the GPU is pinned to bit for bit) against the reference: composed per op on
eigen-convention matrices built here with np.linalg.eigh of the pi-symmetrised
Q, V^T Pi V = I: P = V exp(lambda r t), EV = Vi^T, tip table = Vi . bits, root
weights = pi V.  f64 is asserted at 1e-12 relative for the lnL and at LNL_RTOL
of scale for d1, d2; f32 is printed and held to the caps the GPU tests use
(1e-5 for the lnL, 1e-2 of scale for d1, d2).  The helpers below (problems,
eigen inputs, the composition) are shared with the GPU tests."""
import functools

import numpy as np
import pytest

import felsenstein_ref as F
import psr_ref
import psr_trees as T

LNL_RTOL = 1e-10
F32_LNL_CAP, F32_D_CAP = 1e-5, 1e-2
EDGE_T = (1e-8, 0.05, 0.5, 3.0, 10.0)
EXCH = np.array([1.2, 3.9, 0.8, 1.1, 4.6, 1.0])
FREQS = np.array([0.31, 0.19, 0.22, 0.28])
TREES = {
    "balanced 16": lambda: T.balanced(16, True),
    "caterpillar 48": lambda: T.caterpillar(48, True),
    "random 24": lambda: T.random_tree(24, True, 3),
}


# ---- shared with tests/test_gpu_likelihood_ref.py ----

def eigen_sym(Q, pi):
    """(lambda, V, Vi) with V^T Pi V = I, from eigh of Pi^1/2 Q Pi^-1/2."""
    s = np.sqrt(pi)
    B = s[:, None] * Q / s[None, :]
    lam, U = np.linalg.eigh((B + B.T) / 2)
    return lam, U / s[:, None], U.T * s[None, :]


def psr_rates(ncat):
    """1 for one category, else 0.1 to 3 (with rates from 0.05 to 4 the f32
    restatement's d2 on the caterpillar at t = 1e-8 misses the 1e-2 cap)."""
    return np.ones(1) if ncat == 1 else np.geomspace(0.1, 3.0, ncat)


@functools.lru_cache(maxsize=None)
def psr_problem(tree, n, ncat, seed=0, simulated=False, t_root=0.5):
    """A per-site-rate problem on a tree of TREES: model, branch lengths,
    categories (a few past ncat: clamped), weights and tip codes -- random with
    5 % gaps, or simulated down the tree (3 % gaps) with the root's children
    t_root apart.  Treat the result as read-only: it is cached."""
    ops, nslots, flags = TREES[tree]()
    ops = [tuple(map(int, o)) for o in ops]
    ntips = sum(flags)
    rng = np.random.default_rng(1000 * n + 10 * ncat + len(ops) + seed)
    Q, pi = F.gtr_q(EXCH, FREQS)
    rates = psr_rates(ncat)
    cat = rng.integers(0, ncat, n).astype(np.uint8)
    cat[3::7] = np.resize(np.array([ncat, ncat + 1, 200, 255], np.uint8), cat[3::7].size)
    blen = rng.random(2 * len(ops)) * 0.25 + 0.05
    sr = F.site_rates_psr(rates, cat)
    if simulated:
        st = F.simulate(Q, pi, ops, blen, sr[:, 0], rng, t_root)
        codes = {s: (1 << st[s]).astype(np.uint8) for s in range(ntips)}
        gaps = 0.03
    else:
        codes = {s: (1 << rng.integers(0, 4, n)).astype(np.uint8) for s in range(ntips)}
        gaps = 0.05
    for c in codes.values():
        c[rng.random(n) < gaps] = 15
    return dict(tree=tree, Q=Q, pi=pi, exch=EXCH, freqs=FREQS, ops=ops, nslots=nslots, ntips=ntips, n=n, ncat=ncat,
                rates=rates, cat=cat, site_rates=sr, blen=blen, wgt=rng.integers(1, 4, n).astype(np.int32), codes=codes)


@functools.lru_cache(maxsize=None)
def psr_reference(tree, n, ncat, seed=0, simulated=False):
    """prune over the whole tree: {slot: (CLV, log scale)}, the root lnL."""
    p = psr_problem(tree, n, ncat, seed, simulated)
    clv = F.prune(p["Q"], p["ops"], p["blen"], {s: F.tip_states(c) for s, c in p["codes"].items()}, p["site_rates"])
    root = clv[p["ops"][-1][0]]
    return clv, F.root_lnl(root[0], root[1], p["pi"], None, p["wgt"])[0]


def eigen_inputs(p, dt):
    """The eigen-convention inputs of the problem, built with numpy alone, in
    dt: pmats as pmatrix() lays them out ([branch][category][k][l]), EV, the
    16 x 4 tip table; and in f64 the eigenvalues and the root weights."""
    lam, V, Vi = eigen_sym(p["Q"], p["pi"])
    x = p["blen"][:, None, None] * p["rates"][None, :, None] * lam[None, None, :]
    pm = V[None, None, :, :] * np.exp(x)[:, :, None, :]
    bits = np.array([[(c >> s) & 1 for s in range(4)] for c in range(16)], np.float64)
    return dict(lam=lam, pmats=pm.astype(dt).reshape(-1), EV=np.ascontiguousarray(Vi.T).astype(dt).reshape(-1),
                tipvec=(bits @ Vi.T).astype(dt).reshape(-1), w=p["pi"] @ V)


def restate(p, dt, pmats, EV, tipvec, nops=None):
    """psr_ref.node composed op by op (the first nops ops) on coded tips
    expanded through `tipvec`: ({slot: values}, [scaler bytes], [weighted sums])."""
    M = p["ncat"] * 16
    vals = {s: psr_ref.expand_tips(c, dt, tipvec) for s, c in p["codes"].items()}
    scs, sums = [], []
    for par, a, b, pm in p["ops"][:nops]:
        left, right = pmats[2 * pm * M:(2 * pm + 1) * M], pmats[(2 * pm + 1) * M:(2 * pm + 2) * M]
        vals[par], sc, inc = psr_ref.node(vals[a], vals[b], EV, left, right, p["cat"], p["ncat"], p["wgt"])
        scs.append(sc)
        sums.append(inc)
    return vals, scs, sums


def restated_lnl(p, vals, sums, w):
    return psr_ref.root_lnl(vals[p["ops"][-1][0]], p["n"], freq=w, wgt=p["wgt"], scaler_sums=np.array(sums))[0]


def reference_edge(p, clv, t):
    """The reference's (out3, scale) over the branch between the root's children."""
    _, a, b, _ = p["ops"][-1]
    out, scale, _ = F.edge(clv[a][0], clv[a][1], clv[b][0], clv[b][1], p["Q"], p["pi"], p["site_rates"], None, t,
                           p["wgt"])
    return out, scale


def restated_edge(p, vals, sums, lam, t):
    """psr_ref.edge over psr_ref.sumtab of the root's children; nsc: their scaler sums."""
    _, a, b, _ = p["ops"][-1]
    out, _, _ = psr_ref.edge(psr_ref.sumtab(vals[a], vals[b]), lam, p["rates"], p["cat"], t, p["wgt"],
                             nsc=int(np.sum(sums[:len(p["ops"]) - 1])))
    return out


# ---- the reference against closed forms ----

def jc69_pair(n=200, nd=37, seed=1):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, n)
    b = a.copy()
    b[:nd] = (a[:nd] + rng.integers(1, 4, nd)) % 4
    Q, pi = F.gtr_q(np.ones(6), np.full(4, 0.25))
    return Q, pi, np.eye(4)[a], np.eye(4)[b], n - nd, nd


def test_jc69_closed_forms():
    Q, pi, xa, xb, ns, nd = jc69_pair()
    n = ns + nd
    sr = np.ones((n, 1))
    lnl_of = lambda t: ns * np.log((1 + 3 * np.exp(-4 * t / 3)) / 16) + nd * np.log((1 - np.exp(-4 * t / 3)) / 16)  # noqa: E731
    for t in (0.01, 0.3, 2.5):
        clv = F.prune(Q, [(2, 0, 1, 0)], np.array([0.3 * t, 0.7 * t]), {0: xa, 1: xb}, sr)
        got = F.root_lnl(clv[2][0], clv[2][1], pi)[0]
        print(f"t={t}: root lnL {got!r} closed form {lnl_of(t)!r}")
        assert abs(got - lnl_of(t)) <= 1e-12 * abs(lnl_of(t))
        out, _, _ = F.edge(xa, 0.0, xb, 0.0, Q, pi, sr, None, t)
        assert abs(out[0] - lnl_of(t)) <= 1e-12 * abs(lnl_of(t))
    p = nd / n
    topt = -0.75 * np.log(1 - 4 * p / 3)
    out, scale, _ = F.edge(xa, 0.0, xb, 0.0, Q, pi, sr, None, topt)
    e = np.exp(-4 * topt / 3)
    a, a1, a2 = (1 + 3 * e) / 16, -e / 4, e / 3          # the likelihood of an equal pair and its derivatives
    b, b1, b2 = (1 - e) / 16, e / 12, -e / 9             # of an unequal pair
    d2 = ns * (a2 / a - (a1 / a) ** 2) + nd * (b2 / b - (b1 / b) ** 2)
    print(f"t* = {topt!r}: d1 {out[1]:.3e} (scale {scale[1]:.3e}) d2 {out[2]!r} closed form {d2!r}")
    assert abs(out[1]) <= 1e-12 * scale[1]
    assert abs(out[2] - d2) <= 1e-12 * abs(d2) and d2 < 0


def test_root_placement_invariance():
    """A 6-taxon tree under GTR with four Gamma-like rates and under per-site
    rates: the lnL is the same wherever the root sits."""
    rng = np.random.default_rng(6)
    n, ntips = 120, 6
    ops, _, _ = T.random_tree(ntips, True, 2)
    ops = [tuple(map(int, o)) for o in ops]
    edges = F.unroot(ops, rng.random(2 * len(ops)) * 0.4 + 0.02)
    Q, pi = F.gtr_q(EXCH, FREQS)
    tips = {s: F.tip_states((1 << rng.integers(0, 4, n)).astype(np.uint8)) for s in range(ntips)}
    wgt = rng.integers(1, 4, n)
    for sr, catw in ((F.site_rates_gamma([0.1, 0.5, 1.0, 2.4], n), np.array([0.1, 0.2, 0.3, 0.4])),
                     (F.site_rates_psr(psr_rates(7), rng.integers(0, 7, n)), None)):
        lnls = []
        for k, frac in ((0, 0.5), (3, 0.2), (len(edges) - 1, 1.0)):
            rops, blen = F.root_on_edge(edges, ntips, k, frac)
            clv = F.prune(Q, rops, blen, tips, sr)
            root = clv[rops[-1][0]]
            lnls.append(F.root_lnl(root[0], root[1], pi, catw, wgt)[0])
        print("rootings:", lnls)
        assert max(lnls) - min(lnls) <= 1e-12 * abs(lnls[0])


def test_edge_derivatives_against_central_differences():
    """d1 against (f(t + h) - f(t - h)) / 2h and d2 against the second difference
    of the reference's own lnL, h = 1e-3 t.  Step-size bound, as
    tests/test_gpu_edge.py states its own: the truncation errors are
    h^2 f''' / 6 and h^2 f'''' / 12, about 1e-6 of the derivative for f^(k) ~
    1 / t^k; the rounding of the differences is 1e-16 |lnL| / h and
    4e-16 |lnL| / h^2, with |lnL| ~ 1e4 and scales of d1, d2 ~ 1e3 / t, 1e3 /
    t^2 at most 1e-6 of the scales too.  Bar: 1e-5 of the scales."""
    p = psr_problem("balanced 16", 257, 7, simulated=True)
    clv, _ = psr_reference("balanced 16", 257, 7, simulated=True)
    f = lambda t: reference_edge(p, clv, t)  # noqa: E731
    for t in (0.05, 0.5, 3.0):
        h = 1e-3 * t
        (o, scale), (lo, _), (hi, _) = f(t), f(t - h), f(t + h)
        fd1, fd2 = (hi[0] - lo[0]) / (2 * h), (hi[0] - 2 * o[0] + lo[0]) / (h * h)
        print(f"t={t}: d1 {o[1]!r} fd {fd1!r} err/scale {abs(o[1] - fd1) / scale[1]:.2e}; "
              f"d2 {o[2]!r} fd {fd2!r} err/scale {abs(o[2] - fd2) / scale[2]:.2e}")
        assert abs(o[1] - fd1) <= 1e-5 * scale[1]
        assert abs(o[2] - fd2) <= 1e-5 * scale[2]


# ---- the restatements against the reference ----

@pytest.mark.parametrize("ncat", [1, 7, 25, 32])
@pytest.mark.parametrize("tree", list(TREES))
def test_restatements_equal_the_reference(tree, ncat):
    n = {"balanced 16": 257, "caterpillar 48": 263, "random 24": 300}[tree]
    p = psr_problem(tree, n, ncat)
    clv, ref = psr_reference(tree, n, ncat)
    for dt in (np.float64, np.float32):
        e = eigen_inputs(p, dt)
        vals, scs, sums = restate(p, dt, e["pmats"], e["EV"], e["tipvec"])
        got = restated_lnl(p, vals, sums, e["w"])
        rel = abs(got - ref) / abs(ref)
        per_site = np.sum(scs, axis=0)
        print(f"{tree} ncat={ncat} {np.dtype(dt).name}: lnL {got!r} reference {ref!r} rel {rel:.2e}; "
              f"rescales per site {per_site.min()}..{per_site.max()}")
        assert rel <= (1e-12 if dt == np.float64 else F32_LNL_CAP)
        worst = [0.0, 0.0]
        for t in EDGE_T:
            out, scale = reference_edge(p, clv, t)
            rest = restated_edge(p, vals, sums, e["lam"], t)
            err = np.abs(rest - out) / scale
            worst = [max(worst[0], err[1]), max(worst[1], err[2])]
            assert err[0] <= (1e-12 if dt == np.float64 else F32_LNL_CAP), (t, err)
            assert np.all(err[1:] <= (LNL_RTOL if dt == np.float64 else F32_D_CAP)), (t, err)
        print(f"{tree} ncat={ncat} {np.dtype(dt).name}: edge d1 {worst[0]:.2e} d2 {worst[1]:.2e} of scale "
              f"(largest over t in {EDGE_T})")
    if tree == "caterpillar 48":
        assert per_site.max() >= 4  # the deep tree rescales a site again and again
