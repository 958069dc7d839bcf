"""GPU tests of plfx_branch_sumtables_psr (plfx.h section 13): the outer CLV
W(c) and the sum table of every branch of a per-site-rate tree, and the scaler
count of every branch.

Bit equality: every W, every table and every edge_scale[e] against the
composition the header defines them by -- one-node plf_psr_gen calls, one
edge_sumtable_psr_gen call per table, integer sums in numpy
(tests/branch_ref.py) -- for the fused sibling-pair kernel and for
PLFX_BRANCH_NOFUSE, with guard bytes around every workspace slab and every
clv[] buffer.  State space: lnL, d1, d2 of every branch against
tests/felsenstein_ref.py re-rooted on that branch, and against the root lnL
(the pulley principle).  The model inputs are built with numpy
(test_felsenstein_ref.eigen_sym), so the CPU test at the end of the file can
replay the scaling case with tests/psr_ref.py."""
import functools

import numpy as np
import pytest

import branch_ref as B
import felsenstein_ref as F
import plfx
import psr_prot_ref as PR
import psr_ref
import psr_trees as T
from test_felsenstein_ref import EXCH, FREQS, eigen_sym, psr_rates
from test_gpu_psr import bits, dev, np_dtype, same, tdtype

gpu = pytest.mark.gpu
GUARD = 64        # elements either side of every CLV buffer
PAD, SENT = 256, 0xA5  # bytes either side of the workspace, and what they and every slab's padding hold
TMIN, TMAX = 1e-8, 10.0

TREES = {
    "caterpillar4": lambda: T.caterpillar(4, False),
    "caterpillar4_coded": lambda: T.caterpillar(4, True),
    "balanced8": lambda: T.balanced(8, False),
    "balanced8_coded": lambda: T.balanced(8, True),
    "random13": lambda: T.random_tree(13, False, 5),
    "random13_coded": lambda: T.random_tree(13, True, 11),
    "mixed": lambda: T.mixed(False),
    "mixed_swapped": lambda: T.mixed(True),
    "one_coded_root_child": B.one_coded_root_child,
}


@functools.lru_cache(maxsize=None)
def model(S):
    if S == 4:
        Q, pi = F.gtr_q(EXCH, FREQS)
        table = np.array([[(c >> s) & 1 for s in range(4)] for c in range(16)], np.float64)
    else:
        rng = np.random.default_rng(77)
        Q, pi = F.gtr_q(rng.random(S * (S - 1) // 2) * 2 + 0.05, rng.random(S) + 0.1)
        table = PR.tip_table(np.float64)
    lam, V, Vi = eigen_sym(Q, pi)
    return dict(Q=Q, pi=pi, lam=lam, V=V, Vi=Vi, table=table, w=pi @ V)


def pmatrices(m, rates, blen, dt):
    """[branch][category][state][eigen index], what pmatrix(EIGEN) lays out."""
    x = np.asarray(blen)[:, None, None] * rates[None, :, None] * m["lam"][None, None, :]
    return (m["V"][None, None, :, :] * np.exp(x)[:, :, None, :]).astype(dt).reshape(-1)


@functools.lru_cache(maxsize=None)
def problem(tree, S, dtname, n, ncat, shrink=0, seed=0):
    """Everything a call reads, on the host.  Dense leaves are the expansion of
    their codes times 2^-shrink; some rate_cat bytes are past ncat; wgt in 0..3."""
    dt = np_dtype(dtname)
    ops, nslots, coded = TREES[tree]()
    ops = [tuple(map(int, o)) for o in ops]
    m = model(S)
    rng = np.random.default_rng(7919 * len(ops) + 31 * n + ncat + seed)
    leaves = sorted(set(range(nslots)) - {o[0] for o in ops})
    rates = psr_rates(ncat)
    cat = rng.integers(0, ncat, n).astype(np.uint8)
    cat[3::7] = np.resize(np.array([ncat, ncat + 1, 200, 255], np.uint8), cat[3::7].size)
    blen = rng.random(2 * len(ops)) * 0.25 + 0.05
    if S == 4:
        codes = {s: (1 << rng.integers(0, 4, n)).astype(np.uint8) for s in leaves}
        gap = 15
    else:
        codes = {s: rng.integers(0, 20, n).astype(np.uint8) for s in leaves}
        gap = 23
    for k in codes.values():
        k[rng.random(n) < 0.05] = gap
    tv = (m["table"] @ m["Vi"].T).astype(dt).reshape(-1)
    expand = psr_ref.expand_tips if S == 4 else PR.expand_tips
    dense = {s: (expand(codes[s], dt, tv) * dt(2.0 ** -shrink)).astype(dt) for s in leaves if not coded[s]}
    rp = ops[-1][3]
    return dict(tree=tree, S=S, dt=dt, ops=ops, nslots=nslots, coded=list(coded), leaves=leaves, n=n, ncat=ncat,
                rates=rates, cat=cat, wgt=rng.integers(0, 4, n).astype(np.int32), blen=blen, codes=codes, dense=dense,
                pm=pmatrices(m, rates, blen, dt), root_pm=pmatrices(m, rates, [blen[2 * rp] + blen[2 * rp + 1]], dt),
                EV=np.ascontiguousarray(m["Vi"].T).astype(dt).reshape(-1), tv=tv, m=m)


class Device:
    """The problem on the device after traverse_psr_gen: guarded CLV buffers."""

    def __init__(self, c, p, fma=False):
        import torch

        S, n, td = p["S"], p["n"], tdtype(p["dt"])
        self.p, self.fma = p, fma
        self.bufs, self.clv, self.tips = [], [], []
        for s in range(p["nslots"]):
            if p["coded"][s]:
                self.clv.append(None)
                self.tips.append(dev(p["codes"][s]))
                continue
            buf = torch.full((S * n + 2 * GUARD,), -7.0, dtype=td, device="cuda")
            if s in p["dense"]:
                buf[GUARD:GUARD + S * n] = dev(p["dense"][s])
            self.bufs.append(buf)
            self.clv.append(buf[GUARD:GUARD + S * n])
            self.tips.append(None)
        self.any_coded = any(p["coded"])
        self.opsa = np.array(p["ops"], np.int32).reshape(-1, 4)
        self.pm, self.root_pm, self.EV, self.tv = dev(p["pm"]), dev(p["root_pm"]), dev(p["EV"]), dev(p["tv"])
        self.cat, self.wgt = dev(p["cat"]), dev(p["wgt"])
        self.sums = torch.full((len(p["ops"]),), -1, dtype=torch.int64, device="cuda")
        if n:
            c.traverse_psr_gen(S, self.opsa, self.clv, self.pm, self.EV, n, self.cat, p["ncat"], wgt=self.wgt,
                               scaler_sums=self.sums, tips=self.tips if self.any_coded else None, tipvec=self.tv, fma=fma)
        else:
            self.sums.zero_()
        torch.cuda.synchronize()
        self.snapshot = [b.cpu().numpy().copy() for b in self.bufs]

    def side(self, slot, tip_key, dense_key):
        return {tip_key: self.tips[slot]} if self.p["coded"][slot] else {dense_key: self.clv[slot]}

    def unchanged(self):
        return all(same(b.cpu().numpy(), s) for b, s in zip(self.bufs, self.snapshot))


def compose(c, d):
    """Section 13 by its definition: every W as a one-node plf_psr_gen call,
    every table as an edge_sumtable_psr_gen call.  Returns host arrays
    (W[e] of the non-root edges, table[e]), the W sums and the device tables."""
    import torch

    p = d.p
    S, n, ncat, ops, td = p["S"], p["n"], p["ncat"], p["ops"], tdtype(p["dt"])
    nops, root, M = len(ops), len(ops) - 1, p["ncat"] * p["S"] * p["S"]
    level, up, _ = B.structure(ops)
    mat = lambda b: d.pm[b * M:(b + 1) * M]  # noqa: E731
    new = lambda: torch.zeros(S * n, dtype=td, device="cuda")  # noqa: E731
    W, tab, wsum = {}, {}, torch.zeros(2 * nops, dtype=torch.int64, device="cuda")
    _, a, b, _ = ops[root]
    W[2 * root], W[2 * root + 1] = d.side(b, "tip1", "x1"), d.side(a, "tip1", "x1")
    for j in sorted(range(root), key=lambda j: (level[j], j)):
        r, s = up[j] // 2, up[j] % 2
        pup = d.root_pm if r == root else mat(2 * ops[r][3] + s)
        ch = ops[j][1:3]
        for k in (0, 1):
            e, x3 = 2 * j + k, new()
            nd = dict(x3=x3, left=pup, right=mat(2 * ops[j][3] + 1 - k), scaler_sum=wsum[e:e + 1], **W[up[j]],
                      **d.side(ch[1 - k], "tip2", "x2"))
            c.plf_psr_gen(S, nd, d.EV, n, d.cat, ncat, wgt=d.wgt, tipvec=d.tv, fma=d.fma)
            W[e] = dict(x1=x3)
    for e in range(2 * root):
        tab[e] = new()
        c.edge_sumtable_psr_gen(S, W[e]["x1"], tab[e], n, tipvec=d.tv, **d.side(ops[e // 2][1 + e % 2], "tip1", "x1"))
    if p["coded"][b]:  # the root edge: a coded child is side 1
        a, b = b, a
    tab[2 * root] = tab[2 * root + 1] = new()
    c.edge_sumtable_psr_gen(S, d.clv[b], tab[2 * root], n, tipvec=d.tv, **d.side(a, "tip1", "x1"))
    torch.cuda.synchronize()
    return ({e: W[e]["x1"].cpu().numpy() for e in range(2 * root)}, {e: t.cpu().numpy() for e, t in tab.items()},
            wsum.cpu().numpy(), tab)


def run(c, d, nofuse=False, scale=True, stream=None, ws_buf=None):
    """One call on a sentinel-filled, guarded workspace: (buffer, tables, edge_scale tensor)."""
    import torch

    p = d.p
    nops = len(p["ops"])
    nbytes = plfx.branch_sumtables_psr_workspace(p["dt"], p["S"], nops, p["n"])
    buf = torch.full((nbytes + 2 * PAD,), SENT, dtype=torch.uint8, device="cuda") if ws_buf is None else ws_buf
    es = torch.full((2 * nops,), -5, dtype=torch.int64, device="cuda") if scale else None
    tabs = c.branch_sumtables_psr(p["S"], d.opsa, d.clv, d.pm, d.root_pm, d.EV, p["n"], d.cat, p["ncat"], d.sums,
                                  buf[PAD:PAD + nbytes], wgt=d.wgt, edge_scale=es,
                                  tips=d.tips if d.any_coded else None, tipvec=d.tv, fma=d.fma, nofuse=nofuse,
                                  stream=stream)
    return buf, tabs, es


def check(d, comp, res, nofuse, what):
    """The workspace byte for byte, the returned tables, edge_scale, the guards."""
    import torch

    torch.cuda.synchronize()
    p = d.p
    W, tab, wsum, _ = comp
    buf, tabs, es = res
    ops, S, n, dt = p["ops"], p["S"], p["n"], p["dt"]
    nops, root = len(ops), len(ops) - 1
    cb = S * n * np.dtype(dt).itemsize
    slab = (cb + 255) // 256 * 256
    raw = buf.cpu().numpy()
    assert np.all(raw[:PAD] == SENT) and np.all(raw[-PAD:] == SENT), what
    ws = raw[PAD:-PAD]
    level, up, _ = B.structure(ops)
    for e in range(2 * root):  # the outer CLVs
        j, child = e // 2, ops[e // 2][1 + e % 2]
        wv_coded = up[j] // 2 == root and p["coded"][ops[root][2 - up[j] % 2]]
        fused = S == 4 and not nofuse and not wv_coded
        region = ws[e * slab:(e + 1) * slab]
        if p["coded"][child] and fused:
            assert np.all(region == SENT), (what, e, "a coded child's W is never written by the fused kernel")
        else:
            assert same(region[:cb].view(dt), W[e]), (what, "W", e)
            assert np.all(region[cb:] == SENT), (what, "padding of W", e)
    t0 = 2 * root * slab
    for e in range(2 * nops):  # the tables
        k = min(e, 2 * root)
        region = ws[t0 + k * slab:t0 + (k + 1) * slab]
        assert same(region[:cb].view(dt), tab[e]), (what, "table", e)
        assert np.all(region[cb:] == SENT), (what, "padding of table", e)
        assert same(tabs[e].cpu().numpy(), tab[e]) and tabs[e].data_ptr() == buf.data_ptr() + PAD + t0 + k * slab
    assert tabs[2 * root].data_ptr() == tabs[2 * root + 1].data_ptr()
    c0 = t0 + (2 * nops - 1) * slab
    assert np.all(ws[c0 + 5 * nops * 8:] == SENT), (what, "padding of the counters")
    if es is not None:
        got_wsum = ws[c0:c0 + 2 * root * 8].view(np.int64)
        assert got_wsum.tolist() == wsum[:2 * root].tolist(), (what, "W sums")
        want = B.edge_scale(ops, d.sums.cpu().numpy(), wsum)
        assert es.cpu().numpy().tolist() == want.tolist(), (what, "edge_scale")
        assert want[2 * root] == want[2 * root + 1]
    assert d.unchanged(), (what, "a clv[] buffer or its guards changed")


def sizes(dt):
    return (1, 63, 64, 65, 256 * plfx.branch_pair_sites_per_lane(dt) + 1, 5000)


@gpu
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("tree", sorted(TREES))
def test_every_w_table_and_count_is_the_composition(ctx, tree, dt):
    """n over the one-site case, the tail of a trip and more than one block,
    ncat 1 / 25 / 32 rotated against n from tree to tree so that every pair
    occurs; fused and PLFX_BRANCH_NOFUSE against one composition."""
    ns = sizes(np_dtype(dt))
    assert ns[4] in (513, 1025)
    rot = sorted(TREES).index(tree)
    for i, n in enumerate(ns):
        ncat = (1, 25, 32)[(i + rot) % 3]
        p = problem(tree, 4, dt, n, ncat)
        assert (p["cat"] >= ncat).any() or n < 4
        d = Device(ctx, p)
        comp = compose(ctx, d)
        for nofuse in (False, True):
            check(d, comp, run(ctx, d, nofuse), nofuse, f"{tree} {dt} n={n} ncat={ncat} nofuse={nofuse}")
        check(d, comp, run(ctx, d, False, scale=False), False, f"{tree} {dt} n={n} no edge_scale")


@functools.lru_cache(maxsize=None)
def restated_w_sums(tree, dtname, n, ncat, shrink):
    """The traversal and every W with tests/psr_ref.py: (scaler sums, W sums)."""
    p = problem(tree, 4, dtname, n, ncat, shrink)
    ops, M = p["ops"], p["ncat"] * 16
    root = len(ops) - 1
    vals = {s: p["dense"][s] if s in p["dense"] else psr_ref.expand_tips(p["codes"][s], p["dt"], p["tv"])
            for s in p["leaves"]}
    mat = lambda b: p["pm"][b * M:(b + 1) * M]  # noqa: E731
    sums = []
    for par, a, b, m in ops:
        vals[par], _, inc = psr_ref.node(vals[a], vals[b], p["EV"], mat(2 * m), mat(2 * m + 1), p["cat"], ncat, p["wgt"])
        sums.append(inc)
    level, up, _ = B.structure(ops)
    W, wsum = {2 * root: vals[ops[root][2]], 2 * root + 1: vals[ops[root][1]]}, [0] * (2 * len(ops))
    for j in sorted(range(root), key=lambda j: (level[j], j)):
        r, s = up[j] // 2, up[j] % 2
        pup = p["root_pm"] if r == root else mat(2 * ops[r][3] + s)
        for k in (0, 1):
            W[2 * j + k], _, wsum[2 * j + k] = psr_ref.node(W[up[j]], vals[ops[j][2 - k]], p["EV"], pup,
                                                           mat(2 * ops[j][3] + 1 - k), p["cat"], ncat, p["wgt"])
    return sums, wsum


SCALING = [("balanced8", "f64"), ("random13", "f32"), ("mixed", "f64")]


@gpu
@pytest.mark.parametrize("tree,dt", SCALING)
def test_outer_clvs_rescale_and_the_counts_are_exact(ctx, tree, dt):
    """Dense leaves times 2^-20: the outer CLVs rescale.  The W sums and the
    traversal's sums are the psr_ref restatement's, edge_scale the integer sums."""
    n, ncat = 257, 25
    p = problem(tree, 4, dt, n, ncat, 20)
    sums, wsum = restated_w_sums(tree, dt, n, ncat, 20)
    assert any(wsum), "the inputs do not make a W rescale: change them"
    d = Device(ctx, p)
    assert d.sums.cpu().numpy().tolist() == sums
    comp = compose(ctx, d)
    assert comp[2].tolist() == wsum
    for nofuse in (False, True):
        res = run(ctx, d, nofuse)
        check(d, comp, res, nofuse, f"{tree} {dt} scaled nofuse={nofuse}")
        assert res[2].cpu().numpy().tolist() == B.edge_scale(p["ops"], sums, wsum).tolist()


@gpu
@pytest.mark.parametrize("dt,fma", [("f64", False), ("f64", True), ("f32", False)])
@pytest.mark.parametrize("tree", ["caterpillar4_coded", "random13", "random13_coded"])
def test_twenty_states_run_unfused(ctx, tree, dt, fma):
    for n in (1, 65, 1000):
        p = problem(tree, 20, dt, n, 25)
        d = Device(ctx, p, fma)
        comp = compose(ctx, d)
        for nofuse in (False, True):
            check(d, comp, run(ctx, d, nofuse), True, f"{tree} {dt} S=20 n={n} fma={fma} nofuse={nofuse}")


@gpu
@pytest.mark.parametrize("S,tree,n", [(4, "random13_coded", 257), (4, "balanced8", 65), (20, "caterpillar4_coded", 40),
                                      (20, "random13_coded", 24)])
def test_every_branch_against_the_state_space_reference(ctx, S, tree, n):
    """f64.  For every edge k of the unrooted tree: felsenstein_ref re-rooted on
    k -> prune -> edge at the edge's length; branch_derivatives_psr's lnL, d1,
    d2 within LNL_RTOL * scale, and every edge's lnL within LNL_RTOL * |lnL| of
    root_lnl_psr_gen (the pulley principle)."""
    import torch

    from test_gpu_likelihood_ref import LNL_RTOL

    ncat = 25
    p = problem(tree, S, "f64", n, ncat)
    m, ops = p["m"], p["ops"]
    nops, root, ntips = len(ops), len(ops) - 1, len(p["leaves"])
    assert p["leaves"] == list(range(ntips))
    d = Device(ctx, p)
    nbytes = plfx.branch_sumtables_psr_workspace(np.float64, S, nops, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    lam = dev(m["lam"])
    lnl, d1, d2 = ctx.branch_derivatives_psr(S, d.opsa, d.clv, d.pm, d.root_pm, d.EV, n, d.cat, ncat, d.sums, ws, lam,
                                             dev(p["rates"]), p["blen"], wgt=d.wgt,
                                             tips=d.tips if d.any_coded else None, tipvec=d.tv, tmin=TMIN, tmax=TMAX)
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    ctx.root_lnl_psr_gen(S, d.clv[ops[root][0]], n, out, freq=dev(m["w"]), wgt=d.wgt, scaler_sums=d.sums)
    torch.cuda.synchronize()
    got = np.stack([x.cpu().numpy() for x in (lnl, d1, d2)], axis=1)
    root_lnl = float(out.item())
    sr = F.site_rates_psr(p["rates"], p["cat"])
    tips = {s: (m["table"][np.minimum(p["codes"][s], m["table"].shape[0] - 1) if S == 20 else p["codes"][s] & 15])
            for s in p["leaves"]}
    edges = F.unroot(ops, p["blen"])
    worst = np.zeros(3)
    for k in range(len(edges)):
        rops, rblen = F.root_on_edge(edges, ntips, k, 0.3)
        clv = F.prune(m["Q"], rops[:-1], rblen, tips, sr)
        _, a, b, _ = rops[-1]
        ref, scale, _ = F.edge(clv[a][0], clv[a][1], clv[b][0], clv[b][1], m["Q"], m["pi"], sr, None, edges[k][2],
                               p["wgt"])
        for e in ((2 * root, 2 * root + 1) if k == 0 else (k - 1,)):
            for q in range(3):
                worst[q] = max(worst[q], abs(got[e, q] - ref[q]) / scale[q])
                assert abs(got[e, q] - ref[q]) <= LNL_RTOL * scale[q], (tree, S, "edge", e, ("lnL", "d1", "d2")[q])
            assert abs(got[e, 0] - root_lnl) <= LNL_RTOL * abs(got[e, 0]), (tree, S, "pulley", e)
    print(f"S={S} {tree}: largest |gpu - ref| / scale: lnL {worst[0]:.2e} d1 {worst[1]:.2e} d2 {worst[2]:.2e}; "
          f"pulley spread {np.ptp(got[:, 0]) / abs(root_lnl):.2e}")


@gpu
def test_two_runs_and_a_graph_replay_are_the_eager_bits():
    import torch

    p = problem("random13_coded", 4, "f64", 1025, 25, 20)
    with plfx.Context(0, lazy_tables=True) as c:
        d = Device(c, p)
        first = run(c, d)
        torch.cuda.synchronize()
        raw, es = first[0].cpu().numpy().copy(), first[2].cpu().numpy().copy()
        again = run(c, d)
        torch.cuda.synchronize()
        assert np.array_equal(again[0].cpu().numpy(), raw) and np.array_equal(again[2].cpu().numpy(), es)
        cold = torch.cuda.Stream()
        buf = torch.full_like(first[0], SENT)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cold):
            _, _, ges = run(c, d, stream=cold, ws_buf=buf)
        for _ in range(2):
            buf.fill_(SENT)
            ges.fill_(-5)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(buf.cpu().numpy(), raw) and np.array_equal(ges.cpu().numpy(), es)
        del g
        torch.cuda.synchronize()


@gpu
def test_no_sites_launch_nothing_and_zero_edge_scale(ctx):
    import torch

    p = problem("balanced8_coded", 4, "f64", 0, 25)
    d = Device(ctx, p)
    buf, tabs, es = run(ctx, d)
    torch.cuda.synchronize()
    assert np.all(buf.cpu().numpy() == SENT)
    assert es.cpu().numpy().tolist() == [0] * (2 * len(p["ops"]))
    assert len(tabs) == 2 * len(p["ops"]) and all(t.numel() == 0 for t in tabs)


@gpu
def test_refusals_launch_nothing():
    """Outputs pre-filled with a sentinel stay as they were."""
    import torch

    p = problem("caterpillar4_coded", 4, "f64", 65, 25)
    with plfx.Context(0, lazy_tables=True) as c:
        d = Device(c, p)
        nops = len(p["ops"])
        nbytes = plfx.branch_sumtables_psr_workspace(np.float64, 4, nops, 65)
        assert plfx.branch_sumtables_psr_workspace(np.float64, 20, nops, 65) > nbytes
        buf = torch.full((nbytes + 2 * PAD,), SENT, dtype=torch.uint8, device="cuda")
        es = torch.full((2 * nops,), -5, dtype=torch.int64, device="cuda")
        ws = buf[PAD:PAD + nbytes]

        def call(ops=d.opsa, clv=d.clv, tips=d.tips, ws_=ws, S=4, pm=d.pm, EV=d.EV, tv=d.tv, n=65, ncat=25, sums=d.sums,
                 root_pm=d.root_pm):
            with pytest.raises(plfx.PlfxError) as ei:
                c.branch_sumtables_psr(S, ops, clv, pm, root_pm, EV, n, d.cat, ncat, sums, ws_, wgt=d.wgt, edge_scale=es,
                                       tips=tips, tipvec=tv)
            assert ei.value.code == plfx.ERR_INVALID, str(ei.value)

        both = np.array([[2, 0, 1, 0]], np.int32)  # the root op's two children coded
        call(ops=both, clv=d.clv[:3], tips=d.tips[:2] + [None])
        twice = d.opsa.copy()
        twice[2, 2] = twice[1, 2]  # the root op reads a slot op 1 has read
        call(ops=twice)
        call(ops=np.array([[4, 0, 1, 0], [5, 2, 3, 1]], np.int32))  # a forest: op 0's parent is never read
        call(ws_=buf[PAD:PAD + nbytes - 1])                    # one byte short
        call(ws_=buf[PAD + 128:PAD + 128 + nbytes])            # misaligned
        call(tv=None)                                          # coded tips without the eigen table
        call(ncat=0, pm=d.pm), call(ncat=33)
        call(sums=None)                                        # edge_scale without scaler_sums
        wide = [None if t is None else torch.zeros(20 * 65, dtype=torch.float64, device="cuda") for t in d.clv]
        EV20 = torch.zeros(400, dtype=torch.float64, device="cuda")
        pm20 = torch.zeros(2 * nops * 25 * 400, dtype=torch.float64, device="cuda")
        tv20 = torch.zeros(24 * 20, dtype=torch.float64, device="cuda")
        call(S=20, clv=wide, EV=EV20, pm=pm20, root_pm=pm20, tv=tv20)  # a 4-state workspace used for 20 states
        L = c._L
        tabs = (plfx.C.c_void_p * (2 * nops))(*([0xDEAD] * (2 * nops)))
        top = (plfx.TravOp * nops)(*[plfx.TravOp(*map(int, r)) for r in d.opsa])
        slots = (plfx.C.c_void_p * p["nslots"])(*[None if t is None else t.data_ptr() for t in d.clv])
        tp = (plfx.C.c_void_p * p["nslots"])(*[None if t is None else t.data_ptr() for t in d.tips])
        rc = L.plfx_branch_sumtables_psr(c.h, plfx.F64, 4, 2, top, nops, slots, tp, p["nslots"], d.pm.data_ptr(), nops,
                                         d.root_pm.data_ptr(), d.EV.data_ptr(), 65, d.cat.data_ptr(), 25, None,
                                         d.sums.data_ptr(), d.tv.data_ptr(), ws.data_ptr(), nbytes, tabs, es.data_ptr(),
                                         None)
        assert rc == plfx.ERR_INVALID and list(tabs) == [0xDEAD] * (2 * nops)  # PLFX_VALU is no flag of this call
        torch.cuda.synchronize()
        assert np.all(buf.cpu().numpy() == SENT) and np.all(es.cpu().numpy() == -5)
        assert d.unchanged()
        res = run(c, d)  # the context is usable
        check(d, compose(c, d), res, False, "after the refusals")


@gpu
def test_tables_feed_the_device_newton_to_the_same_optima(ctx):
    """sumtabs handed to optimize_branches_psr_gen(max_evals=64): every edge's
    t_opt is what the same call returns on the composition's tables."""
    import torch

    p = problem("random13_coded", 4, "f64", 257, 25)
    d = Device(ctx, p)
    comp = compose(ctx, d)
    _, tabs, _ = run(ctx, d)
    nedges = 2 * len(p["ops"])
    lam, rates = dev(p["m"]["lam"]), dev(p["rates"])
    t0 = dev(np.full(nedges, 0.1))
    got, want = (torch.zeros(nedges, dtype=torch.float64, device="cuda") for _ in range(2))
    ctx.optimize_branches_psr_gen(4, tabs, 257, lam, rates, d.cat, t0, got, TMIN, TMAX, 64, wgt=d.wgt)
    ctx.optimize_branches_psr_gen(4, [comp[3][e] for e in range(nedges)], 257, lam, rates, d.cat, t0, want, TMIN, TMAX,
                                  64, wgt=d.wgt)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))
    assert np.all((got.cpu().numpy() >= TMIN) & (got.cpu().numpy() <= TMAX))


@pytest.mark.parametrize("tree,dt", SCALING)
def test_scaling_inputs_make_an_outer_clv_rescale_on_the_cpu(tree, dt):
    """The premise of the GPU scaling test, with tests/psr_ref.py alone."""
    sums, wsum = restated_w_sums(tree, dt, 257, 25, 20)
    assert sum(sums) > 0 and any(w > 0 for w in wsum)
    n_scaled = lambda t: sum(restated_w_sums(t, dt, 257, 25, 20)[1])  # noqa: E731
    assert n_scaled(tree) > sum(restated_w_sums(tree, dt, 257, 25, 0)[1])  # the 2^-20 is what adds rescales
