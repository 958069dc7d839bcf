"""GPU tests of plfx.h section 12b: the rate scan with a state count
(plfx_psr_rate_scan_gen), the per-site lnL with per-site scaling
(plfx_site_lnl_psr_gen) and, end to end, the categorisation -- for 20 states,
and for 4 states against section 12's own entry points.

Problems: a random reversible 20-state model per problem, sequences simulated
down three trees under four true rates geomspace(0.1, 3, 4) with branches of
0.1..0.5, 3 % gaps (code 23), scanned over the twelve candidates
geomspace(0.25, 8, 12).  The reference is tests/felsenstein_ref.py, per
candidate r_k: prune + root_lnl with every site at rate r_k (expm, no eigen
code).  The restatement is tests/psr_prot_ref.py composed op by op on the
device's own matrices, plus the per-site rescale counts times log(2^-32).

Measured for these three problems on the CPU (the restatement over numpy
eigen inputs): the f64 restatement is within 9.3e-13 absolute, 2.8e-14 of
max(1, |ref|), of the reference; the f32 one within 5.2e-5 absolute, 1.54e-6
of that scale, under the 1e-5 cap; the smallest gap between a site's best and
second-best reference lnL is 6.1e-3, 4.9e-4 and 7.5e-3, at least nine times the
f32 absolute error; the rescale counts are 0..4, 0..2 and 0..2 and differ
between the candidates at 60 of 65, 165 of 257 and 99 of 130 sites.  With
candidates from 0.05 on, or branches of 0.05..0.3, the f32 restatement misses
the cap (up to 5.7e-5): those inputs are not used.  On the device's own
matrices the figures move a little: the GPU's all_lnl is within 6.2e-14 (f64)
and 1.8e-6 (f32) of max(1, |ref|), the f32 restatement within 6.5e-5 absolute.
The tests assert the premises they rely on (counts > 0, counts varying, the
f32 restatement under the cap) and print what they measure.

Tolerances: f64 |got - ref| <= LNL_RTOL * max(1, |ref|) per entry; f32 the
`within` rule of tests/test_gpu_likelihood_ref.py per entry on that scale with
F32_LNL_CAP -- the rules of tests/test_gpu_psr_rate_scan.py."""
import functools

import numpy as np
import pytest

import felsenstein_ref as F
import plfx
import psr_prot_ref as R
import psr_trees as T
from test_felsenstein_ref import F32_LNL_CAP, LNL_RTOL, psr_problem
from test_gpu_psr import bits, dev, np_dtype, tdtype
from test_gpu_psr_rate_scan import CAND as DNA_CAND
from test_gpu_psr_rate_scan import inputs as dna_inputs
from test_gpu_psr_rate_scan import layout as dna_layout

pytestmark = pytest.mark.gpu

S = 20
CAND = np.geomspace(0.25, 8.0, 12)
TRUE_RATES = np.geomspace(0.1, 3.0, 4)
TREES = {"caterpillar 24": lambda: T.caterpillar(24, True), "random 12": lambda: T.random_tree(12, True, 3),
         "balanced 16": lambda: T.balanced(16, True)}
PROBLEMS = [("caterpillar 24", 65), ("random 12", 257), ("balanced 16", 130)]
LOG_MINLIK = R.LOG_MINLIK
EIGEN = plfx.PMAT_EIGEN
SENTINEL = -7.0
TABLE = R.tip_table(np.float64)


@pytest.fixture(scope="module")
def fctx():
    """A context created under PLFX_FUSE=1 (read at creation): 20 states must not care."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PLFX_FUSE", "1")
        c = plfx.Context(0, lazy_tables=True)
    yield c
    c.close()


# ---- the problems ----

@functools.lru_cache(maxsize=None)
def problem(tree, n):
    """Treat the result as read-only: it is cached."""
    ops, nslots, flags = TREES[tree]()
    ops = [tuple(map(int, o)) for o in ops]
    nops, ntips = len(ops), sum(flags)
    rng = np.random.default_rng(1000 * n + nops)
    exch = rng.random(S * (S - 1) // 2) * 2 + 0.05
    freqs = rng.random(S) + 0.1
    Q, pi = F.gtr_q(exch, freqs)
    true_cat = rng.integers(0, 4, n)
    blen = rng.random(2 * nops) * 0.4 + 0.1
    st = F.simulate(Q, pi, ops, blen, TRUE_RATES[true_cat], rng, 0.5)
    codes = {s: st[s].astype(np.uint8) for s in range(ntips)}
    for c in codes.values():
        c[rng.random(n) < 0.03] = 23
    return dict(tree=tree, Q=Q, pi=pi, exch=exch, freqs=freqs, ops=ops, nslots=nslots, ntips=ntips, n=n,
                true_cat=true_cat, blen=blen, codes=codes, wgt=rng.integers(1, 4, n).astype(np.int32))


def inputs(p, dt, cand=CAND, codes=None):
    """The device tensors of a scan of problem p, and on the host what the kernels read."""
    e = plfx.model_eigen(p["exch"], p["freqs"])
    EV64 = plfx.model_ev(e, S, EIGEN)
    tv = (TABLE @ EV64.reshape(S, S)).astype(dt).reshape(-1)  # tv[code][k] = sum_s table[code][s] * Vi[k][s]
    EV = EV64.astype(dt)
    w = plfx.model_root_weights(e, p["freqs"], EIGEN)
    codes = p["codes"] if codes is None else codes
    return dict(e=e, eig=dev(e), EV=EV, tv=tv, w=w, EVd=dev(EV), tvd=dev(tv), wd=dev(w), blen=dev(p["blen"]),
                cand=dev(np.asarray(cand, np.float64)), ncand=len(cand), wgt=dev(p["wgt"]),
                tips=[dev(codes[s]) for s in range(p["ntips"])] + [None] * (p["nslots"] - p["ntips"]),
                ops=np.array(p["ops"], np.int32).reshape(-1, 4))


def layout(dt, nops, ntips, npmats, n, group, states=S):
    """The workspace's parts as plfx.h section 12b documents them, each array rounded up to 256 bytes."""
    es, vn = np.dtype(dt).itemsize, group * n
    up = lambda v: -(-v // 256) * 256  # noqa: E731
    clv, row = up(vn * states * es), up(vn)
    tip0 = nops * clv
    sc0 = tip0 + ntips * row
    cat0 = sc0 + nops * row
    pm0 = cat0 + row
    return dict(clv=clv, row=row, tip0=tip0, sc0=sc0, cat0=cat0, pm0=pm0,
                end=pm0 + up(2 * npmats * group * states * states * es))


def outputs(n, ncand):
    import torch

    return dict(best_idx=torch.full((n,), -3, dtype=torch.int32, device="cuda"),
                best_lnl=torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda"),
                all_lnl=torch.full((ncand * n,), SENTINEL, dtype=torch.float64, device="cuda"),
                out_lnl=torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda"))


def workspace(p, dt, group, states=S):
    import torch

    nops = len(p["ops"])
    size = plfx.psr_rate_scan_workspace_gen(dt, states, nops, p["ntips"], nops, p["n"], group)
    assert size == layout(dt, nops, p["ntips"], nops, p["n"], group, states)["end"]
    return torch.full((size,), 0xAB, dtype=torch.uint8, device="cuda")


def launch(c, p, d, group, ws, o, stream=None, states=S, **kw):
    a = dict(group=group, freq=d["wd"], wgt=d["wgt"], all_lnl=o["all_lnl"], out_lnl=o["out_lnl"], stream=stream)
    a.update(kw)
    c.psr_rate_scan_gen(states, d["ops"], d["tips"], d["blen"], d["eig"], d["EVd"], d["tvd"], d["cand"], p["n"], ws,
                        o["best_idx"], o["best_lnl"], **a)


def host(o, n, ncand):
    import torch

    torch.cuda.synchronize()
    return dict(all=o["all_lnl"].cpu().numpy().reshape(ncand, n), idx=o["best_idx"].cpu().numpy(),
                best=o["best_lnl"].cpu().numpy(), out=float(o["out_lnl"].item()))


def scan(c, p, dt, group, d=None):
    d = d or inputs(p, dt)
    ws, o = workspace(p, dt, group), outputs(p["n"], d["ncand"])
    launch(c, p, d, group, ws, o)
    r = host(o, p["n"], d["ncand"])
    r.update(ws=ws, d=d)
    return r


def same_rows(a, b):
    """Equal bits, NaN by position (a NaN row compares by where it is NaN)."""
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(bits(a[~nan]), bits(b[~nan]))


def same_bits(a, b):
    return (same_rows(a["all"], b["all"]) and np.array_equal(a["idx"], b["idx"])
            and np.array_equal(bits(a["best"]), bits(b["best"])))


# ---- the reference and the restatement ----

def tip_vectors(p):
    return {s: TABLE[np.minimum(k, 23)] for s, k in p["codes"].items()}


@functools.lru_cache(maxsize=None)
def reference(tree, n):
    """all_lnl of the reference, (12, n): prune + root_lnl with every site at rate r_k."""
    p = problem(tree, n)
    tips = tip_vectors(p)
    rows = []
    for r in CAND:
        clv = F.prune(p["Q"], p["ops"], p["blen"], tips, np.full((n, 1), r))
        root = clv[p["ops"][-1][0]]
        rows.append(F.root_lnl(root[0], root[1], p["pi"])[1])
    ref = np.array(rows)
    top = np.sort(ref, axis=0)
    print(f"{tree} n={n}: smallest best-to-second gap of the reference {np.min(top[-1] - top[-2]):.2e}")
    return ref


def device_pmats(c, d, dt, rates):
    """pmatrix(EIGEN, 20 states) for `rates`: what the node kernels read."""
    import torch

    pm = torch.empty(d["blen"].numel() * len(rates) * S * S, dtype=tdtype(dt), device="cuda")
    c.pmatrix(d["eig"], dev(np.asarray(rates, np.float64)), d["blen"], pm, states=S, convention=EIGEN)
    torch.cuda.synchronize()
    return pm


def restated(p, d, dt, pm, ncat, cat):
    """(per-site lnL, per-site rescale counts) of the restatement under categories `cat`."""
    M = ncat * S * S
    vals = {s: R.expand_tips(k, dt, d["tv"]) for s, k in p["codes"].items()}
    cnt = np.zeros(p["n"], np.int64)
    for par, a, b, m in p["ops"]:
        vals[par], sc, _ = R.node(vals[a], vals[b], d["EV"], pm[2 * m * M:(2 * m + 1) * M],
                                  pm[(2 * m + 1) * M:(2 * m + 2) * M], cat, ncat)
        cnt += sc
    site = R.root_lnl(vals[p["ops"][-1][0]], p["n"], freq=d["w"])[1]
    return site + cnt.astype(np.float64) * LOG_MINLIK, cnt


def restated_scan(c, p, d, dt):
    pm = device_pmats(c, d, dt, CAND).cpu().numpy()
    rows = [restated(p, d, dt, pm, len(CAND), np.full(p["n"], k, np.uint8)) for k in range(len(CAND))]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])


def assert_within(got, ref, rest, dt, what):
    """Per entry, the module's tolerance rule."""
    scale = np.maximum(1.0, np.abs(ref))
    err, margin = np.abs(got - ref) / scale, np.abs(rest - ref) / scale
    print(f"{what}: largest |gpu - ref| / scale {err.max():.2e}, |rest - ref| / scale {margin.max():.2e} "
          f"(absolute {np.abs(rest - ref).max():.2e})")
    if np.dtype(dt) == np.float64:
        assert np.all(err <= LNL_RTOL), what
    else:
        assert np.all(margin <= F32_LNL_CAP), (what, "the restatement itself misses the cap: change the input")
        assert np.all(err <= margin + LNL_RTOL), what


# ---- 1: against the reference ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("tree,n", PROBLEMS)
def test_scan_equals_the_reference(ctx, tree, n, dt):
    """all_lnl within the tolerance rule; the scaler rows hold 0 / 1 and sum to
    the restatement's counts; the category bytes are g; best_idx is the
    reference's argmax at every site and best_lnl the matching all_lnl bits."""
    dt = np_dtype(dt)
    p = problem(tree, n)
    ref = reference(tree, n)
    r = scan(ctx, p, dt, len(CAND))  # one pass: the workspace still holds every candidate's rows
    rest, cnt = restated_scan(ctx, p, r["d"], dt)
    name = f"{tree} n={n} {np.dtype(dt).name}"
    assert_within(r["all"], ref, rest, dt, name + " all_lnl")

    nops, G = len(p["ops"]), len(CAND)
    lay = layout(dt, nops, p["ntips"], nops, n, G)
    w = r["ws"].cpu().numpy()
    rows = np.stack([w[lay["sc0"] + j * lay["row"]:][:G * n] for j in range(nops)])
    assert set(np.unique(rows).tolist()) <= {0, 1}
    got_cnt = rows.astype(np.int64).sum(axis=0).reshape(G, n)
    varying = int(np.sum(cnt.max(axis=0) != cnt.min(axis=0)))
    print(f"{name}: rescales per virtual site {cnt.min()}..{cnt.max()}, sites whose count varies over the "
          f"candidates {varying}/{n}")
    assert cnt.max() > 0 and varying > 0  # the premises: scaling happens, and not the same for every candidate
    assert np.array_equal(got_cnt, cnt)
    cat = w[lay["cat0"]:][:G * n].reshape(G, n)
    assert np.array_equal(cat, np.repeat(np.arange(G, dtype=np.uint8)[:, None], n, axis=1))

    assert np.array_equal(r["idx"], np.argmax(ref, axis=0))  # no site excluded
    assert np.array_equal(bits(r["best"]), bits(r["all"][r["idx"], np.arange(n)]))
    assert np.array_equal(r["idx"], np.argmax(r["all"], axis=0))  # ties (none here) would keep the lower index
    host_sum = float(np.sum(p["wgt"].astype(np.float64) * r["best"]))
    assert abs(r["out"] - host_sum) <= LNL_RTOL * abs(host_sum)


# ---- 2: bit-identity over group ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("tree,n", PROBLEMS)
def test_group_does_not_change_a_bit(ctx, fctx, tree, n, dt):
    dt = np_dtype(dt)
    p = problem(tree, n)
    d = inputs(p, dt)
    one = scan(ctx, p, dt, 1, d)
    out = np.float64(one["out"]).view(np.uint64)
    for c, what in ((ctx, "plain"), (fctx, "PLFX_FUSE=1")):
        for group in (1, 5, 12):  # twelve passes; passes 5, 5, 2; one pass
            r = scan(c, p, dt, group, d)
            assert same_bits(r, one), (what, group)
            assert np.float64(r["out"]).view(np.uint64) == out, (what, group)
    assert np.isfinite(one["out"]) and np.all(np.isfinite(one["all"]))


# ---- 3: rows equal the composition ----

def compose(c, p, d, dt, pm, k, stride):
    """Row k as the calls of sections 11b and 12b give it: traverse_psr_gen
    (ncat = 12, every site in category k, scaler rows `stride` apart) then
    site_lnl_psr_gen; and site_lnl_psr_gen without rows beside root_lnl_psr_gen."""
    import torch

    n, nops = p["n"], len(p["ops"])
    clv = [None] * p["ntips"] + [torch.empty(S * n, dtype=tdtype(dt), device="cuda")
                                 for _ in range(p["nslots"] - p["ntips"])]
    sc = torch.full((nops, stride), 9, dtype=torch.uint8, device="cuda")
    c.traverse_psr_gen(S, d["ops"], clv, pm, d["EVd"], n, dev(np.full(n, k, np.uint8)), len(CAND),
                       scalers=[sc[j] for j in range(nops)], tips=d["tips"], tipvec=d["tvd"])
    site = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    root = clv[p["ops"][-1][0]]
    c.site_lnl_psr_gen(S, root, n, site, freq=d["wd"], scalers=sc)
    plain = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    c.site_lnl_psr_gen(S, root, n, plain, freq=d["wd"])
    want = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    c.root_lnl_psr_gen(S, root, n, out, freq=d["wd"], site_lnl=want)
    torch.cuda.synchronize()
    return site.cpu().numpy(), plain.cpu().numpy(), want.cpu().numpy()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_rows_equal_the_composition(ctx, n, dt):
    """Row k of all_lnl is traverse_psr_gen + site_lnl_psr_gen bit for bit
    (scaler stride n and n + 3), and site_lnl_psr_gen with no scaler rows is
    root_lnl_psr_gen's site_lnl bit for bit."""
    dt = np_dtype(dt)
    p = problem("caterpillar 24", n)
    d = inputs(p, dt)
    r = scan(ctx, p, dt, 5, d)
    pm = device_pmats(ctx, d, dt, CAND)
    scaled = 0
    for k in range(len(CAND)):
        site, plain, want = compose(ctx, p, d, dt, pm, k, n + 3 * (k % 2))
        assert np.array_equal(bits(r["all"][k]), bits(site)), k
        assert np.array_equal(bits(plain), bits(want)), k
        scaled += int(np.sum(site != plain))
    assert scaled > 0  # the correction was exercised


def test_default_root_weights_are_a_twentieth_each(ctx):
    """freq = None in the scan, in site_lnl_psr_gen and in root_lnl_psr_gen: the same bits."""
    import torch

    dt, n = np.float64, 65
    p = problem("balanced 16", n)
    d = inputs(p, dt)
    ws, o = workspace(p, dt, 12), outputs(n, len(CAND))
    launch(ctx, p, d, 12, ws, o, freq=None)
    r = host(o, n, len(CAND))
    given = dict(d, wd=dev(np.full(S, 0.05)))
    assert same_bits(r, scan(ctx, p, dt, 12, given))
    nops = len(p["ops"])
    lay = layout(dt, nops, p["ntips"], nops, n, 12)
    root = ws[(nops - 1) * lay["clv"]:][:12 * n * S * 8].view(torch.float64)  # the last op's CLV, 12 * n virtual sites
    want = torch.full((12 * n,), SENTINEL, dtype=torch.float64, device="cuda")
    ctx.root_lnl_psr_gen(S, root, 12 * n, torch.zeros(1, dtype=torch.float64, device="cuda"), site_lnl=want)
    sc = ws[lay["sc0"]:][:nops * lay["row"]].view(nops, lay["row"])
    site = torch.full((12 * n,), SENTINEL, dtype=torch.float64, device="cuda")
    ctx.site_lnl_psr_gen(S, root, 12 * n, site, scalers=sc)
    torch.cuda.synchronize()
    cnt = sc[:, :12 * n].cpu().numpy().astype(np.int64).sum(axis=0)
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(site.cpu().numpy()), bits(want.cpu().numpy() + cnt.astype(np.float64) * LOG_MINLIK))
    assert np.array_equal(bits(site.cpu().numpy()), bits(r["all"].reshape(-1)))  # the scan's own rows, whole


# ---- 4: states = 4 through the _gen entries is section 12 ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_four_states_through_the_gen_entries_are_section_12(ctx, fctx, dt):
    import torch

    dt = np_dtype(dt)
    n, group, G = 130, 5, len(DNA_CAND)
    p = psr_problem("balanced 16", n, 4, simulated=True)
    d = dna_inputs(p, dt)
    nops = len(p["ops"])
    size = plfx.psr_rate_scan_workspace(dt, nops, p["ntips"], nops, n, group)
    assert plfx.psr_rate_scan_workspace_gen(dt, 4, nops, p["ntips"], nops, n, group) == size
    for c in (ctx, fctx):
        res = []
        for gen in (False, True):
            ws, o = torch.full((size,), 0xAB, dtype=torch.uint8, device="cuda"), outputs(n, G)
            a = (d["ops"], d["tips"], d["blen"], d["eig"], d["EVd"], d["tvd"], d["cand"], n, ws, o["best_idx"],
                 o["best_lnl"])
            kw = dict(group=group, freq=d["wd"], wgt=d["wgt"], all_lnl=o["all_lnl"], out_lnl=o["out_lnl"])
            c.psr_rate_scan_gen(4, *a, **kw) if gen else c.psr_rate_scan(*a, **kw)
            res.append((host(o, n, G), ws.cpu().numpy()))
        (old, ws_old), (new, ws_new) = res
        assert same_bits(old, new) and np.float64(old["out"]).view(np.uint64) == np.float64(new["out"]).view(np.uint64)
        assert np.array_equal(ws_old, ws_new)  # CLVs, scaler rows, matrices: the same code ran
    # site_lnl_psr_gen(4) on the last pass's root CLV and scaler rows: site_lnl_psr's bits
    lay = dna_layout(dt, nops, p["ntips"], nops, n, group)
    gc = G % group or group
    root = ws[(nops - 1) * lay["clv"]:][:gc * n * 4 * np.dtype(dt).itemsize].view(tdtype(dt))
    sc = ws[lay["sc0"]:][:nops * lay["row"]].view(nops, lay["row"])
    got = []
    for gen in (False, True):
        site = torch.full((gc * n,), SENTINEL, dtype=torch.float64, device="cuda")
        a, kw = (root, gc * n, site), dict(freq=d["wd"], scalers=sc)
        ctx.site_lnl_psr_gen(4, *a, **kw) if gen else ctx.site_lnl_psr(*a, **kw)
        torch.cuda.synchronize()
        got.append(site.cpu().numpy())
    assert np.array_equal(bits(got[0]), bits(got[1]))
    assert np.array_equal(bits(got[1]), bits(new["all"][G - gc:].reshape(-1)))


# ---- 5: site_lnl_psr_gen on a mixed-category traversal ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_site_lnl_of_a_mixed_category_traversal(fctx, dt):
    """The caterpillar with seven categories in random order and category bytes
    past ncat (clamped): the per-site lnL with its own correction is the
    reference's, and the scaler rows sum to the restatement's counts."""
    import torch

    dt = np_dtype(dt)
    tree, n, ncat = "caterpillar 24", 65, 7
    p = problem(tree, n)
    rates = np.geomspace(0.25, 8.0, ncat)
    rng = np.random.default_rng(5)
    cat = rng.integers(0, ncat, n).astype(np.uint8)
    cat[3::7] = np.resize(np.array([ncat, ncat + 1, 200, 255], np.uint8), cat[3::7].size)
    assert (cat >= ncat).sum() >= 4
    clv_ref = F.prune(p["Q"], p["ops"], p["blen"], tip_vectors(p), F.site_rates_psr(rates, cat))
    root = p["ops"][-1][0]
    ref = F.root_lnl(clv_ref[root][0], clv_ref[root][1], p["pi"])[1]
    d = inputs(p, dt, rates)
    nops = len(p["ops"])
    pm = device_pmats(fctx, d, dt, rates)
    clv = [None] * p["ntips"] + [torch.empty(S * n, dtype=tdtype(dt), device="cuda")
                                 for _ in range(p["nslots"] - p["ntips"])]
    sc = torch.full((nops, n), 9, dtype=torch.uint8, device="cuda")
    fctx.traverse_psr_gen(S, d["ops"], clv, pm, d["EVd"], n, dev(cat), ncat, scalers=[sc[j] for j in range(nops)],
                          tips=d["tips"], tipvec=d["tvd"])
    site = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    fctx.site_lnl_psr_gen(S, clv[root], n, site, freq=d["wd"], scalers=sc)
    torch.cuda.synchronize()
    rest, cnt = restated(p, d, dt, pm.cpu().numpy(), ncat, cat)
    print(f"{tree} n={n}: rescales per site {cnt.min()}..{cnt.max()}")
    assert cnt.max() > 0 and cnt.max() != cnt.min()
    assert np.array_equal(sc.cpu().numpy().astype(np.int64).sum(axis=0), cnt)
    assert_within(site.cpu().numpy(), ref, rest, dt, f"{tree} n={n} {np.dtype(dt).name} site lnL, 7 categories")


# ---- 6: the tie and NaN rules ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_ties_keep_the_lower_candidate_and_a_nan_never_wins(ctx, dt):
    dt = np_dtype(dt)
    tree, n = "random 12", 257
    p = problem(tree, n)
    plain = scan(ctx, p, dt, 5)
    tie = CAND.copy()
    tie[7] = tie[3]
    for group in (5, 12):  # candidates 3 and 7 in different passes, and in one
        r = scan(ctx, p, dt, group, inputs(p, dt, tie))
        assert np.array_equal(bits(r["all"][3]), bits(r["all"][7]))
        assert np.array_equal(bits(r["all"][3]), bits(plain["all"][3]))
        assert not np.any(r["idx"] == 7) and np.any(r["idx"] == 3)
        assert np.array_equal(bits(r["best"]), bits(r["all"][r["idx"], np.arange(n)]))
    nan = CAND.copy()
    k = int(np.bincount(plain["idx"], minlength=12).argmax())  # the candidate most sites like best
    nan[k] = np.nan
    for group in (5, 12):
        r = scan(ctx, p, dt, group, inputs(p, dt, nan))
        assert np.all(np.isnan(r["all"][k])) and not np.any(r["idx"] == k)
        others = np.delete(np.arange(12), k)
        assert np.array_equal(bits(r["all"][others]), bits(plain["all"][others]))
        want = others[np.argmax(plain["all"][others], axis=0)]
        assert np.array_equal(r["idx"], want)
        assert np.array_equal(bits(r["best"]), bits(r["all"][r["idx"], np.arange(n)]))
        assert np.isfinite(r["out"])
    r = scan(ctx, p, dt, 5, inputs(p, dt, np.array([np.nan])))
    assert np.all(np.isnan(r["all"])) and np.all(r["idx"] == 0) and np.all(np.isneginf(r["best"]))


# ---- 7: one block ----

def test_one_block_walks_every_site(ctx, monkeypatch):
    """PLFX_MAX_BLOCKS=1: one block makes both trips over 257 sites (a whole
    tile of 256 and one site) in every kernel of the scan and is its own last
    block; out_lnl is summed in another order."""
    monkeypatch.setenv("PLFX_MAX_BLOCKS", "1")
    tree, n = "random 12", 257
    p = problem(tree, n)
    with plfx.Context(0, lazy_tables=True) as c:
        for dt in (np.float64, np.float32):
            d = inputs(p, dt)
            want = scan(ctx, p, dt, 5, d)
            for group in (5, 12):
                got = scan(c, p, dt, group, d)
                assert same_bits(got, want), (dt, group)
                assert abs(got["out"] - want["out"]) <= LNL_RTOL * abs(want["out"])


# ---- 8: the loop closed ----

def lnl_under(c, p, d, dt, rates, cat, perm):
    """traverse_psr_gen + root_lnl_psr_gen under the categories `cat` with
    `rates`, the sites in the order `perm` (codes, weights and categories alike)."""
    import torch

    n, nops = p["n"], len(p["ops"])
    pm = device_pmats(c, d, dt, rates)
    clv = [None] * p["ntips"] + [torch.empty(S * n, dtype=tdtype(dt), device="cuda")
                                 for _ in range(p["nslots"] - p["ntips"])]
    tips = [dev(p["codes"][s][perm]) for s in range(p["ntips"])] + [None] * (p["nslots"] - p["ntips"])
    wgt = dev(p["wgt"][perm])
    sums = torch.full((nops,), -1, dtype=torch.int64, device="cuda")
    c.traverse_psr_gen(S, d["ops"], clv, pm, d["EVd"], n, dev(cat[perm]), len(rates), wgt=wgt, scaler_sums=sums,
                       tips=tips, tipvec=d["tvd"])
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    c.root_lnl_psr_gen(S, clv[p["ops"][-1][0]], n, out, freq=d["wd"], wgt=wgt, scaler_sums=sums)
    torch.cuda.synchronize()
    return float(out.item())


@pytest.mark.parametrize("tree,n", [("random 12", 257), ("caterpillar 24", 65)])
def test_scan_then_categorize_closes_the_loop(ctx, tree, n):
    dt = np.float64
    p = problem(tree, n)
    clv = F.prune(p["Q"], p["ops"], p["blen"], tip_vectors(p), TRUE_RATES[p["true_cat"]][:, None])
    root = clv[p["ops"][-1][0]]
    ref_true = F.root_lnl(root[0], root[1], p["pi"], None, p["wgt"])[0]
    cand = np.concatenate([TRUE_RATES, np.geomspace(0.25, 8.0, 8)])
    assert len(set(cand.tolist())) == 12
    d = inputs(p, dt, cand)
    r = scan(ctx, p, dt, 5, d)
    host_sum = float(np.sum(p["wgt"].astype(np.float64) * r["best"]))
    print(f"{tree}: out_lnl {r['out']!r}, host sum {host_sum!r}, reference under the true rates {ref_true!r}")
    assert abs(r["out"] - host_sum) <= LNL_RTOL * abs(host_sum)
    assert r["out"] >= ref_true  # every site's best is at least its lnL at its true rate, a candidate

    cat, rates, scale = plfx.psr_categorize(cand, r["idx"], p["wgt"], 12)
    kept = sorted(set(r["idx"].tolist()), key=lambda k: (cand[k], k))
    assert rates.size == len(kept) and np.array_equal(cat, np.array([kept.index(k) for k in r["idx"]], np.uint8))
    perm = plfx.psr_site_order(cat, len(kept))
    assert np.all(np.diff(cat[perm].astype(np.int64)) >= 0) and sorted(perm.tolist()) == list(range(n))
    lnl = lnl_under(ctx, p, d, dt, cand[kept], cat, perm)  # the unscaled rates: every site at its best candidate
    print(f"{tree}: {len(kept)} categories, scale {scale!r}, lnL under rate_cat {lnl!r}")
    assert abs(lnl - r["out"]) <= LNL_RTOL * abs(lnl)


# ---- 9: capture ----

def test_captured_scan_replays_to_the_eager_bits():
    """Captured on a stream whose first use is the capture; replayed twice, the
    tip codes changed in place in between."""
    import torch

    dt, tree, n, group = np.float64, "random 12", 257, 5
    p = problem(tree, n)
    other = {s: np.roll(c, 11 + s) for s, c in p["codes"].items()}
    with plfx.Context(0, lazy_tables=True) as c:
        first = scan(c, p, dt, group)
        second = scan(c, p, dt, group, inputs(p, dt, codes=other))
        assert not same_bits(first, second)
        d, ws, o = inputs(p, dt), workspace(p, dt, group), outputs(n, len(CAND))
        cold = torch.cuda.Stream()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cold):
            launch(c, p, d, group, ws, o, stream=cold)
        for want, codes in ((first, p["codes"]), (second, other)):
            for s in range(p["ntips"]):
                d["tips"][s].copy_(torch.from_numpy(np.ascontiguousarray(codes[s])))
            for t in o.values():
                t.fill_(-3 if t.dtype == torch.int32 else SENTINEL)
            torch.cuda.synchronize()
            g.replay()
            got = host(o, n, len(CAND))
            assert same_bits(got, want)
            assert np.float64(got["out"]).view(np.uint64) == np.float64(want["out"]).view(np.uint64)
        del g
        torch.cuda.synchronize()


# ---- 10: refusals ----

def test_refusals_touch_nothing(ctx):
    import torch

    dt, n = np.float64, 65
    p = problem("balanced 16", n)
    d = inputs(p, dt)
    ws, o = workspace(p, dt, 5), outputs(n, len(CAND))
    dense = list(d["tips"])
    dense[3] = None
    too_many = dev(np.geomspace(0.25, 8.0, plfx.PSR_SCAN_MAX_RATES + 1))
    big_all = torch.full(((plfx.PSR_SCAN_MAX_RATES + 1) * n,), SENTINEL, dtype=torch.float64, device="cuda")
    ws4 = workspace(p, dt, 5, states=4)
    assert ws4.numel() < ws.numel()
    INV, UNS = plfx.ERR_INVALID, plfx.ERR_UNSUPPORTED

    def call(code, what, group=5, ws_=ws, **kw):
        dd = dict(d)
        for k in ("tips", "tvd", "cand"):
            if k in kw:
                dd[k] = kw.pop(k)
        with pytest.raises(plfx.PlfxError) as e:
            launch(ctx, p, dd, group, ws_, o, **kw)
        assert e.value.code == code, (what, str(e.value))

    call(UNS, "a dense leaf", tips=dense)
    call(INV, "group 0", group=0)
    call(INV, "group 33", group=33)
    call(INV, "ncand 0", cand=d["cand"][:0])
    call(INV, "ncand 1025", cand=too_many, all_lnl=big_all)
    call(INV, "a short workspace", ws_=ws[:ws.numel() - 1])
    call(INV, "a misaligned workspace", ws_=torch.cat([ws, ws[:256]])[128:])
    call(INV, "a workspace sized for 4 states", ws_=ws4)
    call(INV, "a null tipvec", tvd=None)
    call(UNS, "states 5", states=5)
    # the C entry itself: states 5 is PLFX_ERR_UNSUPPORTED whatever else is passed
    L, h, sh = ctx._L, ctx.h, ctx._sh(None)
    assert L.plfx_psr_rate_scan_gen(h, 1, 5, None, 0, None, 0, None, 0, None, None, None, None, 0, 0, None, None, n,
                                    None, 0, None, None, None, None, sh) == UNS
    torch.cuda.synchronize()
    assert np.all(o["best_idx"].cpu().numpy() == -3)
    for k in ("best_lnl", "all_lnl", "out_lnl"):
        assert np.all(o[k].cpu().numpy() == SENTINEL), k
    assert np.all(big_all.cpu().numpy() == SENTINEL)
    assert np.all(ws.cpu().numpy() == 0xAB) and np.all(ws4.cpu().numpy() == 0xAB)  # not even the set-up ran
    # n == 0 launches nothing and zeroes out_lnl; and the context still works
    ctx.psr_rate_scan_gen(S, d["ops"], d["tips"], d["blen"], d["eig"], d["EVd"], d["tvd"], d["cand"], 0, ws,
                          o["best_idx"], o["best_lnl"], group=5, out_lnl=o["out_lnl"])
    torch.cuda.synchronize()
    assert float(o["out_lnl"].item()) == 0.0 and np.all(ws.cpu().numpy() == 0xAB)
    assert np.all(o["best_idx"].cpu().numpy() == -3) and np.all(o["best_lnl"].cpu().numpy() == SENTINEL)
    launch(ctx, p, d, 5, ws, o)
    assert same_bits(host(o, n, len(CAND)), scan(ctx, p, dt, 12, d))
    # site_lnl_psr_gen's own refusals
    x = torch.zeros(S * n + 2, dtype=torch.float64, device="cuda")
    site = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    sc = torch.zeros((2, n), dtype=torch.uint8, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    for what, code, a in [("states 5", UNS, (1, 5, ptr(x), n, None, ptr(sc), 2, n, ptr(site))),
                          ("bad dtype", INV, (2, S, ptr(x), n, None, ptr(sc), 2, n, ptr(site))),
                          ("n < 0", INV, (1, S, ptr(x), -1, None, ptr(sc), 2, n, ptr(site))),
                          ("null x", INV, (1, S, None, n, None, ptr(sc), 2, n, ptr(site))),
                          ("misaligned x", INV, (1, S, ptr(x) + 8, n, None, ptr(sc), 2, n, ptr(site))),
                          ("null site_lnl", INV, (1, S, ptr(x), n, None, ptr(sc), 2, n, None)),
                          ("nsc < 0", INV, (1, S, ptr(x), n, None, ptr(sc), -1, n, ptr(site))),
                          ("null scalers", INV, (1, S, ptr(x), n, None, None, 2, n, ptr(site))),
                          ("stride < n", INV, (1, S, ptr(x), n, None, ptr(sc), 2, n - 1, ptr(site)))]:
        assert L.plfx_site_lnl_psr_gen(h, *a, sh) == code, what
    with pytest.raises(plfx.PlfxError) as e:
        ctx.site_lnl_psr_gen(5, x, n, site)
    assert e.value.code == UNS
    assert L.plfx_site_lnl_psr_gen(h, 1, S, ptr(x), 0, None, None, 0, 0, ptr(site), sh) == plfx.OK  # n == 0: nothing
    torch.cuda.synchronize()
    assert np.all(site.cpu().numpy() == SENTINEL)
