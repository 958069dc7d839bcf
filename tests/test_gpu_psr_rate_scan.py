"""GPU tests of plfx.h section 12: the per-site rate scan (plfx_psr_rate_scan),
the per-site lnL with per-site scaling (plfx_site_lnl_psr) and, end to end, the
categorisation (plfx_psr_categorize).

Problems: sequences simulated down three trees under four true rates
(psr_problem(tree, n, 4, simulated=True)), scanned over the twelve candidates
geomspace(0.05, 8, 12).  The reference is tests/felsenstein_ref.py, per
candidate r_k: prune + root_lnl with every site at rate r_k (expm, no eigen
code).  The restatement is tests/psr_ref.py composed op by op on the device's
own matrices, plus the per-site rescale counts times log(2^-32).

Measured for these three problems (on the restatement over the device's own
matrices): the smallest gap between a site's best and second-best reference
lnL is 1.0e-3; the f64 restatement is within 2.0e-12 (absolute) of the
reference and the f32 one within 1.4e-4 absolute, 3.9e-6 of max(1, |ref|),
under the 1e-5 cap and a tenth of the gap; the rescale counts reach 6
(caterpillar), 3 and 2, and differ between the candidates at 65 of 65, 230 of
257 and 69 of 130 sites.  The tests assert the premises they rely on (counts
> 0, counts varying) and print what they measure.

Tolerances: f64 |got - ref| <= LNL_RTOL * max(1, |ref|) per entry, the rule of
tests/test_gpu_psr.py for site_lnl; f32 the `within` rule of
tests/test_gpu_likelihood_ref.py per entry on that scale with F32_LNL_CAP."""
import functools

import numpy as np
import pytest

import felsenstein_ref as F
import plfx
import psr_ref
from test_felsenstein_ref import F32_LNL_CAP, LNL_RTOL, psr_problem, psr_rates, psr_reference, restate
from test_gpu_psr import bits, dev, np_dtype, tdtype

pytestmark = pytest.mark.gpu

CAND = np.geomspace(0.05, 8.0, 12)
PROBLEMS = [("caterpillar 48", 65), ("random 24", 257), ("balanced 16", 130)]
LOG_MINLIK = psr_ref.LOG_MINLIK
EIGEN = plfx.PMAT_EIGEN
SENTINEL = -7.0


@pytest.fixture(scope="module")
def fctx():
    """A context that fuses the level pairs (PLFX_FUSE=1 is read at creation)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PLFX_FUSE", "1")
        c = plfx.Context(0, lazy_tables=True)
    yield c
    c.close()


# ---- inputs, the scan, the layout of its workspace ----

def inputs(p, dt, cand=CAND, codes=None):
    """The device tensors of a scan of problem p, and on the host what the kernels read."""
    e = plfx.model_eigen(p["exch"], p["freqs"])
    EV = plfx.model_ev(e, 4, EIGEN).astype(dt)
    tv = plfx.model_tip_vectors(e, EIGEN).astype(dt)
    w = plfx.model_root_weights(e, p["freqs"], EIGEN)
    codes = p["codes"] if codes is None else codes
    return dict(e=e, eig=dev(e), EV=EV, tv=tv, w=w, EVd=dev(EV), tvd=dev(tv), wd=dev(w), blen=dev(p["blen"]),
                cand=dev(np.asarray(cand, np.float64)), ncand=len(cand), wgt=dev(p["wgt"]),
                tips=[dev(codes[s]) for s in range(p["ntips"])] + [None] * (p["nslots"] - p["ntips"]),
                ops=np.array(p["ops"], np.int32).reshape(-1, 4))


def layout(dt, nops, ntips, npmats, n, group):
    """The workspace's parts as plfx.h documents them, each array rounded up to 256 bytes."""
    es, vn = np.dtype(dt).itemsize, group * n
    up = lambda v: -(-v // 256) * 256  # noqa: E731
    clv, row = up(vn * 4 * es), up(vn)
    tip0 = nops * clv
    sc0 = tip0 + ntips * row
    cat0 = sc0 + nops * row
    pm0 = cat0 + row
    return dict(clv=clv, row=row, tip0=tip0, sc0=sc0, cat0=cat0, pm0=pm0, end=pm0 + up(2 * npmats * group * 16 * es))


def outputs(n, ncand):
    import torch

    return dict(best_idx=torch.full((n,), -3, dtype=torch.int32, device="cuda"),
                best_lnl=torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda"),
                all_lnl=torch.full((ncand * n,), SENTINEL, dtype=torch.float64, device="cuda"),
                out_lnl=torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda"))


def workspace(p, dt, group):
    import torch

    nops = len(p["ops"])
    size = plfx.psr_rate_scan_workspace(dt, nops, p["ntips"], nops, p["n"], group)
    assert size == layout(dt, nops, p["ntips"], nops, p["n"], group)["end"]
    return torch.full((size,), 0xAB, dtype=torch.uint8, device="cuda")


def launch(c, p, d, group, ws, o, stream=None, **kw):
    a = dict(group=group, freq=d["wd"], wgt=d["wgt"], all_lnl=o["all_lnl"], out_lnl=o["out_lnl"], stream=stream)
    a.update(kw)
    c.psr_rate_scan(d["ops"], d["tips"], d["blen"], d["eig"], d["EVd"], d["tvd"], d["cand"], p["n"], ws,
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


def same_bits(a, b):
    return (np.array_equal(bits(a["all"]), bits(b["all"])) and np.array_equal(a["idx"], b["idx"])
            and np.array_equal(bits(a["best"]), bits(b["best"])))


# ---- the reference and the restatement ----

@functools.lru_cache(maxsize=None)
def reference(tree, n):
    """all_lnl of the reference, (12, n): prune + root_lnl with every site at rate r_k."""
    p = psr_problem(tree, n, 4, simulated=True)
    tips = {s: F.tip_states(c) for s, c in p["codes"].items()}
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
    """pmatrix(EIGEN) for `rates`, read back: what the node kernels read."""
    import torch

    pm = torch.empty(d["blen"].numel() * len(rates) * 16, dtype=tdtype(dt), device="cuda")
    c.pmatrix(d["eig"], dev(np.asarray(rates, np.float64)), d["blen"], pm, states=4, convention=EIGEN)
    torch.cuda.synchronize()
    return pm


def restated(p, d, dt, pm, ncat, cat):
    """(per-site lnL, per-site rescale counts) of the restatement under categories `cat`."""
    q = dict(p, ncat=ncat, cat=cat)
    vals, scs, _ = restate(q, dt, pm, d["EV"], d["tv"])
    cnt = np.sum(np.array(scs, np.int64), axis=0)
    site = psr_ref.root_lnl(vals[p["ops"][-1][0]], p["n"], freq=d["w"])[1]
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


# ---- 1-3: against the reference ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("tree,n", PROBLEMS)
def test_scan_equals_the_reference(ctx, tree, n, dt):
    """all_lnl within the tolerance rule; the rescale counts the device's scaler
    rows imply are the restatement's; best_idx is the reference's argmax at
    every site and best_lnl the matching all_lnl entry."""
    dt = np_dtype(dt)
    p = psr_problem(tree, n, 4, simulated=True)
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


# ---- 4: bit-identity ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("tree,n", PROBLEMS)
def test_group_and_fusion_do_not_change_a_bit(ctx, fctx, tree, n, dt):
    dt = np_dtype(dt)
    p = psr_problem(tree, n, 4, simulated=True)
    d = inputs(p, dt)
    one = scan(ctx, p, dt, 1, d)
    for group in (5, 12):  # passes 5, 5, 2; one pass
        assert same_bits(scan(ctx, p, dt, group, d), one), group
    for group in (5, 12):
        assert same_bits(scan(fctx, p, dt, group, d), one), ("fused", group)
    assert np.isfinite(one["out"]) and np.all(np.isfinite(one["all"]))


def compose(c, p, d, dt, pm, k, stride):
    """Row k as the calls of section 11 give it: traverse_psr (ncat = 12, every
    site in category k, scaler rows `stride` apart) then site_lnl_psr."""
    import torch

    n, nops = p["n"], len(p["ops"])
    clv = [None] * p["ntips"] + [torch.empty(4 * n, dtype=tdtype(dt), device="cuda")
                                 for _ in range(p["nslots"] - p["ntips"])]
    sc = torch.full((nops, stride), 9, dtype=torch.uint8, device="cuda")
    c.traverse_psr(d["ops"], clv, pm, d["EVd"], n, dev(np.full(n, k, np.uint8)), len(CAND),
                   scalers=[sc[j] for j in range(nops)], tips=d["tips"], tipvec=d["tvd"])
    site = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    root = clv[p["ops"][-1][0]]
    c.site_lnl_psr(root, n, site, freq=d["wd"], scalers=sc)
    plain = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    c.site_lnl_psr(root, n, plain, freq=d["wd"])
    want = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    c.root_lnl_psr(root, n, out, freq=d["wd"], site_lnl=want)
    torch.cuda.synchronize()
    return site.cpu().numpy(), plain.cpu().numpy(), want.cpu().numpy()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_rows_equal_the_composition_of_section_11(ctx, n, dt):
    """Row k of all_lnl is traverse_psr + site_lnl_psr bit for bit, and
    site_lnl_psr with no scaler rows is root_lnl_psr's site_lnl bit for bit."""
    dt = np_dtype(dt)
    p = psr_problem("caterpillar 48", n, 4, simulated=True)
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


# ---- 5: site_lnl_psr on a mixed-category traversal ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("tree,n", [("caterpillar 48", 65), ("random 24", 257)])
def test_site_lnl_of_a_mixed_category_traversal(fctx, tree, n, dt):
    """Seven categories, random codes, category bytes past ncat (clamped): the
    per-site lnL with its own correction is the reference's."""
    import torch

    dt = np_dtype(dt)
    p = psr_problem(tree, n, 7)
    assert (p["cat"] >= 7).sum() >= 4
    clv_ref, _ = psr_reference(tree, n, 7)
    root = p["ops"][-1][0]
    ref = F.root_lnl(clv_ref[root][0], clv_ref[root][1], p["pi"])[1]
    d = inputs(p, dt, p["rates"])
    nops = len(p["ops"])
    pm = device_pmats(fctx, d, dt, p["rates"])
    clv = [None] * p["ntips"] + [torch.empty(4 * n, dtype=tdtype(dt), device="cuda")
                                 for _ in range(p["nslots"] - p["ntips"])]
    sc = torch.full((nops, n), 9, dtype=torch.uint8, device="cuda")
    fctx.traverse_psr(d["ops"], clv, pm, d["EVd"], n, dev(p["cat"]), 7, scalers=[sc[j] for j in range(nops)],
                      tips=d["tips"], tipvec=d["tvd"])
    site = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    fctx.site_lnl_psr(clv[root], n, site, freq=d["wd"], scalers=sc)
    torch.cuda.synchronize()
    rest, cnt = restated(p, d, dt, pm.cpu().numpy(), 7, p["cat"])
    assert cnt.max() > 0 and cnt.max() != cnt.min()
    assert np.array_equal(sc.cpu().numpy().astype(np.int64).sum(axis=0), cnt)
    assert_within(site.cpu().numpy(), ref, rest, dt, f"{tree} n={n} {np.dtype(dt).name} site lnL, 7 categories")


# ---- 6: the property, and the loop closed ----

def lnl_under(c, p, d, dt, rates, cat):
    """traverse_psr + root_lnl_psr under the categories `cat` with `rates`."""
    import torch

    n, nops = p["n"], len(p["ops"])
    pm = device_pmats(c, d, dt, rates)
    clv = [None] * p["ntips"] + [torch.empty(4 * n, dtype=tdtype(dt), device="cuda")
                                 for _ in range(p["nslots"] - p["ntips"])]
    sums = torch.full((nops,), -1, dtype=torch.int64, device="cuda")
    c.traverse_psr(d["ops"], clv, pm, d["EVd"], n, dev(cat), len(rates), wgt=d["wgt"], scaler_sums=sums,
                   tips=d["tips"], tipvec=d["tvd"])
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    c.root_lnl_psr(clv[p["ops"][-1][0]], n, out, freq=d["wd"], wgt=d["wgt"], scaler_sums=sums)
    torch.cuda.synchronize()
    return float(out.item())


@pytest.mark.parametrize("tree,n", [("random 24", 257), ("caterpillar 48", 65)])
def test_scan_then_categorize_closes_the_loop(ctx, tree, n):
    dt = np.float64
    p = psr_problem(tree, n, 4, simulated=True)
    _, ref_true = psr_reference(tree, n, 4, 0, True)
    others = np.geomspace(0.05, 8.0, 8)
    cand = np.concatenate([psr_rates(4), others])
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
    lnl = lnl_under(ctx, p, d, dt, cand[kept], cat)  # the unscaled rates: every site at its best candidate
    print(f"{tree}: {len(kept)} categories, scale {scale!r}, lnL under rate_cat {lnl!r}")
    assert abs(lnl - r["out"]) <= LNL_RTOL * abs(lnl)

    cat4, rates4, scale4 = plfx.psr_categorize(cand, r["idx"], p["wgt"], 4)
    assert rates4.size == 4 < len(kept)
    lnl4 = lnl_under(ctx, p, d, dt, rates4 / scale4, cat4)
    print(f"{tree}: 4 categories, lnL {lnl4!r}")
    assert lnl4 <= r["out"]


# ---- 7: capture ----

def test_captured_scan_replays_to_the_eager_bits():
    """Captured on a stream whose first use is the capture; replayed twice, the
    tip codes changed in place in between."""
    import torch

    dt, tree, n, group = np.float64, "random 24", 257, 5
    p = psr_problem(tree, n, 4, simulated=True)
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


# ---- 8: refusals ----

def test_refusals_through_the_wrapper_touch_nothing(ctx):
    import torch

    dt, n = np.float64, 65
    p = psr_problem("balanced 16", n, 4, simulated=True)
    d = inputs(p, dt)
    ws, o = workspace(p, dt, 5), outputs(n, len(CAND))
    dense = list(d["tips"])
    dense[3] = None
    too_many = dev(np.geomspace(0.05, 8.0, plfx.PSR_SCAN_MAX_RATES + 1))
    big_all = torch.full(((plfx.PSR_SCAN_MAX_RATES + 1) * n,), SENTINEL, dtype=torch.float64, device="cuda")
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
    call(INV, "a null tipvec", tvd=None)
    with pytest.raises(plfx.PlfxError) as e:
        launch(ctx, p, d, 5, ws, o, states=20)
    assert e.value.code == UNS
    torch.cuda.synchronize()
    assert np.all(o["best_idx"].cpu().numpy() == -3)
    for k in ("best_lnl", "all_lnl", "out_lnl"):
        assert np.all(o[k].cpu().numpy() == SENTINEL), k
    assert np.all(big_all.cpu().numpy() == SENTINEL)
    assert np.all(ws.cpu().numpy() == 0xAB)  # not even the set-up ran
    # n == 0 launches nothing and zeroes out_lnl; and the context still works
    ctx.psr_rate_scan(d["ops"], d["tips"], d["blen"], d["eig"], d["EVd"], d["tvd"], d["cand"], 0, ws, o["best_idx"],
                      o["best_lnl"], group=5, out_lnl=o["out_lnl"])
    torch.cuda.synchronize()
    assert float(o["out_lnl"].item()) == 0.0 and np.all(ws.cpu().numpy() == 0xAB)
    launch(ctx, p, d, 5, ws, o)
    assert same_bits(host(o, n, len(CAND)), scan(ctx, p, dt, 12, d))
    # site_lnl_psr's own refusals
    x = torch.zeros(4 * n + 2, dtype=torch.float64, device="cuda")
    site = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    sc = torch.zeros((2, n), dtype=torch.uint8, device="cuda")
    L, h, sh = ctx._L, ctx.h, ctx._sh(None)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    for what, a in [("bad dtype", (2, ptr(x), n, None, ptr(sc), 2, n, ptr(site))),
                    ("n < 0", (1, ptr(x), -1, None, ptr(sc), 2, n, ptr(site))),
                    ("null x", (1, None, n, None, ptr(sc), 2, n, ptr(site))),
                    ("misaligned x", (1, ptr(x) + 8, n, None, ptr(sc), 2, n, ptr(site))),
                    ("null site_lnl", (1, ptr(x), n, None, ptr(sc), 2, n, None)),
                    ("nsc < 0", (1, ptr(x), n, None, ptr(sc), -1, n, ptr(site))),
                    ("null scalers", (1, ptr(x), n, None, None, 2, n, ptr(site))),
                    ("stride < n", (1, ptr(x), n, None, ptr(sc), 2, n - 1, ptr(site)))]:
        assert L.plfx_site_lnl_psr(h, *a, sh) == INV, what
    torch.cuda.synchronize()
    assert np.all(site.cpu().numpy() == SENTINEL)
