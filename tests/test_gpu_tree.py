"""GPU tests of the multi-node extensions (BASELINE configs 3 and 4): batched
independent nodes, traversal descriptors with level scheduling, and the root
log-likelihood.  The reference has no traversal driver; on its
side a sweep is its plf() called once per inner node, and that composition of
the unmodified reference build pins the 4-state sweeps here
(`test_tree64_reference_golden` against tests/golden/tree64.npz, the full-size
window against oracle.ref_traverse).  The other tests check against the
oracle's sequential restatement (itself pinned by the same fixture,
tests/test_tree_golden.py).  The root lnL stays "parity unpinned".  Bar: CLVs
and scaler sums bit-exact; lnL within 1e-12 relative (device log() and a
different, fixed summation order)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LNL_RTOL = 1e-12


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("count", [1, 5, 32, 41])
def test_batch_independent_nodes(ctx, oracle, dtype, count):
    import torch

    n = 3001
    rng = np.random.default_rng(count)
    d = oracle.gen_hostmem(n, dtype, 100 + count)
    EV = d["EV"]
    w = (rng.integers(0, 5, n)).astype(np.int32)
    nodes, exp = [], []
    for i in range(count):
        x1 = (rng.random(16 * n) * (1e-12 if i % 3 == 0 else 1.0)).astype(dtype)
        x2 = rng.random(16 * n).astype(dtype)
        L = rng.random(64).astype(dtype)
        R = rng.random(64).astype(dtype)
        exp.append(oracle.plf(x1, x2, EV, L, R, w))
        nodes.append(dict(x1=dev(x1), x2=dev(x2), x3=torch.empty(16 * n, dtype=dev(x1).dtype, device="cuda"),
                          left=dev(L), right=dev(R),
                          scaler=torch.empty(n, dtype=torch.uint8, device="cuda") if i % 2 == 0 else None,
                          scaler_sum=torch.zeros(1, dtype=torch.int64, device="cuda") if i % 4 != 3 else None))
    ctx.plf_batch_dev(nodes, dev(EV), n, dev(w))
    torch.cuda.synchronize()
    for i, (nd, (e3, esc, einc)) in enumerate(zip(nodes, exp)):
        assert np.array_equal(bits(nd["x3"].cpu().numpy()), bits(e3)), i
        if nd["scaler"] is not None:
            assert np.array_equal(nd["scaler"].cpu().numpy(), esc), i
        if nd["scaler_sum"] is not None:
            assert int(nd["scaler_sum"].item()) == einc, i


def _tree_case(oracle, ntips, n, dtype, seed):
    rng = np.random.default_rng(seed)
    ops = oracle.balanced_tree_ops(ntips)
    nslots = ntips + ops.shape[0]
    tips = [rng.random(16 * n).astype(dtype) for _ in range(ntips)]
    pm = (rng.random(ops.shape[0] * 2 * 64) * 0.25).astype(dtype)   # P, EV x0.25
    EV = (rng.random(16) * 0.25).astype(dtype)
    wgt = rng.integers(1, 4, n).astype(np.int32)
    return ops, nslots, tips, pm, EV, wgt


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_traverse_balanced_tree(ctx, oracle, dtype):
    import torch

    n = 2049
    ops, nslots, tips, pm, EV, wgt = _tree_case(oracle, 16, n, dtype, 7)
    clv_h = [t.copy() for t in tips] + [np.zeros(16 * n, dtype) for _ in range(nslots - 16)]
    esums, escal = oracle.traverse(4, 4, ops, clv_h, pm, EV, n, wgt, want_scalers=True)
    assert esums.sum() > 0  # deep levels underflow: the scaler path is exercised
    clv = [dev(t) for t in tips] + [torch.zeros(16 * n, dtype=dev(tips[0]).dtype, device="cuda")
                                    for _ in range(nslots - 16)]
    sums = torch.zeros(ops.shape[0], dtype=torch.int64, device="cuda")
    scal = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(ops.shape[0])]
    ctx.traverse(ops, clv, dev(pm), dev(EV), n, dev(wgt), scal, sums)
    torch.cuda.synchronize()
    for s in range(16, nslots):
        assert np.array_equal(bits(clv[s].cpu().numpy()), bits(clv_h[s])), s
    assert np.array_equal(sums.cpu().numpy(), esums)
    for j in range(ops.shape[0]):
        assert np.array_equal(scal[j].cpu().numpy(), escal[j])
    # root lnL with model weights
    catw = np.array([0.1, 0.2, 0.3, 0.4])
    freq = np.array([0.3, 0.2, 0.25, 0.25])
    root = nslots - 1
    exp, esite = oracle.root_lnl(4, 4, clv_h[root], n, catw, freq, wgt, esums, site=True)
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    site = torch.zeros(n, dtype=torch.float64, device="cuda")
    ctx.root_lnl(clv[root], n, out, dev(catw), dev(freq), dev(wgt), sums, site)
    torch.cuda.synchronize()
    got = float(out.item())
    assert abs(got - exp) <= LNL_RTOL * abs(exp)
    assert np.allclose(site.cpu().numpy(), esite, rtol=1e-14, atol=0)


def test_traverse_slot_reuse_hazards(ctx, oracle):
    """A caterpillar that recycles CLV slots (write-after-read and
    write-after-write hazards): the level schedule must equal sequential order."""
    import torch

    n = 777
    rng = np.random.default_rng(3)
    tips = [rng.random(16 * n) for _ in range(5)]
    # slots 0..4 tips, 5 and 6 scratch
    ops = np.array([[5, 0, 1, 0], [6, 5, 2, 1], [5, 6, 3, 2], [6, 5, 4, 3], [5, 2, 3, 4],
                    [0, 1, 4, 0]], np.int32)
    pm = rng.random(5 * 128) * 0.5
    EV = rng.random(16)
    clv_h = [t.copy() for t in tips] + [np.zeros(16 * n), np.zeros(16 * n)]
    esums, _ = oracle.traverse(4, 4, ops, clv_h, pm, EV, n)
    clv = [dev(t) for t in tips] + [torch.zeros(16 * n, dtype=torch.float64, device="cuda") for _ in range(2)]
    sums = torch.zeros(ops.shape[0], dtype=torch.int64, device="cuda")
    ctx.traverse(ops, clv, dev(pm), dev(EV), n, None, None, sums)
    torch.cuda.synchronize()
    for s in range(7):
        assert np.array_equal(bits(clv[s].cpu().numpy()), bits(clv_h[s])), s
    assert np.array_equal(sums.cpu().numpy(), esums)


def test_traverse_rejects_bad_ops(ctx):
    import plfx
    import torch

    n = 16
    clv = [torch.zeros(16 * n, dtype=torch.float64, device="cuda") for _ in range(3)]
    pm = torch.zeros(128, dtype=torch.float64, device="cuda")
    EV = torch.zeros(16, dtype=torch.float64, device="cuda")
    for bad in ([[2, 0, 5, 0]], [[2, 0, 1, 1]], [[0, 0, 1, 0]]):
        with pytest.raises(plfx.PlfxError):
            ctx.traverse(np.array(bad, np.int32), clv, pm, EV, n)


def test_traverse_rejects_negative_n(ctx, oracle):
    """n < 0 is refused before anything is launched, fused groups included (an
    8-taxon tree is one three-level pass): nothing is written."""
    import plfx
    import torch

    ops = oracle.balanced_tree_ops(8)
    clv = [torch.full((16 * 8,), 3.0, dtype=torch.float64, device="cuda") for _ in range(15)]
    pm = torch.ones(7 * 128, dtype=torch.float64, device="cuda")
    EV = torch.ones(16, dtype=torch.float64, device="cuda")
    sums = torch.full((7,), -7, dtype=torch.int64, device="cuda")
    with pytest.raises(plfx.PlfxError, match="n < 0") as e:
        ctx.traverse(ops, clv, pm, EV, -1, None, None, sums)
    assert e.value.code == plfx.ERR_INVALID
    torch.cuda.synchronize()
    assert ctx.last_schedule() == dict.fromkeys(plfx.SCHED_KEYS, 0)
    assert all(bool((t == 3.0).all()) for t in clv) and bool((sums == -7).all())


def test_tree64_full_size_window(ctx, oracle):
    """BASELINE config 3 shape: 64-taxon balanced tree, 63 inner nodes, 2^20
    sites, f64, on the GPU; sites are independent, so a 4096-site window is
    checked bit-exactly against the oracle run on that window, and the full
    root lnL against the oracle's lnL of the GPU's root CLV."""
    import torch

    n = 1 << 20
    ntips = 64
    ops = oracle.balanced_tree_ops(ntips)
    nslots = ntips + ops.shape[0]
    g = torch.Generator(device="cuda")
    g.manual_seed(20250117)
    clv = [torch.rand(16 * n, dtype=torch.float64, device="cuda", generator=g) for _ in range(ntips)]
    clv += [torch.empty(16 * n, dtype=torch.float64, device="cuda") for _ in range(nslots - ntips)]
    pm = torch.rand(ops.shape[0] * 128, dtype=torch.float64, device="cuda", generator=g) * 0.25
    EV = torch.rand(16, dtype=torch.float64, device="cuda", generator=g) * 0.25
    sums = torch.zeros(ops.shape[0], dtype=torch.int64, device="cuda")
    scal = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(ops.shape[0])]
    ctx.traverse(ops, clv, pm, EV, n, None, scal, sums)
    sched = ctx.last_schedule()
    assert sched["deep6"] == 1 and sched["launches"] == 1, sched  # PLFX_FUSE=3 default
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    ctx.root_lnl(clv[-1], n, out, scaler_sums=sums)
    torch.cuda.synchronize()
    # per-op sums equal the scaler bytes they summarise
    gsums = sums.cpu().numpy()
    for j in range(ops.shape[0]):
        assert int(scal[j].sum().item()) == gsums[j]
    assert gsums.sum() > 0
    # window check
    lo, m = 500_003, 4096
    win = [t[16 * lo:16 * (lo + m)].cpu().numpy().copy() for t in clv[:ntips]]
    win += [np.zeros(16 * m) for _ in range(nslots - ntips)]
    rwin = [w.copy() for w in win]
    esums, escal = oracle.traverse(4, 4, ops, win, pm.cpu().numpy(), EV.cpu().numpy(), m, want_scalers=True)
    for s in range(ntips, nslots):
        assert np.array_equal(bits(clv[s][16 * lo:16 * (lo + m)].cpu().numpy()), bits(win[s])), s
    for j in range(ops.shape[0]):
        assert np.array_equal(scal[j][lo:lo + m].cpu().numpy(), escal[j])
    if oracle.ref_available(np.float64):
        # the same window through the reference's own plf(), one call per node
        rsums, rscal = oracle.ref_traverse(ops, rwin, pm.cpu().numpy(), EV.cpu().numpy(), m, want_scalers=True)
        for s in range(ntips, nslots):
            assert np.array_equal(bits(rwin[s]), bits(win[s])), s
        assert np.array_equal(rsums, esums)
        for j in range(ops.shape[0]):
            assert np.array_equal(rscal[j], escal[j])
    root = clv[-1].cpu().numpy()
    exp = oracle.root_lnl(4, 4, root, n, scaler_sums=gsums)
    assert abs(float(out.item()) - exp) <= LNL_RTOL * abs(exp)


@pytest.mark.parametrize("fuse", ["3", "2", "1", "0"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mode", ["dense", "coded", "mixed", "tipvec"])
def test_tree64_reference_golden(oracle, dtype, mode, fuse, monkeypatch):
    """configs[2] pinned by the reference itself: the 64-taxon sweep under
    every schedule (PLFX_FUSE 3: one six-level pass; 2: three-level passes +
    level pairs; 1: level pairs; 0: batched levels) reproduces
    tests/golden/tree64.npz -- the unmodified reference plf() called per inner
    node (oracle.ref_traverse) -- byte for byte: every parent CLV (sha256), the
    per-site scaler bytes and the weighted sums; dense, state-coded and mixed
    tips (tip/tip, tip/inner and inner/inner nodes), and coded tips through a
    caller tip-vector table."""
    import plfx
    import torch

    g = np.load(__import__("conftest").GOLDEN / "tree64.npz", allow_pickle=False)
    k = f"{'f32' if dtype == np.float32 else 'f64'}_{mode}"
    c = oracle.tree_golden_case(dtype, mode, int(g["n"]), int(g["seed"]))
    assert oracle.tree_case_digest(c) == str(g[f"{k}_inputs_sha256"])
    n, ops = c["n"], c["ops"]
    nops = ops.shape[0]
    monkeypatch.setenv("PLFX_FUSE", fuse)
    ctx = plfx.Context(0)
    try:
        tt = torch.float64 if dtype == np.float64 else torch.float32
        clv = [None if cd is not None else dev(t) for t, cd in zip(c["tips"], c["codes"])]
        clv += [torch.zeros(16 * n, dtype=tt, device="cuda") for _ in range(nops)]
        tips = [None if cd is None else dev(cd) for cd in c["codes"]] + [None] * nops
        sums = torch.full((nops,), -7, dtype=torch.int64, device="cuda")
        scal = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        ctx.traverse(ops, clv, dev(c["pm"]), dev(c["EV"]), n, dev(c["wgt"]), scal, sums, tips=tips,
                     tipvec=None if c["tipvec"] is None else dev(c["tipvec"]))
        torch.cuda.synchronize()
        sched = ctx.last_schedule()
    finally:
        ctx.close()
    if fuse == "3" and mode in ("dense", "coded"):
        assert sched["deep6"] == 1, sched
    got = [oracle.clv_digest(clv[int(p)].cpu().numpy()) for p in ops[:, 0]]
    bad = [j for j, (a, b) in enumerate(zip(got, g[f"{k}_x3_sha256"])) if a != str(b)]
    assert not bad, f"parent CLVs of ops {bad[:8]} differ from the reference composition ({sched})"
    assert np.array_equal(sums.cpu().numpy(), g[f"{k}_sums"])
    assert np.array_equal(np.stack([s.cpu().numpy() for s in scal]), g[f"{k}_scaler"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("tipmode", ["dense", "mixed", "coded", "left"])
def test_fused_level_pairs_match_unfused(ctx, oracle, tipmode, dtype, monkeypatch):
    """Traversals run fused three-level subtrees (f64: 7 nodes in one pass)
    and fused level pairs (parent + both children).  A 32-taxon tree with a
    caterpillar tail and dense, mixed, all-coded or left-coded tips: the
    default schedule, pairs only (PLFX_FUSE=1) and level by level (PLFX_FUSE=0)
    produce identical CLVs, scaler bytes and sums, equal to the oracle."""
    import plfx
    import torch

    n = 3001
    rng = np.random.default_rng(12)
    ops = [list(r) for r in oracle.balanced_tree_ops(32)]      # slots 32..62, root 62
    nb = len(ops)
    ops += [[63, 62, 0, nb], [64, 63, 5, nb + 1], [65, 64, 63, nb + 2]]  # tail reuses tips/inner
    ops = np.array(ops, np.int32)
    nslots, nops = 66, ops.shape[0]
    codes = [oracle.random_tip_codes(rng, n, 0.2) for _ in range(32)]
    is_coded = [{"dense": False, "mixed": t % 4 != 3, "coded": True, "left": t % 2 == 0}[tipmode]
                for t in range(32)]
    dense = [rng.random(16 * n).astype(dtype) for _ in range(32)]
    pm = (rng.random(nops * 128) * 0.3).astype(dtype)
    EV = (rng.random(16) * 0.3).astype(dtype)
    wgt = rng.integers(1, 5, n).astype(np.int32)
    host = [oracle.expand_tips(codes[t], dtype) if is_coded[t] else dense[t].copy() for t in range(32)]
    host += [np.zeros(16 * n, dtype) for _ in range(nslots - 32)]
    esums, escal = oracle.traverse(4, 4, ops, host, pm, EV, n, wgt, want_scalers=True)
    assert esums.sum() > 0

    def run(c):
        clv = [None if is_coded[t] else dev(dense[t]) for t in range(32)]
        tt = torch.float64 if dtype == np.float64 else torch.float32
        clv += [torch.zeros(16 * n, dtype=tt, device="cuda") for _ in range(nslots - 32)]
        tips = [dev(codes[t]) if is_coded[t] else None for t in range(32)] + [None] * (nslots - 32)
        sums = torch.full((nops,), -7, dtype=torch.int64, device="cuda")
        scal = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        c.traverse(ops, clv, dev(pm), dev(EV), n, dev(wgt), scal, sums, tips=tips)
        torch.cuda.synchronize()
        return clv, sums.cpu().numpy(), [x.cpu().numpy() for x in scal]

    results = [run(ctx)]
    for level in ("1", "0"):
        monkeypatch.setenv("PLFX_FUSE", level)
        c = plfx.Context(0)
        try:
            results.append(run(c))
        finally:
            c.close()
    for r in results:
        for s in range(32, nslots):
            assert np.array_equal(bits(r[0][s].cpu().numpy()), bits(host[s])), s
        assert np.array_equal(r[1], esums)
        for j in range(nops):
            assert np.array_equal(r[2][j], escal[j]), j


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("tipmode", ["dense", "mixed", "coded", "left", "tipvec"])
def test_fused_six_level_subtrees(oracle, tipmode, dtype, monkeypatch):
    """PLFX_FUSE=3 (the default): complete six-level subtrees over dense
    leaves run as one 63-node pass (plf_dna_f64_deep_kernel, f32:
    plf_dna_cat_deep_kernel), also over all-coded leaves (the coded-leaf
    pass's LDS tip tables).  A 128-taxon balanced tree (two such
    passes, then the root) with a tail that reuses tips and inner slots, n not
    a multiple of the trip; with mixed / left-coded tips (or a caller tipvec
    table over a mix) the scheduler keeps the three-level passes: CLVs, scaler
    bytes and sums bit-identical to the oracle in every case."""
    import plfx
    import torch

    n = 1001
    rng = np.random.default_rng(31)
    ntax = 128
    ops = [list(r) for r in oracle.balanced_tree_ops(ntax)]  # root = slot 2*ntax-2
    nb = len(ops)
    root = 2 * ntax - 2
    ops += [[root + 1, root, 0, nb], [root + 2, root + 1, 5, nb + 1], [root + 3, root + 2, root + 1, nb + 2]]
    ops = np.array(ops, np.int32)
    nslots, nops = root + 4, ops.shape[0]
    codes = [oracle.random_tip_codes(rng, n, 0.2) for _ in range(ntax)]
    is_coded = [{"dense": False, "mixed": t % 4 != 3, "coded": True, "left": t % 2 == 0,
                 "tipvec": t % 3 != 0}[tipmode] for t in range(ntax)]
    tv = rng.random(64).astype(dtype) if tipmode == "tipvec" else None
    dense = [rng.random(16 * n).astype(dtype) for _ in range(ntax)]
    pm = (rng.random(nops * 128) * 0.3).astype(dtype)
    EV = (rng.random(16) * 0.3).astype(dtype)
    wgt = rng.integers(1, 5, n).astype(np.int32)
    host = [oracle.expand_tips(codes[t], dtype, tipvec=tv) if is_coded[t] else dense[t].copy()
            for t in range(ntax)]
    host += [np.zeros(16 * n, dtype) for _ in range(nslots - ntax)]
    esums, escal = oracle.traverse(4, 4, ops, host, pm, EV, n, wgt, want_scalers=True)
    assert esums.sum() > 0

    monkeypatch.setenv("PLFX_FUSE", "3")
    c = plfx.Context(0)
    try:
        clv = [None if is_coded[t] else dev(dense[t]) for t in range(ntax)]
        tt = torch.float64 if dtype == np.float64 else torch.float32
        clv += [torch.zeros(16 * n, dtype=tt, device="cuda") for _ in range(nslots - ntax)]
        tips = [dev(codes[t]) if is_coded[t] else None for t in range(ntax)] + [None] * (nslots - ntax)
        sums = torch.full((nops,), -7, dtype=torch.int64, device="cuda")
        scal = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        c.traverse(ops, clv, dev(pm), dev(EV), n, dev(wgt), scal, sums, tips=tips,
                   tipvec=None if tv is None else dev(tv))
        torch.cuda.synchronize()
        sched = c.last_schedule()
    finally:
        c.close()
    deep = tipmode in ("dense", "coded")
    assert sched["deep6"] == (2 if deep else 0), sched
    for s_ in range(ntax, nslots):
        assert np.array_equal(bits(clv[s_].cpu().numpy()), bits(host[s_])), s_
    assert np.array_equal(sums.cpu().numpy(), esums)
    for j in range(nops):
        assert np.array_equal(scal[j].cpu().numpy(), escal[j]), j


@pytest.mark.parametrize("dtype,coded", [(np.float64, False), (np.float32, False), (np.float64, True),
                                         (np.float32, True)])
@pytest.mark.parametrize("n", [1, 7, 17, 33, 4099])
def test_six_level_pass_tiny_alignments(oracle, n, dtype, coded, monkeypatch):
    """The 63-node pass on alignments shorter than one trip (one wave
    active, partial 8/16-site blocks) and past it: a 64-taxon balanced tree
    (dense leaves, or all leaves coded) equals the oracle bit for bit,
    sums included, with nothing written past n."""
    import plfx
    import torch

    rng = np.random.default_rng(100 + n)
    ntax = 64
    ops = np.array(oracle.balanced_tree_ops(ntax), np.int32)
    nslots, nops = 2 * ntax - 1, ops.shape[0]
    dense = [rng.random(16 * n).astype(dtype) for _ in range(ntax)]
    dense[0][::3] *= 1e-30 if dtype == np.float64 else 1e-20  # some sites scale
    codes = [oracle.random_tip_codes(rng, n, 0.2) for _ in range(ntax)]
    pm = (rng.random(nops * 128) * 0.3).astype(dtype)
    if coded:  # tiny P entries on the first tip's matrices: some sites scale
        pm[:128] *= 1e-30
    EV = (rng.random(16) * 0.3).astype(dtype)
    wgt = rng.integers(1, 5, n).astype(np.int32)
    leaves = [oracle.expand_tips(codes[t], dtype) for t in range(ntax)] if coded else dense
    host = [d.copy() for d in leaves] + [np.zeros(16 * n, dtype) for _ in range(nslots - ntax)]
    esums, escal = oracle.traverse(4, 4, ops, host, pm, EV, n, wgt, want_scalers=True)
    monkeypatch.setenv("PLFX_FUSE", "3")
    c = plfx.Context(0)
    try:
        tt = torch.float64 if dtype == np.float64 else torch.float32
        # oversized buffers with sentinels past n: a tail write would land there
        big = [torch.full((16 * (n + 24),), -1.0, dtype=tt, device="cuda") for _ in range(nslots - ntax)]
        clv = [None if coded else dev(d) for d in dense] + [b[:16 * n] for b in big]
        tips = [dev(codes[t]) for t in range(ntax)] + [None] * (nslots - ntax) if coded else None
        sums = torch.full((nops,), -7, dtype=torch.int64, device="cuda")
        sbig = [torch.full((n + 24,), 7, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        c.traverse(ops, clv, dev(pm), dev(EV), n, dev(wgt), [x[:n] for x in sbig], sums, tips=tips)
        torch.cuda.synchronize()
        sched = c.last_schedule()
    finally:
        c.close()
    assert sched["deep6"] == 1 and sched["launches"] == 1, sched   # the 63-node pass ran
    for s_ in range(ntax, nslots):
        assert np.array_equal(bits(clv[s_].cpu().numpy()), bits(host[s_])), s_
        assert (big[s_ - ntax][16 * n:].cpu().numpy() == -1.0).all(), s_
    assert np.array_equal(sums.cpu().numpy(), esums)
    for j in range(nops):
        got = sbig[j].cpu().numpy()
        assert np.array_equal(got[:n], escal[j]), j
        assert (got[n:] == 7).all(), j


@pytest.mark.parametrize("dtype,coded", [(np.float64, False), (np.float32, False), (np.float64, True),
                                         (np.float32, True)])
def test_six_level_pass_chunk_queue(oracle, dtype, coded, monkeypatch):
    """The deep passes' wave-level chunk queue (plf_dna.hpp WaveQueue): one
    512-thread block (PLFX_MAX_BLOCKS=1: 8 waves) over 4099 sites -- dozens of
    dequeued chunks per wave, a ragged last one -- and the whole sweep twice
    on the same stream (the queue words reset themselves): CLVs, scaler bytes
    and sums bit-identical to the oracle both times."""
    import plfx
    import torch

    n = 4099
    rng = np.random.default_rng(4242)
    ntax = 64
    ops = np.array(oracle.balanced_tree_ops(ntax), np.int32)
    nslots, nops = 2 * ntax - 1, ops.shape[0]
    dense = [rng.random(16 * n).astype(dtype) for _ in range(ntax)]
    dense[0][::3] *= 1e-30 if dtype == np.float64 else 1e-20
    codes = [oracle.random_tip_codes(rng, n, 0.2) for _ in range(ntax)]
    pm = (rng.random(nops * 128) * 0.3).astype(dtype)
    if coded:
        pm[:128] *= 1e-30
    EV = (rng.random(16) * 0.3).astype(dtype)
    wgt = rng.integers(1, 5, n).astype(np.int32)
    leaves = [oracle.expand_tips(codes[t], dtype) for t in range(ntax)] if coded else dense
    host = [d.copy() for d in leaves] + [np.zeros(16 * n, dtype) for _ in range(nslots - ntax)]
    esums, escal = oracle.traverse(4, 4, ops, host, pm, EV, n, wgt, want_scalers=True)
    monkeypatch.setenv("PLFX_FUSE", "3")
    monkeypatch.setenv("PLFX_MAX_BLOCKS", "1")
    c = plfx.Context(0)
    try:
        tt = torch.float64 if dtype == np.float64 else torch.float32
        for rep in range(2):
            clv = [None if coded else dev(d) for d in dense] + [torch.full((16 * n,), float("nan"), dtype=tt,
                                                                         device="cuda")
                                                              for _ in range(nslots - ntax)]
            tips = [dev(codes[t]) for t in range(ntax)] + [None] * (nslots - ntax) if coded else None
            sums = torch.full((nops,), -7, dtype=torch.int64, device="cuda")
            scal = [torch.full((n,), 7, dtype=torch.uint8, device="cuda") for _ in range(nops)]
            c.traverse(ops, clv, dev(pm), dev(EV), n, dev(wgt), scal, sums, tips=tips)
            torch.cuda.synchronize()
            assert c.last_schedule()["deep6"] == 1
            for s_ in range(ntax, nslots):
                assert np.array_equal(bits(clv[s_].cpu().numpy()), bits(host[s_])), (rep, s_)
            assert np.array_equal(sums.cpu().numpy(), esums), rep
            for j in range(nops):
                assert np.array_equal(scal[j].cpu().numpy(), escal[j]), (rep, j)
    finally:
        c.close()


def _balanced_ops(tips, slot, pmat):
    """Level-order ops of a balanced subtree over `tips` (a power of two)."""
    ops, level = [], list(tips)
    while len(level) > 1:
        nxt = []
        for i in range(0, len(level), 2):
            ops.append([slot, level[i], level[i + 1], pmat])
            nxt.append(slot)
            slot, pmat = slot + 1, pmat + 1
        level = nxt
    return ops, level[0], slot, pmat


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("tipmode", ["dense", "half"])
def test_fused_depth4_depth5_subtrees(oracle, tipmode, dtype, monkeypatch):
    """The deep pass at depth 5 and 4 (31 and 15 ops): a 53-taxon tree made
    of a balanced 16-taxon subtree, a balanced 32-taxon subtree and a
    caterpillar over the rest.  Dense tips: both subtrees run as one deep pass
    each; "half": the first 16 tips of the 32-taxon subtree are coded, so it
    falls back to a depth-4 deep pass over its dense half plus three-level
    passes.  CLVs, scaler bytes and sums bit-identical to the oracle."""
    import plfx
    import torch

    n = 777
    rng = np.random.default_rng(45)
    ntax = 53
    ops_a, ra, slot, pmat = _balanced_ops(range(0, 16), ntax, 0)
    ops_b, rb, slot, pmat = _balanced_ops(range(16, 48), slot, pmat)
    ops = ops_a + ops_b + [[slot, ra, rb, pmat]]
    slot, pmat = slot + 1, pmat + 1
    for t in range(48, ntax):
        ops.append([slot, slot - 1, t, pmat])
        slot, pmat = slot + 1, pmat + 1
    ops = np.array(ops, np.int32)
    nslots, nops = slot, ops.shape[0]
    codes = [oracle.random_tip_codes(rng, n, 0.2) for _ in range(ntax)]
    is_coded = [tipmode == "half" and 16 <= t < 32 for t in range(ntax)]
    dense = [rng.random(16 * n).astype(dtype) for _ in range(ntax)]
    pm = (rng.random(nops * 128) * 0.3).astype(dtype)
    EV = (rng.random(16) * 0.3).astype(dtype)
    wgt = rng.integers(1, 5, n).astype(np.int32)
    host = [oracle.expand_tips(codes[t], dtype) if is_coded[t] else dense[t].copy() for t in range(ntax)]
    host += [np.zeros(16 * n, dtype) for _ in range(nslots - ntax)]
    esums, escal = oracle.traverse(4, 4, ops, host, pm, EV, n, wgt, want_scalers=True)
    assert esums.sum() > 0

    monkeypatch.setenv("PLFX_FUSE", "3")
    c = plfx.Context(0)
    try:
        tt = torch.float64 if dtype == np.float64 else torch.float32
        clv = [None if is_coded[t] else dev(dense[t]) for t in range(ntax)]
        clv += [torch.zeros(16 * n, dtype=tt, device="cuda") for _ in range(nslots - ntax)]
        tips = [dev(codes[t]) if is_coded[t] else None for t in range(ntax)] + [None] * (nslots - ntax)
        sums = torch.full((nops,), -7, dtype=torch.int64, device="cuda")
        scal = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        c.traverse(ops, clv, dev(pm), dev(EV), n, dev(wgt), scal, sums, tips=tips)
        torch.cuda.synchronize()
        sched = c.last_schedule()
    finally:
        c.close()
    if tipmode == "dense":  # the 16-taxon subtree one depth-4 pass, the 32-taxon one depth-5
        assert sched["deep5"] == 1 and sched["deep4"] == 1, sched
    else:  # the mixed 32-taxon subtree splits: its dense half and its coded half
        # (the coded-leaf pass) run depth-4 each, beside the 16-taxon subtree's
        assert sched["deep5"] == 0 and sched["deep4"] >= 3, sched
    for s_ in range(ntax, nslots):
        assert np.array_equal(bits(clv[s_].cpu().numpy()), bits(host[s_])), s_
    assert np.array_equal(sums.cpu().numpy(), esums)
    for j in range(nops):
        assert np.array_equal(scal[j].cpu().numpy(), escal[j]), j


def _run_schedule_case(oracle, tree, mode, fuse, monkeypatch):
    """One traversal (f64, 33 sites, sums and scaler bytes) of a tree of
    tests/test_trav_plan.py under PLFX_FUSE=fuse, checked bit for bit against
    the oracle; returns Context.last_schedule()."""
    import plfx
    import torch
    from test_trav_plan import _mask, _tree

    n, dtype = 33, np.float64
    ops, nslots, ntax = _tree(tree)
    nops = ops.shape[0]
    is_coded = _mask(nslots, ntax, mode)[:ntax]
    rng = np.random.default_rng(77)
    codes = [oracle.random_tip_codes(rng, n, 0.2) for _ in range(ntax)]
    dense = [rng.random(16 * n).astype(dtype) for _ in range(ntax)]
    pm = (rng.random(nops * 128) * 0.3).astype(dtype)
    EV = (rng.random(16) * 0.3).astype(dtype)
    wgt = rng.integers(1, 5, n).astype(np.int32)
    host = [oracle.expand_tips(codes[t], dtype) if is_coded[t] else dense[t].copy() for t in range(ntax)]
    host += [np.zeros(16 * n, dtype) for _ in range(nslots - ntax)]
    esums, escal = oracle.traverse(4, 4, ops, host, pm, EV, n, wgt, want_scalers=True)
    assert esums.sum() > 0
    monkeypatch.setenv("PLFX_FUSE", str(fuse))
    c = plfx.Context(0)
    try:
        clv = [None if is_coded[t] else dev(dense[t]) for t in range(ntax)]
        clv += [torch.zeros(16 * n, dtype=torch.float64, device="cuda") for _ in range(nslots - ntax)]
        tips = [dev(codes[t]) if is_coded[t] else None for t in range(ntax)] + [None] * (nslots - ntax)
        sums = torch.full((nops,), -7, dtype=torch.int64, device="cuda")
        scal = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        c.traverse(ops, clv, dev(pm), dev(EV), n, dev(wgt), scal, sums, tips=tips)
        torch.cuda.synchronize()
        sched = c.last_schedule()
    finally:
        c.close()
    for s_ in range(ntax, nslots):
        assert np.array_equal(bits(clv[s_].cpu().numpy()), bits(host[s_])), s_
    assert np.array_equal(sums.cpu().numpy(), esums)
    for j in range(nops):
        assert np.array_equal(scal[j].cpu().numpy(), escal[j]), j
    return sched


# kernel launches of each case at PLFX_FUSE 3, 2 (measured before the planner
# was split off plfx_traverse_tips: the issue order of the launches is part of
# what graph captures replay)
SCHEDULE_LAUNCHES = {("b16", "dense"): (1, 2), ("b64", "dense"): (1, 2), ("b64", "left"): (2, 2),
                     ("b64", "mixed"): (4, 4), ("taxa53", "dense"): (8, 9), ("taxa53", "half"): (10, 10)}


@pytest.mark.parametrize("fuse", [3, 2])
@pytest.mark.parametrize("tree,mode", list(SCHEDULE_LAUNCHES))
def test_schedule_is_the_planners(oracle, tree, mode, fuse, monkeypatch):
    """What the library reports and runs is the planner's answer: the counts
    tests/test_trav_plan.py pins on the CPU are last_schedule()'s on the GPU
    (and the launch count is unchanged), with CLVs, scaler bytes and sums
    bit-identical to the oracle."""
    from test_trav_plan import PINNED

    sched = _run_schedule_case(oracle, tree, mode, fuse, monkeypatch)
    counts = next(row[2 + (3 - fuse)] for row in PINNED if row[0] == tree and mode in row[1])
    keys = ("deep6", "deep5", "deep4", "septets", "triples", "unfused")
    assert [sched[k] for k in keys] == counts, sched
    assert sched["launches"] == SCHEDULE_LAUNCHES[(tree, mode)][3 - fuse], sched


def _tree_driver_expected(oracle, taxa, n, seed, alpha=0.5):
    """Re-derive plfx_tree's inputs (std::mt19937 + uniform_real_distribution,
    restated by the oracle) and its GTR+G4 lnL by an independent numpy pruning
    with scipy.linalg.expm."""
    import plfx
    from scipy.linalg import expm

    nops = taxa - 1
    _, u = oracle.mt_draws(seed, 2 * nops + 2 * taxa * n + 16)
    blen = 0.01 + 0.3 * u[:2 * nops]
    k = 2 * nops
    codes = np.empty((taxa, n), np.uint8)
    for t in range(taxa):
        for i in range(n):
            if u[k] < 0.05:
                codes[t, i] = 1 + int(u[k + 1] * 15)
            else:
                codes[t, i] = (1, 2, 4, 8)[int(u[k + 1] * 4) & 3]
            k += 2
    exch = np.array([1.2, 3.9, 0.8, 1.1, 4.6, 1.0])
    freqs = np.array([0.31, 0.19, 0.22, 0.28])
    pi = freqs / freqs.sum()
    R = np.zeros((4, 4))
    R[np.triu_indices(4, 1)] = exch
    R = R + R.T
    Q = R * pi[None, :]
    np.fill_diagonal(Q, -Q.sum(axis=1))
    Q /= -(pi * np.diag(Q)).sum()
    rates = plfx.gamma_rates(alpha, 4)
    ops = oracle.balanced_tree_ops(taxa)
    clvs = {t: (oracle.expand_tips(codes[t]).reshape(n, 4, 4), np.zeros(n)) for t in range(taxa)}
    for p, c1, c2, m in ops:
        out = None
        for child, bl in ((c1, blen[2 * m]), (c2, blen[2 * m + 1])):
            x = clvs[child][0]
            uu = np.stack([x[:, c, :] @ expm(Q * rates[c] * bl).T for c in range(4)], axis=1)
            out = uu if out is None else out * uu
        mx = out.reshape(n, -1).max(axis=1)
        clvs[p] = (out / mx[:, None, None], clvs[c1][1] + clvs[c2][1] + np.log(mx))
    root, logs = clvs[ops[-1][0]]
    return float(np.sum(np.log(np.einsum("c,ncs,s->n", np.full(4, 0.25), root, pi)) + logs))


def test_tree_driver_end_to_end(oracle):
    """The C++ tree driver (host/plfx_tree.cpp: model -> device P -> fused
    traversal -> root lnL): its lnL equals an independent numpy pruning of the
    same inputs within 1e-10; dense tips, coded tips and PLFX_FUSE=0 give the
    bit-identical lnL; f32 within 1e-4; --devices (sites split over a GPU
    list) within 1e-12 of one GPU."""
    import os
    import subprocess
    from pathlib import Path

    exe = Path(__file__).resolve().parents[1] / "amd-versal-phylogenetic-likelihood-function_amd" / "build" / "plfx_tree"
    taxa, n, seed = 16, 3000, 11

    def lnl(*extra, env=None):
        r = subprocess.run([str(exe), str(taxa), str(n), "2", "--seed", str(seed), *extra],
                           capture_output=True, text=True, timeout=120,
                           env={**os.environ, **(env or {})})
        assert r.returncode == 0, r.stderr
        line = [x for x in r.stdout.splitlines() if x.startswith("lnL = ")][-1]
        return line.split("= ")[1]

    expect = _tree_driver_expected(oracle, taxa, n, seed)
    dense, coded = lnl(), lnl("--tips")
    pairs = lnl("--tips", env={"PLFX_FUSE": "1"})
    plain = lnl("--tips", env={"PLFX_FUSE": "0"})
    assert dense == coded == pairs == plain
    assert abs(float(dense) - expect) <= 1e-10 * abs(expect)
    f32 = float(lnl("--dtype", "f32", "--tips"))
    assert abs(f32 - expect) <= 1e-4 * abs(expect)
    # sites split over a GPU list (one context per entry; two on the box's one
    # GPU, three blocks of 1000 sites): per-block lnLs summed in list order
    # (RCCL refuses a device listed twice: such lists reduce on the host)
    for extra in (["--devices", "0,0"], ["--tips", "--devices", "0,0,0"]):
        split = float(lnl(*extra, "--reduce", "host"))
        assert abs(split - float(dense)) <= 1e-12 * abs(float(dense))
        assert abs(split - expect) <= 1e-10 * abs(expect)
    prot = [float(lnl("--states", "20", "--fma", "--tips", *d))
            for d in ([], ["--devices", "0,0", "--reduce", "host"])]
    assert abs(prot[1] - prot[0]) <= 1e-12 * abs(prot[0])


def _run_driver(exe, *args):
    import subprocess

    r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=120)
    return r


def test_tree_driver_rccl_allreduce():
    """The C++ tree driver's one RCCL all-reduce (plfx_rccl.hpp: ncclCommInitAll
    over --devices, a grouped ncclAllReduce of the f64 lnL and the int64
    scaler totals of every inner node) at world 1 on the box's one GPU: the
    same lnL as the host-summed path within 1e-12 and the same scaler totals
    exactly, the reduction named on stdout; a device listed twice is refused
    with a message (no silent fallback to the host sum)."""
    import re
    from pathlib import Path

    exe = Path(__file__).resolve().parents[1] / "amd-versal-phylogenetic-likelihood-function_amd" / "build" / "plfx_tree"
    out = {}
    for red in ("rccl", "host"):
        for extra in ([], ["--tips", "--states", "20", "--fma"]):
            r = _run_driver(exe, 16, 5000, 2, "--seed", 5, "--devices", 0, "--reduce", red, *extra)
            assert r.returncode == 0, r.stderr
            assert f"reduce = {red} (1 " in r.stdout
            lnl = float(re.search(r"^lnL = (\S+)$", r.stdout, re.M).group(1))
            ev = int(re.search(r"scaling events \(last sweep\)\s+\|\s+(\d+)", r.stdout).group(1))
            out[(red, len(extra))] = (lnl, ev)
    for k in (0, 4):
        (a, ea), (b, eb) = out[("rccl", k)], out[("host", k)]
        assert abs(a - b) <= 1e-12 * abs(b) and ea == eb and ea > 0
    # the default: RCCL over >= 2 distinct GPUs, else the host sum (ADVICE r05:
    # a one-GPU run or a repeated list does not depend on RCCL initialising)
    assert "reduce = host (1 part" in _run_driver(exe, 16, 5000, 1, "--devices", 0).stdout
    rep = _run_driver(exe, 16, 5000, 1, "--devices", "0,0")
    assert rep.returncode == 0 and "reduce = host (2 parts" in rep.stdout
    bad = _run_driver(exe, 16, 5000, 1, "--devices", "0,0", "--reduce", "rccl")
    assert bad.returncode != 0 and "distinct GPUs" in bad.stderr


def _random_tree_ops(rng, ntips, recycle):
    """Random topology: merge two random pool members until one is left.
    recycle=True reuses the slots of consumed inner nodes for later parents
    (write-after-read / write-after-write hazards for the scheduler)."""
    pool = list(range(ntips))
    free, nxt, ops = [], ntips, []
    while len(pool) > 1:
        i, j = sorted(rng.choice(len(pool), 2, replace=False))
        a, b = pool[j], pool[i]
        pool.pop(j)
        pool.pop(i)
        if recycle and free:
            p = free.pop(0)
        else:
            p, nxt = nxt, nxt + 1
        ops.append((p, a, b, len(ops)))
        for c in (a, b):
            if c >= ntips and recycle:
                free.append(c)
        pool.append(p)
    return np.array(ops, np.int32), nxt


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_random_trees_match_oracle(ctx, oracle, seed, dtype):
    """Random topologies (with and without slot recycling) and a random mix of
    coded / dense tips: the scheduled (levels + fused pairs) traversal equals
    the oracle's sequential one bit for bit, scaler sums included; the oracle's
    equals the reference's plf() composed per op (oracle/_ref, shipped)."""
    import torch

    rng = np.random.default_rng(seed)
    ntips, n = 24, 1537
    ops, nslots = _random_tree_ops(rng, ntips, recycle=bool(seed % 2))
    nops = ops.shape[0]
    coded = rng.random(ntips) < 0.6
    codes = [oracle.random_tip_codes(rng, n, 0.2) for _ in range(ntips)]
    dense = [rng.random(16 * n).astype(dtype) for _ in range(ntips)]
    pm = (rng.random(nops * 128) * 0.3).astype(dtype)
    EV = (rng.random(16) * 0.3).astype(dtype)
    wgt = rng.integers(1, 4, n).astype(np.int32)
    host = [oracle.expand_tips(codes[t], dtype) if coded[t] else dense[t].copy() for t in range(ntips)]
    host += [np.zeros(16 * n, dtype) for _ in range(nslots - ntips)]
    ref = [h.copy() for h in host]
    esums, escal = oracle.traverse(4, 4, ops, host, pm, EV, n, wgt, want_scalers=True)
    if oracle.ref_available(dtype):  # and the reference's own plf(), one call per op
        rsums, _ = oracle.ref_traverse(ops, ref, pm, EV, n, wgt)
        assert np.array_equal(rsums, esums)
        for s in range(ntips, nslots):
            assert np.array_equal(bits(ref[s]), bits(host[s])), s
    tt = torch.float64 if dtype == np.float64 else torch.float32
    clv = [None if coded[t] else dev(dense[t]) for t in range(ntips)]
    clv += [torch.zeros(16 * n, dtype=tt, device="cuda") for _ in range(nslots - ntips)]
    tips = [dev(codes[t]) if coded[t] else None for t in range(ntips)] + [None] * (nslots - ntips)
    sums = torch.zeros(nops, dtype=torch.int64, device="cuda")
    scal = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(nops)]
    ctx.traverse(ops, clv, dev(pm), dev(EV), n, dev(wgt), scal, sums, tips=tips)
    torch.cuda.synchronize()
    for s in range(ntips, nslots):
        assert np.array_equal(bits(clv[s].cpu().numpy()), bits(host[s])), s
    assert np.array_equal(sums.cpu().numpy(), esums)
    for j in range(nops):
        assert np.array_equal(scal[j].cpu().numpy(), escal[j]), j


@pytest.mark.parametrize("n", [1, 5, 8, 9, 15, 17, 33, 257])
@pytest.mark.parametrize("tipmode", ["dense", "left", "coded"])
@pytest.mark.parametrize("taxa,dtype", [(8, np.float64), (4, np.float64), (8, np.float32),
                                        (4, np.float32)])
def test_single_subtree_tails(ctx, oracle, n, tipmode, taxa, dtype):
    """An 8-taxon balanced tree is exactly one fused seven-node pass (f64; f32:
    two level-pair passes and a node), a 4-taxon tree one level-pair pass.
    Site counts around the kernels' 8- and 16-site blocks (tails, n < one
    block, clamped loads past n) with each tip kind, against the oracle; the
    weights and the scaling threshold are exercised (P x0.02 makes the deeper
    nodes underflow), and nothing may be written past n."""
    import torch

    rng = np.random.default_rng(1000 + n)
    ops = oracle.balanced_tree_ops(taxa)
    nops = taxa - 1
    nslots = taxa + nops
    tt = torch.float64 if dtype == np.float64 else torch.float32
    coded = [{"dense": False, "left": t % 2 == 0, "coded": True}[tipmode] for t in range(taxa)]
    codes = [oracle.random_tip_codes(rng, n, 0.3) for _ in range(taxa)]
    dense = [rng.random(16 * n).astype(dtype) for _ in range(taxa)]
    pm = (rng.random(nops * 128) * 0.02).astype(dtype)
    EV = rng.random(16).astype(dtype)
    wgt = rng.integers(0, 7, n).astype(np.int32)
    host = [oracle.expand_tips(codes[t], dtype) if coded[t] else dense[t].copy() for t in range(taxa)]
    host += [np.zeros(16 * n, dtype) for _ in range(nops)]
    esums, escal = oracle.traverse(4, 4, ops, host, pm, EV, n, wgt, want_scalers=True)
    clv = [None if coded[t] else dev(dense[t]) for t in range(taxa)]
    big = [torch.full((16 * (n + 8),), -1.0, dtype=tt, device="cuda") for _ in range(nops)]
    clv += [b[:16 * n] for b in big]  # views: nothing may land past n
    tips = [dev(codes[t]) if coded[t] else None for t in range(taxa)] + [None] * nops
    sums = torch.full((nops,), -5, dtype=torch.int64, device="cuda")
    scal = [torch.full((n + 8,), 7, dtype=torch.uint8, device="cuda") for _ in range(nops)]
    ctx.traverse(ops, clv, dev(pm), dev(EV), n, dev(wgt), [s[:n] for s in scal], sums, tips=tips)
    torch.cuda.synchronize()
    for s in range(taxa, nslots):
        assert np.array_equal(bits(clv[s].cpu().numpy()), bits(host[s])), s
        assert (big[s - taxa][16 * n:].cpu().numpy() == -1.0).all(), s
    assert np.array_equal(sums.cpu().numpy(), esums)
    for j in range(nops):
        got = scal[j].cpu().numpy()
        assert np.array_equal(got[:n], escal[j]), j
        assert (got[n:] == 7).all(), j  # nothing written past n


def _signed_zero_field(rng, size, dtype, neg=True):
    """Values built to hit the sign of zero: +-0.0 entries, negative entries,
    products that underflow (see test_oracle.test_ump_chain_start_is_exact)."""
    v = rng.random(size).astype(dtype)
    if neg:
        v = v - dtype(0.5)
    r = rng.random(size)
    v[r < 0.3] = dtype(0.0)
    v[(r >= 0.3) & (r < 0.5)] = dtype(-0.0)
    v[(r >= 0.5) & (r < 0.55)] *= np.finfo(dtype).tiny
    return v


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fuse", ["0", "1", "2", "3"])
def test_signed_zero_inputs_bitexact(ctx, oracle, dtype, fuse, monkeypatch):
    """The kernels start ump chains at the first product (plf_dna.hpp,
    site_cat); on inputs full of +-0.0, negative matrix entries and underflow,
    the node kernel and every traversal schedule (one launch per level, fused
    level pairs, fused three-level subtrees, the depth-4 deep pass that
    PLFX_FUSE=3 takes for a 16-taxon tree) still equal the oracle's plf()
    order bit for bit."""
    import plfx
    import torch

    rng = np.random.default_rng(99)
    n = 3001
    tt = torch.float64 if dtype == np.float64 else torch.float32
    # one node through plf_dev
    x1, x2 = _signed_zero_field(rng, 16 * n, dtype), _signed_zero_field(rng, 16 * n, dtype)
    EV, L, R = (_signed_zero_field(rng, s, dtype) for s in (16, 64, 64))
    e3, esc, einc = oracle.plf(x1, x2, EV, L, R)
    o3 = torch.empty(16 * n, dtype=tt, device="cuda")
    sc = torch.empty(n, dtype=torch.uint8, device="cuda")
    s = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.plf_dev(dev(x1), dev(x2), o3, dev(EV), dev(L), dev(R), None, sc, s)
    torch.cuda.synchronize()
    assert np.array_equal(bits(o3.cpu().numpy()), bits(e3))
    assert np.array_equal(sc.cpu().numpy(), esc) and int(s.item()) == einc
    # a 16-taxon tree under the schedule PLFX_FUSE selects (read at context creation)
    monkeypatch.setenv("PLFX_FUSE", fuse)
    with plfx.Context(0) as c2:
        ops = oracle.balanced_tree_ops(16)
        nops = ops.shape[0]
        tips = [_signed_zero_field(rng, 16 * n, dtype) for _ in range(16)]
        pm = _signed_zero_field(rng, nops * 128, dtype)
        wgt = rng.integers(0, 5, n).astype(np.int32)
        host = [t.copy() for t in tips] + [np.zeros(16 * n, dtype) for _ in range(nops)]
        esums, escal = oracle.traverse(4, 4, ops, host, pm, EV, n, wgt, want_scalers=True)
        clv = [dev(t) for t in tips] + [torch.zeros(16 * n, dtype=tt, device="cuda") for _ in range(nops)]
        sums = torch.zeros(nops, dtype=torch.int64, device="cuda")
        scal = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        c2.traverse(ops, clv, dev(pm), dev(EV), n, dev(wgt), scal, sums)
        torch.cuda.synchronize()
        sched = c2.last_schedule()
        if fuse == "3":
            assert sched["deep4"] == 1 and sched["launches"] == 1, sched
        elif fuse == "0":
            assert sched["unfused"] == nops, sched
        for j in range(16, 16 + nops):
            assert np.array_equal(bits(clv[j].cpu().numpy()), bits(host[j])), j
        assert np.array_equal(sums.cpu().numpy(), esums)
        for j in range(nops):
            assert np.array_equal(scal[j].cpu().numpy(), escal[j]), j


def _tree_driver_expected_protein(oracle, taxa, n, seed, alpha=0.5):
    """plfx_tree --states 20: the same draws as the DNA form (branch lengths,
    then two uniforms per tip site: X with probability 0.05, else amino acid
    int(20 u) % 20), its fixed 20-state exchangeabilities / frequencies, and an
    independent numpy pruning with scipy.linalg.expm (per-site rescaling)."""
    import plfx
    from scipy.linalg import expm

    S = 20
    nops = taxa - 1
    _, u = oracle.mt_draws(seed, 2 * nops + 2 * taxa * n + 16)
    blen = 0.01 + 0.3 * u[:2 * nops]
    k = 2 * nops
    codes = np.empty((taxa, n), np.int64)
    for t in range(taxa):
        for i in range(n):
            codes[t, i] = 22 if u[k] < 0.05 else int(u[k + 1] * 20) % 20
            k += 2
    exch = np.array([0.5 + ((j * 37) % 29) / 10.0 for j in range(190)])
    freqs = np.array([1.0 + ((s * 7) % 11) for s in range(S)])
    pi = freqs / freqs.sum()
    R = np.zeros((S, S))
    R[np.triu_indices(S, 1)] = exch
    R = R + R.T
    Q = R * pi[None, :]
    np.fill_diagonal(Q, -Q.sum(axis=1))
    Q /= -(pi * np.diag(Q)).sum()
    rates = plfx.gamma_rates(alpha, 4)
    ops = oracle.balanced_tree_ops(taxa)

    def tipclv(c):
        x = np.zeros((n, 4, S))
        one = np.where(c[:, None] >= 20, 1.0, (np.arange(S)[None, :] == c[:, None]).astype(float))
        x[:] = one[:, None, :]
        return x

    clvs = {t: (tipclv(codes[t]), np.zeros(n)) for t in range(taxa)}
    for p, c1, c2, m in ops:
        out = None
        for child, bl in ((c1, blen[2 * m]), (c2, blen[2 * m + 1])):
            x = clvs[child][0]
            uu = np.stack([x[:, c, :] @ expm(Q * rates[c] * bl).T for c in range(4)], axis=1)
            out = uu if out is None else out * uu
        mx = out.reshape(n, -1).max(axis=1)
        clvs[p] = (out / mx[:, None, None], clvs[c1][1] + clvs[c2][1] + np.log(mx))
    root, logs = clvs[ops[-1][0]]
    return float(np.sum(np.log(np.einsum("c,ncs,s->n", np.full(4, 0.25), root, pi)) + logs))


def test_tree_driver_protein(oracle):
    """plfx_tree --states 20 (20-state model -> device P -> level-batched
    protein traversal -> root lnL): within 1e-10 of an independent numpy
    pruning of the same inputs; dense and coded tips bit-identical; FMA mode
    within 1e-10; f32 within 1e-4."""
    import subprocess
    from pathlib import Path

    exe = Path(__file__).resolve().parents[1] / "amd-versal-phylogenetic-likelihood-function_amd" / "build" / "plfx_tree"
    taxa, n, seed = 16, 1500, 13

    def lnl(*extra):
        r = subprocess.run([str(exe), str(taxa), str(n), "2", "--seed", str(seed), "--states", "20", *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return [x for x in r.stdout.splitlines() if x.startswith("lnL = ")][-1].split("= ")[1]

    expect = _tree_driver_expected_protein(oracle, taxa, n, seed)
    dense, coded = lnl(), lnl("--tips")
    assert dense == coded
    assert abs(float(dense) - expect) <= 1e-10 * abs(expect)
    assert abs(float(lnl("--fma", "--tips")) - expect) <= 1e-10 * abs(expect)
    assert abs(float(lnl("--dtype", "f32", "--tips", "--fma")) - expect) <= 1e-4 * abs(expect)
