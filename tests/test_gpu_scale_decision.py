"""The 2^-32 rescale decision, position by position, in every kernel.

Every kernel ends a site with plf()'s test "all S*4 parent values strictly
below 2^-32 in magnitude", spread over lanes, ballots, LDS masks and register
chains.  The cases of oracle/scale_cases.py (checked on the oracle alone by
tests/test_scale_cases.py) put one deciding value at every position of every
lane, in sites that must scale next to sites that must not.  Each test runs
them through one entry point and asserts CLV bits (NaN by position), scaler
bytes and weighted sums equal to the oracle's, with sentinels past the last
site.  No tolerance anywhere."""
import contextlib
import functools

import numpy as np
import pytest

import scale_cases as SC

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SHIFTS = range(6)
PAD = 24                      # sentinel sites past n in every output
N_DNA = SC.full_sites(4) + SC.TAIL
N_PROT = SC.full_sites(20) + SC.TAIL
# [deep6, deep5, deep4, septets, triples, unfused] of a balanced dense tree
# (tests/test_trav_plan.py PINNED), by (taxa, PLFX_FUSE)
SCHEDULES = {
    (8, 3): [0, 0, 0, 1, 0, 0], (8, 2): [0, 0, 0, 1, 0, 0], (8, 1): [0, 0, 0, 0, 2, 1], (8, 0): [0, 0, 0, 0, 0, 7],
    (16, 3): [0, 0, 1, 0, 0, 0], (16, 2): [0, 0, 0, 2, 0, 1], (16, 1): [0, 0, 0, 0, 5, 0], (16, 0): [0, 0, 0, 0, 0, 15],
    (32, 3): [0, 1, 0, 0, 0, 0], (32, 2): [0, 0, 0, 4, 1, 0], (32, 1): [0, 0, 0, 0, 10, 1], (32, 0): [0, 0, 0, 0, 0, 31],
    (64, 3): [1, 0, 0, 0, 0, 0], (64, 2): [0, 0, 0, 9, 0, 0], (64, 1): [0, 0, 0, 0, 21, 0], (64, 0): [0, 0, 0, 0, 0, 63],
}


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(got, exp):
    nan = np.isnan(exp)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(exp[~nan]))


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tt(dtype):
    import torch

    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


@contextlib.contextmanager
def env_ctx(monkeypatch, **env):
    """A context of its own: the library reads its switches at context creation."""
    import plfx

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = plfx.Context(0)
    try:
        yield c
    finally:
        c.close()
        for k in env:
            monkeypatch.delenv(k)


@pytest.fixture
def small_grid_ctx(monkeypatch):
    """3 blocks (as tests/test_gpu_protein.py): dozens of trips per block, a
    ragged last tile."""
    with env_ctx(monkeypatch, PLFX_MAX_BLOCKS="3") as c:
        yield c


# ---- cases and their oracle results, shared by the tests that follow one another ----

@functools.lru_cache(maxsize=16)
def placed(S, dtype, n, shift, carrier="x1", fma=False):
    c = SC.placed_case(S, dtype, n, shift, carrier)
    return c, SC.run_oracle(c, fma)


@functools.lru_cache(maxsize=16)
def table(S, dtype, n, shift, hotcat=0, fma=False):
    c = SC.tiptip_case(dtype, n, shift, hotcat) if S == 4 else SC.protein_table_case(dtype, n, shift)
    return c, SC.run_oracle(c, fma)


@functools.lru_cache(maxsize=16)
def rand(S, dtype, fma=False):
    c = SC.random_case(S, dtype, 1024 + SC.TAIL, 5, fma)
    return c, SC.run_oracle(c, fma)


@functools.lru_cache(maxsize=2)
def tree(kind, S, dtype, ntips, shift, fma=False):
    n = N_DNA if S == 4 else N_PROT
    if kind == "dense":
        c = SC.tree_case(S, dtype, ntips, n, shift)
    elif kind == "coded":
        c = SC.protein_coded_tree_case(dtype, n, shift)
    else:
        c = SC.random_tree_case(dtype, 1024 + SC.TAIL, 77)
    return c, SC.run_tree_oracle(c, fma)


def sizes(S):
    """The full crossing plus the ragged tail, and a call that is all tail."""
    return [(N_DNA if S == 4 else N_PROT, s) for s in SHIFTS] + [(SC.TAIL, 1)]


# ---- one node: launch and compare ----

def run_node(ctx, c, exp, entry="dense", fma=False, valu=False, what=None):
    """One node of case c through `entry` ("dense": plf_dev / plf_dev_gen;
    "tip1" / "tip2": that child coded as gaps, the other dense; "both": the
    case's codes and table) into oversized sentinel-filled outputs; everything
    equal to the oracle's `exp`, nothing written past n."""
    import torch

    S, n = c["S"], c["n"]
    V = 4 * S
    gap = 15 if S == 4 else 23
    x3 = torch.full((V * (n + PAD),), -3.0, dtype=tt(c["EV"].dtype), device="cuda")
    sc = torch.full((n + PAD,), 0xAB, dtype=torch.uint8, device="cuda")
    s = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    t = {k: dev(c[k]) for k in ("x1", "x2", "EV", "left", "right", "wgt")}
    if entry == "dense":
        if S == 4 and not fma:
            ctx.plf_dev(t["x1"], t["x2"], x3, t["EV"], t["left"], t["right"], t["wgt"], sc, s, n=n)
        else:
            ctx.plf_dev_gen(t["x1"], t["x2"], x3, t["EV"], t["left"], t["right"], S, t["wgt"], sc, s,
                            n=n, fma=fma, valu=valu)
    else:
        junk = (np.arange(n) % 16 << 4) if S == 4 else (np.arange(n) % 3) * 50   # ignored / read as the last row
        gaps = dev((gap + junk).astype(np.uint8))
        kw = {"tip1": dict(tip1=gaps, x2=t["x2"]), "tip2": dict(x1=t["x1"], tip2=gaps),
              "both": dict(tip1=dev(c["c1"]), tip2=dev(c["c2"]), tipvec=dev(c["tipvec"])) if "c1" in c else None}[entry]
        ctx.plf_tips_dev(x3, t["EV"], n, t["left"], t["right"], wgt=t["wgt"], scaler=sc, scaler_sum=s,
                         states=S, fma=fma, **kw)
    torch.cuda.synchronize()
    compare(x3.cpu().numpy(), sc.cpu().numpy(), s.cpu().numpy(), exp, n, V, what)


def compare(x3, sc, s, exp, n, V, what=None):
    e3, esc, einc = exp
    assert same(x3[:V * n], e3), what
    assert np.array_equal(sc[:n], esc), what
    assert s.tolist() == [einc, -1], what
    assert (x3[V * n:] == -3.0).all() and (sc[n:] == 0xAB).all(), what


def node_cases(S, dtype, entry, fma=False):
    """(case, oracle result, label) over the shifts and sizes for one entry."""
    for n, shift in sizes(S):
        if entry == "both":
            hots = range(4) if S == 4 else (0,)
            for h in hots:
                yield (*table(S, dtype, n, shift, h, fma), (n, shift, h))
        else:
            yield (*placed(S, dtype, n, shift, "x2" if entry == "tip1" else "x1", fma), (n, shift))


# ---- DNA dense node ----

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", ["default", "segments", "one_block"])
def test_dna_node(ctx, monkeypatch, dtype, path):
    """plf_dev: four lanes a site, __ballot and a nibble test, the tail copy
    with its `valid &&` term; also the eight-segment mapping and one block
    making every trip."""
    env = {"default": {}, "segments": {"PLFX_NODE_SEGMENTS": "1"}, "one_block": {"PLFX_MAX_BLOCKS": "1"}}[path]
    with contextlib.nullcontext(ctx) if not env else env_ctx(monkeypatch, **env) as c:
        for case, exp, what in node_cases(4, dtype, "dense"):
            run_node(c, case, exp, what=what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dna_host_entries(ctx, dtype):
    """The host-array plf() and the instance-buffer entry, once each."""
    import plfx
    import torch

    case, (e3, esc, einc) = placed(4, dtype, N_DNA, 2)
    n = case["n"]
    x3 = np.full(16 * (n + PAD), -3.0, dtype)
    inc = ctx.plf(case["x1"], case["x2"], x3, case["EV"], n, case["left"], case["right"], case["wgt"])
    assert same(x3[:16 * n], e3) and inc == einc and (x3[16 * n:] == -3.0).all()
    tb = plfx.Testbench(n, 1, 1024, plfx.LAYOUT_SEPARATE, plfx.AIE_WINDOW)
    L, R = tb.pack_instance(0, case["EV"], case["left"], case["right"], case["x1"], case["x2"])
    dO = torch.full((tb.instance_elements_out(),), -3.0, dtype=tt(dtype), device="cuda")
    dS = torch.full((n + PAD,), 0xAB, dtype=torch.uint8, device="cuda")
    ctx.instance_run(dev(L), dev(R), dO, dS, n, 1024, plfx.LAYOUT_SEPARATE)
    torch.cuda.synchronize()
    o, sb = dO.cpu().numpy(), dS.cpu().numpy()
    assert same(o[:16 * n], e3) and np.array_equal(sb[:n], esc)
    assert (o[16 * n:] == -3.0).all() and (sb[n:] == 0xAB).all()


# ---- DNA coded children ----

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", ["tip1", "tip2", "both"])
def test_dna_coded_children(ctx, dtype, entry):
    """plf_tips_dev: tip/inner and inner/tip with the dense child carrying the
    pattern and the coded child all gaps; tip/tip through a caller table of
    thr, below, -thr, 0 and subnormal rows, each category deciding in turn."""
    for case, exp, what in node_cases(4, dtype, entry):
        run_node(ctx, case, exp, entry, what=what)


# ---- batches ----

def run_batch(ctx, S, dtype, nnodes, n):
    """Node j is the placed case of shift j; launched twice."""
    import torch

    V = 4 * S
    cases = [placed(S, dtype, n, j) for j in range(nnodes)]
    c0 = cases[0][0]
    nodes = []
    for j, (c, _) in enumerate(cases):
        nd = {"x1": dev(c["x1"]), "x2": dev(c["x2"]), "left": dev(c["left"]), "right": dev(c["right"]),
              "x3": torch.empty(V * (n + PAD), dtype=tt(dtype), device="cuda"),
              "scaler": torch.empty(n + PAD, dtype=torch.uint8, device="cuda"),
              "scaler_sum": torch.empty(2, dtype=torch.int64, device="cuda")}
        nodes.append(nd)
    EV, wgt = dev(c0["EV"]), dev(c0["wgt"])
    for rep in range(2):
        for nd in nodes:
            nd["x3"].fill_(-3.0)
            nd["scaler"].fill_(0xAB)
            nd["scaler_sum"].fill_(-1)
        ctx.plf_batch_dev(nodes, EV, n, wgt, states=S)
        torch.cuda.synchronize()
        for j, (nd, (_, exp)) in enumerate(zip(nodes, cases)):
            compare(nd["x3"].cpu().numpy(), nd["scaler"].cpu().numpy(), nd["scaler_sum"].cpu().numpy(),
                    exp, n, V, (rep, j))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nnodes", [3, 33])
def test_dna_batch(ctx, dtype, nnodes):
    """plf_batch_dev (blockIdx.y selects the node): node j has shift j, so a
    kernel that mixes nodes up shows."""
    run_batch(ctx, 4, dtype, nnodes, N_DNA)
    run_batch(ctx, 4, dtype, 3, SC.TAIL)


@pytest.mark.parametrize("dtype", DTYPES)
def test_protein_batch(ctx, dtype):
    """plf_batch_dev at S = 20 (the exact LDS batch kernel), 3 nodes of
    different shifts."""
    run_batch(ctx, 20, dtype, 3, N_PROT)
    run_batch(ctx, 20, dtype, 3, SC.TAIL)


# ---- traversals ----

def run_tree(ctx, case, exp, fma=False):
    """The whole traversal of a tree case: every inner CLV, every op's scaler
    bytes and sum equal to the oracle's, nothing past n.  Returns the schedule."""
    import torch

    S, n, ops = case["S"], case["n"], case["ops"]
    V, nops, ntips = 4 * S, case["ops"].shape[0], len(case["tips"])
    host, esums, escal = exp
    dt = tt(case["EV"].dtype)
    coded = case["codes"] is not None
    big = [torch.full((V * (n + PAD),), -3.0, dtype=dt, device="cuda") for _ in range(nops)]
    clv = [None if coded else dev(t) for t in case["tips"]] + [b[:V * n] for b in big]
    tips = [dev(c) for c in case["codes"]] + [None] * nops if coded else None
    sums = torch.full((nops + 1,), -7, dtype=torch.int64, device="cuda")
    sbig = [torch.full((n + PAD,), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(nops)]
    ctx.traverse(ops, clv, dev(case["pm"]), dev(case["EV"]), n, dev(case["wgt"]), [x[:n] for x in sbig], sums,
                 tips=tips, tipvec=None if case["tipvec"] is None else dev(case["tipvec"]), states=S, fma=fma)
    torch.cuda.synchronize()
    sched = ctx.last_schedule()
    for j in range(nops):
        got = big[j].cpu().numpy()
        assert same(got[:V * n], host[ntips + j]), (j, sched)
        assert (got[V * n:] == -3.0).all(), j
        sb = sbig[j].cpu().numpy()
        assert np.array_equal(sb[:n], escal[j]) and (sb[n:] == 0xAB).all(), (j, sched)
    assert sums.cpu().numpy().tolist() == esums.tolist() + [-7]
    return sched


TREES = [(ntips, fuse, None) for ntips in (8, 16, 32, 64) for fuse in (3, 2, 1, 0)] + [(64, 3, "1")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ntips,fuse,blocks", TREES)
def test_dna_traversal(monkeypatch, dtype, ntips, fuse, blocks):
    """Balanced trees of dense taxa under every schedule: the fused pair,
    three-, four-, five- and six-level passes decide in registers at every
    inner level and feed the rescaled values on; the pattern first appears at
    a site's target level and stays as close at every level above."""
    import plfx

    env = {"PLFX_FUSE": str(fuse)}
    if blocks:
        env["PLFX_MAX_BLOCKS"] = blocks
    case, exp = tree("dense", 4, dtype, ntips, ntips % 6)
    with env_ctx(monkeypatch, **env) as c:
        sched = run_tree(c, case, exp)
    assert [sched[k] for k in plfx.SCHED_KEYS[:6]] == SCHEDULES[ntips, fuse], sched


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("leaves", ["dense", "coded"])
def test_protein_traversal(ctx, dtype, fma, leaves):
    """8 protein taxa, one launch per node or batched level: dense leaves with
    the level construction, and all-coded leaves through a caller table, where
    the children staged from the tip/tip tables decide at levels 2 and 3."""
    for shift in (1,) if leaves == "dense" else (0, 1, 2, 3):
        case, exp = tree(leaves, 20, dtype, 8, shift, fma)
        sched = run_tree(ctx, case, exp, fma)
        assert sched["unfused"] == 7, sched


# ---- protein node: the five kernels ----

KERNELS = {   # name: (dtype, fma, valu)
    "exact_f32": (np.float32, False, False),      # plf_prot_lds_kernel<float>
    "exact_f64": (np.float64, False, False),      # scalar-operand exact kernel (dense), LDS kernel (tips)
    "exact_f64_valu": (np.float64, False, True),
    "fma_f64": (np.float64, True, False),         # f64 MFMA: a site is small iff its 4 lanes agree
    "fma_f32": (np.float32, True, False),         # f32 MFMA: the folded ballot and states 16..19
    "fma_f64_valu": (np.float64, True, True),     # per-wave small_mask[0..3]
}
PROT = [(k, e) for k in KERNELS for e in (("dense",) if KERNELS[k][2] else ("dense", "tip1", "tip2", "both"))]


def run_protein(ctx, kernel, entry):
    dtype, fma, valu = KERNELS[kernel]
    for case, exp, what in node_cases(20, dtype, entry, fma):
        run_node(ctx, case, exp, entry, fma, valu, what)


@pytest.mark.parametrize("kernel,entry", PROT)
def test_protein_node(ctx, kernel, entry):
    """plf_dev_gen / plf_tips_dev at S = 20 on the default grid: each of the
    80 positions decides alone at each of the 64 sites of a tile."""
    run_protein(ctx, kernel, entry)


@pytest.mark.parametrize("kernel,entry", PROT)
def test_protein_node_small_grid(small_grid_ctx, kernel, entry):
    """The same on 3 blocks: many trips, a ragged last tile."""
    run_protein(small_grid_ctx, kernel, entry)


# ---- random matrices next to the threshold ----

@pytest.mark.parametrize("dtype", DTYPES)
def test_random_dna_node(ctx, dtype):
    case, exp = rand(4, dtype)
    run_node(ctx, case, exp)


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_dna_six_level_pass(monkeypatch, dtype):
    case, exp = tree("random", 4, dtype, 64, 0)
    assert all(0.25 <= sc.mean() <= 0.75 for sc in exp[2][:32])
    with env_ctx(monkeypatch, PLFX_FUSE="3") as c:
        assert run_tree(c, case, exp)["deep6"] == 1


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_random_protein_node(ctx, kernel):
    dtype, fma, valu = KERNELS[kernel]
    case, exp = rand(20, dtype, fma)
    run_node(ctx, case, exp, "dense", fma, valu)
