"""Every kernel that produces a scaler_sum, at the 2^40 weight bound.

All of them end in ticket_publish (csrc/plf_dna.hpp): an arrival count and a
signed partial sum in one 64-bit word, exact while sum |wgt| < 2^40 (plfx.h).
The rest of the suite draws weights from -1..8, so a 32-bit accumulator, a
lost sign extension of the weight load or a sign slip in the slot arithmetic
of any one kernel would pass it.  Here each family runs with weights that put
the total just under +2^40 and just above -2^40, that cancel after partial
sums beyond +-2^39, with INT32_MIN / INT32_MAX weights (n = 511, all
INT32_MIN included) and with random weights in +-((2^40 - 1) // n).

Expected values: the scaler bytes come from the oracle (oracle.plf,
plf_generic, traverse(want_scalers=True), psr_ref), once per case -- scaling
does not depend on the weights -- and the kernel's bytes must equal them; every
scaler_sum must equal sum sc*w formed in Python ints.  Outputs are prefilled
with sentinels.  After the patterns one call with wgt=None on the same context
and stream must give the count of scaled sites: the workspace went back to
zero.  Nothing here goes past the bound (a wrong election would leave the
workspace dirty for every later test; tests/test_ticket_sum.py covers that on
the CPU).

Grids: the slot arithmetic only works hard when several blocks share one of
the 32 slots, so each family's site count gives a launch of more than 32
blocks and not a multiple of 32, read from a captured graph and asserted; max
and cancel are repeated under PLFX_MAX_BLOCKS = 1 and 3.  Every family test
runs on contexts of its own (a captured stream keeps its workspace).

The host entry Context.plf returns an int: the exact sum modulo 2^32, tested
over two chunks; it accepts sum |w| = 2^40 - 1 and refuses 2^40 at n = 512."""
import functools

import numpy as np
import pytest

import oracle as O
import psr_ref
import scale_cases as SC
from test_gpu_parity import _kernel_base
from test_gpu_scale_decision import dev, env_ctx, tt

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
BOUND = 2**40 - 1
I32MAX, I32MIN = 2**31 - 1, -2**31
N_EXT = 511          # the extremes pattern: 511 * 2^31 < 2^40
PAD = 24             # sentinel bytes past n
SENT = -7            # in every sum before a launch
# Sites per family: a launch has min(ceil(n / sites per block), co-resident
# blocks / nodes in the launch) blocks along x; a block takes 64 sites
# (protein, the f64 level-pair and three-level passes) to 1024 (f32 per-site
# rates).  The sizes below keep the first term the smaller one for at least
# one launch of every kernel, and more than 32 and not a multiple of 32.
N_NODE = 2**16 + 1   # DNA node, tips: 513 (f64), 257 (f32) blocks; PSR: 129, 65
N_SEG = 67700        # the eight-segment mapping rounds down to a multiple of 8: 528 (f64), 264 (f32)
N_BATCH = 12801      # DNA batch: 101 (f64), 51 (f32) blocks a node
N_PROT = 6401        # protein node, batch, tips: 101 blocks
N_PROT_TREE = 2113   # protein traversal: 34 blocks a node
# DNA traversals: at 12801 the 6 three-level passes of taxa53 stay under their
# share (f32: 101 of 128 blocks); the f32 deep pass over b64's coded leaves
# takes 512 sites a block: 33 blocks at 16385
N_TREE = {"taxa53": 12801, "b64": 2**14 + 1}
N_QUEUE = 3 * 64 * 40 + 37   # tests/test_gpu_protein.py: 3 blocks, 121 tiles, the tile queue


# ---- weights ----

def patterns(esc, n):
    """name -> int32 weights for scaler bytes esc (a list of arrays sharing
    one weight array: the scaled set is their union)."""
    scaled = np.flatnonzero(np.any(np.stack(esc) != 0, axis=0))
    assert scaled.size > 0
    W = min(I32MAX, BOUND // scaled.size)
    R = min(I32MAX, BOUND // n)
    rng = np.random.default_rng(n + scaled.size)
    mx, cancel = np.zeros(n, np.int64), np.zeros(n, np.int64)
    mx[scaled] = W
    cancel[scaled[:scaled.size // 2]] = W
    cancel[scaled[scaled.size // 2:]] = -W
    out = {"max": mx, "min": -mx, "cancel": cancel, "random": rng.integers(-R, R + 1, n)}
    return {k: v.astype(np.int32) for k, v in out.items()}


def extremes(n=N_EXT):
    rng = np.random.default_rng(n)
    pick = np.array([I32MIN, I32MAX, -1, 0, 1], np.int64)[rng.integers(0, 5, n)]
    return {"extremes": pick.astype(np.int32), "all INT32_MIN": np.full(n, I32MIN, np.int32)}


# ---- a case: expected scaler bytes per sum, and a launcher ----

class Case:
    """esc[j]: the oracle's scaler bytes behind sum j; has_sum[j]: whether the
    launch is given an output for it; launch(ctx, wgt, stream) enqueues the
    family's call with device weights (or None) into scs (uint8 [n + PAD]
    each) and sums (int64 [len(esc) + 1])."""

    def __init__(self, n, esc, launch, nsc, has_sum=None):
        import torch

        self.n, self.esc, self._launch = n, esc, launch
        self.has_sum = has_sum or [True] * len(esc)
        self.scs = [torch.empty(n + PAD, dtype=torch.uint8, device="cuda") for _ in range(nsc)]
        self.sums = torch.empty(len(esc) + 1, dtype=torch.int64, device="cuda")

    def launch(self, ctx, w, stream=None):
        for t in self.scs:
            t.fill_(0xAB)
        self.sums.fill_(SENT)
        self._launch(ctx, w, self.scs, self.sums, stream)

    def verify(self, w, what):
        """After a launch with host weights w (None: all 1)."""
        import torch

        torch.cuda.synchronize()
        for j, (t, e) in enumerate(zip(self.scs, self.esc)):
            got = t.cpu().numpy()
            assert np.array_equal(got[:self.n], e) and (got[self.n:] == 0xAB).all(), (what, "scaler bytes", j)
        exp = [SENT if not has else int(e.sum()) if w is None else sum(w[e != 0].tolist())
               for e, has in zip(self.esc, self.has_sum)]
        got = self.sums.cpu().tolist()
        print(what, "sums", got[:4], "..." if len(got) > 5 else "")
        assert got == exp + [SENT], what


def run_patterns(ctx, case, pats, what):
    for name, w in pats.items():
        assert sum(abs(v) for v in w.tolist()) < 2**40, name   # the contract
        case.launch(ctx, dev(w))
        case.verify(w, (what, name))


def captured_grids(call):
    """[(kernel identifier, blocks along x, nodes along y, block size)] of the
    launches `call` makes, read from the kernel nodes of a captured graph as
    tests/test_gpu_parity.py _captured_grids does (gridDim.x kept apart: it is
    what a block's slot and a slot's arrivals are computed from); the graph
    is then replayed once."""
    import ctypes as C

    import torch

    import bench

    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=st):
        call(st.cuda_stream)
    hip = C.CDLL("libamdhip64.so")
    hip.hipKernelNameRefByPtr.restype = C.c_char_p
    hip.hipKernelNameRefByPtr.argtypes = [C.c_void_p, C.c_void_p]
    raw, count = C.c_void_p(int(g.raw_cuda_graph())), C.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, C.byref(count)) == 0
    nodes = (C.c_void_p * count.value)()
    assert hip.hipGraphGetNodes(raw, nodes, C.byref(count)) == 0
    out = []
    for nd in nodes:
        kind, p = C.c_int(-1), bench._KernelNodeParams.struct()()
        if hip.hipGraphNodeGetType(C.c_void_p(nd), C.byref(kind)) != 0 or kind.value != 0:
            continue  # not a kernel node
        assert hip.hipGraphKernelNodeGetParams(C.c_void_p(nd), C.byref(p)) == 0
        name = hip.hipKernelNameRefByPtr(p.func, None)
        out.append((_kernel_base(name.decode() if name else None), p.gridDim.x, p.gridDim.y * p.gridDim.z,
                    p.blockDim.x * p.blockDim.y * p.blockDim.z))
    g.instantiate()
    with torch.cuda.stream(st):
        g.replay()
    torch.cuda.synchronize()
    del g
    return out


def grids_of(ctx, case, w, kernels):
    """The launches of `kernels` in the family's call with host weights w,
    from a captured graph; the replay's results are verified too."""
    wd = dev(w)
    got = [g for g in captured_grids(lambda sh: case.launch(ctx, wd, stream=sh)) if g[0] in kernels]
    case.verify(w, "captured")
    return got


def run_family(monkeypatch, make, what, kernels, env=None, every=True):
    """make(n) -> Case on the current device (n None: the family's size).  The
    four patterns and wgt=None at the family's size, the grid, the extremes at
    n = 511, and max and cancel again on 1 and 3 blocks.  kernels: the
    sum-producing kernels the call consists of; each of their launches
    (every=False, traversals, where a level of many nodes takes its share of
    the co-resident blocks: at least one launch of each kernel) has more than
    32 blocks along x and not a multiple of 32."""
    env = env or {}
    with env_ctx(monkeypatch, **env) as c:
        case = make(None)
        pats = patterns(case.esc, case.n)
        run_patterns(c, case, pats, what)
        case.launch(c, None)
        case.verify(None, (what, "wgt=None"))
        grids = grids_of(c, case, pats["cancel"], kernels)
        print(what, "grids", sorted(set(grids)))
        hard = [g for g in grids if g[1] > 32 and g[1] % 32]
        assert {g[0] for g in hard} == set(kernels) and (hard == grids or not every), grids
        small = make(N_EXT)
        run_patterns(c, small, extremes(), (what, N_EXT))
        small.launch(c, None)
        small.verify(None, (what, N_EXT, "wgt=None"))
    for blocks in ("1", "3"):
        with env_ctx(monkeypatch, PLFX_MAX_BLOCKS=blocks, **env) as c:
            run_patterns(c, case, {k: pats[k] for k in ("max", "cancel")}, (what, "blocks", blocks))
            case.launch(c, None)
            case.verify(None, (what, "blocks", blocks, "wgt=None"))


def mixed(esc, n):
    """Both outcomes of the rescale decision occur."""
    ones = int(np.sum(esc))
    assert 0 < ones < np.size(esc) and np.size(esc) % n == 0, ones
    return esc


def shrink(rng, x, n, lo, hi):
    """Each site of the CLV x times 2^-e, e uniform in [lo, hi): exact, and
    sites cross the 2^-32 threshold at different places."""
    f = np.ldexp(1.0, -rng.integers(lo, hi, n)).astype(x.dtype)
    return np.ascontiguousarray((x.reshape(n, -1) * f[:, None]).reshape(-1))


# ---- one node, dense children (DNA and protein) ----

@functools.lru_cache(maxsize=None)
def node_host(S, dtype, n, fma=False, seed=0):
    c = SC.random_case(S, dtype, n, 40 + S + seed, fma)   # every site next to the threshold
    a = [c[k] for k in ("x1", "x2", "EV", "left", "right")]
    esc = O.plf(*a)[1] if S == 4 and not fma else O.plf_generic(S, 4, *a, fma=fma, threads=8)[1]
    return c, mixed(esc, n)


def node_case(S, dtype, n, fma=False, valu=False):
    import torch

    c, esc = node_host(S, dtype, n, fma)
    t = {k: dev(c[k]) for k in ("x1", "x2", "EV", "left", "right")}
    x3 = torch.empty(4 * S * n, dtype=tt(dtype), device="cuda")

    def launch(ctx, w, scs, sums, stream):
        if S == 4:
            ctx.plf_dev(t["x1"], t["x2"], x3, t["EV"], t["left"], t["right"], w, scs[0], sums, n=n, stream=stream)
        else:
            ctx.plf_dev_gen(t["x1"], t["x2"], x3, t["EV"], t["left"], t["right"], S, w, scs[0], sums, n=n,
                            fma=fma, valu=valu, stream=stream)

    return Case(n, [esc], launch, 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("segments", [False, True])
def test_dna_node(monkeypatch, dtype, segments):
    """plf_dev: the default mapping and the eight-segment one."""
    f64 = dtype == np.float64
    run_family(monkeypatch, lambda n: node_case(4, dtype, n or (N_SEG if segments else N_NODE)),
               ("dna node", segments), {"plf_dna_f64_pair_kernel" if f64 else "plf_dna_kernel"},
               {"PLFX_NODE_SEGMENTS": "1"} if segments else {})


@pytest.mark.parametrize("dtype", DTYPES)
def test_scaler_sum(monkeypatch, dtype):
    """plfx_scaler_sum over the node's scaler bytes."""
    def make(n):
        n = n or N_NODE
        esc = node_host(4, dtype, n)[1]
        sc = dev(esc)
        return Case(n, [esc], lambda ctx, w, scs, sums, stream: ctx.scaler_sum(sc, w, sums, n=n, stream=stream), 0)

    run_family(monkeypatch, make, "scaler_sum", {"scaler_sum_kernel"})


# ---- one node, coded children ----

def tip_table(S, dtype):
    """The default table with row r times 2^-3r (DNA) or 2^-2r (protein): two
    coded children scale or not by their codes."""
    if S == 4:
        base = np.array([[(c >> s) & 1 for s in range(4)] for c in range(16)], np.float64)
        return (base * np.ldexp(1.0, -3 * np.arange(16))[:, None]).astype(dtype)
    return (O.protein_tip_table(np.float64) * np.ldexp(1.0, -2 * np.arange(O.PROT_CODES))[:, None]).astype(dtype)


@functools.lru_cache(maxsize=None)
def tips_host(S, dtype, n, both, fma=False):
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(500 + S + n + both)
    codes, expand = (O.random_tip_codes, O.expand_tips) if S == 4 else (O.random_protein_codes, O.expand_protein_tips)
    tv = tip_table(S, dt)
    c = dict(S=S, n=n, tipvec=tv.reshape(-1), c1=codes(rng, n, 0.2), c2=codes(rng, n, 0.2),
             x2=shrink(rng, rng.random(4 * S * n).astype(dt), n, 0, 40), EV=(rng.random(S * S) - 0.25).astype(dt),
             left=rng.random(4 * S * S).astype(dt), right=rng.random(4 * S * S).astype(dt))
    e1 = expand(c["c1"], dt, tipvec=tv)
    e2 = expand(c["c2"], dt, tipvec=tv) if both else c["x2"]
    a = (e1, e2, c["EV"], c["left"], c["right"])
    esc = O.plf(*a)[1] if S == 4 and not fma else O.plf_generic(S, 4, *a, fma=fma, threads=8)[1]
    return c, mixed(esc, n)


def tips_case(S, dtype, n, both, fma=False):
    import torch

    c, esc = tips_host(S, dtype, n, both, fma)
    t = {k: dev(c[k]) for k in ("c1", "c2", "x2", "EV", "left", "right", "tipvec")}
    x3 = torch.empty(4 * S * n, dtype=tt(dtype), device="cuda")
    kw = dict(tip1=t["c1"], tip2=t["c2"]) if both else dict(tip1=t["c1"], x2=t["x2"])

    def launch(ctx, w, scs, sums, stream):
        ctx.plf_tips_dev(x3, t["EV"], n, t["left"], t["right"], wgt=w, scaler=scs[0], scaler_sum=sums,
                         tipvec=t["tipvec"], states=S, fma=fma, stream=stream, **kw)

    return Case(n, [esc], launch, 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("both", [False, True])
def test_dna_tips(monkeypatch, dtype, both):
    """plf_tips_dev: tip1 coded with a dense x2, and both children coded."""
    run_family(monkeypatch, lambda n: tips_case(4, dtype, n or N_NODE, both), ("dna tips", both), {DNA[dtype][0]})


# ---- batches ----

def batch_case(S, dtype, n, count, nosum):
    import torch

    first = node_host(S, dtype, n)
    EV = first[0]["EV"]
    hosts = [first] + [batch_member(S, dtype, n, seed) for seed in range(1, count)]
    V = 4 * S
    nodes = [{k: dev(c[k]) for k in ("x1", "x2", "left", "right")} for c, _ in hosts]
    for nd in nodes:
        nd["x3"] = torch.empty(V * n, dtype=tt(dtype), device="cuda")
    dEV = dev(EV)

    def launch(ctx, w, scs, sums, stream):
        for j, nd in enumerate(nodes):
            nd["scaler"] = scs[j]
            nd.pop("scaler_sum", None)
            if j != nosum:
                nd["scaler_sum"] = sums[j:j + 1]
        ctx.plf_batch_dev(nodes, dEV, n, w, stream=stream, states=S)

    return Case(n, [e for _, e in hosts], launch, count, [j != nosum for j in range(count)])


@functools.lru_cache(maxsize=None)
def batch_member(S, dtype, n, seed):
    """A node of its own under the batch's EV (that of seed 0)."""
    EV = node_host(S, dtype, n, False, 0)[0]["EV"]
    c = SC.random_case(S, dtype, n, 40 + S + seed, False, EV=EV)
    a = [c[k] for k in ("x1", "x2", "EV", "left", "right")]
    esc = O.plf(*a)[1] if S == 4 else O.plf_generic(S, 4, *a, threads=8)[1]
    return c, mixed(esc, n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dna_batch(monkeypatch, dtype):
    """plf_batch_dev: 5 nodes (blockIdx.y), node 3 without a sum."""
    run_family(monkeypatch, lambda n: batch_case(4, dtype, n or N_BATCH, 5, 3), "dna batch", {DNA[dtype][0]})


# ---- DNA traversals ----

@functools.lru_cache(maxsize=4)
def tree_host(tree, mode, dtype, n):
    """A tree of tests/test_trav_plan.py with dense leaves (each site of each
    leaf times 2^-e, e < 16) or coded leaves under tip_table(): the sites
    cross the threshold at different levels."""
    from test_trav_plan import _mask, _tree

    dt = np.dtype(dtype).type
    ops, nslots, ntax = _tree(tree)
    nops = ops.shape[0]
    coded = _mask(nslots, ntax, mode)[:ntax]
    rng = np.random.default_rng(77 + n)
    tv = tip_table(4, dt)
    codes = [O.random_tip_codes(rng, n, 0.2) if coded[t] else None for t in range(ntax)]
    dense = [None if coded[t] else shrink(rng, rng.random(16 * n).astype(dt), n, 0, 16) for t in range(ntax)]
    pm = (rng.random(nops * 128) * 0.3).astype(dt)
    EV = (rng.random(16) * 0.3).astype(dt)
    host = [O.expand_tips(codes[t], dt, tipvec=tv) if coded[t] else dense[t] for t in range(ntax)]
    host += [np.zeros(16 * n, dt) for _ in range(nslots - ntax)]
    escal = O.traverse(4, 4, ops, host, pm, EV, n, None, want_scalers=True)[1]
    mixed(escal, n)
    return dict(ops=ops, nslots=nslots, ntax=ntax, codes=codes, dense=dense, pm=pm, EV=EV, tipvec=tv.reshape(-1)), escal


def tree_case(tree, mode, dtype, n):
    import torch

    c, escal = tree_host(tree, mode, dtype, n)
    ops, ntax, nops = c["ops"], c["ntax"], c["ops"].shape[0]
    clv = [None if c["dense"][t] is None else dev(c["dense"][t]) for t in range(ntax)]
    clv += [torch.empty(16 * n, dtype=tt(dtype), device="cuda") for _ in range(c["nslots"] - ntax)]
    any_coded = any(x is not None for x in c["codes"])
    tips = [None if x is None else dev(x) for x in c["codes"]] + [None] * (c["nslots"] - ntax) if any_coded else None
    pm, EV, tv = dev(c["pm"]), dev(c["EV"]), dev(c["tipvec"]) if any_coded else None

    def launch(ctx, w, scs, sums, stream):
        ctx.traverse(ops, clv, pm, EV, n, w, [x[:n] for x in scs], sums[:nops], tips=tips, tipvec=tv, stream=stream)

    return Case(n, escal, launch, nops)


SCHED = ("deep6", "deep5", "deep4", "septets", "triples", "unfused")
# the kernels behind a schedule's unfused ops (and a node with coded children), level pairs, three-level and deep passes
DNA = {np.float32: ("plf_dna_batch_kernel", "plf_dna_cat_triple_kernel", "plf_dna_cat_septet_kernel",
                    "plf_dna_cat_deep_kernel"),
       np.float64: ("plf_dna_f64_pair_batch_kernel", "plf_dna_f64_triple_kernel", "plf_dna_f64_septet_kernel",
                    "plf_dna_f64_deep_kernel")}
TREES = [("taxa53", "dense"), ("b64", "coded")]   # of test_gpu_tree.SCHEDULE_LAUNCHES


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fuse", [0, 1, 2, 3])
@pytest.mark.parametrize("tree,mode", TREES)
def test_dna_traversal(monkeypatch, dtype, fuse, tree, mode):
    """traverse under every PLFX_FUSE: one launch per level (fuse 0), level
    pairs (1), three-level passes (2) and the deep passes (3), the kinds as
    tests/test_trav_plan.py pins them: block_ticket_sum3 / 7 and the deep
    passes' LDS accumulators.  A level of many nodes takes its share of the
    co-resident blocks, so not every launch of a kind is above 32 blocks."""
    from test_gpu_tree import SCHEDULE_LAUNCHES
    from test_trav_plan import PINNED

    assert any(tree == t for t, _ in SCHEDULE_LAUNCHES)
    counts = next(row[2 + (3 - fuse)] for row in PINNED if row[0] == tree and mode in row[1])

    def make(n):
        return tree_case(tree, mode, dtype, n or N_TREE[tree])

    kernels = {DNA[dtype][k] for k, kind in enumerate(("unfused", "triples", "septets", "deep")) if sum(
        counts[SCHED.index(key)] for key in SCHED if key.startswith(kind))}
    run_family(monkeypatch, make, ("dna traversal", tree, mode, fuse), kernels, {"PLFX_FUSE": str(fuse)},
               every=False)
    with env_ctx(monkeypatch, PLFX_FUSE=str(fuse)) as c:
        case = make(N_EXT)
        case.launch(c, None)
        case.verify(None, "schedule")
        sched = c.last_schedule()
    assert [sched[k] for k in SCHED] == counts, sched


# ---- protein ----

PROT_KERNELS = {   # name: (dtype, fma, valu, kernel)
    "exact_f32": (np.float32, False, False, "plf_prot_lds_kernel"),
    "exact_f64": (np.float64, False, False, "plf_prot_valu_exact_kernel"),
    "fma_f64": (np.float64, True, False, "plf_prot_mfma_kernel"),
    "fma_f32": (np.float32, True, False, "plf_prot_mfma32_kernel"),
    "fma_f64_valu": (np.float64, True, True, "plf_prot_valu_fma_kernel"),
}


@pytest.mark.parametrize("kernel", list(PROT_KERNELS))
def test_protein_node(monkeypatch, kernel):
    """plf_dev_gen at 20 states: the five node kernels."""
    dtype, fma, valu, name = PROT_KERNELS[kernel]
    run_family(monkeypatch, lambda n: node_case(20, dtype, n or N_PROT, fma, valu), ("protein node", kernel), {name})


def test_protein_tile_queue(monkeypatch):
    """The f64 FMA kernel handing out tiles through its device-wide queue,
    whose words share the workspace with the sum's (3 blocks, 121 tiles, as
    tests/test_gpu_protein.py): G <= 32 only."""
    with env_ctx(monkeypatch, PLFX_MAX_BLOCKS="3") as c:
        case = node_case(20, np.float64, N_QUEUE, True)
        pats = patterns(case.esc, case.n)
        run_patterns(c, case, pats, "tile queue")
        case.launch(c, None)
        case.verify(None, ("tile queue", "wgt=None"))
        assert grids_of(c, case, pats["max"], {"plf_prot_mfma_kernel"}) == [("plf_prot_mfma_kernel", 3, 1, 256)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_protein_batch(monkeypatch, dtype):
    """plf_batch_dev at 20 states, 3 nodes, node 1 without a sum."""
    run_family(monkeypatch, lambda n: batch_case(20, dtype, n or N_PROT, 3, 1), "protein batch",
               {"plf_prot_lds_batch_kernel"})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("both", [False, True])
def test_protein_tips(monkeypatch, dtype, both):
    """plf_tips_dev at 20 states: tip1 coded with a dense x2, and tip1 + tip2
    (the code-pair table and its gather)."""
    run_family(monkeypatch, lambda n: tips_case(20, dtype, n or N_PROT, both), ("protein tips", both),
               {"prot_tiptip_gather_kernel" if both else "plf_prot_lds_kernel"})


@functools.lru_cache(maxsize=2)
def prot_tree_host(dtype, n):
    """32 coded taxa under tip_table(): tip/tip nodes, then table children."""
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(2032 + n)
    ops = O.balanced_tree_ops(32)
    nops = ops.shape[0]
    tv = tip_table(20, dt)
    codes = [O.random_protein_codes(rng, n, 0.2) for _ in range(32)]
    pm = (rng.random(nops * 2 * 4 * 400) * 0.1).astype(dt)
    EV = (rng.random(400) * 0.1).astype(dt)
    host = [O.expand_protein_tips(x, dt, tipvec=tv) for x in codes] + [np.zeros(80 * n, dt) for _ in range(nops)]
    escal = O.traverse(20, 4, ops, host, pm, EV, n, None, want_scalers=True)[1]
    mixed(escal, n)
    return dict(ops=ops, codes=codes, pm=pm, EV=EV, tipvec=tv.reshape(-1)), escal


@pytest.mark.parametrize("dtype", DTYPES)
def test_protein_traversal(monkeypatch, dtype):
    """traverse on an all-coded 32-taxon protein tree: 16 tip/tip nodes (the
    code-pair tables and their gather), 8 nodes on table children, then dense
    levels and the root."""
    import torch

    def make(n):
        n = n or N_PROT_TREE
        c, escal = prot_tree_host(dtype, n)
        nops = c["ops"].shape[0]
        clv = [None] * 32 + [torch.empty(80 * n, dtype=tt(dtype), device="cuda") for _ in range(nops)]
        tips = [dev(x) for x in c["codes"]] + [None] * nops
        pm, EV, tv = dev(c["pm"]), dev(c["EV"]), dev(c["tipvec"])
        return Case(n, escal, lambda ctx, w, scs, sums, stream: ctx.traverse(
            c["ops"], clv, pm, EV, n, w, [x[:n] for x in scs], sums[:nops], tips=tips, tipvec=tv, states=20,
            stream=stream), nops)

    run_family(monkeypatch, make, "protein traversal",
               {"prot_tiptip_gather_kernel", "plf_prot_lds_tab_batch_kernel", "plf_prot_lds_batch_kernel",
                "plf_prot_lds_kernel"}, every=False)


# ---- per-site rates ----

@functools.lru_cache(maxsize=None)
def psr_host(dtype, n, count, coded):
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(900 + n + 10 * count + coded)
    ncat = 6
    c = dict(n=n, ncat=ncat, EV=(rng.random(16) - 0.25).astype(dt), cat=rng.integers(0, ncat + 2, n).astype(np.uint8),
             tipvec=tip_table(4, dt).reshape(-1), nodes=[])
    esc = []
    for _ in range(count):
        nd = dict(left=rng.random(16 * ncat).astype(dt), right=rng.random(16 * ncat).astype(dt))
        if coded:
            nd["tip1"], nd["tip2"] = O.random_tip_codes(rng, n, 0.2), O.random_tip_codes(rng, n, 0.2)
            d1, d2 = (psr_ref.expand_tips(nd[k], dt, c["tipvec"]) for k in ("tip1", "tip2"))
        else:
            nd["x1"] = d1 = shrink(rng, rng.random(4 * n).astype(dt), n, 16, 48)
            nd["x2"] = d2 = rng.random(4 * n).astype(dt)
        esc.append(mixed(psr_ref.node(d1, d2, c["EV"], nd["left"], nd["right"], c["cat"], ncat)[1], n))
        c["nodes"].append(nd)
    return c, esc


def psr_case(dtype, n, count, coded, nosum=None):
    import torch

    c, esc = psr_host(dtype, n, count, coded)
    nodes = [{k: dev(v) for k, v in nd.items()} for nd in c["nodes"]]
    for nd in nodes:
        nd["x3"] = torch.empty(4 * n, dtype=tt(dtype), device="cuda")
    EV, cat, tv = dev(c["EV"]), dev(c["cat"]), dev(c["tipvec"]) if coded else None

    def launch(ctx, w, scs, sums, stream):
        for j, nd in enumerate(nodes):
            nd["scaler"] = scs[j]
            nd["scaler_sum"] = None if j == nosum else sums[j:j + 1]
        ctx.plf_psr(nodes, EV, n, cat, c["ncat"], wgt=w, tipvec=tv, stream=stream)

    return Case(n, esc, launch, count, [j != nosum for j in range(count)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["dense", "coded", "batch"])
def test_psr_node(monkeypatch, dtype, kind):
    """plf_psr: one dense node, one with both children coded, and a batch of
    3 (node 1 without a sum)."""
    count, coded, nosum = {"dense": (1, False, None), "coded": (1, True, None), "batch": (3, False, 1)}[kind]
    run_family(monkeypatch, lambda n: psr_case(dtype, n or N_NODE, count, coded, nosum), ("psr", kind),
               {"plf_psr_kernel"})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fuse", [False, True])
def test_psr_traversal(monkeypatch, dtype, fuse):
    """traverse_psr on the random 24-taxon tree of tests/test_gpu_psr_traverse.py,
    level pairs fused (PLFX_FUSE=1: plf_psr_triple_kernel) and not."""
    import torch

    import test_gpu_psr_traverse as PT

    def make(n):
        n = n or N_NODE
        case = PT.tree_case(dtype, "random 24", n, 6)
        nops = len(case["ops"])
        slots = [None] * case["nslots"]
        tips = [None] * case["nslots"]
        for s in range(case["nslots"]):
            if s not in case["inputs"]:
                slots[s] = torch.empty(4 * n, dtype=tt(dtype), device="cuda")
            elif case["flags"][s]:
                tips[s] = dev(case["inputs"][s])
            else:
                slots[s] = dev(case["inputs"][s])
        d = {k: dev(case[k]) for k in ("pmats", "EV", "cat", "tipvec")}
        ops = np.array(case["ops"], np.int32).reshape(-1, 4)
        return Case(n, [r[1] for r in case["ref"]], lambda ctx, w, scs, sums, stream: ctx.traverse_psr(
            ops, slots, d["pmats"], d["EV"], n, d["cat"], case["ncat"], wgt=w, scalers=[x[:n] for x in scs],
            scaler_sums=sums[:nops], stream=stream, tips=tips, tipvec=d["tipvec"]), nops)

    env = {"PLFX_FUSE": "1"} if fuse else {}
    run_family(monkeypatch, make, ("psr traversal", fuse),
               {"plf_psr_kernel", "plf_psr_triple_kernel"} if fuse else {"plf_psr_kernel"}, env, every=False)
    with env_ctx(monkeypatch, **env) as c:
        case = make(N_EXT)
        case.launch(c, None)
        case.verify(None, "schedule")
        sched = c.last_schedule()
    want = PT.T.expected_schedule(PT.TREES["random 24"](), fuse=fuse)
    assert (sched["triples"], sched["unfused"], sched["launches"]) == tuple(want), sched
    assert (want[0] >= 3) == fuse and want[1] >= 3


# ---- the host entry ----

def wrap32(v):
    """v reduced modulo 2^32 to a signed 32-bit int."""
    return (v + 2**31) % 2**32 - 2**31


def host_plf(ctx, c, w, fill=-3.0):
    x3 = np.full(16 * c["n"] + PAD, fill, c["x1"].dtype)
    return ctx.plf(c["x1"], c["x2"], x3, c["EV"], c["n"], c["left"], c["right"], w), x3


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_entry_wraps_to_int32(ctx, dtype):
    """Context.plf over two chunks (2^18 + 5 sites) with an exact scaled sum
    beyond 2^31: the value returned is that sum modulo 2^32 as a signed 32-bit
    int (plfx.h; the reference's int accumulation wraps the same way)."""
    n = 2**18 + 5
    c, esc = node_host(4, dtype, n)
    w = (30000 + np.arange(n) % 7919).astype(np.int32)
    exact = sum(w[esc != 0].tolist())
    print("exact", exact, "wrapped", wrap32(exact))
    assert exact > 2**31 and sum(w.tolist()) < 2**40
    inc, x3 = host_plf(ctx, c, w)
    assert inc == wrap32(exact) != exact
    assert (x3[16 * n:] == -3.0).all() and not (x3[:16 * n] == -3.0).any()
    inc, _ = host_plf(ctx, c, -w)
    assert inc == wrap32(-exact)


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_entry_refuses_from_2_to_the_40(ctx, dtype):
    """n = 512, the smallest size that can reach the bound.  511 x INT32_MIN
    and one INT32_MAX, sum |w| = 2^40 - 1: accepted, the sum exact after the
    wrap.  512 x INT32_MIN, sum |w| = 2^40: PLFX_ERR_INVALID, x3 untouched."""
    import plfx

    n = 512
    c, esc = node_host(4, dtype, n)
    scaled = np.flatnonzero(esc)
    for at in (int(scaled[0]), int(np.flatnonzero(esc == 0)[0])):   # the INT32_MAX at a scaled site, and not
        w = np.full(n, I32MIN, np.int32)
        w[at] = I32MAX
        assert sum(abs(v) for v in w.tolist()) == 2**40 - 1
        inc, x3 = host_plf(ctx, c, w)
        exact = sum(w[esc != 0].tolist())
        print("exact", exact, "wrapped", wrap32(exact), "got", inc)
        assert inc == wrap32(exact)
        assert (x3[16 * n:] == -3.0).all() and not (x3[:16 * n] == -3.0).any()
    w = np.full(n, I32MIN, np.int32)
    with pytest.raises(plfx.PlfxError) as e:
        host_plf(ctx, c, w)
    assert e.value.code == plfx.ERR_INVALID
    x3 = np.full(16 * n + PAD, -3.0, c["x1"].dtype)
    with pytest.raises(plfx.PlfxError):
        ctx.plf(c["x1"], c["x2"], x3, c["EV"], n, c["left"], c["right"], w)
    assert (x3 == -3.0).all()
    inc, _ = host_plf(ctx, c, None)   # the context still works
    assert inc == int(esc.sum())
