"""GPU tests of plfx.h section 11d, PROTCAT FMA mode: the protein per-site-rate
node on the f64 matrix cores (plfx_plf_psr_dev_ex), the traversal
(plfx_traverse_psr_ex) and the rate scan (plfx_psr_rate_scan_ex) with
PLFX_FMA.

The reference is tests/psr_prot_fma_ref.py: oracle.plf_generic(20, 1, ...,
fma=True) on the sites of each clamped category.  Node results are compared
bit for bit: values, scaler bytes and the weighted scaler sum.
tests/test_psr_prot_fma_abi.py shows on the CPU that this reference differs in
bits from the exact restatement on these very inputs, so a pass here is a
statement about the matrix-core kernel and not about the exact one.  The
inputs, the category patterns, the rescale construction and the trees are
those of tests/test_gpu_psr_prot.py; f64 throughout (f32 is refused)."""
import functools

import numpy as np
import pytest

import plfx
import psr_prot_fma_ref as RF
import psr_prot_ref as R
from test_gpu_psr import bits, dev, same
from test_gpu_psr_prot import (BLOCK_SITES, GUARD, KINDS, LNL_RTOL, NCATS, NULLS, S, category_patterns, check_node,
                               make_node, protein_problem, scale_case, tree_problem)

pytestmark = pytest.mark.gpu

F64 = np.float64
SIZES = (1, 15, 16, 17, 48, 63, 64, 65, 255, 256, 257)  # sub-tile (16), wave (64) and block (256) edges


def with_fma_ref(d):
    """A copy of a make_node / scale_case dict whose reference is the FMA one."""
    d = dict(d)
    d["ref"] = RF.node_fma(d["dense"][0], d["dense"][1], d["EV"], d["left"], d["right"], d["cat"], d["ncat"], d["wgt"])
    d["ref_unit"] = int(d["ref"][1].sum())
    return d


@functools.lru_cache(maxsize=None)
def fma_case(n, ncat, kind, seed=0, default_table=False):
    """Read-only: cached."""
    return with_fma_ref(make_node(F64, n, ncat, kind, seed, default_table=default_table))


def run_node(c, d, wgt=True, scaler=True, scaler_sum=True, cat=None, stream=None, dense=False, fma=True):
    """One node through Context.plf_psr_gen(fma=True): (x3 buffer with its
    guard, scaler bytes, sum).  dense: the coded children expanded on the host."""
    import torch

    n = d["n"]
    buf = torch.full((S * n + GUARD,), -7.0, dtype=torch.float64, device="cuda")
    sc = torch.full((n + GUARD,), 9, dtype=torch.uint8, device="cuda") if scaler else None
    ss = torch.full((1,), -5, dtype=torch.int64, device="cuda") if scaler_sum else None
    nd = dict(x3=buf, left=dev(d["left"]), right=dev(d["right"]), scaler=sc, scaler_sum=ss)
    if dense:
        nd.update(x1=dev(d["dense"][0]), x2=dev(d["dense"][1]))
    else:
        nd.update({k: dev(d[k]) for k in ("x1", "x2", "tip1", "tip2") if k in d})
    tv = None if (d["tipvec"] is None or dense) else dev(d["tipvec"])
    c.plf_psr_gen(S, nd, dev(d["EV"]), n, dev(d["cat"] if cat is None else cat), d["ncat"],
                  wgt=dev(d["wgt"]) if wgt else None, tipvec=tv, stream=stream, fma=fma)
    return buf, sc, ss


# ---- 1: tile and sub-tile edges ----

@pytest.mark.parametrize("kind", range(4), ids=KINDS)
def test_node_is_bit_exact_at_the_tile_and_sub_tile_edges(ctx, kind):
    j = scaled = 0
    for n in SIZES:
        for ncat in NCATS:
            d = fma_case(n, ncat, kind)
            scaled += d["ref_unit"]
            check_node(d, *run_node(ctx, d), what=(n, ncat, "all outputs"))
            null = NULLS[j % 3]  # wgt, scaler, scaler_sum NULL in turn
            j += 1
            check_node(d, *run_node(ctx, d, **null), wgt=null.get("wgt", True), what=(n, ncat, null))
    total = 3 * sum(SIZES)
    assert total // 8 <= scaled <= total - total // 8  # both outcomes of the rescale on a good share of the sites


def test_the_mode_is_not_the_exact_one(ctx):
    """The flag reaches the kernel: on these inputs exact mode gives other bits
    (and the exact reference's), FMA mode the FMA reference's."""
    import torch

    d = fma_case(257, 25, 0)
    exact = run_node(ctx, d, fma=False)
    fma = run_node(ctx, d)
    torch.cuda.synchronize()
    a, b = exact[0].cpu().numpy()[:S * 257], fma[0].cpu().numpy()[:S * 257]
    assert same(a, make_node(F64, 257, 25, 0)["ref"][0]) and same(b, d["ref"][0])
    assert np.mean(bits(a) != bits(b)) > 0.25


# ---- 2: categories inside a sub-tile ----

def sub_tile_patterns():
    """name -> (ncat, 80 category bytes): a wave of four sub-tiles and one more sub-tile."""
    n = 64 + 16
    out = {}
    for p in range(1, 16):  # the category changes after position p of the first sub-tile
        cat = np.full(n, 3)
        cat[:p] = 7
        out[f"change after {p}"] = (32, cat)
    cat = np.full(n, 20)
    cat[:16] = np.arange(16)[::-1]
    out["16 categories in one sub-tile"] = (32, cat)
    out["32 categories in a wave"] = (32, (5 * np.arange(n) + 3) % 32)
    cat = np.repeat([1, 2, 3, 4, 2], 16)
    cat[[2, 9, 15, 48, 50, 63]] = 9  # category 9 in sub-tiles 0 and 3 only
    out["a category in sub-tiles 0 and 3 only"] = (32, cat)
    cat = np.resize(np.array([24, 25, 200, 255, 3, 24, 31], np.uint8), n)  # bytes >= ncat are category 24
    out["bytes past ncat"] = (25, cat)
    return out


@pytest.mark.parametrize("kind", [0, 3], ids=["dense/dense", "tip/tip"])
def test_categories_inside_a_sub_tile(ctx, kind):
    import torch

    n = 64 + 16
    perm = np.random.default_rng(11).permutation(n)
    for name, (ncat, cat) in sub_tile_patterns().items():
        d = with_fma_ref(make_node(F64, n, ncat, kind, seed=5, cat=cat))
        got = run_node(ctx, d)
        check_node(d, *got, what=name)
        # a permutation of the sites permutes the outputs
        q = dict(d, cat=d["cat"][perm], wgt=d["wgt"][perm])
        for k in ("x1", "x2"):
            if k in d:
                q[k] = np.ascontiguousarray(d[k].reshape(n, S)[perm].reshape(-1))
        for k in ("tip1", "tip2"):
            if k in d:
                q[k] = d[k][perm]
        pg = run_node(ctx, q)
        torch.cuda.synchronize()
        a, b = got[0].cpu().numpy()[:S * n].reshape(n, S), pg[0].cpu().numpy()[:S * n].reshape(n, S)
        assert same(a[perm], b), name
        assert np.array_equal(got[1].cpu().numpy()[:n][perm], pg[1].cpu().numpy()[:n]), name
        assert int(got[2].item()) == int(pg[2].item()), name
    if kind == 0:  # and the patterns of the exact node's test, over a block and a site
        for name, cat in category_patterns(257, 32).items():
            d = with_fma_ref(make_node(F64, 257, 32, kind, seed=5, cat=cat))
            check_node(d, *run_node(ctx, d), what=name)


# ---- 3: one block over many trips ----

def test_one_block_walks_every_site(monkeypatch):
    """PLFX_MAX_BLOCKS=1: one block per node makes all four trips (three whole
    tiles of 256 sites and 17 sites) and is its own last block."""
    monkeypatch.setenv("PLFX_MAX_BLOCKS", "1")
    n = 3 * BLOCK_SITES + 17
    with plfx.Context(0, lazy_tables=True) as c:
        for kind in range(4):
            rand = make_node(F64, n, 25, kind)
            for what, cat in (("random", rand["cat"]), ("sorted", np.sort(rand["cat"]))):
                d = with_fma_ref(dict(rand, cat=cat))
                check_node(d, *run_node(c, d), what=(kind, what))


# ---- 4: coded children ----

@pytest.mark.parametrize("default_table", [False, True], ids=["custom table", "default table"])
def test_coded_children_equal_the_dense_call_on_their_expansion(ctx, default_table):
    import torch

    for kind in (1, 2, 3):
        d = fma_case(131, 25, kind, 9, default_table)
        for s in (1, 2):
            if f"tip{s}" in d:  # every row of the table, 24 and 255 (which read row 23)
                assert set(range(24)) | {24, 255} <= set(d[f"tip{s}"].tolist())
        if not default_table:
            tv = d["tipvec"]
            assert np.all((tv != 0) & (tv != 1))  # a table of values that are neither 0 nor 1
        coded = run_node(ctx, d)
        check_node(d, *coded, what=(kind, "coded"))
        expanded = run_node(ctx, d, dense=True)
        check_node(d, *expanded, what=(kind, "expanded"))
        torch.cuda.synchronize()
        assert same(coded[0].cpu().numpy(), expanded[0].cpu().numpy())


# ---- 5: batches ----

def test_batch_of_33_mixed_nodes_equals_one_node_calls(ctx):
    """33 nodes with distinct matrices, the four kinds of children in turn (one
    launch per kind), then 33 dense/dense nodes (across the 32-node launch
    boundary); some without scaler bytes or a sum, each sum its node's own."""
    import torch

    n, ncat, count = 257, 25, 33
    sums = set()
    for mode in ("mixed", "dense"):
        cases = [make_node(F64, n, ncat, i % 4 if mode == "mixed" else 0, 100 + i) for i in range(count)]
        cat, wgt, EV, tv = (dev(cases[0][k]) for k in ("cat", "wgt", "EV", "tipvec"))
        nodes = []
        for i, d in enumerate(cases):
            nd = dict(x3=torch.full((S * n + GUARD,), -7.0, dtype=torch.float64, device="cuda"), left=dev(d["left"]),
                      right=dev(d["right"]),
                      scaler=None if i % 7 == 3 else torch.full((n,), 9, dtype=torch.uint8, device="cuda"),
                      scaler_sum=None if i % 5 == 4 else torch.full((1,), -5, dtype=torch.int64, device="cuda"))
            nd.update({k: dev(d[k]) for k in ("x1", "x2", "tip1", "tip2") if k in d})
            nodes.append(nd)
        ctx.plf_psr_gen(S, nodes, EV, n, cat, ncat, wgt=wgt, tipvec=tv, fma=True)
        torch.cuda.synchronize()
        for i, (d, nd) in enumerate(zip(cases, nodes)):
            one = dict(nd, x3=torch.full((S * n + GUARD,), -7.0, dtype=torch.float64, device="cuda"),
                       scaler=torch.full((n,), 9, dtype=torch.uint8, device="cuda"),
                       scaler_sum=torch.full((1,), -5, dtype=torch.int64, device="cuda"))
            ctx.plf_psr_gen(S, one, EV, n, cat, ncat, wgt=wgt, tipvec=tv, fma=True)
            torch.cuda.synchronize()
            assert same(nd["x3"].cpu().numpy(), one["x3"].cpu().numpy()), i
            if nd["scaler"] is not None:
                assert np.array_equal(nd["scaler"].cpu().numpy(), one["scaler"].cpu().numpy()), i
            if nd["scaler_sum"] is not None:
                assert int(nd["scaler_sum"].item()) == int(one["scaler_sum"].item()), i
            # and the one-node call is the reference (the shared EV / cat / wgt / table are node 0's)
            x = [R.expand_tips(d[f"tip{s}"], F64, cases[0]["tipvec"]) if f"tip{s}" in d else d[f"x{s}"] for s in (1, 2)]
            x3, esc, einc = RF.node_fma(x[0], x[1], cases[0]["EV"], d["left"], d["right"], cases[0]["cat"], ncat,
                                        cases[0]["wgt"])
            assert same(one["x3"].cpu().numpy()[:S * n], x3), i
            assert np.array_equal(one["scaler"].cpu().numpy(), esc) and int(one["scaler_sum"].item()) == einc, i
            sums.add((mode, einc))
    assert len(sums) > 2  # the mixed nodes' sums differ: none was given another's


# ---- 6: the rescale decision, position by position ----

@pytest.mark.parametrize("carrier", [1, 2])
def test_rescale_decision_position_by_position(ctx, carrier):
    """scale_case: permutation matrices, so every fused chain is 0 + one
    product of a value with 1 -- exact, as the unfused one: the two references
    agree, and the decision at, just under and at minus 2^-32 is the
    construction's, at each of the 20 positions."""
    exact = scale_case(F64, carrier)
    d = with_fma_ref(exact)
    assert same(d["ref"][0], exact["ref"][0]) and np.array_equal(d["ref"][1], exact["ref"][1])
    assert np.array_equal(d["ref"][1], d["must"].astype(np.uint8))
    assert np.isnan(d["ref"][0].reshape(-1, S)[64]).all()  # 0 * NaN in every chain of the site: never scales
    assert d["ref"][2] == int(d["wgt"].astype(np.int64)[d["must"]].sum())
    check_node(d, *run_node(ctx, d), what="weighted")
    check_node(d, *run_node(ctx, d, wgt=False), wgt=False, what="unit weights")


# ---- 7: the scaler sum at its bound ----

N_BOUND = 32 * BLOCK_SITES + 1  # 33 blocks: the smallest grid above the 32 slots, and not a multiple of 32


@pytest.mark.parametrize("kind", [0, 3], ids=["dense/dense", "tip/tip"])
def test_scaler_sum_at_the_weight_bound(monkeypatch, kind):
    """tests/test_gpu_sum_bound.py's construction on the FMA node: weights that
    put the sum just inside +-2^40, that cancel beyond +-2^39, random ones, and
    INT32_MIN / INT32_MAX on 511 of the scaled sites spread over the 33 blocks
    (sum |wgt| < 2^40, the contract); then wgt NULL: the workspace went back to
    zero.  The grid is read from a captured graph."""
    import torch

    import test_gpu_sum_bound as B

    n = N_BOUND
    d = fma_case(n, 25, kind)
    esc = B.mixed(d["ref"][1], n)
    t = {k: dev(d[k]) for k in ("x1", "x2", "tip1", "tip2", "left", "right", "EV", "cat") if k in d}
    tv = dev(d["tipvec"])
    x3 = torch.empty(S * n, dtype=torch.float64, device="cuda")

    def launch(c, w, scs, sums, stream):
        nd = dict(x3=x3, left=t["left"], right=t["right"], scaler=scs[0], scaler_sum=sums[:1])
        nd.update({k: t[k] for k in ("x1", "x2", "tip1", "tip2") if k in t})
        c.plf_psr_gen(S, nd, t["EV"], n, t["cat"], 25, wgt=w, tipvec=tv, stream=stream, fma=True)

    pats = B.patterns([esc], n)
    scaled = np.flatnonzero(esc)
    pick = scaled[np.linspace(0, scaled.size - 1, B.N_EXT).astype(np.int64)]
    assert np.unique(pick // BLOCK_SITES).size >= 32  # spread over the grid (the last block is one site)
    ext = np.zeros(n, np.int64)
    ext[pick] = np.resize(np.array([B.I32MIN, B.I32MAX, B.I32MIN], np.int64), pick.size)
    pats["extremes"] = ext.astype(np.int32)
    allmin = np.zeros(n, np.int64)
    allmin[pick] = B.I32MIN
    pats["INT32_MIN"] = allmin.astype(np.int32)
    with B.env_ctx(monkeypatch) as c:
        case = B.Case(n, [esc], launch, 1)
        B.run_patterns(c, case, pats, ("psr prot fma", kind))
        case.launch(c, None)
        case.verify(None, ("psr prot fma", kind, "wgt=None"))
        grids = B.grids_of(c, case, pats["cancel"], {"plf_psr_prot_mfma_kernel"})
        assert grids == [("plf_psr_prot_mfma_kernel", 33, 1, 256)], grids
    torch.cuda.synchronize()
    assert same(x3.cpu().numpy(), d["ref"][0])


# ---- 8: the traversal ----

def tree_inputs(p):
    """The device tensors of tree_problem p (made once: a capturing stream takes no upload)."""
    t = {k: dev(p[k]) for k in ("pmats", "EV", "cat", "wgt", "tipvec")}
    t["tips"] = [dev(p["codes"][s]) if p["flags"][s] else None for s in range(p["nslots"])]
    return t


def run_tree(c, p, fma=True, stream=None, out=None, t=None):
    import torch

    n = p["n"]
    t = t or tree_inputs(p)
    clv = out["clv"] if out else [None if p["flags"][s] else torch.full((S * n + GUARD,), -7.0, dtype=torch.float64,
                                                                        device="cuda") for s in range(p["nslots"])]
    scalers = out["scalers"] if out else [torch.full((n,), 9, dtype=torch.uint8, device="cuda") for _ in p["ops"]]
    sums = out["sums"] if out else torch.full((len(p["ops"]),), -5, dtype=torch.int64, device="cuda")
    c.traverse_psr_gen(S, np.array(p["ops"], np.int32), clv, t["pmats"], t["EV"], n, t["cat"], p["ncat"],
                       wgt=t["wgt"], scalers=scalers, scaler_sums=sums, tips=t["tips"], tipvec=t["tipvec"],
                       stream=stream, fma=fma)
    return dict(clv=clv, scalers=scalers, sums=sums)


def root_lnl_abs(c, x, n, wgt, sums):
    """Root lnL of |x| (the problems' EV is signed, so a site's sum may be
    negative: the same function of the CLV for both modes)."""
    import torch

    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    c.root_lnl_psr_gen(S, x[:S * n].abs().contiguous(), n, out, wgt=wgt, scaler_sums=sums)
    torch.cuda.synchronize()
    return float(out.item())


@pytest.mark.parametrize("name", ["balanced 8", "caterpillar 6"])
def test_traversal_equals_the_ops_one_by_one(ctx, name):
    import torch

    import psr_trees as T
    from test_gpu_psr_prot import TREES

    p = tree_problem(F64, name)
    n, ncat, M = p["n"], p["ncat"], p["ncat"] * S * S
    assert n == 65 and ncat == 25 and p["codes"]  # coded tips
    r = run_tree(ctx, p)
    torch.cuda.synchronize()
    sched = ctx.last_schedule()
    assert [sched[k] for k in ("deep6", "deep5", "deep4", "septets", "triples")] == [0] * 5  # no pairs
    assert sched["unfused"] == len(p["ops"])
    assert sched["launches"] == T.expected_schedule(TREES[name](), fuse=False)[2]
    EV, cat, wgt, tv, pm = (dev(p[k]) for k in ("EV", "cat", "wgt", "tipvec", "pmats"))
    one = dict(enumerate(r["clv"]))
    vals = {s: R.expand_tips(c_, F64, p["tipvec"]) for s, c_ in p["codes"].items()}
    total = 0
    for j, (par, a, b, m) in enumerate(p["ops"]):
        nd = dict(x3=torch.full((S * n + GUARD,), -7.0, dtype=torch.float64, device="cuda"),
                  left=pm[2 * m * M:(2 * m + 1) * M], right=pm[(2 * m + 1) * M:(2 * m + 2) * M],
                  scaler=torch.full((n,), 9, dtype=torch.uint8, device="cuda"),
                  scaler_sum=torch.full((1,), -5, dtype=torch.int64, device="cuda"))
        for side, s in ((1, a), (2, b)):
            if p["flags"][s]:
                nd[f"tip{side}"] = dev(p["codes"][s])
            else:
                nd[f"x{side}"] = one[s]
        ctx.plf_psr_gen(S, nd, EV, n, cat, ncat, wgt=wgt, tipvec=tv, fma=True)
        torch.cuda.synchronize()
        one[par] = nd["x3"]
        assert same(r["clv"][par].cpu().numpy(), nd["x3"].cpu().numpy()), j
        assert np.array_equal(r["scalers"][j].cpu().numpy(), nd["scaler"].cpu().numpy()), j
        assert int(r["sums"][j].item()) == int(nd["scaler_sum"].item()), j
        # and the op is the reference's
        vals[par], esc, einc = RF.node_fma(vals[a], vals[b], p["EV"], p["pmats"][2 * m * M:(2 * m + 1) * M],
                                           p["pmats"][(2 * m + 1) * M:(2 * m + 2) * M], p["cat"], ncat, p["wgt"])
        assert same(nd["x3"].cpu().numpy()[:S * n], vals[par]), j
        assert np.array_equal(nd["scaler"].cpu().numpy(), esc) and int(nd["scaler_sum"].item()) == einc, j
        total += einc
    assert total > 0  # the rescale fired somewhere in the tree
    # the likelihood is the exact traversal's
    e = run_tree(ctx, p, fma=False)
    root = p["ops"][-1][0]
    got, ref = root_lnl_abs(ctx, r["clv"][root], n, wgt, r["sums"]), root_lnl_abs(ctx, e["clv"][root], n, wgt, e["sums"])
    print(f"{name}: lnL fma {got!r} exact {ref!r} rel {abs(got - ref) / abs(ref):.2e}")
    assert np.isfinite(ref) and abs(got - ref) <= LNL_RTOL * abs(ref)
    assert not same(r["clv"][root].cpu().numpy(), e["clv"][root].cpu().numpy())  # and not its bits


# ---- 9: the rate scan ----

def test_rate_scan_in_fma_mode(ctx):
    """A 6-taxon tree, 65 sites, 5 candidates: the same bits for group 1, 2 and
    5, every row equal to the per-candidate composition pmatrix +
    traverse_psr_gen(fma=True) + site_lnl_psr_gen, the total to root_lnl_psr_gen's."""
    import torch

    import test_gpu_psr_prot_rate_scan as RS

    p = protein_problem(65)
    assert p["ntips"] == 6 and p["n"] == 65
    n, nops = 65, len(p["ops"])
    cand = np.geomspace(0.3, 4.0, 5)
    d = RS.inputs(p, F64, cand)
    res = {}
    for group in (1, 2, 5):  # five passes; passes 2, 2, 1; one pass
        ws, o = RS.workspace(p, F64, group), RS.outputs(n, 5)
        RS.launch(ctx, p, d, group, ws, o, fma=True)
        res[group] = RS.host(o, n, 5)
    for group in (2, 5):
        assert RS.same_bits(res[group], res[1]), group
        assert bits(np.float64(res[group]["out"])) == bits(np.float64(res[1]["out"])), group
    assert np.all(np.isfinite(res[1]["all"]))
    pm = RS.device_pmats(ctx, d, F64, cand)
    scaled = 0
    for k in range(5):
        clv = [None] * 6 + [torch.empty(S * n, dtype=torch.float64, device="cuda") for _ in range(p["nslots"] - 6)]
        sc = torch.full((nops, n), 9, dtype=torch.uint8, device="cuda")
        sums = torch.zeros(nops, dtype=torch.int64, device="cuda")
        ctx.traverse_psr_gen(S, d["ops"], clv, pm, d["EVd"], n, dev(np.full(n, k, np.uint8)), 5, wgt=d["wgt"],
                             scalers=[sc[j] for j in range(nops)], scaler_sums=sums, tips=d["tips"], tipvec=d["tvd"],
                             fma=True)
        root = clv[p["ops"][-1][0]]
        site = torch.full((n,), RS.SENTINEL, dtype=torch.float64, device="cuda")
        ctx.site_lnl_psr_gen(S, root, n, site, freq=d["wd"], scalers=sc)
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        ctx.root_lnl_psr_gen(S, root, n, out, freq=d["wd"], wgt=d["wgt"], scaler_sums=sums)
        torch.cuda.synchronize()
        row = res[1]["all"][k]
        assert np.array_equal(bits(row), bits(site.cpu().numpy())), k
        total = float(np.sum(p["wgt"] * row))
        assert abs(float(out.item()) - total) <= LNL_RTOL * abs(total), k
        scaled += int(sc.sum().item())
    # exact mode: the same likelihoods, other bits
    ws, o = RS.workspace(p, F64, 2), RS.outputs(n, 5)
    RS.launch(ctx, p, d, 2, ws, o)
    exact = RS.host(o, n, 5)
    assert np.all(np.abs(exact["all"] - res[1]["all"]) <= LNL_RTOL * np.maximum(1.0, np.abs(exact["all"])))
    assert not np.array_equal(bits(exact["all"]), bits(res[1]["all"]))
    print(f"rate scan: {scaled} scaled (site, op, candidate) triples; out {res[1]['out']!r} exact {exact['out']!r}")


# ---- 10: flags ----

def raw_node(c, d, states, flags, dtype=plfx.F64, n=None, sentinel=-7.0):
    """One dense/dense node through the C entry: plfx_plf_psr_dev_gen (flags
    None) or plfx_plf_psr_dev_ex.  Returns (code, x3, scaler bytes, sum)."""
    import torch

    L, h = c._L, c.h
    n = d["n"] if n is None else n
    td = torch.float32 if d["x1"].dtype == np.float32 else torch.float64
    x3 = torch.full((states * d["n"],), sentinel, dtype=td, device="cuda")
    sc = torch.full((d["n"],), 9, dtype=torch.uint8, device="cuda")
    ss = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    keep = [dev(d[k]) for k in ("x1", "x2", "left", "right", "EV", "cat", "wgt")]
    x1, x2, left, right, EV, cat, wgt = (t.data_ptr() for t in keep)
    nd = plfx.PsrNode(None, x1, None, x2, x3.data_ptr(), left, right, sc.data_ptr(), ss.data_ptr())
    tail = (plfx.C.byref(nd), 1, EV, n, cat, d["ncat"], wgt, None, None)
    if flags is None:
        rc = L.plfx_plf_psr_dev_gen(h, dtype, states, *tail)
    else:
        rc = L.plfx_plf_psr_dev_ex(h, dtype, states, flags, *tail)
    torch.cuda.synchronize()
    return rc, x3.cpu().numpy(), sc.cpu().numpy(), int(ss.item())


def same_result(a, b):
    return a[0] == b[0] == plfx.OK and same(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_flags_zero_is_the_gen_call_and_four_states_stay_exact():
    import test_gpu_psr as G

    with plfx.Context(0, lazy_tables=True) as c:
        d20 = make_node(F64, 257, 25, 0)
        gen = raw_node(c, d20, 20, None)
        assert same(gen[1], d20["ref"][0]) and gen[3] == d20["ref"][2]
        assert same_result(raw_node(c, d20, 20, 0), gen)
        fma = raw_node(c, d20, 20, plfx.FMA)
        assert fma[0] == plfx.OK and same(fma[1], fma_case(257, 25, 0)["ref"][0]) and not same(fma[1], gen[1])
        for dt in (np.float64, np.float32):  # DNA is always exact, f32 included
            d4 = dict(G.node_case(dt, 257, 25, 0), n=257, ncat=25)
            gen = raw_node(c, d4, 4, None, plfx.F64 if dt == np.float64 else plfx.F32)
            assert same(gen[1], d4["ref"][0])
            for flags in (0, plfx.FMA):
                assert same_result(raw_node(c, d4, 4, flags, plfx.F64 if dt == np.float64 else plfx.F32), gen), flags


def test_refused_flags_enqueue_nothing_and_leave_the_context_usable():
    import torch

    import test_gpu_psr_prot_rate_scan as RS

    INV, UNS = plfx.ERR_INVALID, plfx.ERR_UNSUPPORTED
    d = make_node(F64, 65, 4, 0)
    d32 = make_node(np.float32, 65, 4, 0)
    p = protein_problem(65)
    n, nops = 65, len(p["ops"])
    with plfx.Context(0, lazy_tables=True) as c:
        L, h = c._L, c.h
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        # the traversal: one op over two dense children
        V = S * n
        big = torch.full((3 * V,), -7.0, dtype=torch.float64, device="cuda")
        big[:V].copy_(dev(d["x1"]))
        big[V:2 * V].copy_(dev(d["x2"]))
        pmats = torch.cat([dev(d["left"]), dev(d["right"])])
        EV, cat = dev(d["EV"]), dev(d["cat"])
        tsum = torch.full((1,), -5, dtype=torch.int64, device="cuda")

        def traverse(flags, dtype=plfx.F64, states=S):
            op = plfx.TravOp(2, 0, 1, 0)
            slots = (plfx.C.c_void_p * 3)(ptr(big[:V]), ptr(big[V:2 * V]), ptr(big[2 * V:]))
            return L.plfx_traverse_psr_ex(h, dtype, states, flags, plfx.C.byref(op), 1, slots, None, 3, ptr(pmats), 1,
                                          ptr(EV), n, ptr(cat), 4, None, None, ptr(tsum), None, None)

        # the scan
        sd = RS.inputs(p, F64, np.geomspace(0.3, 4.0, 5))
        ws, o = RS.workspace(p, F64, 2), RS.outputs(n, 5)
        top = (plfx.TravOp * nops)(*[plfx.TravOp(*map(int, r)) for r in sd["ops"]])
        tp = (plfx.C.c_void_p * p["nslots"])(*[ptr(t) for t in sd["tips"]])

        def scan(flags, dtype=plfx.F64, states=S):
            return L.plfx_psr_rate_scan_ex(h, dtype, states, flags, top, nops, tp, p["nslots"], ptr(sd["blen"]), nops,
                                           ptr(sd["eig"]), ptr(sd["EVd"]), ptr(sd["tvd"]), ptr(sd["cand"]), 5, 2,
                                           ptr(sd["wd"]), ptr(sd["wgt"]), n, ptr(ws), ws.numel(), ptr(o["best_idx"]),
                                           ptr(o["best_lnl"]), ptr(o["all_lnl"]), ptr(o["out_lnl"]), None)

        def node_refused(want, dd, states, flags, dtype=plfx.F64):
            rc, x3, sc, ss = raw_node(c, dd, states, flags, dtype)
            assert rc == want, (flags, states, L.plfx_last_error(h))
            assert np.all(x3 == -7.0) and np.all(sc == 9) and ss == -5  # nothing ran

        for flags in (plfx.VALU, plfx.FMA | plfx.VALU, 4, -1, 1 << 30):
            for states in (4, 20):
                node_refused(INV, d, states, flags)
                assert b"flags" in L.plfx_last_error(h)
                assert traverse(flags, states=states) == INV and b"flags" in L.plfx_last_error(h), (flags, states)
                assert scan(flags, states=states) == INV and b"flags" in L.plfx_last_error(h), (flags, states)
        # f32 in FMA mode: not built
        node_refused(UNS, d32, 20, plfx.FMA, plfx.F32)
        assert b"f64" in L.plfx_last_error(h)
        assert traverse(plfx.FMA, plfx.F32) == UNS and scan(plfx.FMA, plfx.F32) == UNS
        with pytest.raises(plfx.PlfxError) as ei:  # and through the wrapper
            t32 = {k: dev(d32[k]) for k in ("x1", "x2", "left", "right", "EV")}
            c.plf_psr_gen(S, dict(x1=t32["x1"], x2=t32["x2"], x3=torch.empty(V, dtype=torch.float32, device="cuda"),
                                  left=t32["left"], right=t32["right"]), t32["EV"], n, cat, 4, fma=True)
        assert ei.value.code == UNS
        torch.cuda.synchronize()
        assert np.all(big[2 * V:].cpu().numpy() == -7.0) and tsum.item() == -5
        assert np.all(o["all_lnl"].cpu().numpy() == RS.SENTINEL) and o["out_lnl"].item() == RS.SENTINEL
        # the context still works, in both modes
        ref = with_fma_ref(d)
        assert traverse(plfx.FMA) == plfx.OK and scan(plfx.FMA) == plfx.OK
        torch.cuda.synchronize()
        assert same(big[2 * V:].cpu().numpy(), ref["ref"][0]) and tsum.item() == ref["ref_unit"]
        assert np.all(np.isfinite(o["all_lnl"].cpu().numpy()))
        check_node(ref, *run_node(c, ref), what="after the refusals")


def test_no_sites_zero_the_sums_and_launch_nothing(ctx):
    import torch

    d = fma_case(65, 25, 0)
    buf = torch.full((S * 65,), -7.0, dtype=torch.float64, device="cuda")
    ss = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    nd = dict(x1=dev(d["x1"]), x2=dev(d["x2"]), x3=buf, left=dev(d["left"]), right=dev(d["right"]), scaler_sum=ss)
    ctx.plf_psr_gen(S, nd, dev(d["EV"]), 0, dev(d["cat"]), 25, wgt=dev(d["wgt"]), fma=True)
    torch.cuda.synchronize()
    assert int(ss.item()) == 0 and np.all(buf.cpu().numpy() == -7.0)
    p = tree_problem(F64, "balanced 8")
    r = run_tree(ctx, dict(p, n=0))
    torch.cuda.synchronize()
    assert r["sums"].cpu().numpy().tolist() == [0] * len(p["ops"])
    assert ctx.last_schedule()["launches"] == 0


# ---- 11: capture ----

def test_graph_replays_equal_the_eager_run():
    """An FMA batch and an FMA traversal captured in one HIP graph, replayed twice."""
    import torch

    n, ncat = 257, 25
    with plfx.Context(0, lazy_tables=True) as c:
        cases = [make_node(F64, n, ncat, i % 4, 100 + i) for i in range(5)]
        cat, wgt, EV, tv = (dev(cases[0][k]) for k in ("cat", "wgt", "EV", "tipvec"))
        nodes = []
        for d in cases:
            nd = dict(x3=torch.zeros(S * n, dtype=torch.float64, device="cuda"), left=dev(d["left"]),
                      right=dev(d["right"]), scaler=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                      scaler_sum=torch.zeros(1, dtype=torch.int64, device="cuda"))
            nd.update({k: dev(d[k]) for k in ("x1", "x2", "tip1", "tip2") if k in d})
            nodes.append(nd)
        p = tree_problem(F64, "balanced 8", n=n, ncat=ncat)
        tree = dict(clv=[None if p["flags"][s] else torch.zeros(S * n, dtype=torch.float64, device="cuda")
                         for s in range(p["nslots"])],
                    scalers=[torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in p["ops"]],
                    sums=torch.zeros(len(p["ops"]), dtype=torch.int64, device="cuda"))
        outs = ([t for nd in nodes for t in (nd["x3"], nd["scaler"], nd["scaler_sum"])] +
                [t for t in tree["clv"] if t is not None] + tree["scalers"] + [tree["sums"]])
        tin = tree_inputs(p)

        def call(stream):
            c.plf_psr_gen(S, nodes, EV, n, cat, ncat, wgt=wgt, tipvec=tv, stream=stream, fma=True)
            run_tree(c, p, stream=stream, out=tree, t=tin)

        call(None)
        torch.cuda.synchronize()
        first = [t.cpu().numpy().copy() for t in outs]
        assert same(first[0], with_fma_ref(cases[0])["ref"][0])
        cold = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cold):
            call(cold)
        for _ in range(2):
            for t in outs:
                t.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for t, f in zip(outs, first):
                a = t.cpu().numpy()
                assert same(a, f) if a.dtype.kind == "f" else np.array_equal(a, f)
        del g
        torch.cuda.synchronize()
