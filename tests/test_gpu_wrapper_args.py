"""GPU tests of the Python wrapper's tensor-argument checks (plfx/__init__.py):
the C ABI cannot see a tensor's dtype, size, device or strides, so the wrapper
refuses what the kernels would misread, and what it refuses is pinned here
method by method and argument by argument.

Shapes: n = 33 sites, ncat = 4, f64, one node or the three-op tree
psr_trees.mixed (two coded tips, two dense inputs).  For each tensor argument
of traverse, traverse_psr, plf_psr, root_lnl, root_lnl_psr, edge_sumtable,
edge_sumtable_psr, edge_derivatives, edge_derivatives_psr and plf_tips_dev the
call is made with, in turn, a tensor of a wrong dtype, one with one element
fewer than the wrapper's minimum, a CPU tensor and -- where the wrapper demands
contiguity -- a strided view.  Each must raise PlfxError(ERR_INVALID), leave
every sentinel-filled output untouched, and the good call right after must
return the bits the first good call returned.

The clauses are per argument (the table next to each call): `d` dtype, `s`
size, `c` device, `k` contiguity.  Where the wrapper does not demand
contiguity (no `k`: scaler_sums of the traversals, a node's scaler_sum, `out`
of root_lnl, EV of plf_psr, EV / left / right of plf_tips_dev) a strided view
whose first elements are the argument's is accepted and gives the same bits:
the library reads and writes the memory at data_ptr() as a dense array.  The
scaler_sums of root_lnl and edge_derivatives have no minimum size (their
count is the tensor's), so no `s`.  tipvec has no device clause: a CPU table
would be handed to the kernel, so that call is not made."""
import numpy as np
import pytest
import torch

import plfx
import psr_trees as T

pytestmark = pytest.mark.gpu

N, NCAT = 33, 4
F64, U8, I32, I64 = torch.float64, torch.uint8, torch.int32, torch.int64
WRONG = {F64: torch.float16, U8: torch.int8, I32: I64, I64: I32}
SENTINEL = {F64: -7.25, U8: 0xA5, I64: -7}


def rnd(rng, m):
    return torch.from_numpy(rng.random(m) * 0.9 + 0.1).cuda()


def codes(rng, m=N):
    return torch.from_numpy(rng.integers(1, 16, m).astype(np.uint8)).cuda()


def cats(rng):
    return torch.from_numpy(rng.integers(0, NCAT, N).astype(np.uint8)).cuda()


def weights(rng):
    return torch.from_numpy(rng.integers(1, 6, N).astype(np.int32)).cuda()


def out(dtype, m):
    return torch.zeros(m, dtype=dtype, device="cuda")


def eigen(rng):
    return torch.from_numpy(plfx.model_eigen(rng.random(6) + 0.5, rng.random(4) + 0.5)).cuda()


def strided(t, m=None):
    """(view, base): a non-contiguous view of max(numel, 2) elements whose
    data_ptr() is base's, base[:numel] holding t's elements."""
    m = max(t.numel(), 2) if m is None else m
    base = torch.zeros(2 * m, dtype=t.dtype, device=t.device)
    base[:t.numel()] = t.reshape(-1)
    view = base[::2]
    assert not view.is_contiguous() and view.data_ptr() == base.data_ptr() and view.numel() >= t.numel()
    return view, base


def raw(t):
    return t.reshape(-1).view(torch.uint8)


# ---- the calls: (call(ctx, a), arguments a, {name: (minimum count, clauses)}, output names) ----

def tree_args(rng, V, M):
    """psr_trees.mixed: slots 0, 1 coded tips, 2, 3 dense inputs, 4..6 written."""
    a = {f"tip{s}": codes(rng) for s in (0, 1)}
    a.update({f"clv{s}": rnd(rng, V * N) for s in (2, 3)})
    a.update({f"clv{s}": out(F64, V * N) for s in (4, 5, 6)})
    a.update({f"sc{j}": out(U8, N) for j in range(3)})
    a.update(pmats=rnd(rng, 2 * 3 * M), EV=rnd(rng, 16) * 0.3, wgt=weights(rng), sums=out(I64, 3),
             tipvec=rnd(rng, 64))
    spec = {f"tip{s}": (N, "dsck") for s in (0, 1)}
    spec.update({f"clv{s}": (V * N, "dsck") for s in range(2, 7)})
    spec.update({f"sc{j}": (N, "dsck") for j in range(3)})
    spec.update(pmats=(2 * 3 * M, "dsck"), EV=(16, "dsck"), wgt=(N, "dsck"), sums=(3, "dsc"), tipvec=(64, "dsk"))
    return a, spec, ["clv4", "clv5", "clv6", "sc0", "sc1", "sc2", "sums"]


def tree_lists(a):
    ops = np.array(T.mixed(False)[0], np.int32)
    clv = [None, None] + [a[f"clv{s}"] for s in range(2, 7)]
    tips = [a["tip0"], a["tip1"]] + [None] * 5
    return ops, clv, tips, [a[f"sc{j}"] for j in range(3)]


def case_traverse(rng):
    a, spec, outs = tree_args(rng, 16, 64)

    def call(ctx, a, **kw):
        ops, clv, tips, sc = tree_lists(a)
        ctx.traverse(ops, clv, a["pmats"], a["EV"], N, wgt=a["wgt"], scalers=sc, scaler_sums=a["sums"], tips=tips,
                     tipvec=a["tipvec"], **kw)

    return call, a, spec, outs


def case_traverse_psr(rng):
    a, spec, outs = tree_args(rng, 4, 16 * NCAT)
    a["cat"], spec["cat"] = cats(rng), (N, "dsck")

    def call(ctx, a, **kw):
        ops, clv, tips, sc = tree_lists(a)
        ctx.traverse_psr(ops, clv, a["pmats"], a["EV"], N, a["cat"], NCAT, wgt=a["wgt"], scalers=sc,
                         scaler_sums=a["sums"], tips=tips, tipvec=a["tipvec"], **kw)

    return call, a, spec, outs


def node_args(rng, V, M, coded):
    """One node, child `coded` (1 or 2) as codes, the other dense."""
    dense = 3 - coded
    a = {f"tip{coded}": codes(rng), f"x{dense}": rnd(rng, V * N), "x3": out(F64, V * N), "left": rnd(rng, M),
         "right": rnd(rng, M), "EV": rnd(rng, 16) * 0.3, "wgt": weights(rng), "scaler": out(U8, N),
         "scaler_sum": out(I64, 1), "tipvec": rnd(rng, 64)}
    spec = {f"tip{coded}": (N, "dsck"), f"x{dense}": (V * N, "dsck"), "x3": (V * N, "dsck"), "wgt": (N, "dsck"),
            "scaler": (N, "dsck"), "scaler_sum": (1, "dsc"), "tipvec": (64, "dsk")}
    return a, spec, ["x3", "scaler", "scaler_sum"]


def case_plf_psr(coded):
    def make(rng):
        a, spec, outs = node_args(rng, 4, 16 * NCAT, coded)
        a["cat"] = cats(rng)
        spec.update(left=(16 * NCAT, "dsck"), right=(16 * NCAT, "dsck"), EV=(16, "dsc"), cat=(N, "dsck"))
        keys = [k for k in ("tip1", "x1", "tip2", "x2", "x3", "left", "right", "scaler", "scaler_sum") if k in a]

        def call(ctx, a, **kw):
            ctx.plf_psr({k: a[k] for k in keys}, a["EV"], N, a["cat"], NCAT, wgt=a["wgt"], tipvec=a["tipvec"], **kw)

        return call, a, spec, outs

    return make


def case_plf_tips_dev(coded):
    def make(rng):
        a, spec, outs = node_args(rng, 16, 64, coded)
        spec.update(left=(64, "dsc"), right=(64, "dsc"), EV=(16, "dsc"))

        def call(ctx, a):
            ctx.plf_tips_dev(a["x3"], a["EV"], N, a["left"], a["right"], x1=a.get("x1"), x2=a.get("x2"),
                             tip1=a.get("tip1"), tip2=a.get("tip2"), wgt=a["wgt"], scaler=a["scaler"],
                             scaler_sum=a["scaler_sum"], tipvec=a["tipvec"])

        return call, a, spec, outs

    return make


def case_root_lnl(psr):
    def make(rng):
        V = 4 if psr else 16
        a = dict(x=rnd(rng, V * N), out=out(F64, 1), freq=rnd(rng, 4), wgt=weights(rng),
                 sums=torch.tensor([1, 2, 3], dtype=I64, device="cuda"), site_lnl=out(F64, N))
        spec = dict(x=(V * N, "dsck"), out=(1, "dsc"), freq=(4, "dsck"), wgt=(N, "dsck"), sums=(None, "dck"),
                    site_lnl=(N, "dsck"))
        if not psr:
            a["catw"], spec["catw"] = rnd(rng, 4), (4, "dsck")

        def call(ctx, a, **kw):
            if psr:
                ctx.root_lnl_psr(a["x"], N, a["out"], freq=a["freq"], wgt=a["wgt"], scaler_sums=a["sums"],
                                 site_lnl=a["site_lnl"], **kw)
            else:
                ctx.root_lnl(a["x"], N, a["out"], catw=a["catw"], freq=a["freq"], wgt=a["wgt"],
                             scaler_sums=a["sums"], site_lnl=a["site_lnl"])

        return call, a, spec, ["out", "site_lnl"]

    return make


def case_edge_sumtable(psr, coded):
    def make(rng):
        V = 4 if psr else 16
        a = dict(x2=rnd(rng, V * N), sumtab=out(F64, V * N))
        spec = dict(x2=(V * N, "dsck"), sumtab=(V * N, "dsck"))
        if coded:
            a.update(tip1=codes(rng), tipvec=rnd(rng, 64))
            spec.update(tip1=(N, "dsck"), tipvec=(64, "dsk"))
        else:
            a["x1"], spec["x1"] = rnd(rng, V * N), (V * N, "dsck")

        def call(ctx, a, **kw):
            fn = ctx.edge_sumtable_psr if psr else ctx.edge_sumtable
            fn(a["x2"], a["sumtab"], N, x1=a.get("x1"), tip1=a.get("tip1"), tipvec=a.get("tipvec"), **kw)

        return call, a, spec, ["sumtab"]

    return make


def case_edge_derivatives(psr):
    def make(rng):
        V = 4 if psr else 16
        # positive entries: every site likelihood is positive whatever the basis
        a = dict(sumtab=rnd(rng, V * N), eigen=eigen(rng), rates=rnd(rng, 4), wgt=weights(rng), t=rnd(rng, 1),
                 out=out(F64, 3), site_lnl=out(F64, N), sums=torch.tensor([1, 2, 3], dtype=I64, device="cuda"))
        # the wrapper's minimum for eigen is 4 values and for rates 1 (the library reads S + 2 S^2 and ncat)
        spec = dict(sumtab=(V * N, "dsck"), eigen=(4, "dsck"), rates=(1, "dsck"), wgt=(N, "dsck"), t=(1, "dsck"),
                    out=(3, "dsck"), site_lnl=(N, "dsck"), sums=(None, "dck"))
        if psr:
            a["cat"], spec["cat"] = cats(rng), (N, "dsck")
        else:
            a["catw"], spec["catw"] = rnd(rng, 4), (4, "dsck")

        def call(ctx, a, **kw):
            if psr:
                ctx.edge_derivatives_psr(a["sumtab"], N, a["eigen"], a["rates"], a["cat"], a["t"], a["out"],
                                         wgt=a["wgt"], scaler_sums=a["sums"], site_lnl=a["site_lnl"], **kw)
            else:
                ctx.edge_derivatives(a["sumtab"], N, a["eigen"], a["rates"], a["t"], a["out"], catw=a["catw"],
                                     wgt=a["wgt"], scaler_sums=a["sums"], site_lnl=a["site_lnl"])

        return call, a, spec, ["out", "site_lnl"]

    return make


CASES = {
    "traverse": case_traverse,
    "traverse_psr": case_traverse_psr,
    "plf_psr tip/dense": case_plf_psr(1),
    "plf_psr dense/tip": case_plf_psr(2),
    "root_lnl": case_root_lnl(False),
    "root_lnl_psr": case_root_lnl(True),
    "edge_sumtable dense": case_edge_sumtable(False, False),
    "edge_sumtable coded": case_edge_sumtable(False, True),
    "edge_sumtable_psr dense": case_edge_sumtable(True, False),
    "edge_sumtable_psr coded": case_edge_sumtable(True, True),
    "edge_derivatives": case_edge_derivatives(False),
    "edge_derivatives_psr": case_edge_derivatives(True),
    "plf_tips_dev tip/dense": case_plf_tips_dev(1),
    "plf_tips_dev dense/tip": case_plf_tips_dev(2),
}
PSR_CASES = [k for k in CASES if "psr" in k]


# ---- the checks ----

def fill(a, outs):
    for k in outs:
        a[k].fill_(SENTINEL[a[k].dtype])


def written(a, outs, skip=None):
    """The outputs that no longer hold the sentinel everywhere."""
    torch.cuda.synchronize()
    return [k for k in outs if k != skip and not bool((a[k] == SENTINEL[a[k].dtype]).all())]


def run_good(ctx, call, a, outs):
    fill(a, outs)
    call(ctx, a)
    torch.cuda.synchronize()
    return {k: raw(a[k]).clone() for k in outs}


def same_bits(got, want):
    return [k for k in want if not torch.equal(got[k], want[k])]


def variants(t, count, clauses):
    """(label, tensor) of every refused form of argument t."""
    if "d" in clauses:
        yield "wrong dtype", torch.zeros(8 * t.numel(), dtype=WRONG[t.dtype], device="cuda")  # no fewer bytes
    if "s" in clauses:
        yield "one element too few", torch.zeros(count - 1, dtype=t.dtype, device="cuda")
    if "c" in clauses:
        yield "CPU tensor", t.cpu()
    if "k" in clauses:
        yield "strided view", strided(t)[0]


@pytest.mark.parametrize("name", list(CASES))
def test_tensor_argument_checks(ctx, name):
    call, a, spec, outs = CASES[name](np.random.default_rng(len(name) + 5))
    assert set(spec) == set(a)  # every tensor argument has its clauses
    good = run_good(ctx, call, a, outs)
    assert written(a, outs) == outs  # the good call writes every output
    for k, (count, clauses) in spec.items():
        for label, bad in variants(a[k], count, clauses):
            fill(a, outs)
            with pytest.raises(plfx.PlfxError) as ei:
                call(ctx, dict(a, **{k: bad}))
            assert ei.value.code == plfx.ERR_INVALID, (k, label, str(ei.value))
            assert written(a, outs, skip=k) == [], (k, label)
            assert same_bits(run_good(ctx, call, a, outs), good) == [], (k, label)
        if "k" not in clauses:  # contiguity is not demanded: the memory at data_ptr() is what counts
            view, base = strided(a[k])
            fill(a, outs)
            if k in outs:
                base.fill_(SENTINEL[base.dtype])
            call(ctx, dict(a, **{k: view}))
            torch.cuda.synchronize()
            got = {o: raw(base[:a[o].numel()] if o == k else a[o]) for o in outs}
            assert same_bits(got, good) == [], (k, "strided view accepted")


@pytest.mark.parametrize("name", PSR_CASES)
def test_psr_refuses_protein(ctx, name):
    """states=20 on a per-site-rate method: PLFX_ERR_UNSUPPORTED, nothing written."""
    call, a, spec, outs = CASES[name](np.random.default_rng(len(name) + 5))
    good = run_good(ctx, call, a, outs)
    fill(a, outs)
    with pytest.raises(plfx.PlfxError) as ei:
        call(ctx, a, states=20)
    assert ei.value.code == plfx.ERR_UNSUPPORTED
    assert written(a, outs) == []
    assert same_bits(run_good(ctx, call, a, outs), good) == []
