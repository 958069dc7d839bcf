"""What the per-site-rate methods of plfx.Context hand to the C ABI, recorded
on the CPU: the context's library is a recorder and the tensors are stand-ins
with made-up addresses, so no library is loaded and no GPU is touched.

Every PSR method and its `_gen` twin must form the same call but for the state
count; a `_gen` call with 20 states must place every pointer where plfx.h puts
it and refuse a tensor one element short; a state count that is not built must
be refused before anything is called; and the Gamma edge methods, which share
the PSR methods' helpers, must keep their own layout."""
import ctypes as C
import itertools

import pytest
import torch

import plfx

N, NCAT, STREAM = 3, 2, 7
DTYPES = (torch.float32, torch.float64)
OPS = ("plf_psr", "traverse_psr", "root_lnl_psr", "edge_sumtable_psr", "edge_sumtables_psr",
       "edge_derivatives_psr", "optimize_branch_psr", "optimize_branches_psr")
SYMBOL = {"plf_psr": "plfx_plf_psr_dev", "traverse_psr": "plfx_traverse_psr", "root_lnl_psr": "plfx_root_lnl_psr",
          "edge_sumtable_psr": "plfx_edge_sumtable_psr", "edge_sumtables_psr": "plfx_edge_sumtable_psr_batch",
          "edge_derivatives_psr": "plfx_edge_derivatives_psr", "optimize_branch_psr": "plfx_edge_optimize_psr",
          "optimize_branches_psr": "plfx_edge_optimize_psr_dev"}
TRAV_OPS = [[1, 0, 0, 0], [2, 0, 1, 1]]  # slot 0 is the coded tip


class Recorder:
    """Stands for the loaded library: any attribute is a function that records its call."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, [_plain(a) for a in args]))
            return 0

        return fn


def _plain(a):
    if isinstance(a, C.c_void_p):
        return a.value
    if isinstance(a, (C.Array, C.Structure)):
        return bytes(a)
    if type(a).__name__ == "CArgObject":  # byref() of a host out-argument
        return "byref"
    return a


class Stand:
    """What the wrapper asks of a torch device tensor, at a made-up address."""
    _next = itertools.count(0x1000, 0x100)
    is_cuda = True

    def __init__(self, dtype, count, addr=None):
        self.dtype, self.count, self.shape = dtype, count, (count,)
        self.addr = next(Stand._next) if addr is None else addr

    def numel(self):
        return self.count

    def dim(self):
        return 1

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.addr


@pytest.fixture
def ctx():
    c = object.__new__(plfx.Context)
    c._L, c.h, c.device, c._used = Recorder(), C.c_void_p(1), 0, {}
    yield c
    c.h = None


class Inputs:
    """The stand-ins of one operation, each of exactly the smallest size the
    wrapper takes for S states; `short` names the one made an element shorter.
    `sized` lists the names whose size the wrapper checks against a minimum.
    The addresses depend on the order of creation alone, so two Inputs of one
    operation are the same stand-ins."""

    def __init__(self, S, dt, short=None):
        self.S, self.dt, self.short, self.sized = S, dt, short, []
        self.addrs = itertools.count(0x1000, 0x100)

    def mk(self, name, dtype, count, sized=True):
        if sized:
            self.sized.append(name)
        t = Stand(dtype, count - (1 if name == self.short else 0), next(self.addrs))
        setattr(self, name, t)
        return t

    def tipvec(self):
        return self.mk("tipvec", self.dt, 16 * 4 if self.S == 4 else plfx.PROT_CODES * 20)


def _addr(t):
    return None if t is None else t.addr


def _ptrs(ts):
    return bytes((C.c_void_p * len(ts))(*[_addr(t) for t in ts]))


def run(ctx, op, gen, S, dt, short=None, states=None):
    """Call `op` (its _gen twin with gen) on fresh stand-ins for S states; returns
    the argument list plfx.h gives the _gen entry for them."""
    a = Inputs(S, dt, short)
    u8, i32, i64, f64 = torch.uint8, torch.int32, torch.int64, torch.float64
    states = S if states is None else states
    code = plfx.F32 if dt == torch.float32 else plfx.F64
    head = [1, code, states]

    def call(*args, **kw):
        if gen:
            getattr(ctx, op + "_gen")(states, *args, stream=STREAM, **kw)
        else:
            getattr(ctx, op)(*args, states=states, stream=STREAM, **kw)

    if op == "plf_psr":
        nd = dict(tip1=a.mk("tip1", u8, N), x2=a.mk("x2", dt, S * N), x3=a.mk("x3", dt, S * N),
                  left=a.mk("left", dt, NCAT * S * S), right=a.mk("right", dt, NCAT * S * S),
                  scaler=a.mk("scaler", u8, N), scaler_sum=a.mk("scaler_sum", i64, 1))
        a.mk("EV", dt, S * S), a.mk("rate_cat", u8, N), a.mk("wgt", i32, N), a.tipvec()
        want = head + [bytes(plfx.PsrNode(a.tip1.addr, None, None, a.x2.addr, a.x3.addr, a.left.addr, a.right.addr,
                                          a.scaler.addr, a.scaler_sum.addr)),
                       1, a.EV.addr, N, a.rate_cat.addr, NCAT, a.wgt.addr, a.tipvec.addr, STREAM]
        call([nd], a.EV, N, a.rate_cat, NCAT, wgt=a.wgt, tipvec=a.tipvec)
    elif op == "traverse_psr":
        clv = [None, a.mk("clv1", dt, S * N), a.mk("clv2", dt, S * N)]
        tips = [a.mk("tip0", u8, N), None, None]
        a.mk("pmats", dt, 2 * 2 * NCAT * S * S), a.mk("EV", dt, S * S), a.mk("rate_cat", u8, N), a.mk("wgt", i32, N)
        sc = [a.mk("scaler0", u8, N), a.mk("scaler1", u8, N)]
        a.mk("scaler_sums", i64, 2), a.tipvec()
        want = head + [b"".join(bytes(plfx.TravOp(*r)) for r in TRAV_OPS), 2, _ptrs(clv), _ptrs(tips), 3, a.pmats.addr,
                       2, a.EV.addr, N, a.rate_cat.addr, NCAT, a.wgt.addr, _ptrs(sc), a.scaler_sums.addr,
                       a.tipvec.addr, STREAM]
        call(TRAV_OPS, clv, a.pmats, a.EV, N, a.rate_cat, NCAT, wgt=a.wgt, scalers=sc, scaler_sums=a.scaler_sums,
             tips=tips, tipvec=a.tipvec)
    elif op == "root_lnl_psr":
        a.mk("x", dt, S * N), a.mk("out", f64, 1), a.mk("freq", f64, S), a.mk("wgt", i32, N)
        a.mk("scaler_sums", i64, 2, sized=False), a.mk("site_lnl", f64, N)
        want = head + [a.x.addr, N, a.freq.addr, a.wgt.addr, a.scaler_sums.addr, 2, a.out.addr, a.site_lnl.addr,
                       STREAM]
        call(a.x, N, a.out, freq=a.freq, wgt=a.wgt, scaler_sums=a.scaler_sums, site_lnl=a.site_lnl)
    elif op == "edge_sumtable_psr":
        a.mk("x2", dt, S * N), a.mk("sumtab", dt, S * N), a.mk("tip1", u8, N), a.tipvec()
        want = head + [a.tip1.addr, None, a.x2.addr, N, a.tipvec.addr, a.sumtab.addr, STREAM]
        call(a.x2, a.sumtab, N, tip1=a.tip1, tipvec=a.tipvec)
    elif op == "edge_sumtables_psr":
        e0 = dict(x1=a.mk("x1", dt, S * N), x2=a.mk("x2", dt, S * N), sumtab=a.mk("sumtab0", dt, S * N))
        e1 = dict(tip1=a.mk("tip1", u8, N), x2=a.x2, sumtab=a.mk("sumtab1", dt, S * N))
        a.tipvec()
        want = head + [bytes(plfx.PsrEdge(None, a.x1.addr, a.x2.addr, a.sumtab0.addr)) +
                       bytes(plfx.PsrEdge(a.tip1.addr, None, a.x2.addr, a.sumtab1.addr)),
                       2, N, a.tipvec.addr, STREAM]
        call([e0, e1], N, tipvec=a.tipvec)
    else:
        a.mk("eigen", f64, S), a.mk("rates", f64, NCAT, sized=False), a.mk("rate_cat", u8, N), a.mk("wgt", i32, N)
        model = [N, a.eigen.addr, a.rates.addr, NCAT, a.rate_cat.addr, a.wgt.addr]
        if op == "edge_derivatives_psr":
            a.mk("sumtab", dt, S * N), a.mk("t", f64, 1), a.mk("out", f64, 3)
            a.mk("scaler_sums", i64, 2, sized=False), a.mk("site_lnl", f64, N)
            want = head + [a.sumtab.addr] + model + [a.t.addr, a.scaler_sums.addr, 2, a.out.addr, a.site_lnl.addr,
                                                     STREAM]
            call(a.sumtab, N, a.eigen, a.rates, a.rate_cat, a.t, a.out, wgt=a.wgt, scaler_sums=a.scaler_sums,
                 site_lnl=a.site_lnl)
        elif op == "optimize_branch_psr":
            a.mk("sumtab", dt, S * N)
            want = head + [a.sumtab.addr] + model + [0.25, 1e-6, 5.0, 9, "byref", bytes(24), "byref", STREAM]
            call(a.sumtab, N, a.eigen, a.rates, a.rate_cat, 0.25, tmin=1e-6, tmax=5.0, max_evals=9, wgt=a.wgt)
        else:
            tabs = [a.mk("sumtab0", dt, S * N), a.mk("sumtab1", dt, S * N)]
            a.mk("t0", f64, 2), a.mk("t_opt", f64, 2), a.mk("out3", f64, 6), a.mk("evals", i32, 2)
            want = head + [_ptrs(tabs), 2] + model + [a.t0.addr, 1e-6, 5.0, 9, a.t_opt.addr, a.out3.addr, a.evals.addr,
                                                      STREAM]
            call(tabs, N, a.eigen, a.rates, a.rate_cat, a.t0, a.t_opt, tmin=1e-6, tmax=5.0, max_evals=9, out3=a.out3,
                 evals=a.evals, wgt=a.wgt)
    return want, a.sized


@pytest.mark.parametrize("dt", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("op", OPS)
def test_twin_calls_agree(ctx, op, dt):
    want, _ = run(ctx, op, False, 4, dt)
    (name, args), = ctx._L.calls
    assert name == SYMBOL[op] and args == want[:2] + want[3:]
    ctx._L.calls.clear()
    run(ctx, op, True, 4, dt)
    (name, gen_args), = ctx._L.calls
    assert name == SYMBOL[op] + "_gen" and gen_args[2] == 4
    assert gen_args[:2] + gen_args[3:] == args and gen_args == want


@pytest.mark.parametrize("dt", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("op", OPS)
def test_twenty_states(ctx, op, dt):
    want, sized = run(ctx, op, True, 20, dt)
    (name, args), = ctx._L.calls
    assert name == SYMBOL[op] + "_gen" and args[2] == 20 and args == want
    ctx._L.calls.clear()
    assert len(sized) >= 3
    for short in sized:
        with pytest.raises(plfx.PlfxError) as e:
            run(ctx, op, True, 20, dt, short=short)
        assert e.value.code == plfx.ERR_INVALID, short
        assert ctx._L.calls == [], short


@pytest.mark.parametrize("op", OPS)
def test_refused_state_counts(ctx, op):
    for gen, states, built in ((False, 20, "(4)"), (True, 5, "(4, 20)")):
        with pytest.raises(plfx.PlfxError) as e:
            run(ctx, op, gen, 20, torch.float64, states=states)
        assert e.value.code == plfx.ERR_UNSUPPORTED
        assert f"per-site rate categories: states={states} not built {built}" in str(e.value)
        assert ctx._L.calls == []


@pytest.mark.parametrize("dt", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("S", (4, 20))
def test_gamma_edge_methods_keep_their_layout(ctx, S, dt):
    f64 = torch.float64
    code = plfx.F32 if dt == torch.float32 else plfx.F64
    tabs = [Stand(dt, 4 * S * N), Stand(dt, 4 * S * N)]
    eigen, rates, catw, wgt = Stand(f64, S), Stand(f64, 4), Stand(f64, 4), Stand(torch.int32, N)
    t, out, sums, site = Stand(f64, 1), Stand(f64, 3), Stand(torch.int64, 2), Stand(f64, N)
    t0, t_opt, out3, evals = Stand(f64, 2), Stand(f64, 2), Stand(f64, 6), Stand(torch.int32, 2)
    model = [N, eigen.addr, rates.addr, 4, catw.addr, wgt.addr]
    ctx.edge_derivatives(tabs[0], N, eigen, rates, t, out, catw=catw, wgt=wgt, scaler_sums=sums, site_lnl=site,
                         states=S, stream=STREAM)
    ctx.optimize_branch(tabs[0], N, eigen, rates, 0.25, tmin=1e-6, tmax=5.0, max_evals=9, catw=catw, wgt=wgt,
                        states=S, stream=STREAM)
    ctx.optimize_branches(tabs, N, eigen, rates, t0, t_opt, tmin=1e-6, tmax=5.0, max_evals=9, out3=out3, evals=evals,
                          catw=catw, wgt=wgt, states=S, stream=STREAM)
    assert ctx._L.calls == [
        ("plfx_edge_derivatives", [1, code, S, tabs[0].addr] + model + [t.addr, sums.addr, 2, out.addr, site.addr,
                                                                        STREAM]),
        ("plfx_edge_optimize", [1, code, S, tabs[0].addr] + model + [0.25, 1e-6, 5.0, 9, "byref", bytes(24), "byref",
                                                                     STREAM]),
        ("plfx_edge_optimize_dev", [1, code, S, _ptrs(tabs), 2] + model + [t0.addr, 1e-6, 5.0, 9, t_opt.addr,
                                                                           out3.addr, evals.addr, STREAM]),
    ]
