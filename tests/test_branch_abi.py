"""CPU checks of plfx.h section 13, all-branch derivatives
(plfx_branch_sumtables_psr, plfx_branch_sumtables_psr_workspace): the header
declares them and PLFX_BRANCH_NOFUSE on a free bit, the library exports them,
the Python binding lists and resolves them, the workspace size follows the
documented layout, the Context method places every argument where plfx.h puts
it (a recorder stands for the library, as tests/test_wrapper_psr_calls.py), and
the new side library's gfx950 code object holds the twelve instantiations of
the sibling-pair kernel while libplfx.so and the other side libraries hold
none.  No GPU work."""
import ctypes as C
import inspect
import re
import subprocess

import numpy as np
import pytest
import torch

import plfx
from conftest import PKG, ROOT
from test_wrapper_psr_calls import STREAM, Recorder, Stand, _addr, _ptrs

HEADER = ROOT / "include" / "plfx.h"
LIB = PKG / "plfx" / "libplfx.so"
BRANCH_LIB = PKG / "plfx" / "libplfx_psr_branch.so"
NAMES = ("plfx_branch_sumtables_psr", "plfx_branch_sumtables_psr_workspace", "plfx_branch_pair_sites_per_lane")
KERNEL = "psr_branch_pair_kernel"
N, NCAT = 3, 2
OPS = [[3, 0, 1, 0], [4, 3, 2, 1]]  # slot 0 is the coded tip


def test_header_declares_the_section():
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert "(13)" in raw
    assert re.search(r"\bint\s+plfx_branch_sumtables_psr\s*\(\s*plfx_ctx\s*\*\s*ctx\s*,\s*int\s+dtype\s*,\s*int\s+states\s*,"
                     r"\s*int\s+flags\s*,", text)
    assert re.search(r"\bint\s+plfx_branch_sumtables_psr_workspace\s*\(\s*int\s+dtype\s*,\s*int\s+states\s*,\s*int\s+nops"
                     r"\s*,\s*int64_t\s+n\s*,\s*size_t\s*\*\s*bytes\s*\)", text)
    flag = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", raw).group(1))  # noqa: E731
    nofuse = flag("PLFX_BRANCH_NOFUSE")
    assert nofuse == plfx.BRANCH_NOFUSE and bin(nofuse).count("1") == 1
    assert not nofuse & (flag("PLFX_FMA") | flag("PLFX_VALU"))  # a free bit


def test_library_exports_the_symbols():
    assert LIB.exists(), "run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NAMES:
        assert name in exported, name
    assert all(s.startswith("plfx_") for s in exported if "branch" in s)  # nothing else of the feature leaks out


def test_binding_lists_and_resolves_them():
    L = plfx.load()
    for name in NAMES:
        assert name in plfx.EXPORTS and getattr(L, name).argtypes
    assert len(L.plfx_branch_sumtables_psr.argtypes) == 24
    for m in ("branch_sumtables_psr", "branch_derivatives_psr"):
        p = inspect.signature(getattr(plfx.Context, m)).parameters
        assert p["fma"].default is False and p["nofuse"].default is False, m
    assert plfx.branch_pair_sites_per_lane(np.float64) == 2 and plfx.branch_pair_sites_per_lane(np.float32) == 4
    assert plfx.branch_pair_sites_per_lane(7) == 0


@pytest.mark.parametrize("dtype,size", [(np.float32, 4), (np.float64, 8)])
def test_workspace_follows_the_documented_layout(dtype, size):
    for states in (4, 20):
        for nops, n in ((1, 1), (3, 65), (12, 5000), (63, 0)):
            slab = (n * states * size + 255) // 256 * 256
            want = (2 * (nops - 1) + 2 * nops - 1) * slab + (5 * nops * 8 + 255) // 256 * 256
            assert plfx.branch_sumtables_psr_workspace(dtype, states, nops, n) == want
    assert plfx.branch_sumtables_psr_workspace(dtype, 20, 12, 65) > plfx.branch_sumtables_psr_workspace(dtype, 4, 12, 65)
    for bad in ((dtype, 4, 0, 65), (dtype, 4, 3, -1), (5, 4, 3, 65)):
        with pytest.raises(plfx.PlfxError) as e:
            plfx.branch_sumtables_psr_workspace(*bad)
        assert e.value.code == plfx.ERR_INVALID
    with pytest.raises(plfx.PlfxError) as e:
        plfx.branch_sumtables_psr_workspace(dtype, 5, 3, 65)
    assert e.value.code == plfx.ERR_UNSUPPORTED


class Workspace(Stand):
    """A workspace stand-in: slicing gives what the wrapper would view."""

    def __getitem__(self, sl):
        ws = self

        class Slice:
            def view(self, dt):
                return (ws.addr + sl.start, sl.stop - sl.start, dt)

        return Slice()


@pytest.fixture
def ctx():
    c = object.__new__(plfx.Context)
    c._L, c.h, c.device, c._used = Recorder(), C.c_void_p(1), 0, {}
    yield c
    c.h = None


@pytest.mark.parametrize("S", [4, 20])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=("f32", "f64"))
def test_wrapper_places_every_argument(ctx, dt, S):
    u8, i32, i64 = torch.uint8, torch.int32, torch.int64
    mk = lambda d, count: Stand(d, count)  # noqa: E731
    clv = [None] + [mk(dt, S * N) for _ in range(4)]
    tips = [mk(u8, N)] + [None] * 4
    pm, root_pm, EV = mk(dt, 2 * 2 * NCAT * S * S), mk(dt, NCAT * S * S), mk(dt, S * S)
    cat, wgt, sums, es = mk(u8, N), mk(i32, N), mk(i64, 2), mk(i64, 4)
    tv = mk(dt, 16 * 4 if S == 4 else plfx.PROT_CODES * 20)
    ws = Workspace(u8, 4096)
    code = plfx.F32 if dt == torch.float32 else plfx.F64
    for kw, flags in ((dict(), 0), (dict(nofuse=True), plfx.BRANCH_NOFUSE), (dict(fma=True, nofuse=True), 5)):
        ctx._L.calls.clear()
        tabs = ctx.branch_sumtables_psr(S, OPS, clv, pm, root_pm, EV, N, cat, NCAT, sums, ws, wgt=wgt, edge_scale=es,
                                        tips=tips, tipvec=tv, stream=STREAM, **kw)
        (name, args), = ctx._L.calls
        assert name == "plfx_branch_sumtables_psr"
        assert args == [1, code, S, flags, b"".join(bytes(plfx.TravOp(*r)) for r in OPS), 2, _ptrs(clv), _ptrs(tips), 5,
                        pm.addr, 2, root_pm.addr, EV.addr, N, cat.addr, NCAT, wgt.addr, sums.addr, tv.addr, ws.addr, 4096,
                        bytes(8 * 4), es.addr, STREAM]
        # the recorder fills no pointer: every view starts at the workspace and spans one table
        assert tabs == [(ws.addr, S * N * (4 if dt == torch.float32 else 8), dt)] * 4
    ctx._L.calls.clear()
    for short in ("root_pm", "es", "cat"):
        bad = dict(root_pm=root_pm, es=es, cat=cat)
        bad[short] = Stand(bad[short].dtype, bad[short].count - 1)
        with pytest.raises(plfx.PlfxError) as e:
            ctx.branch_sumtables_psr(S, OPS, clv, pm, bad["root_pm"], EV, N, bad["cat"], NCAT, sums, ws, wgt=wgt,
                                     edge_scale=bad["es"], tips=tips, tipvec=tv, stream=STREAM)
        assert e.value.code == plfx.ERR_INVALID and ctx._L.calls == [], short
    with pytest.raises(plfx.PlfxError) as e:
        ctx.branch_sumtables_psr(5, OPS, clv, pm, root_pm, EV, N, cat, NCAT, sums, ws, stream=STREAM)
    assert e.value.code == plfx.ERR_UNSUPPORTED and ctx._L.calls == []
    assert _addr(None) is None


def test_new_library_holds_the_pair_kernels_and_the_others_none():
    from plfx import codeobj

    assert BRANCH_LIB.exists(), "run __graft_entry__.build() first"
    got = codeobj.kernel_instantiations(BRANCH_LIB, KERNEL)
    # <T, U, kSum, kTips>: f64 with 2 sites per lane, f32 with 4
    want = {f"I{t}Li{u}ELb{s}ELi{k}EE" for t, u in (("d", 2), ("f", 4)) for s in (0, 1) for k in (0, 1, 2)}
    assert len(got) == 12 and {s.split(KERNEL)[1][:len("IdLi2ELb0ELi0EE")] for s in got} == want, got
    for lib in ("libplfx.so", "libplfx_psr.so", "libplfx_psr_prot.so", "libplfx_psr_prot_mfma.so", "libplfx_edge.so"):
        assert codeobj.kernel_instantiations(PKG / "plfx" / lib, "psr_branch") == [], lib
    # the per-site-rate library's kernels are where they were, the tiling kernel in it alone
    assert len(codeobj.kernel_instantiations(PKG / "plfx" / "libplfx_psr.so", "psr_tile_kernel")) == 1
    assert codeobj.kernel_instantiations(BRANCH_LIB, "psr_tile_kernel") == []
