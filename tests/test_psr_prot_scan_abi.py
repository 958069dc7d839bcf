"""CPU checks of plfx.h section 12b, the rate scan with a state count
(plfx_site_lnl_psr_gen, plfx_psr_rate_scan_gen,
plfx_psr_rate_scan_workspace_gen): the header declares them with `states` in
its place, the Python binding lists and resolves them, the Context methods
exist, libplfx_psr_prot.so's gfx950 code object holds the new kernel, and the
workspace query is the documented formula.  No GPU work."""
import re

import pytest

from conftest import PKG, ROOT

HEADER = ROOT / "include" / "plfx.h"
PROT_LIB = PKG / "plfx" / "libplfx_psr_prot.so"
NAMES = ("plfx_site_lnl_psr_gen", "plfx_psr_rate_scan_gen", "plfx_psr_rate_scan_workspace_gen")
ALIGN = 256


def test_header_declares_the_three_functions():
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES[:2]:  # the state count follows dtype
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*plfx_ctx\s*\*\s*ctx\s*,\s*int\s+dtype\s*,\s*int\s+states\s*,",
                         text), name
    # no context: dtype first, then the state count
    assert re.search(r"\bint\s+" + NAMES[2] + r"\s*\(\s*int\s+dtype\s*,\s*int\s+states\s*,\s*int\s+nops\s*,", text)
    assert "(12b)" in raw
    # section 12's own three are still declared as they were
    for name in ("plfx_site_lnl_psr", "plfx_psr_rate_scan"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*plfx_ctx\s*\*\s*ctx\s*,\s*int\s+dtype\s*,\s*const\b", text), name
    assert re.search(r"\bint\s+plfx_psr_rate_scan_workspace\s*\(\s*int\s+dtype\s*,\s*int\s+nops\s*,", text)


def test_binding_lists_and_resolves_them():
    import plfx

    L = plfx.load()
    for name in NAMES:
        assert name in plfx.EXPORTS
        fn, base = getattr(L, name), getattr(L, name[:-len("_gen")])
        assert fn.argtypes and len(fn.argtypes) == len(base.argtypes) + 1
    for m in ("site_lnl_psr_gen", "psr_rate_scan_gen"):
        assert callable(getattr(plfx.Context, m))
    assert callable(plfx.psr_rate_scan_workspace_gen)


def test_protein_psr_code_object_holds_the_scan_kernel():
    from plfx import codeobj

    assert PROT_LIB.exists(), "run __graft_entry__.build() first"
    kernel = "psr_site_lnl_prot_kernel"  # <T, kBest>: {f, d} x {Lb0, Lb1}
    got = codeobj.kernel_instantiations(PROT_LIB, kernel)
    assert len(got) == 4 and {s.split(kernel + "I")[1][:4] for s in got} == {"fLb0", "fLb1", "dLb0", "dLb1"}, got
    # the DNA library did not take it, and keeps its own
    psr = PKG / "plfx" / "libplfx_psr.so"
    assert codeobj.kernel_instantiations(psr, kernel) == []
    assert len(codeobj.kernel_instantiations(psr, "psr_site_lnl_kernel")) == 4


def up(v):
    return -(-v // ALIGN) * ALIGN


@pytest.mark.parametrize("states", [4, 20])
@pytest.mark.parametrize("dtype,es", [("float32", 4), ("float64", 8)])
@pytest.mark.parametrize("nops,ntips,npmats,n,group", [(1, 2, 1, 1, 1), (23, 24, 23, 65, 5), (15, 16, 15, 130, 12),
                                                      (63, 64, 63, 10000, 32), (11, 12, 11, 257, 32), (3, 0, 7, 0, 4)])
def test_workspace_query_is_the_formula(states, dtype, es, nops, ntips, npmats, n, group):
    import numpy as np

    import plfx

    vn = group * n
    want = (nops * up(vn * states * es) + (ntips + nops + 1) * up(vn) + up(2 * npmats * group * states * states * es))
    got = plfx.psr_rate_scan_workspace_gen(np.dtype(dtype), states, nops, ntips, npmats, n, group)
    assert got == want
    assert plfx.psr_rate_scan_workspace_gen(plfx.F32 if es == 4 else plfx.F64, states, nops, ntips, npmats, n,
                                            group) == want
    if states == 4:
        assert got == plfx.psr_rate_scan_workspace(np.dtype(dtype), nops, ntips, npmats, n, group)


def test_workspace_query_refusals():
    import plfx

    with pytest.raises(plfx.PlfxError) as e:
        plfx.psr_rate_scan_workspace_gen(plfx.F64, 5, 3, 4, 3, 100, 4)
    assert e.value.code == plfx.ERR_UNSUPPORTED
    for bad in (dict(dtype=2), dict(nops=-1), dict(ntips=-1), dict(npmats=-1), dict(n=-1), dict(group=0),
                dict(group=plfx.PSR_MAX_CATS + 1)):
        a = dict(dtype=plfx.F64, states=20, nops=3, ntips=4, npmats=3, n=100, group=4)
        a.update(bad)
        with pytest.raises(plfx.PlfxError) as e:
            plfx.psr_rate_scan_workspace_gen(**a)
        assert e.value.code == plfx.ERR_INVALID, bad
