"""CPU checks of the two batched per-site-rate edge entry points
(plfx_edge_optimize_psr_dev, plfx_edge_sumtable_psr_batch): the header declares
them, the Python binding lists them and they resolve from the loaded library,
and libplfx_psr.so's gfx950 code object holds their kernels.  No GPU work."""
import re

from conftest import PKG, ROOT

HEADER = ROOT / "include" / "plfx.h"
PSR_LIB = PKG / "plfx" / "libplfx_psr.so"
NAMES = ("plfx_edge_optimize_psr_dev", "plfx_edge_sumtable_psr_batch")


def test_header_declares_both():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert re.search(r"\}\s*plfx_psr_edge\s*;", text)
    assert "There is no device-resident PSR loop" not in HEADER.read_text()


def test_binding_lists_and_resolves_both():
    import ctypes as C

    import plfx

    L = plfx.load()
    for name in NAMES:
        assert name in plfx.EXPORTS
        assert getattr(L, name).argtypes
    assert C.sizeof(plfx.PsrEdge) == 4 * C.sizeof(C.c_void_p)
    assert [f[0] for f in plfx.PsrEdge._fields_] == ["tip1", "x1", "x2", "sumtab"]


def test_psr_code_object_holds_the_new_kernels():
    from plfx import codeobj

    loop = codeobj.kernel_instantiations(PSR_LIB, "edge_opt_psr_kernel")
    # edge_opt_psr_kernel<T, U>: "If" / "Id" open the template arguments
    assert len(loop) == 2 and {s.split("edge_opt_psr_kernelI")[1][0] for s in loop} == {"f", "d"}, loop
    batch = codeobj.kernel_instantiations(PSR_LIB, "edge_sumtable_psr_batch_kernel")
    # <T, kTip>: {f, d} x {Lb0, Lb1}
    got = {s.split("edge_sumtable_psr_batch_kernelI")[1][:4] for s in batch}
    assert len(batch) == 4 and got == {"fLb0", "fLb1", "dLb0", "dLb1"}, batch
    # the one-edge kernels are still there
    assert len(codeobj.kernel_instantiations(PSR_LIB, "edge_sumtable_psr_kernel")) == 4
    assert len(codeobj.kernel_instantiations(PSR_LIB, "edge_deriv_psr_kernel")) == 2
