"""CPU checks of plfx.h section 11d, PROTCAT FMA mode (plfx_plf_psr_dev_ex,
plfx_traverse_psr_ex, plfx_psr_rate_scan_ex): the header declares them with
`flags` after `states`, the Python binding lists and resolves them with one
more argument than their _gen bases, the Context methods take `fma`, the new
library's gfx950 code object holds the eight f64 instantiations of
plf_psr_prot_mfma_kernel and the other per-site-rate libraries none, the
flags do not change what a call lowers to (tests/psr_prot_fma_lower_main.cpp
under ASan + UBSan), and the reference tests/psr_prot_fma_ref.py is a
different function from the exact restatement in bits and the same likelihood
-- on the inputs tests/test_gpu_psr_prot_fma.py uses, so that its assertions
are assertions about the kernel.  No GPU work."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import psr_prot_fma_ref as RF
import psr_prot_ref as R
from conftest import PKG, ROOT
from test_gpu_psr_prot import LNL_RTOL, S, make_node, tree_problem
from test_sanitizers import SAN

HEADER = ROOT / "include" / "plfx.h"
CSRC = PKG / "csrc"
MFMA_LIB = PKG / "plfx" / "libplfx_psr_prot_mfma.so"
NAMES = ("plfx_plf_psr_dev_ex", "plfx_traverse_psr_ex", "plfx_psr_rate_scan_ex")
KERNEL = "plf_psr_prot_mfma_kernel"


def test_header_declares_the_three_functions():
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:  # flags follows the state count
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*plfx_ctx\s*\*\s*ctx\s*,\s*int\s+dtype\s*,\s*int\s+states\s*,"
                         r"\s*int\s+flags\s*,", text), name
        # and the rest is the _gen namesake's argument list
        gen = re.search(r"\bint\s+" + name[:-len("_ex")] + r"_gen\s*\(([^)]*)\)", text).group(1)
        ex = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text).group(1)
        flat = lambda s: " ".join(s.split())  # noqa: E731
        assert flat(ex) == flat(gen).replace("int states,", "int states, int flags,", 1), name
    assert "(11d)" in raw
    assert re.search(r"#define\s+PLFX_VERSION\s+10300\b", raw)


def test_binding_lists_and_resolves_them():
    import plfx

    L = plfx.load()
    for name in NAMES:
        assert name in plfx.EXPORTS
        fn, base = getattr(L, name), getattr(L, name[:-len("_ex")] + "_gen")
        assert fn.argtypes and len(fn.argtypes) == len(base.argtypes) + 1
        assert list(fn.argtypes[:3]) == list(base.argtypes[:3]) and fn.argtypes[3] is plfx.C.c_int
        assert list(fn.argtypes[4:]) == list(base.argtypes[3:])
    for m in ("plf_psr_gen", "traverse_psr_gen", "psr_rate_scan_gen"):
        p = inspect.signature(getattr(plfx.Context, m)).parameters
        assert "fma" in p and p["fma"].default is False, m


def test_new_library_holds_the_eight_kernels_and_the_others_none():
    from plfx import codeobj

    assert MFMA_LIB.exists(), "run __graft_entry__.build() first"
    got = codeobj.kernel_instantiations(MFMA_LIB, KERNEL)
    # <kSum, T1, T2>: three bools and no element type -- f64 alone
    want = {f"ILb{a}ELb{b}ELb{c}EE" for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    assert len(got) == 8 and {s.split(KERNEL)[1][:len("ILb0ELb0ELb0EE")] for s in got} == want, got
    for lib in ("libplfx_psr_prot.so", "libplfx_psr.so", "libplfx_edge.so"):
        assert codeobj.kernel_instantiations(PKG / "plfx" / lib, KERNEL) == [], lib
    # the exact node's kernels are where they were
    assert len(codeobj.kernel_instantiations(PKG / "plfx" / "libplfx_psr_prot.so", "plf_psr_prot_kernel")) == 16


def test_flags_do_not_change_the_lowering(tmp_path):
    exe = tmp_path / "psr_prot_fma_lower_main"
    subprocess.run(["g++", "-std=c++17", *SAN, "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "psr_prot_fma_lower_main.cpp"),
                    *(str(CSRC / f) for f in ("psr_scan_lower.cpp", "psr_lower.cpp", "trav_plan.cpp")), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       # verify_asan_link_order=0: tolerate a preloaded library ahead of the ASan runtime
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0",
                                UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [(w[0], " ".join(w[1:-2])) for w in lines] == [("same", "batch"), ("same", "traversal"),
                                                           ("same", "scan full"), ("same", "scan tail")]
    assert lines[0][-2:] == ["4", "70"]  # 70 nodes of four kinds: 32 + 32 + 6 would be one kind; here 18/18/17/17
    assert all(int(w[-1]) == 7 and int(w[-2]) == 3 for w in lines[1:])  # seven ops on three levels


@pytest.mark.parametrize("kind", range(4))
def test_the_two_references_disagree_in_bits_on_the_node_inputs(oracle, kind):
    d = make_node(np.float64, 257, 25, kind)
    exact = d["ref"]
    fma = RF.node_fma(d["dense"][0], d["dense"][1], d["EV"], d["left"], d["right"], d["cat"], 25, d["wgt"])
    differ = np.mean(exact[0].view(np.uint64) != fma[0].view(np.uint64))
    rel = np.max(np.abs(exact[0] - fma[0]) / np.abs(exact[0]))
    print(f"kind {kind}: {differ:.3f} of the values differ in bits, max relative difference {rel:.2e}")
    assert differ > 0.25  # a bit-identity test tells the modes apart
    assert rel < 1e-9     # and they are the same numbers
    assert np.array_equal(exact[1], fma[1]) and exact[2] == fma[2]  # no value of these inputs sits at the threshold


def test_the_fma_reference_is_the_oracle_per_category(oracle):
    """One category: the helper is oracle.plf_generic(fma=True) itself; and a
    permutation of the sites permutes its outputs."""
    d = make_node(np.float64, 65, 25, 0)
    one = np.zeros(65, np.uint8)
    got = RF.node_fma(d["x1"], d["x2"], d["EV"], d["left"], d["right"], one, 25, d["wgt"])
    x3, sc, inc = oracle.plf_generic(S, 1, d["x1"], d["x2"], d["EV"], d["left"][:400], d["right"][:400], wgt=d["wgt"],
                                     fma=True)
    assert np.array_equal(got[0].view(np.uint64), x3.view(np.uint64)) and np.array_equal(got[1], sc) and got[2] == inc
    perm = np.random.default_rng(3).permutation(65)
    a = RF.node_fma(d["x1"], d["x2"], d["EV"], d["left"], d["right"], d["cat"], 25, d["wgt"])
    b = RF.node_fma(np.ascontiguousarray(d["x1"].reshape(65, S)[perm].reshape(-1)),
                    np.ascontiguousarray(d["x2"].reshape(65, S)[perm].reshape(-1)), d["EV"], d["left"], d["right"],
                    d["cat"][perm], 25, d["wgt"][perm])
    assert np.array_equal(a[0].reshape(65, S)[perm].view(np.uint64), b[0].reshape(65, S).view(np.uint64))
    assert np.array_equal(a[1][perm], b[1]) and a[2] == b[2]


def tree_lnl(p, node):
    """Root lnL of tree_problem p with `node` as the node function.  The
    problem's EV is signed, so a site's sum may be negative: the lnL is taken
    over |L| (the same function of the CLV for both modes)."""
    n, ncat, M = p["n"], p["ncat"], p["ncat"] * S * S
    vals = {s: R.expand_tips(c, np.float64, p["tipvec"]) for s, c in p["codes"].items()}
    sums = []
    for par, a, b, m in p["ops"]:
        vals[par], _, inc = node(vals[a], vals[b], p["EV"], p["pmats"][2 * m * M:(2 * m + 1) * M],
                                 p["pmats"][(2 * m + 1) * M:(2 * m + 2) * M], p["cat"], ncat, p["wgt"])
        sums.append(inc)
    return R.root_lnl(np.abs(vals[p["ops"][-1][0]]), n, wgt=p["wgt"], scaler_sums=np.array(sums))[0]


@pytest.mark.parametrize("name", ["balanced 8", "caterpillar 6"])
def test_the_two_references_agree_in_root_lnl_on_the_tree_problem(oracle, name):
    p = tree_problem(np.float64, name)
    exact, fma = tree_lnl(p, R.node), tree_lnl(p, RF.node_fma)
    print(f"{name}: exact {exact!r} fma {fma!r} rel {abs(exact - fma) / abs(exact):.2e}")
    assert np.isfinite(exact) and abs(exact - fma) <= LNL_RTOL * abs(exact)
