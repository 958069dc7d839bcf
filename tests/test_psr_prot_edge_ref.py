"""CPU tests of plfx.h section 11c (protein per-site rate categories, the
branch-length half):

* tests/psr_prot_edge_ref.py, the numpy restatement the GPU tests compare
  against, pinned to tests/felsenstein_ref.py (state space, expm, S = 20,
  which shares nothing with the library): lnL, d1 and d2 of the middle edge of
  a four-taxon tree with per-site rates, at LNL_RTOL of the scales;
* the ABI: the header declares the five new functions, the binding lists and
  resolves them, and libplfx_psr_prot.so holds the gfx950 kernels.

No GPU work."""
import re

import numpy as np

import felsenstein_ref as F
import psr_prot_edge_ref as E
from conftest import PKG, ROOT
from test_felsenstein_ref import eigen_sym

HEADER = ROOT / "include" / "plfx.h"
PROT_LIB = PKG / "plfx" / "libplfx_psr_prot.so"
NAMES = ("plfx_edge_sumtable_psr_gen", "plfx_edge_sumtable_psr_batch_gen", "plfx_edge_derivatives_psr_gen",
         "plfx_edge_optimize_psr_gen", "plfx_edge_optimize_psr_dev_gen")
METHODS = ("edge_sumtable_psr_gen", "edge_sumtables_psr_gen", "edge_derivatives_psr_gen", "optimize_branch_psr_gen",
           "optimize_branches_psr_gen")
S = 20
LNL_RTOL = 1e-10


def test_edge_is_the_state_space_reference_on_a_four_taxon_tree():
    """((t0, t1) A, (t2, t3) B): A and B from the reference's pruning (per-site
    maximum 1, log scales apart), taken to eigen coordinates with numpy's own
    decomposition; the restated edge over their product against the
    reference's edge between A and B."""
    n, ncat = 300, 25
    rng = np.random.default_rng(20)
    Q, pi = F.gtr_q(rng.random(S * (S - 1) // 2) * 2 + 0.05, rng.random(S) + 0.1)
    lam, _, Vi = eigen_sym(Q, pi)
    rates = np.geomspace(0.05, 4.0, ncat)
    cat = rng.integers(0, ncat + 3, n).astype(np.uint8)  # a few past ncat: clamped
    sr = F.site_rates_psr(rates, cat)
    wgt = rng.integers(0, 4, n).astype(np.int32)
    tips = {s: np.eye(S)[rng.integers(0, S, n)] for s in range(4)}
    for x in tips.values():
        x[rng.random(n) < 0.05] = 1.0  # a few gaps
    clv = F.prune(Q, [(4, 0, 1, 0), (5, 2, 3, 1)], rng.random(4) * 0.25 + 0.05, tips, sr)
    (A, la), (B, lb) = clv[4], clv[5]
    a, b = A[:, 0, :] @ Vi.T, B[:, 0, :] @ Vi.T
    st = E.sumtab(a, b)
    for t in (1e-8, 0.2, 1.5, 10.0):
        ref, scale, ref_site = F.edge(A, la, B, lb, Q, pi, sr, None, t, wgt)
        got, _, site = E.edge(st, lam, rates, cat, t, wgt)
        got[0] += np.sum(wgt * (la + lb))
        for j, name in enumerate(("lnL", "d1", "d2")):
            err = abs(got[j] - ref[j])
            print(f"t={t} {name}: restated {got[j]!r} reference {ref[j]!r} err/scale {err / scale[j]:.2e}")
            assert err <= LNL_RTOL * scale[j], (t, name)
        assert np.all(np.abs(site + la + lb - ref_site) <= LNL_RTOL * np.maximum(1.0, np.abs(ref_site)))


def test_edge_reads_twenty_eigenvalues_and_clamps_the_category():
    rng = np.random.default_rng(3)
    n = 9
    st = rng.random((n, S)) + 0.1
    lam = -rng.random(S + 5)
    rates = np.array([0.5, 2.0])
    cat = np.array([0, 1, 2, 255, 1, 0, 7, 1, 0], np.uint8)
    a = E.edge(st, lam, rates, cat, 0.3)
    b = E.edge(st.ravel(), lam[:S], rates, np.minimum(cat, 1), 0.3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    L = (st * np.exp(np.outer(rates[np.minimum(cat, 1)], lam[:S]) * 0.3)).sum(axis=1)
    assert np.allclose(a[2], np.log(L), rtol=1e-14) and np.isclose(a[0][0], np.log(L).sum(), rtol=1e-14)


# ---- the ABI ----

def test_header_declares_the_five_functions():
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:  # the state count follows dtype
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*plfx_ctx\s*\*\s*ctx\s*,\s*int\s+dtype\s*,\s*int\s+states\s*,",
                         text), name
    assert "(11c)" in raw
    flat = " ".join(raw.replace("*", " ").split())
    assert "branch-length half (the protein versions of plfx_edge_ _psr and" not in flat  # 11b: only the scan is missing
    assert "rate scan does not exist yet" in flat


def test_binding_lists_and_resolves_them():
    import plfx

    L = plfx.load()
    for name in NAMES:
        assert name in plfx.EXPORTS
        assert getattr(L, name).argtypes
    for m in METHODS:
        assert callable(getattr(plfx.Context, m))


def test_protein_psr_code_object_holds_the_edge_kernels():
    from plfx import codeobj

    assert PROT_LIB.exists(), "run __graft_entry__.build() first"
    for kernel in ("edge_deriv_psr_prot_kernel", "edge_opt_psr_prot_kernel"):  # <T>
        got = codeobj.kernel_instantiations(PROT_LIB, kernel)
        assert len(got) == 2 and {s.split(kernel + "I")[1][0] for s in got} == {"f", "d"}, got
    for kernel in ("edge_sumtable_psr_prot_kernel", "edge_sumtable_psr_prot_batch_kernel"):  # <T, kTip>
        got = codeobj.kernel_instantiations(PROT_LIB, kernel)
        assert len(got) == 4 and {s.split(kernel + "I")[1][:4] for s in got} == {"fLb0", "fLb1", "dLb0", "dLb1"}, got
