"""numpy restatements of plfx.h section 11c (protein per-site rate categories,
the branch-length half): the sum table and the three edge sums for S = 20 --
tests/psr_ref.py's sumtab and edge with 20 columns.  A helper module for
tests/test_psr_prot_edge_ref.py (which pins it to tests/felsenstein_ref.py on
the CPU) and tests/test_gpu_psr_prot_edge.py (which compares the GPU against
it)."""
import numpy as np

from psr_prot_ref import LOG_MINLIK, S, clamp


def sumtab(x1, x2):
    assert x1.dtype == x2.dtype
    return x1 * x2  # one multiply, rounded in the dtype


def edge(st, lam, rates, cat, t, wgt=None, nsc=0):
    """out3 = (lnL, d1, d2), the scales of its tolerances as
    tests/test_gpu_edge.py's ref_edge gives them, and log L per site."""
    ncat = len(rates)
    n = np.asarray(cat).size
    st = st.reshape(n, S).astype(np.float64)
    w = np.ones(n) if wgt is None else np.asarray(wgt, np.float64)
    x = np.asarray(rates, np.float64)[clamp(cat, ncat)][:, None] * np.asarray(lam, np.float64)[None, :S]
    e = np.exp(x * t)
    e1 = e * x
    e2 = e1 * x
    L, L1, L2 = ((st * f).sum(axis=1) for f in (e, e1, e2))
    with np.errstate(all="ignore"):
        r1, r2 = L1 / L, L2 / L
        site = np.log(L)
    out = np.array([np.sum(w * site) + nsc * LOG_MINLIK, np.sum(w * r1), np.sum(w * (r2 - r1 * r1))])
    scale = np.array([abs(out[0]), np.sum(np.abs(w) * np.abs(r1)), np.sum(np.abs(w) * (np.abs(r2) + r1 * r1))])
    return out, scale, site
