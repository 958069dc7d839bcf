"""The reference of plfx.h section 11d, the protein per-site-rate node in FMA
mode: oracle.plf_generic(20, 1, ..., fma=True) -- plf()'s loop with one
category and every multiply-add fused -- applied to the sites of each clamped
category with that category's matrices.  A helper module for
tests/test_psr_prot_fma_abi.py (which shows on the CPU that it is a different
function from the exact restatement tests/psr_prot_ref.py, in bits, and the
same likelihood) and tests/test_gpu_psr_prot_fma.py (which compares the GPU
against it bit for bit)."""
import numpy as np

import psr_prot_ref as R

S = R.S


def node_fma(x1, x2, EV, left, right, cat, ncat, wgt=None):
    """(x3, scaler bytes, weighted scaler sum) of one protein PSR node in FMA
    mode.  f64; the sum is taken from the scaler bytes."""
    import oracle as O

    dt = x1.dtype
    assert dt == np.float64 and x2.dtype == dt and EV.dtype == dt and left.dtype == dt and right.dtype == dt
    n = np.asarray(cat).size
    c = R.clamp(cat, ncat)
    a, b = x1.reshape(n, S), x2.reshape(n, S)
    L, Rm = left.reshape(ncat, S * S), right.reshape(ncat, S * S)
    E = np.ascontiguousarray(EV.reshape(-1))
    x3 = np.empty((n, S), dt)
    sc = np.empty(n, np.uint8)
    for k in np.unique(c):
        m = c == k
        o, s, _ = O.plf_generic(S, 1, np.ascontiguousarray(a[m].reshape(-1)), np.ascontiguousarray(b[m].reshape(-1)), E,
                                np.ascontiguousarray(L[k]), np.ascontiguousarray(Rm[k]), fma=True)
        x3[m] = o.reshape(-1, S)
        sc[m] = s
    w = np.ones(n, np.int64) if wgt is None else np.asarray(wgt).astype(np.int64)
    return np.ascontiguousarray(x3.reshape(-1)), sc, int(w[sc != 0].sum())
