"""numpy restatements of plfx.h section 11b (protein per-site rate
categories): the node update and the root lnL for S = 20, as tests/psr_ref.py
restates section 11 for S = 4.  A helper module for tests/test_psr_prot_ref.py
(which pins it to the oracle on the CPU) and tests/test_gpu_psr_prot.py (which
compares the GPU against it).

Every array operation below is one IEEE operation per element in the arrays'
dtype (numpy neither fuses nor reorders them), written in plf()'s order: ump
from +0.0 over ascending l, the product, x3 from +0.0 over ascending k."""
import numpy as np

S = 20
CODES = 24  # rows of the tip table (plfx.h section 8, protein)
LOG_MINLIK = -22.18070977791824990137  # log(2^-32)


def clamp(cat, ncat):
    """The category a site uses: min(rate_cat, ncat - 1)."""
    return np.minimum(np.asarray(cat).astype(np.int64), ncat - 1)


def tip_table(dtype, tipvec=None):
    """The 24 x 20 tip table: the caller's, or the default of plfx.h section 8
    (0..19 one state, 20 = B (N|D), 21 = Z (Q|E), 22 = X and 23 = gap: all)."""
    if tipvec is not None:
        return np.asarray(tipvec, dtype).reshape(CODES, S)
    t = np.zeros((CODES, S), dtype)
    t[np.arange(S), np.arange(S)] = 1
    t[20, [2, 3]] = 1
    t[21, [5, 6]] = 1
    t[22:] = 1
    return t


def expand_tips(codes, dtype, tipvec=None):
    """The dense PSR CLV (n * 20 values) of a coded child: row min(code, 23)."""
    rows = np.minimum(np.asarray(codes, np.uint8), CODES - 1)
    return np.ascontiguousarray(tip_table(dtype, tipvec)[rows].reshape(-1))


def node(x1, x2, EV, left, right, cat, ncat, wgt=None):
    """(x3, scaler bytes, weighted scaler sum) of one protein PSR node."""
    dt = x1.dtype
    assert x2.dtype == dt and EV.dtype == dt and left.dtype == dt and right.dtype == dt
    n = np.asarray(cat).size
    c = clamp(cat, ncat)
    L, R = left.reshape(ncat, S, S)[c], right.reshape(ncat, S, S)[c]  # [site][k][l]
    a, b = x1.reshape(n, S), x2.reshape(n, S)
    E = EV.reshape(S, S)
    with np.errstate(all="ignore"):
        u1, u2 = np.zeros((n, S), dt), np.zeros((n, S), dt)
        for l in range(S):
            u1 = u1 + a[:, None, l] * L[:, :, l]
            u2 = u2 + b[:, None, l] * R[:, :, l]
        p = u1 * u2
        o = np.zeros((n, S), dt)
        for k in range(S):
            o = o + p[:, k, None] * E[None, k, :]
        sc = np.all(np.abs(o) < dt.type(2.0 ** -32), axis=1)  # strict: NaN never scales
        o[sc] = o[sc] * dt.type(2.0 ** 32)
    w = np.ones(n, np.int64) if wgt is None else np.asarray(wgt).astype(np.int64)
    return np.ascontiguousarray(o.reshape(-1)), sc.astype(np.uint8), int(w[sc].sum())


def root_lnl(x, n, freq=None, wgt=None, scaler_sums=None):
    """(lnL, log L per site): sum_i wgt_i log(sum_s freq[s] x[i][s]) + sum(scaler_sums) log(2^-32)."""
    fr = np.full(S, 1.0 / S) if freq is None else np.asarray(freq, np.float64)
    v = x.reshape(n, S).astype(np.float64)
    L = np.zeros(n)
    for s in range(S):
        L = L + fr[s] * v[:, s]
    with np.errstate(all="ignore"):
        site = np.log(L)
    w = np.ones(n) if wgt is None else np.asarray(wgt, np.float64)
    nsc = 0 if scaler_sums is None else int(np.asarray(scaler_sums).sum())
    return float(np.sum(w * site) + nsc * LOG_MINLIK), site
