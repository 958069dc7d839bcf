"""numpy restatements of plfx.h section 11 (per-site rate categories): the
node update, the root lnL, the sum table and the three edge sums.  A helper
module for tests/test_psr_ref.py (which pins it to the oracle on the CPU) and
tests/test_gpu_psr.py (which compares the GPU against it).

Every array operation below is one IEEE operation per element in the arrays'
dtype (numpy neither fuses nor reorders them), written in plf()'s order: ump
from +0.0 over ascending l, the product, x3 from +0.0 over ascending k."""
import numpy as np

LOG_MINLIK = -22.18070977791824990137  # log(2^-32)


def clamp(cat, ncat):
    """The category a site uses: min(rate_cat, ncat - 1)."""
    return np.minimum(np.asarray(cat).astype(np.int64), ncat - 1)


def expand_tips(codes, dtype, tipvec=None):
    """The dense PSR CLV (n * 4 values) of a coded child: tipvec[(code & 15)*4 + s],
    tipvec None = the 0/1 indicator, bit s of the code."""
    tv = (np.array([[(c >> s) & 1 for s in range(4)] for c in range(16)], dtype) if tipvec is None
          else np.asarray(tipvec, dtype).reshape(16, 4))
    return np.ascontiguousarray(tv[np.asarray(codes) & 15].reshape(-1))


def node(x1, x2, EV, left, right, cat, ncat, wgt=None):
    """(x3, scaler bytes, weighted scaler sum) of one PSR node."""
    dt = x1.dtype
    assert x2.dtype == dt and EV.dtype == dt and left.dtype == dt and right.dtype == dt
    n = np.asarray(cat).size
    c = clamp(cat, ncat)
    L, R = left.reshape(ncat, 4, 4)[c], right.reshape(ncat, 4, 4)[c]  # [site][k][l]
    a, b = x1.reshape(n, 4), x2.reshape(n, 4)
    E = EV.reshape(4, 4)
    with np.errstate(all="ignore"):
        u1, u2 = np.zeros((n, 4), dt), np.zeros((n, 4), dt)
        for l in range(4):
            u1 = u1 + a[:, None, l] * L[:, :, l]
            u2 = u2 + b[:, None, l] * R[:, :, l]
        p = u1 * u2
        o = np.zeros((n, 4), dt)
        for k in range(4):
            o = o + p[:, k, None] * E[None, k, :]
        sc = np.all(np.abs(o) < dt.type(2.0 ** -32), axis=1)  # strict: NaN never scales
        o[sc] = o[sc] * dt.type(2.0 ** 32)
    w = np.ones(n, np.int64) if wgt is None else np.asarray(wgt).astype(np.int64)
    return np.ascontiguousarray(o.reshape(-1)), sc.astype(np.uint8), int(w[sc].sum())


def root_lnl(x, n, freq=None, wgt=None, scaler_sums=None):
    """(lnL, log L per site): sum_i wgt_i log(sum_s freq[s] x[i][s]) + sum(scaler_sums) log(2^-32)."""
    fr = np.full(4, 0.25) if freq is None else np.asarray(freq, np.float64)
    v = x.reshape(n, 4).astype(np.float64)
    L = np.zeros(n)
    for s in range(4):
        L = L + fr[s] * v[:, s]
    with np.errstate(all="ignore"):
        site = np.log(L)
    w = np.ones(n) if wgt is None else np.asarray(wgt, np.float64)
    nsc = 0 if scaler_sums is None else int(np.asarray(scaler_sums).sum())
    return float(np.sum(w * site) + nsc * LOG_MINLIK), site


def sumtab(x1, x2):
    assert x1.dtype == x2.dtype
    return x1 * x2  # one multiply, rounded in the dtype


def edge(st, lam, rates, cat, t, wgt=None, nsc=0):
    """out3 = (lnL, d1, d2), the scales of its tolerances as
    tests/test_gpu_edge.py's ref_edge gives them, and log L per site."""
    ncat = len(rates)
    n = np.asarray(cat).size
    st = st.reshape(n, 4).astype(np.float64)
    w = np.ones(n) if wgt is None else np.asarray(wgt, np.float64)
    x = np.asarray(rates, np.float64)[clamp(cat, ncat)][:, None] * np.asarray(lam, np.float64)[None, :4]
    e = np.exp(x * t)
    e1 = e * x
    e2 = e1 * x
    L, L1, L2 = ((st * f).sum(axis=1) for f in (e, e1, e2))
    r1, r2 = L1 / L, L2 / L
    out = np.array([np.sum(w * np.log(L)) + nsc * LOG_MINLIK, np.sum(w * r1), np.sum(w * (r2 - r1 * r1))])
    scale = np.array([abs(out[0]), np.sum(np.abs(w) * np.abs(r1)), np.sum(np.abs(w) * (np.abs(r2) + r1 * r1))])
    return out, scale, np.log(L)
