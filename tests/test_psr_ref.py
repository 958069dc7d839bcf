"""tests/psr_ref.py (the numpy restatement the GPU tests of plfx.h section 11
compare against) pinned to the reference-pinned oracle, on the CPU: a
per-site-rate node is plf()'s loop with one category, run on each category's
sites with that category's matrices."""
import numpy as np
import pytest

import psr_ref


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def case(dtype, n=257, ncat=7, seed=3):
    rng = np.random.default_rng(seed)
    d = dict(x1=rng.random(4 * n), x2=rng.random(4 * n), EV=rng.random(16) - 0.25, left=rng.random(16 * ncat),
             right=rng.random(16 * ncat))
    d["x1"].reshape(n, 4)[::4] *= 1e-12  # every fourth site rescales
    d = {k: v.astype(dtype) for k, v in d.items()}
    d.update(cat=rng.integers(0, ncat, n).astype(np.uint8), wgt=rng.integers(1, 6, n).astype(np.int32), n=n,
             ncat=ncat)
    return d


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_node_is_the_oracle_per_category(oracle, dtype):
    d = case(dtype)
    n, ncat, cat = d["n"], d["ncat"], d["cat"]
    x3, sc, inc = psr_ref.node(d["x1"], d["x2"], d["EV"], d["left"], d["right"], cat, ncat, d["wgt"])
    assert x3.dtype == dtype and 60 <= sc.sum() < n  # 65 sites carry the factor; the rest must not scale
    e3, esc, einc = np.empty_like(x3), np.empty_like(sc), 0
    for c in range(ncat):
        idx = np.flatnonzero(cat == c)
        assert idx.size
        sub = lambda a: np.ascontiguousarray(a.reshape(n, 4)[idx].reshape(-1))  # noqa: E731
        o3, osc, oinc = oracle.plf_generic(4, 1, sub(d["x1"]), sub(d["x2"]), d["EV"],
                                           np.ascontiguousarray(d["left"][16 * c:16 * c + 16]),
                                           np.ascontiguousarray(d["right"][16 * c:16 * c + 16]), d["wgt"][idx])
        e3.reshape(n, 4)[idx] = o3.reshape(-1, 4)
        esc[idx] = osc
        einc += oinc
    assert np.array_equal(bits(x3), bits(e3))
    assert np.array_equal(sc, esc)
    assert inc == einc


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_clamp_and_coded_children(oracle, dtype):
    """Categories >= ncat are ncat - 1; a coded child is its expansion."""
    d = case(dtype, n=65, ncat=4)
    hi = d["cat"].copy()
    hi[d["cat"] == 3] = np.array([4, 31, 200, 255] * 17, np.uint8)[:np.count_nonzero(d["cat"] == 3)]
    a = psr_ref.node(d["x1"], d["x2"], d["EV"], d["left"], d["right"], d["cat"], 4, d["wgt"])
    b = psr_ref.node(d["x1"], d["x2"], d["EV"], d["left"], d["right"], hi, 4, d["wgt"])
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    codes = np.arange(65, dtype=np.uint8) * 7  # every nibble, junk above it
    assert np.array_equal(psr_ref.expand_tips(codes, dtype).reshape(65, 4),
                          oracle.expand_tips(codes, dtype, Ccat=1).reshape(65, 4))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_root_lnl_is_the_oracle_with_one_category(oracle, dtype):
    d = case(dtype)
    n = d["n"]
    freq = np.array([0.1, 0.2, 0.3, 0.4])
    sums = np.array([3, 0, 5], np.int64)
    for kw in (dict(), dict(freq=freq, wgt=d["wgt"], scaler_sums=sums)):
        got, site = psr_ref.root_lnl(d["x2"], n, **kw)
        ref, ref_site = oracle.root_lnl(4, 1, d["x2"], n, catw=np.ones(1), site=True, **kw)
        # the same sums; numpy's log and its pairwise summation may differ from libm's and a
        # sequential loop in the last bits
        assert np.all(np.abs(site - ref_site) <= 4 * np.spacing(np.abs(ref_site)))
        assert abs(got - ref) <= 1e-13 * abs(ref)
