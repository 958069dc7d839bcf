"""CPU tests of plfx.h section 11b (protein per-site rate categories):

* tests/psr_prot_ref.py, the numpy restatement the GPU tests compare against,
  pinned bit for bit to the oracle: a per-site-rate node is plf()'s loop with
  one category (oracle.plf_generic(20, 1, ...)), run on each category's sites
  with that category's matrices -- values, scaler bytes and weighted sums, in
  f32 and f64;
* plfx_psr_site_order: stability, the clamp, n = 0, refusals;
* the ABI: the header declares the four new functions, the binding lists and
  resolves them, and libplfx_psr_prot.so holds the gfx950 kernels.

No GPU work."""
import ctypes as C
import re

import numpy as np
import pytest

import psr_prot_ref as R
from conftest import PKG, ROOT

HEADER = ROOT / "include" / "plfx.h"
PROT_LIB = PKG / "plfx" / "libplfx_psr_prot.so"
NAMES = ("plfx_plf_psr_dev_gen", "plfx_traverse_psr_gen", "plfx_root_lnl_psr_gen", "plfx_psr_site_order")
S = 20


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def case(dtype, n=131, ncat=7, seed=3):
    rng = np.random.default_rng(seed)
    d = dict(x1=rng.random(S * n), x2=rng.random(S * n), EV=rng.random(S * S) - 0.25,
             left=rng.random(S * S * ncat), right=rng.random(S * S * ncat))
    d["x1"].reshape(n, S)[::4] *= 1e-14  # every fourth site rescales (x3 is of the order of 100 otherwise)
    d = {k: v.astype(dtype) for k, v in d.items()}
    d.update(cat=rng.integers(0, ncat, n).astype(np.uint8), wgt=rng.integers(1, 6, n).astype(np.int32), n=n,
             ncat=ncat)
    return d


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_node_is_the_oracle_per_category(oracle, dtype):
    d = case(dtype)
    n, ncat, cat = d["n"], d["ncat"], d["cat"]
    x3, sc, inc = R.node(d["x1"], d["x2"], d["EV"], d["left"], d["right"], cat, ncat, d["wgt"])
    assert x3.dtype == dtype and sc.sum() == -(-n // 4)  # the sites that carry the factor, and no other
    e3, esc, einc = np.empty_like(x3), np.empty_like(sc), 0
    for c in range(ncat):
        idx = np.flatnonzero(cat == c)
        assert idx.size
        sub = lambda a: np.ascontiguousarray(a.reshape(n, S)[idx].reshape(-1))  # noqa: E731
        o3, osc, oinc = oracle.plf_generic(S, 1, sub(d["x1"]), sub(d["x2"]), d["EV"],
                                           np.ascontiguousarray(d["left"][400 * c:400 * c + 400]),
                                           np.ascontiguousarray(d["right"][400 * c:400 * c + 400]), d["wgt"][idx])
        e3.reshape(n, S)[idx] = o3.reshape(-1, S)
        esc[idx] = osc
        einc += oinc
    assert np.array_equal(bits(x3), bits(e3))
    assert np.array_equal(sc, esc)
    assert inc == einc


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_signed_zero_products_start_from_plus_zero(oracle, dtype):
    """Negative values against zero matrix entries: every chain starts from
    +0.0, so a sum of -0.0 products is +0.0, as in the oracle."""
    n = 8
    x1 = -np.ones(S * n, dtype)
    x2 = np.ones(S * n, dtype)
    left = np.zeros(S * S, dtype)
    left[::S + 1] = 1  # the identity
    left[0] = 0        # row 0: twenty products of -0.0
    right = np.ascontiguousarray(np.eye(S, dtype=dtype).reshape(-1))
    EV = np.ascontiguousarray(np.eye(S, dtype=dtype).reshape(-1))
    cat = np.zeros(n, np.uint8)
    x3, sc, inc = R.node(x1, x2, EV, left, right, cat, 1)
    o3, osc, oinc = oracle.plf_generic(S, 1, x1, x2, EV, left, right)
    assert np.array_equal(bits(x3), bits(o3)) and np.array_equal(sc, osc) and inc == oinc
    assert not np.signbit(x3.reshape(n, S)[:, 0]).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_clamp_and_coded_children(oracle, dtype):
    """Categories >= ncat are ncat - 1; a coded child is its expansion."""
    d = case(dtype, n=65, ncat=4)
    hi = d["cat"].copy()
    hi[d["cat"] == 3] = np.array([4, 31, 200, 255] * 17, np.uint8)[:np.count_nonzero(d["cat"] == 3)]
    a = R.node(d["x1"], d["x2"], d["EV"], d["left"], d["right"], d["cat"], 4, d["wgt"])
    b = R.node(d["x1"], d["x2"], d["EV"], d["left"], d["right"], hi, 4, d["wgt"])
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    codes = np.arange(65, dtype=np.uint8) * 4  # every row, then 24.. and 255 -> row 23
    codes[-1] = 255
    tv = np.random.default_rng(1).random((24, S)).astype(dtype)
    for table in (None, tv):
        assert np.array_equal(R.expand_tips(codes, dtype, table).reshape(65, S),
                              oracle.expand_protein_tips(codes, dtype, Ccat=1, tipvec=table).reshape(65, S))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_root_lnl_is_the_oracle_with_one_category(oracle, dtype):
    d = case(dtype)
    n = d["n"]
    freq = np.random.default_rng(2).dirichlet(np.ones(S))
    sums = np.array([3, 0, 5], np.int64)
    for kw in (dict(), dict(freq=freq, wgt=d["wgt"], scaler_sums=sums)):
        got, site = R.root_lnl(d["x2"], n, **kw)
        ref, ref_site = oracle.root_lnl(S, 1, d["x2"], n, catw=np.ones(1), site=True, **kw)
        # the same sums; numpy's log and its pairwise summation may differ from libm's and a
        # sequential loop in the last bits
        assert np.all(np.abs(site - ref_site) <= 4 * np.spacing(np.abs(ref_site)))
        assert abs(got - ref) <= 1e-13 * abs(ref)


# ---- plfx_psr_site_order ----

def test_site_order_is_a_stable_sort_by_clamped_category():
    import plfx

    rng = np.random.default_rng(4)
    for n, ncat in ((1, 1), (257, 25), (1000, 32), (1000, 3)):
        cat = rng.integers(0, 40, n).astype(np.uint8)  # bytes >= ncat among them
        if n >= 4:
            cat[:4] = [ncat, 200, 255, ncat - 1]
        perm = plfx.psr_site_order(cat, ncat)
        assert perm.dtype == np.int64 and perm.shape == (n,)
        assert np.array_equal(np.sort(perm), np.arange(n))  # a permutation
        c = R.clamp(cat, ncat)
        assert np.all(np.diff(c[perm]) >= 0)  # the clamped categories are non-decreasing
        assert np.array_equal(perm, np.argsort(c, kind="stable"))  # sites of one category keep their order


def test_site_order_of_no_sites_and_refusals():
    import plfx

    assert plfx.psr_site_order(np.zeros(0, np.uint8), 5).size == 0
    L = plfx.load()
    cat = np.zeros(4, np.uint8)
    perm = np.full(4, -7, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for args in ((None, 4, 2, p(perm)), (p(cat), 4, 2, None), (p(cat), -1, 2, p(perm)), (p(cat), 4, 0, p(perm)),
                 (p(cat), 4, plfx.PSR_MAX_CATS + 1, p(perm))):
        assert L.plfx_psr_site_order(*args) == plfx.ERR_INVALID, args
    assert np.all(perm == -7)  # a refused call writes nothing
    assert L.plfx_psr_site_order(p(cat), 4, plfx.PSR_MAX_CATS, p(perm)) == plfx.OK
    assert np.array_equal(perm, np.arange(4))
    for bad in (0, plfx.PSR_MAX_CATS + 1):
        with pytest.raises(plfx.PlfxError) as e:
            plfx.psr_site_order(cat, bad)
        assert e.value.code == plfx.ERR_INVALID
    with pytest.raises(plfx.PlfxError):
        plfx.psr_site_order(np.zeros(4, np.int32), 2)


# ---- the ABI ----

def test_header_declares_the_new_functions():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    # the state count follows dtype in the three device entry points
    for name in NAMES[:3]:
        assert re.search(name + r"\s*\(\s*plfx_ctx\s*\*\s*ctx\s*,\s*int\s+dtype\s*,\s*int\s+states\s*,", text), name


def test_binding_lists_and_resolves_them():
    import plfx

    L = plfx.load()
    for name in NAMES:
        assert name in plfx.EXPORTS
        assert getattr(L, name).argtypes
    for m in ("plf_psr_gen", "traverse_psr_gen", "root_lnl_psr_gen"):
        assert callable(getattr(plfx.Context, m))


def test_protein_psr_code_object_holds_the_kernels():
    from plfx import codeobj

    assert PROT_LIB.exists(), "run __graft_entry__.build() first"
    node = codeobj.kernel_instantiations(PROT_LIB, "plf_psr_prot_kernel")
    # plf_psr_prot_kernel<T, kSum, T1, T2>: {f, d} x {Lb0, Lb1}^3
    got = {s.split("plf_psr_prot_kernelI")[1][:13] for s in node}
    want = {t + f"Lb{a}ELb{b}ELb{c}E" for t in "fd" for a in "01" for b in "01" for c in "01"}
    assert len(node) == 16 and got == want, node
    root = codeobj.kernel_instantiations(PROT_LIB, "root_lnl_psr_prot_kernel")
    assert len(root) == 2 and {s.split("root_lnl_psr_prot_kernelI")[1][0] for s in root} == {"f", "d"}, root
