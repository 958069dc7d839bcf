"""The near-threshold cases of oracle/scale_cases.py on the oracle alone: the
conditions that keep tests/test_gpu_scale_decision.py from passing vacuously
(the construction is exact, every position meets every lane in both decisions,
every tile and every tree level holds both), and the same cases through the
sw_emu target, whose 2^-32 decision is a loop of its own (csrc/swemu.cpp)."""
import numpy as np
import pytest

import scale_cases as SC

DTYPES = [np.float32, np.float64]
SHIFTS = range(6)


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(got, exp):
    """Bit equality, NaN by position."""
    nan = np.isnan(exp)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(exp[~nan]))


def one_hot(x3, V, dtype):
    """Per site: the position of the only value at or above 2^-32 in magnitude
    when that value is +-2^-32 exactly and nothing is NaN, else -1."""
    thr = SC.consts(dtype)[0]
    a = np.abs(x3.reshape(-1, V))
    big = a >= thr
    ok = (big.sum(axis=1) == 1) & ~np.isnan(a).any(axis=1) & (a.max(axis=1) == thr)
    return np.where(ok, big.argmax(axis=1), -1)


@pytest.mark.parametrize("S", [4, 20])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("carrier", ["x1", "x2"])
def test_placed_cases_are_exact(oracle, S, dtype, carrier):
    """plf()'s parent is the placed pattern bit for bit, in the exact loop and
    in the fused chains, scaled exactly where the kind says."""
    for shift in SHIFTS:
        for n in (None, SC.TAIL):
            c = SC.placed_case(S, dtype, n, shift, carrier)
            e3, esc = SC.expected_parent(S, c["placed"], c["hot"], c["kind"])
            einc = int((esc.astype(np.int64) * c["wgt"]).sum())
            runs = [SC.run_oracle(c, False), SC.run_oracle(c, True)]
            if S == 4:
                a = [c[k] for k in ("x1", "x2", "EV", "left", "right", "wgt")]
                runs += [oracle.plf_generic(4, 4, *a), oracle.plf_generic(4, 4, *a, fma=True)]
            for x3, sc, inc in runs:
                assert same(x3, e3) and np.array_equal(sc, esc) and inc == einc
            thr, below, sub = SC.consts(dtype)
            assert below < thr and float(below) * 2 > float(thr) and 0 < float(sub) < np.finfo(dtype).tiny


@pytest.mark.parametrize("S", [4, 20])
@pytest.mark.parametrize("dtype", DTYPES)
def test_placed_cases_cross_positions_and_lanes(oracle, S, dtype):
    """Over the shifts, every (position, site-in-tile) pair has an unscaled
    site whose only value at or above the threshold is there and a scaled site
    whose hot value is there; every 64-site tile of every shift holds both
    decisions; the six kinds all occur."""
    V, T = 4 * S, SC.tile(S)
    unscaled = np.zeros((V, T), bool)
    scaled = np.zeros((V, T), bool)
    for shift in SHIFTS:
        c = SC.placed_case(S, dtype, None, shift)
        n = c["n"]
        x3, sc, _ = SC.run_oracle(c)
        pos = one_hot(x3, V, dtype)
        lane = np.arange(n) % T
        m = (sc == 0) & (pos >= 0)
        assert np.array_equal(pos[m], c["hot"][m])
        unscaled[pos[m], lane[m]] = True
        scaled[c["hot"][sc == 1], lane[sc == 1]] = True
        for t in range(0, n, 64):
            assert 0 < sc[t:t + 64].sum() < len(sc[t:t + 64]), (shift, t)
        assert sorted(set(c["kind"].tolist())) == list(range(6))
        tail = SC.placed_case(S, dtype, SC.TAIL, shift)
        assert 0 < SC.run_oracle(tail)[1].sum() < SC.TAIL
    assert unscaled.all() and scaled.all()


@pytest.mark.parametrize("S", [4, 20])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fma", [False, True])
def test_random_family_is_near_the_threshold(oracle, S, dtype, fma):
    """Between a quarter and three quarters of the sites scale, and at least
    80 % have their largest magnitude within 2^-7 relative of 2^-32."""
    c = SC.random_case(S, dtype, 1024 + SC.TAIL, 5, fma)
    x3, sc, _ = SC.run_oracle(c, fma)
    assert 0.25 <= sc.mean() <= 0.75
    top = np.abs(x3.astype(np.float64)).reshape(c["n"], -1).max(axis=1)
    top = np.where(sc == 1, top / SC.TWO32, top)
    assert (np.abs(top * SC.TWO32 - 1) <= 2.0 ** -7).mean() >= 0.8


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiptip_table_coverage(oracle, dtype):
    """What the DNA tip/tip table case reaches: a table row is shared by the
    four categories, so one value decides alone only in the category whose
    matrix factor is 1.  Over the four hot categories all 16 (category, state)
    positions decide alone in an unscaled site (kinds `at` and `neg`, rows
    0..7); the scaling kinds (`under`, `negunder`, `zero`) cannot be given a
    position -- every value of such a site is below the threshold in every
    category -- and the sites of kind `nan` read rows far from the
    threshold (2, 2^-31, all zeros) instead.  Every 64-site tile holds both
    decisions."""
    seen = np.zeros(16, bool)
    for hotcat in range(4):
        for shift in SHIFTS:
            c = SC.tiptip_case(dtype, 4096 + SC.TAIL, shift, hotcat)
            x3, sc, _ = SC.run_oracle(c)
            pos = one_hot(x3, 16, dtype)
            m = (sc == 0) & (pos >= 0)
            assert (pos[m] // 4 == hotcat).all() and m.sum() > 0
            seen[pos[m]] = True
            far = c["kind"] == SC.NAN           # rows 12..14 instead: 2, 2^-31 and all zeros
            assert np.array_equal(sc == 1, np.isin(c["kind"], (SC.UNDER, SC.NEGUNDER, SC.ZERO))
                                  | (far & (np.arange(c["n"]) % 3 == 2)))
            for t in range(0, c["n"], 64):
                assert 0 < sc[t:t + 64].sum() < len(sc[t:t + 64])
    assert seen.all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_protein_table_coverage(oracle, dtype):
    """Protein both-coded node through a caller table: over shifts 0..3 (the
    hot category) every one of the 80 positions decides alone in an unscaled
    site, in both exact and fused mode; every tile holds both decisions."""
    seen = np.zeros(80, bool)
    for shift in SHIFTS:
        c = SC.protein_table_case(dtype, 5120 + SC.TAIL, shift)
        for fma in (False, True):
            x3, sc, _ = SC.run_oracle(c, fma)
            pos = one_hot(x3, 80, dtype)
            m = (sc == 0) & (pos >= 0)
            assert (pos[m] // 20 == c["hotcat"]).all()
            seen[pos[m]] = True
            for t in range(0, c["n"], 64):
                assert 0 < sc[t:t + 64].sum() < len(sc[t:t + 64])
    assert seen.all()


def _level_coverage(case, dtype, fma=False):
    """Per level: (sites that scale, sites that do not, positions deciding alone)
    over the ops of that level, from the oracle's traversal."""
    V = 4 * case["S"]
    host, sums, scal = SC.run_tree_oracle(case, fma)
    ntips = len(case["tips"])
    out = {}
    for j, lv in enumerate(SC.tree_levels(ntips)):
        pos = one_hot(host[case["ops"][j, 0]], V, dtype)
        s, u, seen = out.setdefault(int(lv), [0, 0, np.zeros(V, bool)])
        seen[pos[(scal[j] == 0) & (pos >= 0)]] = True
        out[int(lv)][0] = s + int(scal[j].sum())
        out[int(lv)][1] = u + int(((scal[j] == 0) & (pos >= 0)).sum())
    assert sums.tolist() == [int((sc.astype(np.int64) * case["wgt"]).sum()) for sc in scal]
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ntips", [8, 16, 32, 64])
def test_dna_tree_cases_decide_at_every_level(oracle, dtype, ntips):
    """Every level of every tree scales some sites, leaves others unscaled
    with one value at +-2^-32 deciding alone, and that value visits all 16
    positions at some op of the level."""
    cov = _level_coverage(SC.tree_case(4, dtype, ntips, 4096 + SC.TAIL, ntips % 6), dtype)
    assert sorted(cov) == list(range(1, ntips.bit_length()))
    for lv, (s, u, seen) in cov.items():
        assert s > 0 and u > 0 and seen.all(), (lv, s, u, np.flatnonzero(~seen))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fma", [False, True])
def test_protein_tree_cases_decide_at_every_level(oracle, dtype, fma):
    """The 8-taxon protein tree with dense leaves: all 80 positions at every
    level.  With coded leaves and a caller table, levels 2 and 3 decide (level
    1 is far above the threshold but for the zero row): over the shifts all 80
    parent positions decide alone at both levels (the table has 19 pattern
    rows -- row 19 holds the 2^-16 leaf -- but the ops' different permutations
    carry them to every state)."""
    cov = _level_coverage(SC.tree_case(20, dtype, 8, 5120 + SC.TAIL, 1), dtype, fma)
    for lv, (s, u, seen) in cov.items():
        assert s > 0 and u > 0 and seen.all(), (lv, s, u, np.flatnonzero(~seen))
    seen = {2: np.zeros(80, bool), 3: np.zeros(80, bool)}
    for shift in SHIFTS:
        cov = _level_coverage(SC.protein_coded_tree_case(dtype, 5120 + SC.TAIL, shift), dtype, fma)
        for lv in (2, 3):
            s, u, pos = cov[lv]
            assert s > 0 and u > 0
            seen[lv] |= pos
    for lv in (2, 3):
        assert seen[lv].all(), (lv, np.flatnonzero(~seen[lv]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W,layout,aie", [(8192, 0, 1), (1024, 1, 1), (0, 0, 0)])
def test_swemu_scale_decision(oracle, dtype, W, layout, aie):
    """The DNA placed cases through the emulated accelerator instance (WINDOW
    combined / separate and STREAM): CLV bits, scaler bytes and the weighted
    sum equal plf()'s, nothing stored past the last site."""
    import plfx

    for n, shift in [(None, s) for s in SHIFTS] + [(SC.TAIL, 0)]:
        c = SC.placed_case(4, dtype, n, shift)
        n = c["n"]
        e3, esc, einc = SC.run_oracle(c)
        tb = plfx.Testbench(n, 1, W or 1024, layout, aie)
        L, R = tb.pack_instance(0, c["EV"], c["left"], c["right"], c["x1"], c["x2"])
        x3 = np.full(16 * n + 32, -3.0, dtype)
        sc = np.full(n + 8, 0xAB, np.uint8)
        plfx.swemu_instance_run(L, R, x3, sc, n, W, layout, aie)
        assert same(x3[:16 * n], e3) and np.array_equal(sc[:n], esc)
        assert int((sc[:n].astype(np.int64) * c["wgt"]).sum()) == einc
        assert (x3[16 * n:] == -3.0).all() and (sc[n:] == 0xAB).all()
