"""plfx.psr_categorize (plfx_psr_categorize, csrc/model.cpp; plfx.h section 12)
on the CPU: from the rate scan's best candidate per site to rate_cat and the
normalised category rates.  Bit-equality with a numpy restatement of the rule
the header states, the properties a caller relies on, and every refusal."""
import numpy as np
import pytest

import plfx

MAX_CATS = 32


def restate(cand, idx, wgt, max_cats):
    """The header's rule, statement by statement."""
    cand, idx = np.asarray(cand, np.float64), np.asarray(idx, np.int64)
    w = np.ones(idx.size, np.int64) if wgt is None else np.asarray(wgt, np.int64)
    W = np.zeros(cand.size, np.int64)
    np.add.at(W, idx, w)
    used = sorted(set(idx.tolist()))  # a site of weight 0 counts
    kept = used if len(used) <= max_cats else sorted(used, key=lambda k: (-W[k], k))[:max_cats]
    kept = sorted(kept, key=lambda k: (cand[k], k))  # category c = kept[c]
    cat = np.empty(idx.size, np.uint8)
    for i, k in enumerate(idx):
        if k in kept:
            cat[i] = kept.index(k)
        else:
            d = [abs(cand[k] - cand[q]) for q in kept]
            cat[i] = d.index(min(d))  # the first minimum: ties to the lower category
    sw = swr = 0.0
    for i in range(idx.size):  # f64, in site order
        sw = sw + float(w[i])
        swr = swr + float(w[i]) * cand[kept[cat[i]]]
    scale = sw / swr
    return cat, np.array([cand[k] * scale for k in kept]), scale


def same(got, want):
    (c, r, s), (wc, wr, ws) = got, want
    assert c.dtype == np.uint8 and np.array_equal(c, wc)
    assert r.dtype == np.float64 and np.array_equal(r.view(np.uint64), wr.view(np.uint64))
    assert np.float64(s).view(np.uint64) == np.float64(ws).view(np.uint64)


def rand_case(seed, ncand, n, nused, zero_wgt=False):
    rng = np.random.default_rng(seed)
    cand = np.geomspace(0.05, 8.0, ncand)
    rng.shuffle(cand)  # unsorted candidates
    used = rng.choice(ncand, nused, replace=False)
    idx = np.concatenate([used, rng.choice(used, n - nused)]).astype(np.int32)
    rng.shuffle(idx)
    wgt = rng.integers(1, 5, n).astype(np.int32)
    if zero_wgt:
        wgt[rng.random(n) < 0.3] = 0
    return cand, idx, wgt


@pytest.mark.parametrize("what,nused,max_cats", [("fewer used than max_cats", 5, 8), ("as many", 8, 8),
                                                 ("more", 20, 8), ("more, one category", 20, 1),
                                                 ("the limit", 32, 32), ("past the limit", 40, 32)])
@pytest.mark.parametrize("weights", ["wgt", "no wgt", "zero weights"])
def test_equals_the_restatement(what, nused, max_cats, weights):
    cand, idx, wgt = rand_case(7 * nused + max_cats, 48, 400, nused, weights == "zero weights")
    wgt = None if weights == "no wgt" else wgt
    got = plfx.psr_categorize(cand, idx, wgt, max_cats)
    same(got, restate(cand, idx, wgt, max_cats))
    cat, rates, scale = got
    ncat = rates.size
    assert ncat == min(nused, max_cats) and cat.max() == ncat - 1
    assert np.all(np.diff(rates) > 0)  # ascending categories
    w = np.ones(idx.size) if wgt is None else wgt.astype(np.float64)
    mean = np.sum(w * rates[cat]) / np.sum(w)
    print(f"{what}, {weights}: ncat {ncat}, scale {scale!r}, weighted mean rate - 1 = {mean - 1:.2e}")
    # printed only: 400-term f64 sums round more than the 1e-15 the small cases below are held to
    if nused <= max_cats:  # nothing dropped: the identity, a site keeps its own candidate's rate
        assert np.array_equal(rates[cat], cand[idx] * scale)


@pytest.mark.parametrize("max_cats", [1, 2, 3, 5])
@pytest.mark.parametrize("seed", range(6))
def test_weighted_mean_is_one_within_1e15(seed, max_cats):
    """The weighted mean of the assigned rates, formed exactly (rationals), is 1
    within 1e-15 relative.  Seven sites: the library's sum of w * rate is n - 1
    adds and one multiply per term, each rounded to 2^-53 relative of at most
    the total, then one division and one rounding per category rate -- at most
    (n + 2) * 1.11e-16 = 1e-15 for n = 7.  More sites would need a wider bar."""
    from fractions import Fraction

    rng = np.random.default_rng(seed)
    cand = rng.permutation(np.geomspace(0.05, 8.0, 5))
    idx = np.concatenate([np.arange(5), rng.integers(0, 5, 2)]).astype(np.int32)
    wgt = rng.integers(0, 5, 7).astype(np.int32)
    wgt[0] += 1
    cat, rates, scale = plfx.psr_categorize(cand, idx, wgt, max_cats)
    assert rates.size == min(5, max_cats)
    mean = sum(Fraction(int(w)) * Fraction(float(rates[c])) for w, c in zip(wgt, cat)) / int(wgt.sum())
    print(f"seed {seed} max_cats {max_cats}: mean - 1 = {float(mean - 1):.2e}")
    assert abs(mean - 1) <= Fraction(1, 10 ** 15)


def test_weight_tie_and_distance_tie():
    """Candidates 1, 2, 3, 4, 5 (as k = 4, 2, 0, 3, 1: unsorted).  Weights: rate
    3 has 10, rates 1, 2, 4 and 5 have 4 each; max_cats = 3 keeps rate 3 and,
    of the four tied ones, the two of lowest k: k = 1 (rate 5) and k = 2 (rate
    2).  Dropped: rate 1 (k = 4) goes to rate 2; rate 4 (k = 3) is 1 away from
    both rate 3 and rate 5: the lower category, rate 3."""
    cand = np.array([3.0, 5.0, 2.0, 4.0, 1.0])
    idx = np.array([0] * 10 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4, np.int32)
    cat, rates, scale = plfx.psr_categorize(cand, idx, None, 3)
    same((cat, rates, scale), restate(cand, idx, None, 3))
    assert np.array_equal(rates / scale, [2.0, 3.0, 5.0])
    assert cat.tolist() == [1] * 10 + [2] * 4 + [0] * 4 + [1] * 4 + [0] * 4
    # equal rates: categories ordered by k, and each candidate keeps its own category
    cand = np.array([1.0, 0.5, 1.0])
    cat, rates, scale = plfx.psr_categorize(cand, np.array([2, 0, 1, 2], np.int32), None, 3)
    assert cat.tolist() == [2, 1, 0, 2] and np.array_equal(rates / scale, [0.5, 1.0, 1.0])


def test_weight_zero_sites_count_as_users():
    cand = np.array([0.5, 1.0, 2.0])
    idx = np.array([0, 1, 1, 2], np.int32)
    wgt = np.array([0, 3, 1, 0], np.int32)
    cat, rates, scale = plfx.psr_categorize(cand, idx, wgt, 3)
    assert cat.tolist() == [0, 1, 1, 2] and rates.size == 3 and scale == 1.0
    # and they are the first to go: max_cats = 2 keeps k = 1 (weight 4) and, of the two of weight 0, k = 0
    cat, rates, scale = plfx.psr_categorize(cand, idx, wgt, 2)
    same((cat, rates, scale), restate(cand, idx, wgt, 2))
    assert cat.tolist() == [0, 1, 1, 1] and np.array_equal(rates, [0.5, 1.0])


def test_refusals():
    cand, idx, wgt = np.array([0.5, 1.0, 2.0]), np.array([0, 1, 2, 1], np.int32), np.array([1, 2, 0, 1], np.int32)
    plfx.psr_categorize(cand, idx, wgt, 3)
    bad = [
        ("n < 1", (cand, idx[:0], None, 3)),
        ("max_cats 0", (cand, idx, wgt, 0)),
        ("max_cats 33", (cand, idx, wgt, MAX_CATS + 1)),
        ("no candidates", (cand[:0], idx, wgt, 3)),
        ("index past the candidates", (cand, np.array([0, 3], np.int32), None, 3)),
        ("negative index", (cand, np.array([0, -1], np.int32), None, 3)),
        ("candidate 0", (np.array([0.5, 0.0, 2.0]), idx, wgt, 3)),
        ("negative candidate", (np.array([0.5, -1.0, 2.0]), idx, wgt, 3)),
        ("candidate inf", (np.array([0.5, np.inf, 2.0]), idx, wgt, 3)),
        ("candidate nan", (np.array([0.5, np.nan, 2.0]), idx, wgt, 3)),
        ("an unused candidate that is bad", (np.array([0.5, 1.0, 2.0, -3.0]), idx, wgt, 3)),
        ("negative weight", (cand, idx, np.array([1, -1, 1, 1], np.int32), 3)),
        ("weight sum 0", (cand, idx, np.zeros(4, np.int32), 3)),
    ]
    for what, args in bad:
        with pytest.raises(plfx.PlfxError) as e:
            plfx.psr_categorize(*args)
        assert e.value.code == plfx.ERR_INVALID, what
    with pytest.raises(plfx.PlfxError):
        plfx.psr_categorize(cand, idx, wgt[:3], 3)
