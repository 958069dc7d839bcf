"""Inputs that make the 2^-32 rescale decision close -- TEST INFRASTRUCTURE ONLY.

plf() ends a site by testing whether all S*4 parent values are strictly below
2^-32 in magnitude.  The cases here put every site next to that threshold and
move the one value that decides it over every position and every lane:

* placed cases: every category's `left` / `right` and `EV` are permutation
  matrices (entries exactly 0 and 1) and `x2` is all ones, so each parent value
  is one input value carried to a known position -- products with 0 and 1 and
  sums with 0 are exact, in plf()'s loop and in the fused (fma) chains, for
  S = 4 and 20, f32 and f64.  `placed_case` writes the wanted parent through
  `x1` (or `x2`); `expected_parent` is what plf() must return, bit for bit.
* tree cases (`tree_case`): the same pattern appearing first at a chosen level
  of a balanced tree, as the product of a 2^-16 leaf and a pattern * 2^16 leaf.
* table cases (`tiptip_case`, `protein_table_case`): both children coded, the
  near-threshold values in the caller's tip-vector table, the deciding
  category chosen by power-of-two factors on the permutation matrices.
* `random_case`: dense random matrices, each site's largest parent magnitude
  within 2^-8 of the threshold.

tests/test_scale_cases.py checks on the oracle alone that the cases cover what
they claim; tests/test_gpu_scale_decision.py runs them through every kernel.
"""
from __future__ import annotations

import numpy as np

import oracle as O

KINDS = ("at", "neg", "under", "negunder", "zero", "nan")
AT, NEG, UNDER, NEGUNDER, ZERO, NAN = range(6)
SCALES = (False, False, True, True, True, False)   # per kind: must the site scale
TAIL = 37
CAT = 4
TWO32 = 4294967296.0


def consts(dtype):
    """(thr, below, sub): 2^-32, the value just under it, a subnormal."""
    dt = np.dtype(dtype).type
    thr = dt(2.0 ** -32)
    return thr, np.nextafter(thr, dt(0)), dt(np.finfo(dtype).tiny / 4)


def tile(S):
    """Sites after which the hot position's start advances by one: 64 for
    protein (one LDS / MFMA tile), 256 for DNA (four lanes a site)."""
    return 64 if S == 20 else 256


def full_sites(S):
    """Each (position, site-in-tile) pair exactly once: 5120 protein, 4096 DNA."""
    return tile(S) * CAT * S


def site_plan(S, n, shift):
    """(hot position, kind, weight) of sites 0..n-1."""
    i = np.arange(n, dtype=np.int64)
    hot = (i // tile(S) + i % tile(S)) % (CAT * S)
    kind = (7 * i + i // 64 + shift) % 6
    return hot, kind, (1 + i % 5).astype(np.int32)


def placed_values(S, dtype, n, shift):
    """The wanted unscaled parent [n][4*S] and its plan."""
    dtype = np.dtype(dtype).type
    thr, below, sub = consts(dtype)
    V = CAT * S
    hot, kind, wgt = site_plan(S, n, shift)
    P = np.full((n, V), below, dtype)
    P[kind == NEGUNDER] *= np.where(np.arange(V) % 2, -1, 1).astype(dtype)
    P[kind == ZERO] = sub
    P[np.arange(n), hot] = np.array([thr, -thr, below, -below, 0.0, np.nan], dtype)[kind]
    return P, hot, kind, wgt


def perm(S, b, a=3):
    """k -> (a*k + b) mod S: never the identity for a = 3 (S = 4, 20)."""
    return (a * np.arange(S) + b) % S


def side_perms(S, side, o=0):
    """The four category permutations of `left` (side 0) or `right` (side 1)."""
    return [perm(S, 1 + side + j + o) for j in range(CAT)]


def ev_perm(S):
    return perm(S, 3, 7)


def perm_matrix(S, dtype, perms, factors=None):
    """[c][k][l] with M[c][k][perms[c][k]] = factors[c] (1), else 0."""
    M = np.zeros((len(perms), S, S), dtype)
    for j, p in enumerate(perms):
        M[j, np.arange(S), p] = 1 if factors is None else factors[j]
    return M.reshape(-1)


def carry(S, P, side=0, o=0, inverse=False):
    """The child CLV that one node's permutations carry to parent P (x3[j][ev[k]]
    = x[j][pi_j[k]]), or with inverse=True the parent a child CLV arrives as."""
    n = P.shape[0]
    P = P.reshape(n, CAT, S)
    out = np.empty_like(P)
    ev = ev_perm(S)
    for j, p in enumerate(side_perms(S, side, o)):
        if inverse:
            out[:, j, ev] = P[:, j, p]
        else:
            out[:, j, p] = P[:, j, ev]
    return out.reshape(n, CAT * S)


def expected_parent(S, P, hot, kind):
    """plf()'s parent for wanted values P: scaled sites times 2^32 (exact), a
    NaN spread over its category (0 * NaN in every chain of that category)."""
    E = P.copy()
    sc = np.array(SCALES)[kind]
    E[sc] = (E[sc].astype(np.float64) * TWO32).astype(P.dtype)
    for i in np.flatnonzero(kind == NAN):
        j = hot[i] // S
        E[i, j * S:(j + 1) * S] = np.nan
    return E.reshape(-1), sc.astype(np.uint8)


def placed_case(S, dtype, n=None, shift=0, carrier="x1"):
    """One node whose parent is placed_values(): dict(x1, x2, EV, left, right,
    wgt, n, placed, hot, kind).  carrier: the child that carries the pattern
    (the other is all ones)."""
    if n is None:
        n = full_sites(S) + TAIL
    P, hot, kind, wgt = placed_values(S, dtype, n, shift)
    side = 0 if carrier == "x1" else 1
    x = np.ascontiguousarray(carry(S, P, side).reshape(-1))
    ones = np.ones(n * CAT * S, dtype)
    return dict(x1=x if side == 0 else ones, x2=ones if side == 0 else x,
                EV=perm_matrix(S, dtype, [ev_perm(S)]),
                left=perm_matrix(S, dtype, side_perms(S, 0)),
                right=perm_matrix(S, dtype, side_perms(S, 1)),
                wgt=wgt, n=n, placed=P, hot=hot, kind=kind, S=S)


def run_oracle(case, fma=False):
    """(x3, scaler bytes, weighted sum) of a one-node case from the oracle:
    plf() itself for S = 4 in exact mode, the generic loop otherwise."""
    S = case["S"]
    a = [case[k] for k in ("x1", "x2", "EV", "left", "right", "wgt")]
    if S == 4 and not fma:
        return O.plf(*a)
    return O.plf_generic(S, CAT, *a, fma=fma)


# --------------------------------------------------------------------------
# random matrices, every site next to the threshold
# --------------------------------------------------------------------------
def random_case(S, dtype, n, seed, fma=False, EV=None):
    """Dense random positive x1, x2, P and a signed EV (or the caller's): the
    inputs are normalised so that the oracle's unscaled parent has a largest
    magnitude of about 1 at every site, then each site of x1 is multiplied by
    2^-32 (exact) and by a factor in [1 - 2^-8, 1 + 2^-8]."""
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng(seed)
    V = CAT * S
    x1 = rng.random((n, V))
    x2 = rng.random(V * n).astype(dtype)
    left = rng.random(CAT * S * S).astype(dtype)
    right = rng.random(CAT * S * S).astype(dtype)
    ev = (rng.random(S * S) - 0.25).astype(dtype)
    EV = ev if EV is None else EV
    wgt = (1 + np.arange(n) % 5).astype(np.int32)

    def top(x):
        x3 = O.plf_generic(S, CAT, x, x2, EV, left, right, fma=fma)[0]
        return np.abs(x3.astype(np.float64)).reshape(n, V).max(axis=1, keepdims=True)

    x1 = (x1 / top(np.ascontiguousarray(x1.astype(dtype).reshape(-1)))).astype(dtype)  # largest ~ 1
    f = 1 + (rng.random((n, 1)) * 2 - 1) * 2.0 ** -8
    x1 = (x1 * dtype(2.0 ** -32)) * f.astype(dtype)      # a power of two (exact), then the factor
    return dict(x1=np.ascontiguousarray(x1.reshape(-1)), x2=x2, EV=EV, left=left, right=right,
                wgt=wgt, n=n, S=S)


# --------------------------------------------------------------------------
# both children coded: the values sit in the caller's tip-vector table
# --------------------------------------------------------------------------
def _hot_factors(dtype, hotcat):
    return [dtype(1.0) if j == hotcat else dtype(0.5) for j in range(CAT)]


def tiptip_case(dtype, n, shift, hotcat):
    """DNA tip/tip node through a 16 x 4 table: rows 0..3 `thr` at state r,
    4..7 `-thr`, 8 all `below`, 9 alternating signs, 10 / 11 a zero among
    subnormals, 15 all ones (child 2, with junk in the codes' upper nibble).
    `left` carries 1 in category `hotcat` and 1/2 elsewhere, so a row's `thr`
    decides in that category alone.  A table row is shared by every category:
    the 16 (category, state) positions are reached for the kinds `at` and
    `neg` over the four `hotcat`; the scaling kinds have no single position."""
    dtype = np.dtype(dtype).type
    thr, below, sub = consts(dtype)
    tv = np.full((16, 4), below, dtype)
    for s in range(4):
        tv[s, s], tv[4 + s, s] = thr, -thr
    tv[9] *= np.array([-1, 1, -1, 1], dtype)
    tv[10], tv[11] = sub, sub
    tv[10, 0] = tv[11, 2] = 0
    tv[12:15] = np.array([[2.0], [thr * 2], [0.0]], dtype)
    tv[15] = 1
    hot, kind, wgt = site_plan(4, n, shift)
    i = np.arange(n)
    row = np.array([0, 4, 8, 9, 10, 12])[kind] + np.where(kind <= NEG, hot % 4, 0)
    row = np.where(kind == ZERO, 10 + i % 2, row)
    row = np.where(kind == NAN, 12 + i % 3, row)
    c1 = (row | ((i % 16) << 4)).astype(np.uint8)
    c2 = (15 | ((i * 5 % 16) << 4)).astype(np.uint8)
    return dict(c1=c1, c2=c2, tipvec=tv.reshape(-1), EV=perm_matrix(4, dtype, [ev_perm(4)]),
                left=perm_matrix(4, dtype, side_perms(4, 0), _hot_factors(dtype, hotcat)),
                right=perm_matrix(4, dtype, side_perms(4, 1)), wgt=wgt, n=n, S=4,
                x1=O.expand_tips(c1, dtype, tipvec=tv), x2=O.expand_tips(c2, dtype, tipvec=tv),
                hot_state=hot % 4, kind=kind, hotcat=hotcat)


def protein_table(dtype, shift, scale=1.0):
    """PROT_CODES x 20 table: row r < 20 holds +-thr at state r (sign by the
    parity of r + shift) among `below`, 20 all `below`, 21 alternating signs,
    22 a zero among subnormals, 23 (and every code past it) all ones."""
    dtype = np.dtype(dtype).type
    thr, below, sub = consts(dtype)
    tv = np.full((O.PROT_CODES, 20), below, dtype)
    for r in range(20):
        tv[r, r] = thr if (r + shift) % 2 == 0 else -thr
    tv[21] *= np.where(np.arange(20) % 2, -1, 1).astype(dtype)
    tv[22] = sub
    tv[22, shift % 20] = 0
    tv[:23] *= dtype(scale)
    tv[23] = 1
    return tv


def protein_codes(n, shift):
    hot, kind, wgt = site_plan(20, n, shift)
    i = np.arange(n)
    c1 = np.where((kind <= NEG) | (kind == NAN), hot % 20, 18 + kind).astype(np.uint8)
    c2 = (23 + (i % 3) * 50).astype(np.uint8)       # codes past the table read its last row
    return c1, c2, wgt, hot, kind


def protein_table_case(dtype, n, shift):
    """Protein node with both children coded; category shift % 4 decides."""
    dtype = np.dtype(dtype).type
    tv = protein_table(dtype, shift)
    c1, c2, wgt, hot, kind = protein_codes(n, shift)
    return dict(c1=c1, c2=c2, tipvec=tv.reshape(-1), EV=perm_matrix(20, dtype, [ev_perm(20)]),
                left=perm_matrix(20, dtype, side_perms(20, 0), _hot_factors(dtype, shift % 4)),
                right=perm_matrix(20, dtype, side_perms(20, 1)), wgt=wgt, n=n, S=20,
                x1=O.expand_protein_tips(c1, dtype, tipvec=tv),
                x2=O.expand_protein_tips(c2, dtype, tipvec=tv), kind=kind, hotcat=shift % 4)


# --------------------------------------------------------------------------
# trees: the pattern appears first at a chosen level
# --------------------------------------------------------------------------
def tree_pmats(S, dtype, nops, factors=None):
    """One (left, right) pair of permutation matrices per op, the offsets
    moving with the op; factors: {op: per-category factors of its left}."""
    out = []
    for m in range(nops):
        out.append(perm_matrix(S, dtype, side_perms(S, 0, 2 * m), (factors or {}).get(m)))
        out.append(perm_matrix(S, dtype, side_perms(S, 1, 2 * m)))
    return np.concatenate(out)


def tree_levels(ntips):
    """Level (1 = above the leaves) of every op of balanced_tree_ops(ntips)."""
    lv, cnt, l = [], ntips // 2, 1
    while cnt:
        lv += [l] * cnt
        cnt, l = cnt // 2, l + 1
    return np.array(lv)


def tree_case(S, dtype, ntips, n, shift):
    """Balanced tree over dense leaves, permutation matrices at every node: a
    node's CLV is the permuted elementwise product of the leaves below it
    (times 2^32 per earlier rescale).  Site i has a target level l; every leaf
    is all ones but one leaf in each child subtree of one level-l node: one
    holds 2^-16 everywhere, the other placed_values() * 2^16.  Both are far
    above the threshold; their product -- the pattern, exactly -- first exists
    at level l and stays as close at every level above it."""
    dtype = np.dtype(dtype).type
    V = CAT * S
    depth = ntips.bit_length() - 1
    P, _, _, wgt = placed_values(S, dtype, n, shift)
    ops = O.balanced_tree_ops(ntips)
    i = np.arange(n)
    level = 1 + (i // 7 + i // 64) % depth
    span, half = 1 << level, 1 << (level - 1)
    node = (i // 11) % (ntips // span)
    la = node * span + (i // 13) % half
    lb = node * span + half + (i // 17) % half
    swap = (i // 5) % 2 == 1
    la, lb = np.where(swap, lb, la), np.where(swap, la, lb)
    tips = [np.ones((n, V), dtype) for _ in range(ntips)]
    pat = P * dtype(65536.0)
    for t in range(ntips):
        tips[t][la == t] = dtype(2.0 ** -16)
        tips[t][lb == t] = pat[lb == t]
    return dict(ops=ops, tips=[np.ascontiguousarray(t.reshape(-1)) for t in tips],
                pm=tree_pmats(S, dtype, ops.shape[0]), EV=perm_matrix(S, dtype, [ev_perm(S)]),
                wgt=wgt, n=n, S=S, level=level, codes=None, tipvec=None)


def protein_coded_tree_case(dtype, n, shift):
    """8 protein taxa, every leaf coded through one caller table: the rows of
    protein_table() times 2^16, row 19 replaced by 2^-16 everywhere, row 23 all
    ones.  Site i has a target level 2 or 3; below the two children of one
    node of that level, one odd leaf reads row 19 and one even leaf a pattern
    row, every other leaf row 23.  The level-1 parents come from the tip/tip
    tables far above the threshold; their product is the pattern.  Every
    level-1 op carries 1 in category shift % 4 and 1/2 elsewhere on its left
    (even) child, so that category alone keeps the pattern's magnitude."""
    dtype = np.dtype(dtype).type
    ntips = 8
    tv = protein_table(dtype, shift, 65536.0)
    tv[19] = dtype(2.0 ** -16)      # state 19 gives up its `thr` row
    c1, _, wgt, hot, kind = protein_codes(n, shift)
    c1 = np.where(c1 == 19, 20, c1).astype(np.uint8)
    i = np.arange(n)
    level = 2 + (i // 7 + i // 64) % 2
    span, half = 1 << level, 1 << (level - 1)
    node = (i // 11) % (ntips // span)
    swap = (i // 5) % 2
    la = node * span + swap * half + 2 * ((i // 13) % (half // 2)) + 1
    lb = node * span + (1 - swap) * half + 2 * ((i // 17) % (half // 2))
    codes = []
    for t in range(ntips):
        c = np.full(n, 23, np.uint8)
        c[la == t] = 19
        c[lb == t] = c1[lb == t]
        codes.append(c)
    ops = O.balanced_tree_ops(ntips)
    fac = {m: _hot_factors(dtype, shift % 4) for m in range(4)}
    return dict(ops=ops, tips=[O.expand_protein_tips(c, dtype, tipvec=tv) for c in codes],
                codes=codes, tipvec=tv.reshape(-1), pm=tree_pmats(20, dtype, ops.shape[0], fac),
                EV=perm_matrix(20, dtype, [ev_perm(20)]), wgt=wgt, n=n, S=20, level=level)


def run_tree_oracle(case, fma=False):
    """(CLV of every slot, scaler sums, scaler bytes per op): oracle.traverse,
    or in fma mode the fused loop node by node."""
    S, n, ops = case["S"], case["n"], case["ops"]
    dt = case["tips"][0].dtype
    M = CAT * S * S
    host = [t.copy() for t in case["tips"]] + [np.zeros(CAT * S * n, dt) for _ in range(ops.shape[0])]
    if not fma:
        sums, scal = O.traverse(S, CAT, ops, host, case["pm"], case["EV"], n, case["wgt"], want_scalers=True)
        return host, sums, scal
    sums, scal = [], []
    for p, c1, c2, m in ops:
        pm = case["pm"]
        host[p], sc, inc = O.plf_generic(S, CAT, host[c1], host[c2], case["EV"], pm[2 * m * M:(2 * m + 1) * M],
                                         pm[(2 * m + 1) * M:(2 * m + 2) * M], case["wgt"], fma=True)
        sums.append(inc)
        scal.append(sc)
    return host, np.array(sums, np.int64), scal


def random_tree_case(dtype, n, seed):
    """64 DNA taxa: every level-1 op is a random_case of its own (its two
    leaves and its matrices; one EV for the tree), so the first level of a
    fused pass decides next to the threshold on real matrix-vector arithmetic;
    the levels above use random matrices times 0.3."""
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng(seed)
    ops = O.balanced_tree_ops(64)
    EV = (rng.random(16) - 0.25).astype(dtype)
    pm = (rng.random(ops.shape[0] * 128) * 0.3).astype(dtype)
    tips = []
    for m in range(32):
        c = random_case(4, dtype, n, seed + 1 + m, EV=EV)
        tips += [c["x1"], c["x2"]]
        pm[128 * m:128 * m + 64], pm[128 * m + 64:128 * m + 128] = c["left"], c["right"]
    return dict(ops=ops, tips=tips, pm=pm, EV=EV, wgt=c["wgt"], n=n, S=4, codes=None, tipvec=None)
