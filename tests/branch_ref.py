"""The tree side of plfx_branch_sumtables_psr (plfx.h section 13) restated in
plain Python for tests/test_branch_lower.py (CPU) and
tests/test_gpu_psr_branches.py (GPU): who reads each slot, the pre-order
levels, the edge of each op's parent slot, and the integer sums behind
edge_scale.  A tree is psr_trees' (ops, nslots, coded flag per slot)."""
import numpy as np


def structure(ops):
    """Per op: level (depth from the root op, the last op), up (the edge 2*r + s
    of its parent slot in the op r that reads it, -1 for the root op), and the
    ops w1 / w2 that wrote its children (-1: a leaf)."""
    nops = len(ops)
    writer = {op[0]: j for j, op in enumerate(ops)}
    reader = {}
    for j, (_, c1, c2, _) in enumerate(ops):
        reader[c1], reader[c2] = (j, 0), (j, 1)
    level, up = [0] * nops, [-1] * nops
    for j in range(nops - 2, -1, -1):
        r, s = reader[ops[j][0]]
        level[j], up[j] = level[r] + 1, 2 * r + s
    w = [(writer.get(c1, -1), writer.get(c2, -1)) for _, c1, c2, _ in ops]
    return level, up, w


def edge_scale(ops, scaler_sums, wsum):
    """edge_scale[2*j + s] from the traversal's scaler_sums[j] and the W sums
    wsum[2*j + s] (ignored for the root op's two edges), as exact integers."""
    nops = len(ops)
    level, up, w = structure(ops)
    sub = [0] * nops
    for j in range(nops):
        sub[j] = int(scaler_sums[j]) + sum(sub[k] for k in w[j] if k >= 0)
    s_of = lambda k: sub[k] if k >= 0 else 0
    outer = [0] * (2 * nops)
    for j in range(nops - 1, -1, -1):
        for s in (0, 1):
            outer[2 * j + s] = s_of(w[j][1 - s]) + (int(wsum[2 * j + s]) + outer[up[j]] if up[j] >= 0 else 0)
    return np.array([outer[2 * j + s] + s_of(w[j][s]) for j in range(nops) for s in (0, 1)], dtype=np.int64)


def one_coded_root_child():
    """caterpillar(4) with its last leaf -- a child of the root op -- the only
    coded tip: under the root op's other child W(v) is a code array."""
    ops = [(4, 0, 1, 0), (5, 4, 2, 1), (6, 5, 3, 2)]
    return ops, 7, [False, False, False, True, False, False, False]
