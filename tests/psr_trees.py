"""Op lists of the small trees the plfx_traverse_psr tests share
(tests/test_psr_trav_lower.py on the CPU, tests/test_gpu_psr_traverse.py on the
GPU).  A tree is (ops, nslots, tip flags per slot): ops are (parent, child1,
child2, pmat) rows in post-order with pmat = the op's index, leaves take the
first slots."""
import numpy as np


def balanced(nleaves, coded, slot0=0, op0=0):
    """A balanced tree over nleaves = 2^k leaves, leaves coded tips or dense inputs."""
    ops = []
    nxt = [slot0 + nleaves]

    def build(lo, hi):
        if hi - lo == 1:
            return slot0 + lo
        mid = (lo + hi) // 2
        a, b = build(lo, mid), build(mid, hi)
        p = nxt[0]
        nxt[0] += 1
        ops.append((p, a, b, op0 + len(ops)))
        return p

    build(0, nleaves)
    nslots = 2 * nleaves - 1
    return ops, nslots, [coded] * nleaves + [False] * (nleaves - 1)


def caterpillar(nleaves, coded):
    ops = [(nleaves, 0, 1, 0)]
    for i in range(2, nleaves):
        ops.append((nleaves + i - 1, nleaves + i - 2, i, i - 1))
    return ops, 2 * nleaves - 1, [coded] * nleaves + [False] * (nleaves - 1)


def forest(trees, nleaves, coded):
    """`trees` balanced trees side by side: one level of each holds `trees` times the ops."""
    ops, flags, slot = [], [], 0
    for _ in range(trees):
        o, ns, f = balanced(nleaves, coded, slot0=slot, op0=len(ops))
        ops += o
        flags += f
        slot += ns
    return ops, slot, flags


def mixed(swap_p):
    """One level pair of tip kind 1: slots 0, 1 coded, 2, 3 dense inputs; op 0 has
    its coded child first, op 1 second; op 2 names them in either order."""
    return ([(4, 0, 2, 0), (5, 3, 1, 1), (6, 5, 4, 2) if swap_p else (6, 4, 5, 2)], 7,
            [True, True, False, False, False, False, False])


def random_tree(nleaves, coded, seed):
    """A random binary tree by joining two random roots at a time, children in random order."""
    rng = np.random.default_rng(seed)
    roots = list(range(nleaves))
    ops = []
    while len(roots) > 1:
        i, j = rng.choice(len(roots), 2, replace=False)
        a, b = roots[i], roots[j]
        p = nleaves + len(ops)
        ops.append((p, a, b, len(ops)))
        roots = [r for k, r in enumerate(roots) if k not in (i, j)] + [p]
    return ops, 2 * nleaves - 1, [coded] * nleaves + [False] * (nleaves - 1)


def levels(ops):
    """Dependency level of each op of a tree whose slots are written once."""
    lv, slot_level = [], {}
    for p, a, b, _ in ops:
        l = max(slot_level.get(a, -1), slot_level.get(b, -1)) + 1
        slot_level[p] = l
        lv.append(l)
    return lv


def expected_schedule(tree, fuse=True):
    """(level pairs, unfused ops, launches) of plfx_traverse_psr on a tree whose
    slots are written once -- the planner's rule restated: scanning the ops in
    list order, op p takes the writers a, b of its children when both sit one
    level below p, have the same number of coded children and are still free.
    Per level the pairs go out by tip kind in launches of 10, the other ops by
    kind of children in launches of 32.  (tests/test_psr_trav_lower.py pins
    this to the planner on the CPU.)"""
    ops, _, flags = tree
    lv = levels(ops)
    writer = {op[0]: j for j, op in enumerate(ops)}
    ntips = [int(flags[a]) + int(flags[b]) for _, a, b, _ in ops]
    used, pairs = set(), {}
    for p, (_, c1, c2, _) in enumerate(ops):
        a, b = writer.get(c1), writer.get(c2)
        if not fuse or a is None or b is None or {a, b, p} & used:
            continue
        if lv[a] != lv[b] or lv[p] != lv[a] + 1 or ntips[a] != ntips[b]:
            continue
        used |= {a, b, p}
        pairs[(lv[a], ntips[a])] = pairs.get((lv[a], ntips[a]), 0) + 1
    nodes = {}
    for j, (_, c1, c2, _) in enumerate(ops):
        if j not in used:
            key = (lv[j], int(flags[c1]) | 2 * int(flags[c2]))
            nodes[key] = nodes.get(key, 0) + 1
    launches = sum(-(-c // 10) for c in pairs.values()) + sum(-(-c // 32) for c in nodes.values())
    return sum(pairs.values()), len(ops) - len(used), launches


def shuffled_within_levels(ops, seed):
    """The same tree level by level, the ops of each level in random order (a
    valid order: an op still follows the writers of its children); pmat
    follows the op."""
    rng = np.random.default_rng(seed)
    lv = levels(ops)
    out = []
    for l in sorted(set(lv)):
        block = [op for op, x in zip(ops, lv) if x == l]
        out += [block[i] for i in rng.permutation(len(block))]
    return out
