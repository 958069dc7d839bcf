"""An independent reference for likelihoods and branch derivatives: Felsenstein
pruning in state space, in plain numpy f64 with scipy.linalg.expm.  A helper
module (no tests) for tests/test_felsenstein_ref.py, which checks it against
closed forms on the CPU and measures the numpy restatements against it, and for
tests/test_gpu_likelihood_ref.py, which compares the GPU pipelines against it.

It shares nothing with the library: no eigen decomposition of any kind, no
plfx call.  Q is built here from exchangeabilities and frequencies, transition
matrices are expm(Q r t), the derivatives in t are r Q P and r^2 Q^2 P, and
scaling is a per-site log term kept next to a CLV normalised to maximum 1.

A tree is a post-order op list of (parent, child1, child2, pmat) rows as in
tests/psr_trees.py; op m's children hang on branches blen[2 m], blen[2 m + 1].
A CLV is (n, C, S): C = 4 categories for Gamma, C = 1 for per-site rates;
site_rates (n, C) holds the rate each site uses in each category."""
import numpy as np
from scipy.linalg import expm


def gtr_q(exch, freqs):
    """(Q, pi): the reversible generator with S (S - 1) / 2 exchangeabilities
    (upper triangle, row by row), normalised to one expected substitution."""
    S = len(freqs)
    pi = np.asarray(freqs, np.float64) / np.sum(freqs)
    R = np.zeros((S, S))
    R[np.triu_indices(S, 1)] = exch
    R = R + R.T
    Q = R * pi[None, :]
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q / -(pi * np.diag(Q)).sum(), pi


_CACHE = {}


def transition(Q, r, t):
    """expm(Q r t), cached per distinct (Q, r, t)."""
    key = (Q.tobytes(), float(r), float(t))
    P = _CACHE.get(key)
    if P is None:
        if len(_CACHE) > 200_000:
            _CACHE.clear()
        P = _CACHE[key] = expm(Q * (float(r) * float(t)))
    return P


def site_rates_psr(rates, cat):
    """(n, 1): rates[min(cat, ncat - 1)] per site."""
    rates = np.asarray(rates, np.float64)
    return rates[np.minimum(np.asarray(cat).astype(np.int64), rates.size - 1)][:, None]


def site_rates_gamma(rates, n):
    """(n, C): every site uses all the category rates."""
    return np.tile(np.asarray(rates, np.float64)[None, :], (n, 1))


def tip_states(codes, S=4):
    """(n, S) 0/1 vectors of DNA state-set codes: bit s of the low nibble."""
    assert S == 4
    c = np.asarray(codes).astype(np.int64) & 15
    return ((c[:, None] >> np.arange(4)[None, :]) & 1).astype(np.float64)


def _full(x, C):
    x = np.asarray(x, np.float64)
    return np.repeat(x[:, None, :], C, axis=1) if x.ndim == 2 else x


def _apply(Q, x, site_rates, t, power=0):
    """y[i, c] = r^power Q^power expm(Q r_ic t) x[i, c], grouped by distinct rate."""
    y = np.empty_like(x)
    Qp = np.linalg.matrix_power(Q, power)
    for c in range(x.shape[1]):
        col = site_rates[:, c]
        for r in np.unique(col):
            idx = np.flatnonzero(col == r)
            M = (r ** power) * (Qp @ transition(Q, r, t))
            y[idx, c] = x[idx, c] @ M.T
    return y


def prune(Q, ops, blen, tips, site_rates):
    """{slot: (CLV (n, C, S), log scale (n,))} of every slot: the slots the ops
    write with per-site maximum 1, the tips as given with log scale 0.  tips:
    {slot: (n, S) or (n, C, S) state-space vectors} of the slots the ops only read."""
    site_rates = np.asarray(site_rates, np.float64)
    n, C = site_rates.shape
    clv = {s: (_full(x, C), np.zeros(n)) for s, x in tips.items()}
    for p, c1, c2, m in ops:
        (x1, l1), (x2, l2) = clv[c1], clv[c2]
        v = _apply(Q, x1, site_rates, blen[2 * m]) * _apply(Q, x2, site_rates, blen[2 * m + 1])
        mx = v.reshape(n, -1).max(axis=1)
        clv[p] = (v / mx[:, None, None], l1 + l2 + np.log(mx))
    return clv


def root_lnl(clv, logscale, pi, catw=None, wgt=None):
    """(lnL, log L per site) of a root CLV."""
    n, C, _ = clv.shape
    cw = np.full(C, 1.0 / C) if catw is None else np.asarray(catw, np.float64)
    w = np.ones(n) if wgt is None else np.asarray(wgt, np.float64)
    site = np.log(np.einsum("c,ncs,s->n", cw, clv, pi)) + logscale
    return float(np.sum(w * site)), site


def edge(A, la, B, lb, Q, pi, site_rates, catw, t, wgt=None):
    """The branch of length t between the CLVs A and B (log scales la, lb; 0 for
    none): (out3 = (lnL, d1, d2), the scales of their tolerances as
    tests/test_gpu_edge.py's ref_edge defines them, log L per site).
    L_i = sum_c catw_c sum_s pi_s A_ics [P(r_ic t) B_ic]_s; its derivatives in
    t use r Q P and r^2 Q^2 P."""
    site_rates = np.asarray(site_rates, np.float64)
    n, C = site_rates.shape
    A, B = _full(A, C), _full(B, C)
    cw = np.full(C, 1.0 / C) if catw is None else np.asarray(catw, np.float64)
    w = np.ones(n) if wgt is None else np.asarray(wgt, np.float64)
    L, L1, L2 = (np.einsum("c,ncs,s,ncs->n", cw, A, pi, _apply(Q, B, site_rates, t, k)) for k in (0, 1, 2))
    r1, r2 = L1 / L, L2 / L
    site = np.log(L) + la + lb
    out = np.array([np.sum(w * site), np.sum(w * r1), np.sum(w * (r2 - r1 * r1))])
    scale = np.array([abs(out[0]), np.sum(np.abs(w) * np.abs(r1)), np.sum(np.abs(w) * (np.abs(r2) + r1 * r1))])
    return out, scale, site


def simulate(Q, pi, ops, blen, site_rates_choice, rng, t_root):
    """{slot: (n,) states} of every slot, evolved at the per-site rates
    site_rates_choice (n,) down the tree of `ops`, whose root's two children
    sit at distance t_root from each other (the root's own two branch lengths
    are not used): the first child's states are drawn from pi, the second's
    evolve from them.  So the likelihood of the branch between the two has an
    optimum near t_root."""
    rate = np.asarray(site_rates_choice, np.float64)
    n, S = rate.size, len(pi)

    def evolve(parent, t):
        child = np.empty(n, np.int64)
        for r in np.unique(rate):
            idx = np.flatnonzero(rate == r)
            p = np.clip(transition(Q, r, t)[parent[idx]], 0, None)
            p /= p.sum(axis=1, keepdims=True)
            child[idx] = (rng.random(idx.size)[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, S - 1)
        return child

    _, a, b, _ = ops[-1]
    state = {a: rng.choice(S, n, p=pi)}
    state[b] = evolve(state[a], t_root)
    for p, c1, c2, m in reversed(list(ops[:-1])):
        state[c1], state[c2] = evolve(state[p], blen[2 * m]), evolve(state[p], blen[2 * m + 1])
    return state


# ---- unrooted trees, for the root-placement tests ----

def unroot(ops, blen):
    """The unrooted tree of a rooted op list: [(u, v, length)] over the slots,
    the root's two branches joined into one edge."""
    edges = []
    root, a, b, m = ops[-1]
    edges.append((a, b, blen[2 * m] + blen[2 * m + 1]))
    for p, c1, c2, m in ops[:-1]:
        edges += [(p, c1, blen[2 * m]), (p, c2, blen[2 * m + 1])]
    return edges


def root_on_edge(edges, ntips, k, frac):
    """(ops, blen) of the unrooted tree `edges` (tips are the nodes below
    ntips) rooted on edge k, frac of its length on the side of its first
    node.  Inner nodes are renumbered: op j writes slot ntips + j."""
    adj = {}
    for u, v, t in edges:
        adj.setdefault(u, []).append((v, t))
        adj.setdefault(v, []).append((u, t))
    ops, blen = [], []

    def down(node, parent):
        if node < ntips:
            return node
        (c1, t1), (c2, t2) = [(v, t) for v, t in adj[node] if v != parent]
        s1, s2 = down(c1, node), down(c2, node)
        return emit(s1, t1, s2, t2)

    def emit(s1, t1, s2, t2):
        ops.append((ntips + len(ops), s1, s2, len(ops)))
        blen.extend([t1, t2])
        return ops[-1][0]

    u, v, t = edges[k]
    emit(down(u, v), frac * t, down(v, u), (1 - frac) * t)
    return ops, np.array(blen)
