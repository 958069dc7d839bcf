# PROTCAT FMA mode (plfx.h section 11d) against exact mode on the same buffers,
# in one process, calls alternating: f64, 20 states.  Tuning / record only:
# needs a gfx950 device (no fallback).
#
#   node       plf_psr_gen, ncat 25, dense/dense, at 2^14, 2^18 and 2^20 sites,
#              fma=True against fma=False, in three category orders: sorted,
#              whole runs of 64 sites in shuffled order, uniformly random
#              (tools/psr_prot_bench.py's, and its method: every row captured
#              GRAPH_CALLS times into a graph of its own, timed with device
#              events around `--calls` calls' worth of replays, the rows
#              alternating within every round after a warm-up round; median,
#              min and max over `--rounds` rounds).  Per row the achieved
#              bytes/s from 486 B/site (two CLV rows read, one written, the
#              category byte, the weight, the scaler byte) against the 8 TB/s
#              HBM peak, and at 2^18 the two estimates the mode was proposed
#              on: ~20 us for the bytes at the 6.2-6.35 TB/s stream ceiling,
#              ~8 us of matrix-core time.
#   traversal  the balanced 64-taxon tree with coded tips, ncat 25, sorted
#              categories, at 10^4 and 2^18 sites: traverse_psr_gen both modes
#              (issued eagerly between two device events,
#              tools/psr_prot_scan_bench.py's way).
#   scan       psr_rate_scan_gen, 32 candidates, group 1 / 8 / 32 at the same
#              sizes, both modes (a group whose workspace does not fit the free
#              device memory is left out and said so).
#
#   python tools/psr_prot_fma_bench.py [--calls 100] [--rounds 7] [--parts node trees] [--log profiles/rNN_psr_prot_fma_bench.log]
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import psr_prot_bench as NB  # noqa: E402  (puts the package on the path)
import psr_prot_scan_bench as SB  # noqa: E402
import plfx  # noqa: E402

S, NCAT, NCAND = 20, NB.NCAT, SB.NCAND
NODE_BYTES = 3 * S * 8 + 1 + 4 + 1  # per site
HBM_PEAK_GBS = SB.HBM_PEAK_GBS
EST_BYTES_US, EST_MFMA_US = 20.0, 8.0  # the estimates at 2^18 sites (unmeasured before this tool)

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def node_rows(ctx, n):
    dt = torch.float64
    gen = torch.Generator(device="cuda").manual_seed(n % 1000 + 8)
    rnd = lambda m: torch.rand(m, dtype=dt, device="cuda", generator=gen) * 0.9 + 0.1  # noqa: E731
    x1, x2, x3 = rnd(S * n), rnd(S * n), torch.empty(S * n, dtype=dt, device="cuda")
    EV, left, right = rnd(S * S) * 0.1, rnd(S * S * NCAT) * 0.1, rnd(S * S * NCAT) * 0.1
    wgt = torch.ones(n, dtype=torch.int32, device="cuda")
    sc = torch.empty(n, dtype=torch.uint8, device="cuda")
    ss = torch.zeros(1, dtype=torch.int64, device="cuda")
    nd = dict(x1=x1, x2=x2, x3=x3, left=left, right=right, scaler=sc, scaler_sum=ss)
    rows = {}
    for o, c in NB.categories(n, gen).items():
        for fma in (False, True):
            rows[f"{'fma  ' if fma else 'exact'} {o}"] = lambda s, c=c, fma=fma: ctx.plf_psr_gen(
                S, nd, EV, n, c, NCAT, wgt=wgt, stream=s, fma=fma)
    return rows


def node(ctx, calls, rounds):
    for n in (1 << 14, 1 << 18, 1 << 20):
        say(f"node: f64 ncat={NCAT} dense/dense n={n}, {NODE_BYTES} B/site = {n * NODE_BYTES / 1e6:.1f} MB a call")
        rows = node_rows(ctx, n)
        res = NB.measure(rows, calls, rounds)
        for name in rows:
            med, lo, hi = res[name]
            gbs = n * NODE_BYTES / med / 1e3
            say(f"  {name:28s} {med:9.2f} us/call (min {lo:.2f} max {hi:.2f}) {n / med / 1e3:7.3f} G sites/s "
                f"{gbs:7.0f} GB/s = {gbs / HBM_PEAK_GBS:.2f} of the {HBM_PEAK_GBS / 1e3:.0f} TB/s peak")
        for o in NB.ORDERS:
            e, f = res[f"exact {o}"][0], res[f"fma   {o}"][0]
            say(f"  {o}: fma time / exact time = {f / e:.3f}")
        if n == 1 << 18:
            f = res["fma   sorted"][0]
            say(f"  at 2^18, sorted: measured {f:.1f} us against the estimates {EST_BYTES_US:.0f} us (bytes at the "
                f"stream ceiling) and {EST_MFMA_US:.0f} us (matrix-core cycles): x{f / EST_BYTES_US:.2f} and "
                f"x{f / EST_MFMA_US:.2f}")
        del rows
        torch.cuda.empty_cache()


def eager(variants, rounds):
    us = {k: [] for k in variants}
    for rnd in range(rounds + 1):  # round 0 warms up
        for name, fn in variants.items():
            t = SB.timed(fn)
            if rnd:
                us[name].append(t)
    return us


def traversal_variants(ctx, p):
    n, nops = p["n"], p["nops"]
    pm = torch.empty(2 * nops * NCAT * S * S, dtype=torch.float64, device="cuda")
    rates = torch.from_numpy(np.geomspace(0.1, 4.0, NCAT)).cuda()
    ctx.pmatrix(p["eig"], rates, p["blen"], pm, states=S, convention=plfx.PMAT_EIGEN)
    gen = torch.Generator(device="cuda").manual_seed(5)
    cat = NB.categories(n, gen)["sorted"]
    clv = [None] * p["ntips"] + [torch.empty(S * n, dtype=torch.float64, device="cuda")
                                 for _ in range(p["nslots"] - p["ntips"])]
    sums = torch.zeros(nops, dtype=torch.int64, device="cuda")
    return {("traversal fma" if fma else "traversal exact"): (lambda fma=fma: ctx.traverse_psr_gen(
        S, p["ops"], clv, pm, p["EV"], n, cat, NCAT, wgt=p["wgt"], scaler_sums=sums, tips=p["tips"], tipvec=p["tv"],
        fma=fma)) for fma in (False, True)}


def scan_variants(ctx, p, group):
    n = p["n"]
    size = plfx.psr_rate_scan_workspace_gen(plfx.F64, S, p["nops"], p["ntips"], p["nops"], n, group)
    free, _ = torch.cuda.mem_get_info()
    if size > 0.8 * free:
        say(f"  scan group {group}: workspace {size / 2**30:.1f} GiB does not fit {free / 2**30:.1f} GiB free: left out")
        return {}
    ws = torch.empty(size, dtype=torch.uint8, device="cuda")
    idx, best = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    out = torch.empty(1, dtype=torch.float64, device="cuda")
    return {f"scan group {group} {'fma' if fma else 'exact'}": (lambda fma=fma: ctx.psr_rate_scan_gen(
        S, p["ops"], p["tips"], p["blen"], p["eig"], p["EV"], p["tv"], p["cand"], n, ws, idx, best, group=group,
        freq=p["w"], wgt=p["wgt"], out_lnl=out, fma=fma)) for fma in (False, True)}


def trees(ctx, rounds, sites, groups):
    for n in sites:
        say(f"traversal and scan: balanced {SB.TAXA}-taxon tree, coded tips, f64, n = {n} sites")
        p = SB.problem(n)
        sets = [traversal_variants(ctx, p)] + [scan_variants(ctx, p, g) for g in groups]
        for variants in sets:
            if not variants:
                continue
            us = eager(variants, rounds)
            med = {}
            for name, v in us.items():
                med[name] = statistics.median(v)
                say(f"  {name:<22} median {med[name]:11.1f} us  min {min(v):11.1f}  max {max(v):11.1f}")
            e, f = (next(v for k, v in med.items() if k.endswith(w)) for w in ("exact", "fma"))
            say(f"  {next(iter(variants)).rsplit(' ', 1)[0]}: fma time / exact time = {f / e:.3f}")
            del variants
            torch.cuda.empty_cache()
        del p, sets
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sites", type=int, nargs="+", default=[10_000, 1 << 18])
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--parts", nargs="+", default=["node", "trees"], choices=["node", "trees"])
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("psr_prot_fma_bench needs a GPU")
    say(f"psr_prot_fma_bench: {S} states, f64, {a.rounds} rounds, {torch.cuda.get_device_name(0)}")
    with plfx.Context(0, lazy_tables=True) as ctx:
        if "node" in a.parts:
            node(ctx, a.calls, a.rounds)
        if "trees" in a.parts:
            trees(ctx, a.rounds, a.sites, a.groups)
    if a.log:
        Path(a.log).parent.mkdir(parents=True, exist_ok=True)
        Path(a.log).write_text("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
