"""Timing of ``connect="closest"``, the repair of a disconnected neighbourhood graph: writes profiles/isomap_connect_bench.txt.

    python scripts/isomap_connect_bench.py [--out profiles/isomap_connect_bench.txt] [--sizes 1000 4096 12288]

Table 1, per N and per number of clusters (3-dimensional Gaussian blobs in 16 dimensions, 5 neighbours; C and p are what the graph
turns out to have): the first all-pairs shortest paths (knn_graph + geodesic_distances), component_labels, component_bridges,
repair_geodesics on either route, and the whole ``Isomap(5, 2, connect="closest").fit`` beside the fit of a connected set of the
same size (the Swiss roll of scripts/isomap_embed_bench.py, 10 neighbours), which has nothing to repair.

Table 2, per N: both routes against the share p / N of the points that are endpoints of an added edge, on made-up edges between
random points (the cost of either route depends on N and p alone).  The last column is update / full; the largest share at which it
is still <= 0.9 is printed per N, and the smallest of them over the sizes is what ``_lib.UPDATE_MAX_ENDPOINT_FRACTION`` is set to.

Wall times in ms around ``torch.cuda.synchronize()``: the median of 5 timed runs after one warm-up run.  The matrix a route
overwrites is cloned outside the timed region.
"""
import argparse
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import id_diff_amd
from id_diff_amd import _lib, isomap

RUNS = 5
SHARES = (0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.75, 1.0)


def clusters(n, c, seed, d_ambient=16, d_blob=3, spread=12.0):
    rng = np.random.default_rng(seed)
    sizes = [n // c + (i < n % c) for i in range(c)]
    pts = []
    for m in sizes:
        q, _ = np.linalg.qr(rng.standard_normal((d_ambient, d_blob)))
        pts.append(rng.standard_normal((m, d_blob)) @ q.T + spread * rng.standard_normal(d_ambient))
    P = np.concatenate(pts)
    return P[rng.permutation(n)].astype(np.float32)


def roll(n, seed):
    rng = np.random.default_rng(seed)
    t = 1.5 * np.pi * (1 + 2 * rng.random(n))
    pts = np.stack([t * np.cos(t), 21 * rng.random(n), t * np.sin(t)], axis=1)
    q, _ = np.linalg.qr(np.random.default_rng(7).standard_normal((12, 3)))
    return (pts @ q.T).astype(np.float32)


def timed(fn, setup=None):
    """Median wall time in ms of RUNS calls after one untimed warm-up call, and the last result; ``setup`` runs before each call,
    outside the timed region, and its result is the argument of ``fn``."""
    out = []
    for i in range(RUNS + 1):
        arg = setup() if setup else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn(arg) if setup else fn()
        torch.cuda.synchronize()
        if i:
            out.append(time.perf_counter() - t0)
    return statistics.median(out) * 1e3, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isomap_connect_bench.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 4096, 12288])
    ap.add_argument("--clusters", type=int, nargs="+", default=[3, 10, 30])
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    lines = [f"connect='closest': the repair of a disconnected 5-nearest-neighbour graph, {torch.cuda.get_device_name(0)}",
             f"milliseconds, wall time around a device synchronisation; median of {RUNS} timed runs after one warm-up",
             "",
             f"{'N':>6} {'blobs':>5} {'C':>4} {'p':>5} {'p/N':>6} {'first apsp':>10} {'labels':>7} {'bridges':>8} {'update':>8} {'full':>8} "
             f"{'fit closest':>11} {'fit connected':>13}"]
    for N in args.sizes:
        Xr = torch.from_numpy(roll(N, 1)).cuda()
        t_plain, _ = timed(lambda: isomap.Isomap(10, 2).fit(Xr))
        for c in args.clusters:
            X = torch.from_numpy(clusters(N, c, 100 + c)).cuda()
            dist, idx, _ = _lib.knn(X, 5)
            t_apsp, D0 = timed(lambda: _lib.geodesic_distances(_lib.knn_graph(dist, idx)))
            t_lab, (labels, count) = timed(lambda: _lib.component_labels(D0))
            C = int(count)
            if C < 2:
                lines.append(f"{N:>6} {c:>5} {C:>4}   (connected: nothing to repair)")
                continue
            t_bri, b = timed(lambda: _lib.component_bridges(X, labels, C))
            p = int(torch.unique(torch.cat(b[:2])).numel())
            t_upd, _ = timed(lambda D: _lib.repair_geodesics(D, *b, route="update"), setup=D0.clone)
            t_full, _ = timed(lambda: _lib.repair_geodesics(D0, *b, route="full", knn=(dist, idx)))
            t_fit, _ = timed(lambda: isomap.Isomap(5, 2, connect="closest").fit(X))
            lines.append(f"{N:>6} {c:>5} {C:>4} {p:>5} {p / N:>6.3f} {t_apsp:>10.2f} {t_lab:>7.2f} {t_bri:>8.2f} {t_upd:>8.2f} {t_full:>8.2f} "
                         f"{t_fit:>11.2f} {t_plain:>13.2f}")
            print(lines[-1], flush=True)
    lines += ["", "either route against the share of the points that are endpoints (made-up edges between random points of the 10-blob set)",
              f"{'N':>6} {'p':>6} {'p/N':>6} {'update':>9} {'full':>9} {'update / full':>13}"]
    best = {}
    for N in args.sizes:
        Xh = clusters(N, 10, 110)
        X = torch.from_numpy(Xh).cuda()
        dist, idx, _ = _lib.knn(X, 5)
        D0 = _lib.geodesic_distances(_lib.knn_graph(dist, idx))
        rng = np.random.default_rng(N)
        for share in SHARES:
            p = max(2, int(round(share * N)) // 2 * 2)
            ends = rng.permutation(N)[:p]
            bi, bj = ends[:p // 2], ends[p // 2:]
            bw = np.sqrt(((Xh[bi].astype(np.float64) - Xh[bj].astype(np.float64)) ** 2).sum(axis=1))
            b = (torch.from_numpy(bi).cuda(), torch.from_numpy(bj).cuda(), torch.from_numpy(bw).cuda())
            t_upd, _ = timed(lambda D: _lib.repair_geodesics(D, *b, route="update"), setup=D0.clone)
            t_full, _ = timed(lambda: _lib.repair_geodesics(D0, *b, route="full", knn=(dist, idx)))
            if t_upd <= 0.9 * t_full and best.get(N, 0.0) == (SHARES[SHARES.index(share) - 1] if SHARES.index(share) else 0.0):
                best[N] = share                                   # the largest share up to which EVERY smaller one qualified too
            lines.append(f"{N:>6} {p:>6} {p / N:>6.3f} {t_upd:>9.2f} {t_full:>9.2f} {t_upd / t_full:>13.3f}")
            print(lines[-1], flush=True)
    lines += ["", "largest measured p / N with update <= 0.9 full: " + ", ".join(f"N = {N}: {best.get(N, 0.0)}" for N in args.sizes),
              f"smallest over the sizes: {min(best.get(N, 0.0) for N in args.sizes)}   (_lib.UPDATE_MAX_ENDPOINT_FRACTION = "
              f"{_lib.UPDATE_MAX_ENDPOINT_FRACTION} in this tree)"]
    print("\n".join(lines[-2:]))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
