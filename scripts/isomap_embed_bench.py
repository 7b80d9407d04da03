"""Timing of the Isomap embedding and of the out-of-sample transform: writes profiles/isomap_embed_bench.txt.

    python scripts/isomap_embed_bench.py [--out profiles/isomap_embed_bench.txt] [--sizes 1000 4096 12288]

Per N: ``Isomap(10, 2).fit(X)`` on a Swiss roll in 12 dimensions and ``transform`` of M = N fresh points of the roll, and beside
them, on the same matrices, ``_lib.geodesic_distances`` and ``_lib.sym_eigvals`` alone (both are part of ``fit``), the eigenvector
routine ``_lib.sym_topvecs`` alone, and the number of matrix products of its plan.  Wall times around ``torch.cuda.synchronize()``,
the median of the timed runs after one warm-up run at every size (three timed runs up to N = 4096, one at N = 12288).  No threshold is attached to any figure.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import id_diff_amd
from id_diff_amd import _lib, isomap


def roll(n, seed):
    rng = np.random.default_rng(seed)
    t = 1.5 * np.pi * (1 + 2 * rng.random(n))
    pts = np.stack([t * np.cos(t), 21 * rng.random(n), t * np.sin(t)], axis=1)
    q, _ = np.linalg.qr(np.random.default_rng(7).standard_normal((12, 3)))
    return (pts @ q.T).astype(np.float32)


def timed(fn, runs):
    """Median wall time in ms of ``runs`` calls after one untimed warm-up call, and the last result."""
    out = []
    for i in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        if i:
            out.append(time.perf_counter() - t0)
    return statistics.median(out) * 1e3, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isomap_embed_bench.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 4096, 12288])
    ap.add_argument("--n_neighbors", type=int, default=10)
    args = ap.parse_args()
    lines = [f"Isomap embedding and transform, {torch.cuda.get_device_name(0)}, n_neighbors = {args.n_neighbors}, n_components = 2, M = N",
             "milliseconds, wall time around a device synchronisation; median of the timed runs after one warm-up",
             f"{'N':>6} {'runs':>4} {'fit':>10} {'transform':>10} {'geodesics':>10} {'sym_eigvals':>11} {'sym_topvecs':>11} {'products':>8}  plan, residual / lambda_1"]
    for N in args.sizes:
        runs = 3 if N <= 4096 else 1
        X, Xq = torch.from_numpy(roll(N, 1)).cuda(), torch.from_numpy(roll(N, 2)).cuda()
        t_fit, iso = timed(lambda: isomap.Isomap(args.n_neighbors, 2).fit(X), runs)
        t_tr, _ = timed(lambda: iso.transform(Xq), runs)
        dist, idx, _ = _lib.knn(X, args.n_neighbors)
        t_geo, _ = timed(lambda: _lib.geodesic_distances(_lib.knn_graph(dist, idx)), runs)
        t_eig, lam = timed(lambda: _lib.sym_eigvals(_lib.double_center(iso.dist_matrix_)[0]), runs)
        lam = lam.cpu().numpy()
        K = _lib.double_center(iso.dist_matrix_)[0]
        t_top, _ = timed(lambda: _lib.sym_topvecs(K, 2, lam), runs)
        plan = iso.plan_
        lines.append(f"{N:>6} {runs:>4} {t_fit:>10.2f} {t_tr:>10.2f} {t_geo:>10.2f} {t_eig:>11.2f} {t_top:>11.2f} {plan['products']:>8}  "
                     f"p = {plan['p']}, degree {plan['degree']} x {plan['sweeps']} sweeps, {iso.residual_ / iso.eigenvalues_[0]:.2e}")
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
