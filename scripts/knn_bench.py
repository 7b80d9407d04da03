"""Time the exact self-kNN (_lib.knn, csrc/knn.hip) on the shapes of the paper's datasets.

    python scripts/knn_bench.py [--reps 5] [--warmup 2] [--no-sklearn]

Per shape (N, D, k): median of --reps timed calls after --warmup, CUDA events around each call (workspace allocated
once).  Gram TFLOP/s: 2 N^2 D (the useful contraction) and 2 Np^2 Dp (executed: rows padded to 128, D to 32) per
second, as fractions of the 157.3 TF fp32 matrix-core peak.  n_exact_rows: rows settled by the fp64 brute-force pass.
With sklearn importable, the ball tree of the reference (mle.py:19, n_jobs=1) is timed on the first shape: the tree
build, and kneighbors for the first 2,000 query rows, scaled to all N.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import id_diff_amd  # noqa: E402,F401
from id_diff_amd import _lib  # noqa: E402

PEAK_TF = 157.3
SHAPES = [(50000, 100, 21), (70000, 784, 21), (10000, 12288, 21)]


def data(N, D, seed):
    """A 10-dimensional smooth manifold in R^D plus small noise (the neighbour structure of the ID datasets)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, 10, generator=g)
    W = torch.randn(10, D, generator=g) / 10 ** 0.5
    return torch.tanh(z @ W) + 0.01 * torch.randn(N, D, generator=g)


def time_knn(X, k, reps, warmup):
    N, D = X.shape
    ws = torch.empty((_lib.lib().idiff_knn_workspace_bytes(N, D, k) + 7) // 8, dtype=torch.float64, device=X.device)
    for _ in range(warmup):
        _lib.knn(X, k, workspace=ws)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dist, idx, n_exact = _lib.knn(X, k, workspace=ws)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms, int(n_exact)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "knn_bench needs the MI355X"
    print(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    rows = []
    for si, (N, D, k) in enumerate(SHAPES):
        X = data(N, D, si).to("cuda").contiguous()
        med, ms, n_exact = time_knn(X, k, args.reps, args.warmup)
        Np, Dp = -(-N // 128) * 128, -(-D // 32) * 32
        useful, executed = 2.0 * N * N * D / (med * 1e9), 2.0 * Np * Np * Dp / (med * 1e9)
        row = dict(N=N, D=D, k=k, median_ms=round(med, 3), ms=[round(m, 3) for m in ms], gram_tflops=round(useful, 2),
                   gram_frac_peak=round(useful / PEAK_TF, 3), executed_tflops=round(executed, 2),
                   executed_frac_peak=round(executed / PEAK_TF, 3), n_exact_rows=n_exact)
        print(json.dumps(row), flush=True)
        rows.append(row)
        if si == 0 and not args.no_sklearn:
            try:
                from sklearn.neighbors import NearestNeighbors
            except ImportError:
                print("sklearn not importable: ball-tree timing skipped", flush=True)
                continue
            Xh = X.cpu().numpy()
            t0 = time.perf_counter()
            nn = NearestNeighbors(n_neighbors=k + 1, n_jobs=1, algorithm='ball_tree').fit(Xh)
            t1 = time.perf_counter()
            q = min(N, 2000)
            nn.kneighbors(Xh[:q])
            t2 = time.perf_counter()
            print(json.dumps(dict(sklearn_ball_tree=dict(N=N, D=D, k=k, build_s=round(t1 - t0, 3), query_rows=q,
                                                        query_s=round(t2 - t1, 3),
                                                        all_rows_s_scaled=round((t1 - t0) + (t2 - t1) * N / q, 1)))), flush=True)
    return rows


if __name__ == "__main__":
    main()
