"""Time local PCA (_lib.local_pca, csrc/lpca.hip) alone and ``lpca.local_dims`` end to end.

    python scripts/lpca_bench.py [--reps 5] [--warmup 2] [--host-queries 2000] [--out profiles/lpca_bench.txt]

Per case (N, D, k, n_vec): median of --reps timed calls after --warmup, CUDA events around the launch (the status read-back,
which synchronises, is inside: it is part of every call of the wrapper); the ``_lib.knn`` call that precedes the kernel,
timed the same way; ``lpca.local_dims`` by a host clock around the whole call (kNN, kernel, read-back, threshold rule);
``lpca.local_spectra_host`` (fp64 numpy, 16 BLAS threads) on the first --host-queries queries, scaled to N; and the bytes
the gather implies: N (k + 1) D 4 per pass over the rows (two passes with vectors) plus the fp64 results written.
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import id_diff_amd  # noqa: E402,F401
from id_diff_amd import _lib, lpca  # noqa: E402

CASES = [(80000, 100, 20, 0), (80000, 100, 64, 0), (80000, 100, 20, 10), (10000, 3072, 20, 0)]


def data(N, D, seed):
    """A 10-dimensional smooth manifold in R^D plus small noise (scripts/knn_bench.py: the neighbour structure of the ID data)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, 10, generator=g)
    W = torch.randn(10, D, generator=g) / 10 ** 0.5
    return torch.tanh(z @ W) + 0.01 * torch.randn(N, D, generator=g)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [round(m, 3) for m in ms]


def gather_bytes(N, D, k, n_vec):
    passes = 2 if n_vec else 1
    return passes * N * (k + 1) * D * 4 + N * min(k, D) * 8 + N * n_vec * D * 8 + N * (k + 1) * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-queries", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "lpca_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lpca_bench needs the MI355X"
    torch.set_num_threads(16)
    lines = [f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}; reps {args.reps} after {args.warmup} warm-up calls; "
             f"host restatement on {args.host_queries} queries scaled to N, 16 threads"]
    print(lines[0], flush=True)
    for si, (N, D, k, n_vec) in enumerate(CASES):
        X = data(N, D, si).to("cuda").contiguous()
        ws = torch.empty((_lib.lib().idiff_knn_workspace_bytes(N, D, k) + 7) // 8, dtype=torch.float64, device=X.device)
        knn_ms, _ = timed(lambda: _lib.knn(X, k, workspace=ws), args.reps, args.warmup)
        _, idx, _ = _lib.knn(X, k, workspace=ws)
        centre = torch.arange(N, dtype=torch.int64, device=X.device)
        ker_ms, ker_all = timed(lambda: _lib.local_pca(X, centre, idx, n_vec), args.reps, args.warmup)
        e2e = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lpca.local_dims(X, k)
            e2e.append((time.perf_counter() - t0) * 1e3)
        q = min(N, args.host_queries)
        Xh, idxh = X.cpu(), idx[:q].cpu()
        t0 = time.perf_counter()
        lpca.local_spectra_host(Xh, idxh, n_vectors=n_vec)
        host_s = (time.perf_counter() - t0) * N / q
        gb = gather_bytes(N, D, k, n_vec) / 1e9
        row = dict(N=N, D=D, k=k, n_vec=n_vec, knn_ms=round(knn_ms, 2), kernel_ms=round(ker_ms, 2), kernel_ms_all=ker_all,
                   kernel_us_per_query=round(ker_ms * 1e3 / N, 3), local_dims_ms=round(float(np.median(e2e)), 2),
                   host_restatement_s_scaled=round(host_s, 1), gather_GB=round(gb, 3), gather_GBps=round(gb / (ker_ms * 1e-3), 1))
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
        del X, ws, idx
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
