"""Time the simplex skewness (_lib.simplex_skewness, csrc/simplex.hip) beside local PCA and a torch restatement, and
``simplex.scale_curve`` end to end.

    python scripts/simplex_bench.py [--reps 5] [--warmup 2] [--out profiles/simplex_bench.txt]

Per case (N, D, k, scales), in ONE process: ``_lib.simplex_skewness``, ``_lib.local_pca(n_vectors=0)`` at the same (N, D, k) and a
chunked torch fp64 restatement of the skewness on the same card are timed in alternation -- one call of each per round, --reps
rounds after --warmup, so that a drift of the card's clocks reaches all three alike -- with CUDA events around the wrapper call (the
status read-back, which synchronises, is inside: it is part of every call).  Reported: the median and the spread (min .. max) of each,
the ``_lib.knn`` call that precedes them timed the same way, and ``simplex.scale_curve`` / ``simplex.local_dims`` by a host clock around
the whole call (kNN, kernel, read-back, inversion of the reference curve) with the share of kNN in it.
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
from id_diff_amd import _lib, simplex  # noqa: E402

CASES = [(80000, 100, 20, (20,)), (80000, 100, 64, (64,)), (80000, 100, 64, simplex.SCALES), (10000, 3072, 20, (20,))]
TORCH_BYTES = 1 << 30                 # most bytes of the fp64 [q, m, D] rows one chunk of the torch restatement gathers


def data(N, D, seed):
    """A 10-dimensional smooth manifold in R^D plus small noise (scripts/lpca_bench.py: the neighbour structure of the ID data)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, 10, generator=g)
    W = torch.randn(10, D, generator=g) / 10 ** 0.5
    return torch.tanh(z @ W) + 0.01 * torch.randn(N, D, generator=g)


def torch_skewness(X, centre, idx, scales):
    """``simplex.skewness_host`` in torch fp64 on the device, the queries in chunks."""
    Q, k = idx.shape
    out = torch.empty(Q, len(scales), 3, dtype=torch.float64, device=X.device)
    step = max(1, TORCH_BYTES // (8 * (k + 1) * X.shape[1]))
    for q0 in range(0, Q, step):
        c = centre[q0:q0 + step]
        Y = X[torch.cat([c[:, None], idx[q0:q0 + step]], dim=1)].double() - X[c].double()[:, None, :]
        G = Y @ Y.transpose(1, 2)
        for s, kk in enumerate(scales):
            m = kk + 1
            Gs = G[:, :m, :m]
            r = Gs.sum(dim=2) / m
            g = r.sum(dim=1) / m
            B = Gs - (r[:, :, None] + r[:, None, :]) + g[:, None, None]
            diag = torch.diagonal(B, dim1=1, dim2=2).clamp_min(0.0)
            nrm = diag.sqrt()
            i, j = torch.triu_indices(m, m, 1, device=X.device)
            area = (diag[:, i] * diag[:, j] - B[:, i, j] ** 2).clamp_min(0.0).sqrt().sum(dim=1)
            dot = B[:, i, j].abs().sum(dim=1)
            w = (nrm[:, i] * nrm[:, j]).sum(dim=1)
            out[q0:q0 + step, s, 0], out[q0:q0 + step, s, 1], out[q0:q0 + step, s, 2] = area / w, dot / w, w
    return out


def alternate(fns, reps, warmup):
    """One call of each function per round; ms per function over the timed rounds."""
    ms = [[] for _ in fns]
    for r in range(warmup + reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                ms[i].append(a.elapsed_time(b))
    return ms


def stat(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(min(ms), 3), max=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "simplex_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "simplex_bench needs the MI355X"
    lines = [f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {args.reps} alternating rounds after {args.warmup} "
             f"warm-up rounds; ms, CUDA events around the wrapper call (status read-back inside)"]
    print(lines[0], flush=True)
    for N, D, k, scales in CASES:
        X = data(N, D, D).to("cuda").contiguous()        # one data set per (N, D): the k = 20 and k = 64 rows compare
        ws = torch.empty((_lib.lib().idiff_knn_workspace_bytes(N, D, k) + 7) // 8, dtype=torch.float64, device=X.device)
        _, idx, _ = _lib.knn(X, k, workspace=ws)
        centre = torch.arange(N, dtype=torch.int64, device=X.device)
        got = _lib.simplex_skewness(X, centre, idx, scales)
        want = torch_skewness(X, centre, idx, scales)
        diff = float((got[..., :2] - want[..., :2]).abs().max())
        knn, skew, pca, tor = alternate([lambda: _lib.knn(X, k, workspace=ws), lambda: _lib.simplex_skewness(X, centre, idx, scales),
                                         lambda: _lib.local_pca(X, centre, idx, 0), lambda: torch_skewness(X, centre, idx, scales)],
                                        args.reps, args.warmup)
        e2e = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            simplex.scale_curve(X, scales)
            e2e.append((time.perf_counter() - t0) * 1e3)
        row = dict(N=N, D=D, k=k, scales=list(scales), knn_ms=stat(knn), simplex_ms=stat(skew), local_pca_ms=stat(pca),
                   torch_fp64_ms=stat(tor), simplex_over_local_pca=round(float(np.median(skew) / np.median(pca)), 3),
                   simplex_us_per_query=round(float(np.median(skew)) * 1e3 / N, 3), max_abs_diff_to_torch=diff,
                   scale_curve_ms=stat(e2e), knn_share_of_scale_curve=round(float(np.median(knn) / np.median(e2e)), 3))
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
        del X, ws, idx, got, want
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
