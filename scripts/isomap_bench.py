"""Time the stages of the Isomap reconstruction-error curve (id_diff_amd/isomap.py, csrc/geodesic.hip) on swiss-roll data.

    python scripts/isomap_bench.py [--sizes 1000 4096 8192] [--reps 5] [--warmup 1] [--no-scipy] [--out profiles/isomap_bench.txt]

Per N: the median of --reps timed windows after --warmup, device events around each window, of (a window of the two short stages,
knn_graph and double_center, holds as many back-to-back calls as fill about 20 ms, and the time is per call)
    knn_graph        idiff_knn_graph_f64 (fill, edges, symmetrise)
    apsp             idiff_apsp_f64, all 3 ceil(N / 64) launches; rate = 2 N^3 fp64 operations (N^3 adds, N^3 mins) per second, as a
                     fraction of an ASSUMED fp64 vector add/min peak: 256 CUs x 4 SIMDs x 16 lanes per clock x 2.4 GHz = 39.3 Tops/s.
                     MI355X_MICROARCH's table gives the fp32 vector rate only (157.3 TF = 32 lanes per clock, 2 operations per FMA);
                     that fp64 issues at half of it is this script's assumption (it agrees with AMD's published 78.6 TF fp64 vector
                     figure) and has not been measured in this project; an add or a min is one operation, not the two of an FMA.
                     The third phase does ((nt - 1) / nt)^2 of these operations, nt = ceil(N / 64), and its kernel cannot be slower
                     than the whole call: the call's rate times that share is a lower bound of the third phase's own rate (its
                     kernel time alone comes from a kernel trace, a run of its own).
    double_center    idiff_double_center_f64
    eigensolve       _lib.sym_eigvals on a copy of the centred kernel (the copy is outside the timed window)
With scipy importable, scipy.sparse.csgraph.shortest_path(directed=False) on the same graph is timed per N <= 4096: the median of 3
calls after one warm-up (host clock; it is single-threaded C whatever the thread pools are set to, and on this sparse graph its
method 'auto' is Dijkstra, O(N^2 k log N), far less work than the N^3 of Floyd-Warshall), and the ratio to `apsp` reported.
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

PEAK_TOPS = 256 * 4 * 16 * 2.4e9 / 1e12
N_NEIGHBORS = 10


def swiss_roll(N, seed):
    """The swiss roll of sklearn.datasets.make_swiss_roll, embedded in R^12 by a random isometry (fp32)."""
    rng = np.random.default_rng(seed)
    t = 1.5 * np.pi * (1 + 2 * rng.random(N))
    roll = np.stack([t * np.cos(t), 21 * rng.random(N), t * np.sin(t)], axis=1)
    q, _ = np.linalg.qr(rng.standard_normal((12, 3)))
    return (roll @ q.T).astype(np.float32)


def timed(fn, reps, warmup, setup=None, batch=False):
    """Median milliseconds per call of fn(setup()) over reps windows after warmup; setup runs outside the events.  ``batch``: a
    window holds as many back-to-back calls as fill about 20 ms (sized from the first warm-up window of one call)."""
    ms, inner = [], 1
    for i in range(warmup + reps):
        arg = setup() if setup is not None else None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn(arg)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b) / inner)
        elif batch and i == 0:
            inner = int(min(200, max(1, 20.0 / max(a.elapsed_time(b), 1e-3))))
    return float(np.median(ms)), [round(m, 4) for m in ms]


def bench(N, reps, warmup, with_scipy):
    X = torch.from_numpy(swiss_roll(N, N)).to("cuda")
    dist, idx, _ = _lib.knn(X, N_NEIGHBORS)
    row = dict(N=N, n_neighbors=N_NEIGHBORS)
    row["knn_graph_ms"], _ = timed(lambda _: _lib.knn_graph(dist, idx), reps, max(warmup, 2), batch=True)
    G = _lib.knn_graph(dist, idx)
    row["apsp_ms"], row["apsp_all_ms"] = timed(_lib.geodesic_distances, reps, warmup, setup=G.clone)
    nt = -(-N // _lib.APSP_TILE)
    tops = 2.0 * N ** 3 / (row["apsp_ms"] * 1e9)
    row["apsp_tops"], row["apsp_frac_peak"] = round(tops, 2), round(tops / PEAK_TOPS, 3)
    row["phase3_share_of_ops"] = round(((nt - 1) / nt) ** 2, 4)
    row["phase3_frac_peak_lower_bound"] = round(tops * ((nt - 1) / nt) ** 2 / PEAK_TOPS, 3)
    D = _lib.geodesic_distances(G.clone())
    row["connected"] = bool(torch.isfinite(D).all())
    if row["connected"]:
        row["double_center_ms"], _ = timed(lambda _: _lib.double_center(D), reps, max(warmup, 2), batch=True)
        K, _ = _lib.double_center(D)
        row["eigensolve_ms"], _ = timed(_lib.sym_eigvals, reps, warmup, setup=K.clone)
    if with_scipy and N <= 4096:
        try:
            from scipy.sparse import csr_matrix
            from scipy.sparse.csgraph import shortest_path
        except ImportError:
            row["scipy"] = "not importable"
        else:
            d, j = dist.cpu().numpy(), idx.cpu().numpy()
            g = csr_matrix((d.reshape(-1), (np.repeat(np.arange(N), N_NEIGHBORS), j.reshape(-1))), shape=(N, N))
            runs = []
            for _ in range(4):                                  # the first is the warm-up
                t0 = time.perf_counter()
                ref = shortest_path(g, directed=False)
                runs.append((time.perf_counter() - t0) * 1e3)
            row["scipy_shortest_path_ms"] = round(float(np.median(runs[1:])), 1)
            row["scipy_all_ms"] = [round(r, 1) for r in runs]
            row["scipy_over_apsp"] = round(row["scipy_shortest_path_ms"] / row["apsp_ms"], 2)
            got = D.cpu().numpy()
            fin = np.isfinite(ref)
            row["max_rel_diff_to_scipy"] = float((np.abs(got[fin] - ref[fin]) / np.maximum(ref[fin], 1e-300)).max())
            row["same_inf_pattern"] = bool(np.array_equal(np.isfinite(got), fin))
    for key in ("knn_graph_ms", "apsp_ms", "double_center_ms", "eigensolve_ms"):
        if key in row:
            row[key] = round(row[key], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 4096, 8192])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "isomap_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "isomap_bench needs the MI355X"
    lines = [f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, reps {args.reps}, warmup {args.warmup}, "
             f"assumed fp64 vector add/min peak {PEAK_TOPS:.1f} Tops/s"]
    print(lines[0], flush=True)
    for N in args.sizes:
        lines.append(json.dumps(bench(N, args.reps, args.warmup, not args.no_scipy)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
