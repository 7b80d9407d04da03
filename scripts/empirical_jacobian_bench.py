"""Time the sampling-free scale curve (csrc/empirical_jacobian.hip + the batched eigenvalues) beside the Monte-Carlo path it spares:
``empirical.local_dims`` once per bandwidth.

    python scripts/empirical_jacobian_bench.py --case a|b|c [--reps 5] [--warmup 2] [--out profiles/empirical_jacobian_bench.txt]

One case a process (start each under its own time limit, and nothing after one that failed); the lines are APPENDED to --out.
Cases (P points x S bandwidths, N, D): a (100 x 11, 8000, 100), b (100 x 11, 40000, 100), c (100 x 1, 8000, 192: the eigenvalues of
D > 128 take the matrices in turn).  The cloud is the 'Line' curve (sin k t, k = 1 .. D) at N draws of t, the points its first 100
rows, the bandwidths 0.2 * 2^(j / 2), j = -4 .. 6 (c: 0.2 alone).  Per case:

  kernel       one launch of idiff_empirical_jacobian_f64 for the P S queries (outputs preallocated)
  eigenvalues  _lib.sym_eigvals_batched on a copy of C made inside the window (the call overwrites its input; the copy is ~0.1 ms)
  spectra      empirical.jacobian_spectra end to end, host copies included (wall clock around a synchronise)
  monte_carlo  empirical.local_dims for the same points, once per bandwidth (wall clock around a synchronise)

kernel and eigenvalues: a window is `calls` back-to-back calls between two device events, the figure the window over `calls`; all
four: the median over --reps after --warmup.  "flops" credits the kernel with N D^2 + 3 N D multiply-adds a query (the upper
triangle of C twice over, the logits of both passes, the mean); the Monte-Carlo path does 4 rows N D a point, rows = the driver's.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import id_diff_amd  # noqa: E402,F401
from id_diff_amd import _lib, dim_reduction, empirical  # noqa: E402

CASES = {"a": (8000, 100, 11), "b": (40000, 100, 11), "c": (8000, 192, 1)}
POINTS = 100


def make(N, D):
    t = torch.rand(N, generator=torch.Generator().manual_seed(N))
    return torch.sin(t[:, None] * torch.arange(1, D + 1, dtype=torch.float32)[None, :]).to("cuda").contiguous()


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls       # milliseconds per call


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "empirical_jacobian_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "empirical_jacobian_bench needs the MI355X"
    N, D, S = CASES[args.case]
    sigmas = 0.2 * 2.0 ** (np.arange(-4, 7) / 2.0) if S > 1 else np.array([0.2])
    lines = []

    def emit(obj):
        line = obj if isinstance(obj, str) else json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    emit(f"case {args.case}: device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {POINTS} points x {S} bandwidths "
         f"{np.round(sigmas, 4).tolist()}, N = {N}, D = {D}")
    X = make(N, D)
    xq = X[:POINTS].repeat_interleave(S, dim=0).contiguous()
    sq = torch.from_numpy(sigmas.astype(np.float32)).to("cuda").repeat(POINTS)
    Q = xq.shape[0]
    C = torch.empty(Q, D, D, device="cuda", dtype=torch.float64)
    work = torch.empty_like(C)
    mean = torch.empty(Q, D, device="cuda", dtype=torch.float64)
    ess = torch.empty(Q, device="cuda")
    rows = dim_reduction.batching((D,), 500)[2]
    device = {"kernel": lambda: _lib.empirical_jacobian(xq, X, sq, C=C, mean=mean, ess=ess),
              "eigenvalues": lambda: _lib.sym_eigvals_batched(work.copy_(C))}
    host = {"spectra": lambda: empirical.jacobian_spectra(X, sigmas, points=np.arange(POINTS)),
            "monte_carlo": lambda: [empirical.local_dims(X, float(s), points=np.arange(POINTS)) for s in sigmas]}
    eig, e = host["spectra"]()
    dims = empirical.dims_from_jacobian(eig)
    mc = np.stack([empirical.local_dims(X, float(s), points=np.arange(POINTS))[0] for s in sigmas], axis=1)
    emit(dict(case=args.case, check="dimension 1 read at the listed share of the points, bandwidth by bandwidth",
              jacobian=[round(float((dims[:, s] == 1).mean()), 2) for s in range(S)],
              monte_carlo=[round(float((mc[:, s] == 1).mean()), 2) for s in range(S)],
              median_ess=[round(float(np.median(e[:, s])), 1) for s in range(S)]))
    calls = {"kernel": 5, "eigenvalues": 5 if D <= 128 else 1}
    times = {name: [] for name in list(device) + list(host)}
    for rep in range(args.warmup + args.reps):
        for name, fn in device.items():
            ms = window(fn, calls[name])
            if rep >= args.warmup:
                times[name].append(ms)
        for name, fn in host.items():
            ms = wall(fn)
            if rep >= args.warmup:
                times[name].append(ms)
    med = {name: float(np.median(ms)) for name, ms in times.items()}
    flops = {"kernel": 2.0 * Q * (N * D * D + 3.0 * N * D), "monte_carlo": 4.0 * S * POINTS * rows * N * D}
    for name, ms in times.items():
        row = dict(case=args.case, arm=name, queries=Q, N=N, D=D, median_ms=round(med[name], 3), min_ms=round(min(ms), 3),
                   max_ms=round(max(ms), 3))
        if name in flops:
            row.update(counted_GFLOP=round(flops[name] / 1e9, 1), TFLOPs=round(flops[name] / (med[name] * 1e-3) / 1e12, 2))
        emit(row)
    emit(dict(case=args.case, monte_carlo_over_spectra=round(med["monte_carlo"] / med["spectra"], 1),
              monte_carlo_over_kernel_plus_eigenvalues=round(med["monte_carlo"] / (med["kernel"] + med["eigenvalues"]), 1),
              counted_flops_ratio=round(flops["monte_carlo"] / flops["kernel"], 1), monte_carlo_rows_per_point=rows))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
