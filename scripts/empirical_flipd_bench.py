"""Time FLIPD on the empirical score (csrc/empirical_flipd.hip) beside a torch fp64 restatement on the same card and beside the
scale curve of the Jacobian method, and ``jacobian.flipd`` of an fcn network beside the other two routes to the same points' ID.

    python scripts/empirical_flipd_bench.py --case a|b|c|d|e|paper|small [--reps 5] [--warmup 2] [--peak TFLOPS]
                                            [--out profiles/empirical_flipd_bench.txt]

One case a process (start each under its own time limit, and nothing after one that failed); the lines are APPENDED to --out.

Cloud cases (P queries, N points, D; the cloud is the 'Line' curve sin(k t), k = 1 .. D, at N draws of t; the queries are its first P
rows, each left out of its own softmax; S = 11 bandwidths base * 2^(j / 2), j = -4 .. 6, with base = 0.2 (D / 100)^1.5 (8000 / N), four
times the spacing of neighbours along the curve: 0.2 at the line config's shape):
  a (8000, 8000, 100)   b (100, 8000, 100: the split path)   c (8000, 40000, 100)   d (4000, 4000, 1024: the blobs' shape)
  e (10000, 10000, 3072)
Arms:
  kernel       _lib.empirical_flipd with the default splits, outputs and workspace preallocated; a window is `calls` back-to-back calls
               between two device events, the figure the window over `calls`
  torch_fp64   the restatement: per chunk of queries r^2 = |q|^2 + |y|^2 - 2 q y^T on the centred fp64 cloud (one fp64 matmul), its row
               minimum, and per bandwidth exp, the three sums and the two quotients; same window
  scale_curve  (D = 100 only) empirical.scale_curve on the same points and grid: a D x D matrix and an eigensolve per (point, sigma);
               wall clock around a synchronise, host copies included (as is flipd_curve, the like-for-like arm: `curve`)
"of the fp64 matrix rate": the 2 P N D flops of the distance product over the kernel's time, against --peak (what scripts/mfma_peak.hip
sustained in the same job; 77.8 TFLOP/s when not given).  The kernel also does P N S fp64 exponentials, which the matrix cores do not
help with: their rate is printed beside it.

Network cases (100 points of the unit sphere, random weights: the arithmetic does not depend on them): paper = configs/.../ksphere/10dim.py
(D = 100, 2048 x 5), small = configs/.../ksphere/train_small.py (D = 8, 128 x 2).  Arms, all wall clock around a synchronise, the
result copied to the host: flipd_exact, flipd_hutchinson (1 probe) and flipd_hutchinson_8, jacobian.local_dims, and the driver's
sampled path (scripts/fcn_jacobian_bench.py's loop).

Medians over --reps after --warmup.  Before any timing the kernel is compared with the restatement.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import id_diff_amd  # noqa: E402,F401
from id_diff_amd import _lib, empirical, jacobian  # noqa: E402

CLOUDS = {"a": (8000, 8000, 100), "b": (100, 8000, 100), "c": (8000, 40000, 100), "d": (4000, 4000, 1024), "e": (10000, 10000, 3072)}
NETS = ("paper", "small")
CHUNK_BYTES = 1 << 30                      # of one [rows, N] fp64 matrix of the restatement


def sigma_grid(N, D):
    return 0.2 * (D / 100.0) ** 1.5 * (8000.0 / N) * 2.0 ** (np.arange(-4, 7) / 2.0)


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


def make(N, D):
    t = torch.rand(N, generator=torch.Generator().manual_seed(N))
    return torch.sin(t[:, None] * torch.arange(1, D + 1, dtype=torch.float32)[None, :]).to("cuda").contiguous()


def torch_flipd(xq, pack, sg, exclude, flipd, ess):
    """The restatement in torch fp64, chunk by chunk of queries."""
    Y, h, c, D = pack["Y"], pack["h"], pack["c"], pack["D"]
    N = Y.shape[0]
    step = max(1, CHUNK_BYTES // (8 * N))
    inv2 = 0.5 / (sg.double() ** 2)
    for lo in range(0, xq.shape[0], step):
        q = xq[lo:lo + step].double() - c
        r2 = ((q * q).sum(dim=1, keepdim=True) + 2.0 * h[None, :] - 2.0 * (q @ Y[:, :D].T)).clamp_min_(0.0)
        rows = torch.arange(q.shape[0], device=xq.device)
        r2[rows, exclude[lo:lo + step]] = float("inf")
        m = r2.min(dim=1, keepdim=True).values
        r2f = torch.where(torch.isinf(r2), torch.zeros_like(r2), r2)
        for s in range(sg.numel()):
            e = torch.exp(-(r2 - m) * inv2[s])
            tot = e.sum(dim=1)
            flipd[lo:lo + step, s] = (e * r2f).sum(dim=1) / (tot * sg[s].double() ** 2)
            ess[lo:lo + step, s] = (tot * tot / (e * e).sum(dim=1)).float()


def cloud_case(args, emit):
    P, N, D = CLOUDS[args.case]
    SIGMAS = sigma_grid(N, D)
    S = len(SIGMAS)
    X = make(N, D)
    xq = X[:P].contiguous()
    pack = _lib.empirical_pack(X)
    sg = torch.from_numpy(SIGMAS.astype(np.float32)).to("cuda")
    exclude = np.arange(P)
    exd = torch.from_numpy(exclude).to("cuda")
    splits = _lib.empirical_flipd_splits(P, N, D)
    emit(f"case {args.case}: device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, P = {P} queries, N = {N}, D = {D}, "
         f"S = {S} bandwidths {np.round(SIGMAS, 4).tolist()}, splits = {splits}")
    ws = torch.empty(4 * P * S * splits, device="cuda", dtype=torch.float64)
    out = {k: (torch.empty(P, S, device="cuda", dtype=torch.float64), torch.empty(P, S, device="cuda")) for k in ("kernel", "torch_fp64")}
    device = {"kernel": lambda: _lib.empirical_flipd(xq, pack, sg, exclude=exclude, flipd=out["kernel"][0], ess=out["kernel"][1],
                                                     splits=splits, workspace=ws),
              "torch_fp64": lambda: torch_flipd(xq, pack, sg, exd, *out["torch_fp64"])}
    host = {"curve": lambda: empirical.flipd_curve(X, sigmas=SIGMAS, points=exclude)}
    if D == 100:
        host["scale_curve"] = lambda: empirical.scale_curve(X, sigmas=SIGMAS, points=exclude)
    for fn in device.values():
        fn()
    torch.cuda.synchronize()
    f, t = out["kernel"][0], out["torch_fp64"][0]
    emit(dict(case=args.case, check="kernel against the restatement: max |flipd - torch| / max(1, |torch|), and the same of the ESS",
              flipd=float(((f - t).abs() / t.abs().clamp_min(1.0)).max()),
              ess=float(((out["kernel"][1] - out["torch_fp64"][1]).abs() / out["torch_fp64"][1]).max()),
              median_flipd=[round(float(v), 3) for v in f.median(dim=0).values.tolist()],
              median_ess=[round(float(v), 1) for v in out["kernel"][1].median(dim=0).values.tolist()]))
    calls = {"kernel": 5, "torch_fp64": 1}
    times = {name: [] for name in list(device) + list(host)}
    for rep in range(args.warmup + args.reps):
        for name, fn in device.items():
            ms = window(fn, calls[name])
            if rep >= args.warmup:
                times[name].append(ms)
    for name, fn in host.items():                                        # seconds each at the large shapes: one warm-up, two timed
        for rep in range(3):
            ms = wall(fn)
            if rep >= 1:
                times[name].append(ms)
    med = {name: float(np.median(ms)) for name, ms in times.items()}
    flops, exps = 2.0 * P * N * D, float(P) * N * S
    for name, ms in times.items():
        row = dict(case=args.case, arm=name, P=P, N=N, D=D, S=S, median_ms=round(med[name], 3), min_ms=round(min(ms), 3),
                   max_ms=round(max(ms), 3))
        if name == "kernel":
            rate = flops / (med[name] * 1e-3) / 1e12
            row.update(distance_GFLOP=round(flops / 1e9, 1), TFLOPs=round(rate, 2), of_the_fp64_matrix_rate=round(rate / args.peak, 3),
                       peak_TFLOPs=args.peak, Gexp_per_s=round(exps / (med[name] * 1e-3) / 1e9, 1))
        emit(row)
    emit(dict(case=args.case, torch_over_kernel=round(med["torch_fp64"] / med["kernel"], 2),
              **({"scale_curve_over_curve": round(med["scale_curve"] / med["curve"], 1)} if "scale_curve" in med else {})))


def net_case(args, emit):
    from fcn_jacobian_bench import CASES, POINTS, sampled_dims
    from id_diff_amd import dim_reduction, sde_lib
    from id_diff_amd.configs.utils import read_config
    from id_diff_amd.models import utils as mutils
    from id_diff_amd.models.fcn import FCN
    dev = torch.device("cuda:0")
    config = read_config(CASES[args.case])
    config.device = "cuda:0"
    D, H, L, B = config.model.state_size, config.model.hidden_nodes, config.model.hidden_layers, config.training.batch_size
    emit(f"case {args.case}: device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {POINTS} points, D = {D}, "
         f"{L + 1} x Linear(., {H}) + ELU, loader batch {B}")
    torch.manual_seed(0)
    model = FCN(config).to(dev).eval()
    sde, eps = sde_lib.configure_sde(config)
    x = torch.randn(POINTS, D, generator=torch.Generator().manual_seed(1))
    x = (x / x.norm(dim=1, keepdim=True)).contiguous()
    xs = x.to(dev)
    points = [(row, B) for row in x]
    score_fn = mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=True)
    builder = dim_reduction.ScoreMatrixBuilder(score_fn, sde, eps, dev)
    arms = {"flipd_exact": lambda: jacobian.flipd(model, sde, xs).cpu(),
            "flipd_hutchinson": lambda: jacobian.flipd(model, sde, xs, exact=False, n_probes=1).cpu(),
            "flipd_hutchinson_8": lambda: jacobian.flipd(model, sde, xs, exact=False, n_probes=8).cpu(),
            "jacobian_local_dims": lambda: jacobian.local_dims(model, sde, xs),
            "sampled": lambda: sampled_dims(config, builder, points)}
    exact, h1, h8 = arms["flipd_exact"](), arms["flipd_hutchinson"](), arms["flipd_hutchinson_8"]()
    emit(dict(case=args.case, check="random weights: FLIPD (exact) min / median / max, and Hutchinson's deviation from it",
              exact=[round(float(v), 4) for v in (exact.min(), exact.median(), exact.max())],
              hutchinson_1_rms=round(float((h1 - exact).pow(2).mean().sqrt()), 4),
              hutchinson_8_rms=round(float((h8 - exact).pow(2).mean().sqrt()), 4)))
    times = {name: [] for name in arms}
    for rep in range(args.warmup + args.reps):
        for name, fn in arms.items():
            ms = wall(fn)
            if rep >= args.warmup:
                times[name].append(ms)
    med = {name: float(np.median(ms)) for name, ms in times.items()}
    for name, ms in times.items():
        emit(dict(case=args.case, arm=name, points=POINTS, D=D, median_ms=round(med[name], 3), min_ms=round(min(ms), 3),
                  max_ms=round(max(ms), 3)))
    emit(dict(case=args.case, local_dims_over_flipd_exact=round(med["jacobian_local_dims"] / med["flipd_exact"], 2),
              sampled_over_flipd_exact=round(med["sampled"] / med["flipd_exact"], 2),
              flipd_exact_over_hutchinson=round(med["flipd_exact"] / med["flipd_hutchinson"], 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=sorted(CLOUDS) + list(NETS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak", type=float, default=77.8, help="fp64 matrix TFLOP/s scripts/mfma_peak.hip sustained in the same job")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "empirical_flipd_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "empirical_flipd_bench needs the MI355X"
    lines = []

    def emit(obj):
        line = obj if isinstance(obj, str) else json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    (cloud_case if args.case in CLOUDS else net_case)(args, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
