"""Time the Stein-divergence pass (csrc/stein.hip) beside a torch restatement on the same card, beside the network forwards of the same
point, and against the HBM rate the same job sustains.

    python scripts/stein_bench.py [--reps 7] [--warmup 2] [--limit 240] [--out profiles/stein_bench.txt]       every shape, in turn
    python scripts/stein_bench.py --shape 1x4480x3072 ...                                                      one shape, this process

Without --shape this process touches no GPU: it starts one fresh child per shape under its own time limit (--limit seconds) and stops
at the first child that fails or runs out of time.  The lines are APPENDED to --out.

Shapes (P, M, D): (1, 1501, 100) a Euclidean config's point, (1, 4480, 3072) config 3's point, (8, 4480, 3072) eight of them.
Arms (a window is `calls` back-to-back calls between two device events; the figure is the window over `calls`, median over --reps):
  stein_rows        _lib.stein_rows, noise regenerated from the Philox stream, rows and sums preallocated (both launches)
  stein_rows_givenZ the same with Z read from memory
  colmean+stein     _lib.column_means (the fp64 means the spectrum centres with) and stein_rows: what the driver adds per launch group
  torch             the restatement: perturb_randn(z_out=Z) to materialise the noise, then (Z.double() * (S.double() - mean)).sum(-1) and
                    (Z.double() ** 2).sum(-1) -- a' and q only, no sums
  forwards          the score evaluations of the same P points: the 10dim fcn network on M rows (D = 100), config 3's NCSN++ on launch sets
                    of 2240 rows (D = 3072), random weights; wall clock around a synchronise
  hbm_copy          a 1 GiB device-to-device copy: the rate the card sustains in this job (read + write bytes over time)
"GBps" of the stein arms: the bytes the pass has to move (S read once: 4 P M D; given Z: twice that) over its time.  Before any timing
the Philox arm is compared bit for bit with the given-Z arm.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1501, 100), (1, 4480, 3072), (8, 4480, 3072))


def one_shape(args, emit):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import id_diff_amd  # noqa: F401
    from id_diff_amd import _lib, sde_lib
    from id_diff_amd.configs.utils import read_config
    from id_diff_amd.models import utils as mutils
    assert torch.cuda.is_available(), "stein_bench needs the MI355X"
    dev = torch.device("cuda:0")
    P, M, D = (int(v) for v in args.shape.split("x"))
    seeds = [1000003 * (p + 1) + 42 for p in range(P)]

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls * 1e3                                 # microseconds per call

    S = torch.randn(P, M, D, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 100.0 + 3.0
    Z = torch.empty(P, M, D, device=dev)
    x, std, out = torch.zeros(D, device=dev), torch.ones(M, device=dev), torch.empty(M, D, device=dev)

    def draw():
        for p in range(P):
            _lib.perturb_randn(x, std, None, out, M, D, 0, seeds[p], z_out=Z[p])
    draw()
    mean = _lib.column_means(S)
    rows, sums = torch.empty(P, M, 2, device=dev, dtype=torch.float64), torch.empty(P, 5, device=dev, dtype=torch.float64)
    seeds_dev = seeds                                                          # (the wrapper copies P integers per call: part of its cost)
    r1, s1 = (t.clone() for t in _lib.stein_rows(S, mean, seeds=seeds_dev, rows_out=rows, sums_out=sums))
    r2, s2 = _lib.stein_rows(S, mean, Z=Z, rows_out=rows, sums_out=sums)
    assert torch.equal(r1, r2) and torch.equal(s1, s2), "Philox and given-Z arms differ"
    want = (Z.double() * (S.double() - mean[:, None, :])).sum(-1)
    assert float((r1[..., 0] - want).abs().max()) <= 1e-9 * float(want.abs().max()), "kernel and restatement differ"
    del want

    def torch_arm():
        draw()
        a = (Z.double() * (S.double() - mean[:, None, :])).sum(-1)
        q = (Z.double() ** 2).sum(-1)
        return a, q

    arms = {"stein_rows": lambda: _lib.stein_rows(S, mean, seeds=seeds_dev, rows_out=rows, sums_out=sums),
            "stein_rows_givenZ": lambda: _lib.stein_rows(S, mean, Z=Z, rows_out=rows, sums_out=sums),
            "colmean+stein": lambda: _lib.stein_rows(S, _lib.column_means(S), seeds=seeds_dev, rows_out=rows, sums_out=sums),
            "torch": torch_arm}
    calls = 20 if P * M * D < 5e7 else 5
    med = {}
    for name, fn in arms.items():
        for _ in range(args.warmup):
            window(fn, calls)
        us = [window(fn, calls) for _ in range(args.reps)]
        med[name] = float(np.median(us))
        moved = 4.0 * P * M * D * (2 if name == "stein_rows_givenZ" else 1)
        emit(dict(shape=[P, M, D], arm=name, calls_per_window=calls, median_us=round(med[name], 2), min_us=round(min(us), 2),
                  max_us=round(max(us), 2), **({} if name == "torch" else {"GBps": round(moved / med[name] / 1e3, 1)})))

    # the card's streaming rate in this job
    n = 1 << 28
    src, dst = torch.empty(n, device=dev), torch.empty(n, device=dev)
    for _ in range(args.warmup):
        window(lambda: dst.copy_(src), 5)
    hbm = float(np.median([window(lambda: dst.copy_(src), 5) for _ in range(args.reps)]))
    hbm_rate = 8.0 * n / hbm / 1e3
    emit(dict(shape=[P, M, D], arm="hbm_copy", bytes_moved=8 * n, median_us=round(hbm, 2), GBps=round(hbm_rate, 1)))
    del src, dst

    # the forwards of the same point(s)
    cfg = read_config('configs/dimension_estimation/paper/' + ('euclidean_data/ksphere/10dim.py' if D == 100 else
                                                               'image_data/cifar_shaped/ncsnpp.py'))
    cfg.model.allow_random_init = True
    torch.manual_seed(0)
    model = mutils.create_model(cfg).to(dev).eval()
    sde, eps = sde_lib.configure_sde(cfg)
    score_fn = mutils.get_score_fn(sde, model)
    step = M if D == 100 else 2240
    shape = (D,) if D == 100 else (3, 32, 32)
    batch, t = torch.rand(step, *shape, device=dev), torch.full((step,), float(eps), device=dev)

    def forwards():
        with torch.no_grad():
            for _ in range(P * (M // step)):
                score_fn(batch, t)
    walls = []
    for i in range(args.warmup + min(args.reps, 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        forwards()
        torch.cuda.synchronize()
        if i >= args.warmup:
            walls.append((time.perf_counter() - t0) * 1e6)
    fwd = float(np.median(walls))
    emit(dict(shape=[P, M, D], arm="forwards", model=cfg.model.name, rows_per_launch=step, launches=P * (M // step), median_us=round(fwd, 1)))
    emit(dict(shape=[P, M, D], torch_over_stein=round(med["torch"] / med["stein_rows"], 2),
              stein_share_of_forwards=round(med["colmean+stein"] / fwd, 5),
              stein_rows_frac_of_hbm_copy_rate=round(4.0 * P * M * D / med["stein_rows"] / 1e3 / hbm_rate, 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default=None, help="PxMxD: time this shape in this process")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stein_bench.txt"))
    args = ap.parse_args()
    if args.shape is None:
        for shape in SHAPES:
            cmd = [sys.executable, os.path.abspath(__file__), "--shape", "x".join(map(str, shape)), "--reps", str(args.reps), "--warmup",
                   str(args.warmup), "--out", args.out]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc:
                raise SystemExit(f"stein_bench: shape {shape} ended with status {rc}; nothing further is started")
        return
    lines = []

    def emit(obj):
        line = obj if isinstance(obj, str) else json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    one_shape(args, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
