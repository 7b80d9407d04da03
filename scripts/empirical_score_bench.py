"""Time the fused empirical-score kernel (csrc/empirical_score.hip) beside a chunked torch fp64 restatement on the same GPU.

    python scripts/empirical_score_bench.py [--reps 5] [--warmup 2] [--peak-binary PATH] [--out profiles/empirical_score_bench.txt]

Shapes (B, N, D): (1501, 8000, 100) one point's score matrix on the line's train split, (131072, 8000, 100) a whole launch group of
the driver, (131072, 40000, 100) the same on a cloud five times the size.  The cloud is the 'Line' curve (sin k t, k = 1 .. 100) at N
draws of t, the rows are points of it plus sigma = 0.2 noise.  Per shape, alternating in every repetition:

  kernel    one launch of idiff_empirical_score_f32 (out and ess preallocated; the cloud packed once, outside the window)
  torch     for row chunks of 2^26 / N rows: torch.cdist(x, X)^2 in fp64, softmax(-d2 / (2 sigma^2)), w @ X - x -- three library
            calls per chunk and a [chunk, N] fp64 matrix that goes to memory and back between them

A window is `calls` back-to-back calls between two device events, ended by a synchronise; the figure is the window over `calls`, median
over --reps after --warmup windows.  The two arms are compared on the same rows before anything is timed.  "TFLOP/s" is the 4 B N D
flops of the two products over that time -- a whole-call rate, exponentials, tile loads and tails included -- and "of measured peak"
divides it by the fp64 matrix rate scripts/mfma_peak.hip sustains on this card (random operands, the long run); the script builds that
program with hipcc unless --peak-binary names one.  The kernel pads D = 100 to 112 and N to a multiple of 32, so it issues more matrix
work than it is credited with here.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import id_diff_amd  # noqa: E402,F401
from id_diff_amd import _lib  # noqa: E402

SHAPES = [(1501, 8000, 100), (131072, 8000, 100), (131072, 40000, 100)]
SIGMA = 0.2


def measured_fp64_peak(binary):
    """TFLOP/s of the last 'fp64 16x16x4 random operands' line scripts/mfma_peak.hip prints, and the line itself."""
    with tempfile.TemporaryDirectory() as tmp:
        if binary is None:
            binary = os.path.join(tmp, "mfma_peak")
            subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3",
                            os.path.join(ROOT, "scripts", "mfma_peak.hip"), "-o", binary], check=True)
        text = subprocess.run([binary], check=True, capture_output=True, text=True, timeout=120).stdout
    rows = [ln for ln in text.splitlines() if ln.startswith("fp64 16x16x4 random operands")]
    return float(re.search(r"([\d.]+) TFLOP/s", rows[-1]).group(1)), rows[-1].strip()


def make(B, N, D):
    g = torch.Generator().manual_seed(N)
    t = torch.rand(N, generator=g)
    X = torch.sin(t[:, None] * torch.arange(1, D + 1, dtype=torch.float32)[None, :])
    x = X[torch.randint(N, (B,), generator=g)] + SIGMA * torch.randn(B, D, generator=g)
    return x.to("cuda").contiguous(), X.to("cuda").contiguous()


def torch_score(x, X64, out):
    chunk = max(256, (1 << 26) // X64.shape[0])
    for lo in range(0, x.shape[0], chunk):
        xc = x[lo:lo + chunk].double()
        w = torch.softmax(torch.cdist(xc, X64).square_().mul_(-0.5 / SIGMA ** 2), dim=1)
        out[lo:lo + chunk] = torch.addmm(xc, w, X64, beta=-1.0)
    return out


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls       # milliseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak-binary", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "empirical_score_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "empirical_score_bench needs the MI355X"
    lines = []

    def emit(obj):
        line = obj if isinstance(obj, str) else json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    emit(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, sigma = {SIGMA}")
    peak, peak_line = measured_fp64_peak(args.peak_binary)
    emit("scripts/mfma_peak.hip: " + peak_line)
    for B, N, D in SHAPES:
        x, X = make(B, N, D)
        pack = _lib.empirical_pack(X)
        X64 = X.double()
        sigma = torch.full((B,), SIGMA, device="cuda")
        out, ess = torch.empty_like(x), torch.empty(B, device="cuda")
        ref = torch.empty(B, D, device="cuda", dtype=torch.float64)
        arms = {"kernel": lambda: _lib.empirical_score(x, pack, sigma, None, out=out, ess=ess),
                "torch": lambda: torch_score(x, X64, ref)}
        arms["kernel"](), arms["torch"]()
        torch.cuda.synchronize()
        emit(dict(B=B, N=N, D=D, check="kernel against the torch fp64 restatement on the same rows",
                  max_abs_difference=float((out.double() - ref).abs().max()), max_abs_value=float(ref.abs().max()),
                  median_ess=float(ess.median())))
        flops = 4.0 * B * N * D
        calls = {"kernel": 20 if B < 10000 else 2, "torch": 5 if B < 10000 else 1}
        times = {name: [] for name in arms}
        for rep in range(args.warmup + args.reps):
            for name, fn in arms.items():
                ms = window(fn, calls[name])
                if rep >= args.warmup:
                    times[name].append(ms)
        base = float(np.median(times["torch"]))
        for name, ms in times.items():
            med = float(np.median(ms))
            emit(dict(B=B, N=N, D=D, arm=name, calls_per_window=calls[name], median_ms=round(med, 3), min_ms=round(min(ms), 3),
                      max_ms=round(max(ms), 3), TFLOPs=round(flops / (med * 1e-3) / 1e12, 2),
                      of_measured_fp64_matrix_peak=round(flops / (med * 1e-3) / 1e12 / peak, 3), torch_over_this=round(base / med, 2)))
        del x, X, X64, pack, out, ref
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
