"""Time the fused union-of-spheres score kernel (csrc/ksphere_union.hip) beside ``ksphere_exact.forward``.

    python scripts/ksphere_union_bench.py [--reps 9] [--warmup 3] [--out profiles/ksphere_union_bench.txt]

n = 100, sigma = 0.01 (labels 0), rows = points of the data set plus sigma * noise, B = 1501 (one point's score matrix at batch size
500) and B = 131072 (the most rows the vector configs hand a model at once).  Per B, alternating in every repetition:

  ksphere_exact.forward           the 10-sphere: two GEMMs, torch element-wise work, add_scale, affine_act and a host
                                  synchronisation on kappa.min() (about a dozen launches)
  union kernel, J = 1 / J = 2     one launch of idiff_ksphere_union_score_f32 on the 10-sphere / on the union [10, 30]; no host read
  union forward, J = 1 / J = 2    ``ksphere_union_exact.forward``: sigma, mult, the launch and the read of the refusal count

A window is `calls` back-to-back calls between two device events, ended by a synchronise; the figure is the window over `calls`,
median over --reps after --warmup windows.  "GB/s" is the bytes the kernel has to move (x read once, out written once: 8 B n) over
that time, beside the 6.3 TB/s a streaming kernel achieves on the MI355X.  Outputs of the J = 1 kernel and of ksphere_exact are
compared on the same rows before anything is timed.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import id_diff_amd  # noqa: E402,F401
from id_diff_amd import _lib  # noqa: E402
from id_diff_amd.configs.utils import read_config  # noqa: E402
from id_diff_amd.lightning_data_modules.KSphereDataset import KSphereDataset  # noqa: E402
from id_diff_amd.models import utils as mutils  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
KSPHERE = "configs/dimension_estimation/paper/euclidean_data/ksphere/"


def setup(J, B):
    cfg = read_config(KSPHERE + ("10dim.py" if J == 1 else "union.py"))
    cfg.data.data_samples = 512
    torch.manual_seed(0)
    pts = KSphereDataset(cfg).data
    x = pts[torch.randint(len(pts), (B,), generator=torch.Generator().manual_seed(1))]
    x = (x + 0.01 * torch.randn(x.shape, generator=torch.Generator().manual_seed(2))).to("cuda").contiguous()
    cfg.model.name = 'ksphere_union_exact'
    union = mutils.create_model(cfg).to("cuda").eval()
    exact = None
    if J == 1:
        cfg.model.name = 'ksphere_exact'
        exact = mutils.create_model(cfg).to("cuda").eval()
    return x, union, exact


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3        # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ksphere_union_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ksphere_union_bench needs the MI355X"
    lines = []

    def emit(obj):
        line = obj if isinstance(obj, str) else json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    emit(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, n = 100, sigma = 0.01")
    for B in (1501, 131072):
        calls = 200 if B == 1501 else 20
        arms = {}
        with torch.no_grad():
            for J in (1, 2):
                x, union, exact = setup(J, B)
                labels = torch.zeros(B, device="cuda")
                sigma = torch.full((B,), 0.01, device="cuda")
                mult = (-1.0 / sigma).contiguous()
                out, refused = torch.empty_like(x), torch.zeros(1, device="cuda", dtype=torch.int32)
                q = union.packed()["Q"]
                if exact is not None:
                    want, got = exact(x, labels), union(x, labels)
                    emit(dict(B=B, check="union J = 1 against ksphere_exact on the same rows",
                              max_abs_difference=float((want - got).abs().max()), max_abs_value=float(want.abs().max())))
                    arms["ksphere_exact.forward"] = (lambda m=exact, x=x, t=labels: m(x, t))
                arms[f"union kernel J={J}"] = (lambda x=x, q=q, c=union.comp, s=sigma, m=mult, o=out, r=refused:
                                               _lib.ksphere_union_score(x, q, c, s, m, out=o, refused=r))
                arms[f"union forward J={J}"] = (lambda m=union, x=x, t=labels: m(x, t))
            times = {name: [] for name in arms}
            for rep in range(args.warmup + args.reps):
                for name, fn in arms.items():
                    us = window(fn, calls)
                    if rep >= args.warmup:
                        times[name].append(us)
        base = float(np.median(times["ksphere_exact.forward"]))
        for name, us in times.items():
            med = float(np.median(us))
            emit(dict(B=B, arm=name, calls_per_window=calls, median_us=round(med, 2), min_us=round(min(us), 2), max_us=round(max(us), 2),
                      GBps=round(8.0 * B * 100 / med / 1e3, 1), frac_of_6p3_TBps=round(8.0 * B * 100 / (med * 1e-6) / HBM_ACHIEVABLE, 3),
                      ksphere_exact_over_this=round(base / med, 2)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
