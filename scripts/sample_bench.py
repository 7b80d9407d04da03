"""Time the predictor-corrector sampler on the fcn score network: the fcn fast path of id_diff_amd.sampling beside what the pieces
that existed before it can do (``FCN.forward`` through ``get_score_fn`` plus the update as torch element-wise ops with
``torch.randn_like``), and the generic path of the sampler (``score_fn`` + one idiff_sampler_step_f32 per update), on the same weights.

    python scripts/sample_bench.py [--out profiles/sample_bench.txt] [--repeats 5]

Shapes: the paper's (1000 samples, D = 100, 5 x 2048, N = 1000, VE 0.01 .. 4, reverse_diffusion / none) and train_small's (1000 samples,
D = 8, 2 x 128, N = 1000).  Method: device events around the whole sampler, one warm-up of every arm, then ``repeats`` rounds in which the
arms alternate; the median is reported.  Weights are the seeded initialisation: the launches do not depend on their values.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import id_diff_amd  # noqa: E402,F401
from id_diff_amd import sampling, sde_lib  # noqa: E402
from id_diff_amd.configs.config_dict import ConfigDict  # noqa: E402
from id_diff_amd.models import utils as mutils  # noqa: E402
from id_diff_amd.models.fcn import FCN  # noqa: E402

SHAPES = {'paper (D=100, 5 x 2048)': dict(B=1000, D=100, H=2048, L=5, sigma_min=0.01, sigma_max=4.0),
          'train_small (D=8, 2 x 128)': dict(B=1000, D=8, H=128, L=2, sigma_min=0.1, sigma_max=2.0)}
N = 1000


def torch_sampler(model, sde, B, D, schedule):
    """The parent's pieces: FCN.forward behind get_score_fn, the update in torch element-wise ops, torch.randn_like for the noise."""
    score_fn = mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=True)
    dev = model.device
    ones = torch.ones(B, device=dev)
    times = torch.from_numpy(sampling.time_grid(sde, 1e-5)).to(dev)

    def run():
        with torch.no_grad():
            x = torch.randn(B, D, device=dev) * sde.sigma_max
            for i, step in enumerate(schedule):
                a, b, c = step['predictor']
                score = score_fn(x, ones * times[i])
                z = torch.randn_like(x)
                x_mean = a * x + b * score
                x = x_mean + c * z
        return x_mean

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sample_bench.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"sample_bench: {torch.cuda.get_device_name(0)}, N = {N} steps, reverse_diffusion / none, VE; device events around the whole "
             f"sampler, median of {args.repeats} after one warm-up, arms alternating", ""]
    for name, s in SHAPES.items():
        cfg = ConfigDict()
        cfg.model = ConfigDict(name='fcn', state_size=s['D'], hidden_layers=s['L'], hidden_nodes=s['H'], dropout=0.0)
        torch.manual_seed(0)
        model = FCN(cfg).to(dev).eval()
        sde = sde_lib.VESDE(sigma_min=s['sigma_min'], sigma_max=s['sigma_max'], N=N)
        sampler = sampling.get_pc_sampler(sde, (s['B'], s['D']), 'reverse_diffusion', 'none', 0.15, continuous=True, eps=1e-5)
        schedule = sampling.build_schedule(sde, 'reverse_diffusion', 'none', 0.15, 1, False, 1e-5)
        gemms = s['L'] + 2
        arms = {'fcn fast path': (lambda: sampler(model, seed=1, fast=True), f"{gemms} gemm + 1 step = {gemms + 1}"),
                'generic path': (lambda: sampler(model, seed=1, fast=False),
                                 f"score_fn ({gemms} gemm + concat + 2 fills + 6 element-wise) + 1 step = {gemms + 10}"),
                'torch update': (torch_sampler(model, sde, s['B'], s['D'], schedule),
                                 f"score_fn ({gemms} gemm + concat + 2 fills + 6 element-wise) + randn_like + 5 element-wise = {gemms + 15}")}
        times = {k: [] for k in arms}
        for k, (fn, _) in arms.items():
            fn()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for k, (fn, _) in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e-3)
        lines.append(f"{name}, {s['B']} samples")
        for k, (_, launches) in arms.items():
            med = statistics.median(times[k])
            lines.append(f"  {k:14s} {med:8.4f} s per {N}-step run  {med / N * 1e6:8.1f} us per step  (min {min(times[k]):.4f}, max {max(times[k]):.4f})"
                         f"  launches per step: {launches}")
        fast, torch_arm = statistics.median(times['fcn fast path']), statistics.median(times['torch update'])
        lines.append(f"  fast path vs torch update: {torch_arm / fast:.2f} x" + ("" if fast < torch_arm else "  -- the fast path is NOT faster here"))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
