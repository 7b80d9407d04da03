"""Time the sampling-free ID of an fcn network (csrc/fcn_jacobian.hip, jacobian.py) beside the sampled path it spares, and the fused
layer kernel beside the unfused route it replaces.

    python scripts/fcn_jacobian_bench.py --case paper|small [--reps 5] [--warmup 2] [--out profiles/fcn_jacobian_bench.txt]

One case a process (start each under its own time limit, and nothing after one that failed); the lines are APPENDED to --out.
Cases: paper = the paper's k-sphere shape (configs/.../ksphere/10dim.py: D = 100, Linear(101, 2048), 5 x Linear(2048, 2048),
Linear(2048, 100); loader batch 500, so 1501 score rows a point), small = configs/.../ksphere/train_small.py (D = 8, 128 x 2; batch 256,
769 rows a point).  Random weights (the arithmetic does not depend on them), 100 points of the unit sphere.  Per case:

  (a) jacobian     jacobian.local_dims end to end: forward of the centres, seed, layers, Gram, eigenvalues, host copy, the rule
      sampled      the driver's sampled path on the same points: the loop of dim_reduction.get_manifold_dimension (launch groups,
                   build_many, SpectrumPipeline, checked_spectra, estimate_dim) on a ScoreMatrixBuilder of the same network
      both a wall clock around a synchronise
  (b) layer_fused  one idiff_jvp_layer_f32 launch for the 100 points of a hidden layer (R = D rows a point, N = K = hidden_nodes)
      layer_batched   what it replaces: batched idiff_gemm_f32 with strideB = 0, then torch's g = where(a > 0, 1, a + 1) and the broadcast multiply
      layer_flat   the same with the points' rows stacked into ONE [P R, K] product (the weight is shared), then the same multiply
      layer_flat_fp32   layer_flat with idiff_gemm_f32 held to its fp32 arithmetic (IDIFF_NO_SPLIT for the launch): the like-for-like
                   route, since idiff_gemm_f32 otherwise cuts every operand into three bf16 pieces and runs on the bf16 matrix cores
      a window is `calls` back-to-back calls between two device events

Medians over --reps after --warmup.  A layer does 2 P R N K flops; its share of the 157 TFLOP/s fp32 matrix peak is printed.  Before
any timing the three layer routes are compared element-wise, and the dimensions both paths read are printed.
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
from id_diff_amd import _lib, dim_reduction, jacobian, sde_lib  # noqa: E402
from id_diff_amd.configs.utils import read_config  # noqa: E402
from id_diff_amd.models import utils as mutils  # noqa: E402
from id_diff_amd.models.fcn import FCN  # noqa: E402
from id_diff_amd.plot_utils import estimate_dim  # noqa: E402

KSPHERE = "configs/dimension_estimation/paper/euclidean_data/ksphere/"
CASES = {"paper": KSPHERE + "10dim.py", "small": KSPHERE + "train_small.py"}
POINTS = 100
FP32_MATRIX_PEAK = 157e12


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


def sampled_dims(config, builder, points):
    """The single-rank loop of dim_reduction.get_manifold_dimension behind its set-up: -> dims."""
    ids = list(range(len(points)))
    batched, groups = dim_reduction._launch_groups(config, points, ids)
    keep = [dim_reduction._sv_count(x.shape, b) for x, b in points]
    with torch.no_grad():
        pipe = dim_reduction.SpectrumPipeline(builder.device, overlap=True)
        for g in groups:
            pipe.submit(*dim_reduction._group_scores(builder, points, g, batched, lambda p: 42 + 1000003 * (p + 1)))
        local = [sv for block in pipe.results() for sv in block] if batched else pipe.results()
        local = torch.stack(local)
    return [estimate_dim(sv[:keep[p]].tolist()) if keep[p] >= 3 else -1 for sv, p in zip(dim_reduction.checked_spectra(local), ids)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fcn_jacobian_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fcn_jacobian_bench needs the MI355X"
    dev = torch.device("cuda:0")
    config = read_config(CASES[args.case])
    config.device = "cuda:0"
    D, H, L, B = config.model.state_size, config.model.hidden_nodes, config.model.hidden_layers, config.training.batch_size
    rows = dim_reduction.batching((D,), B)[2]          # of ONE un-batched sample, as the driver counts them
    lines = []

    def emit(obj):
        line = obj if isinstance(obj, str) else json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    emit(f"case {args.case}: device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {POINTS} points, D = {D}, "
         f"{L + 1} x Linear(., {H}) + ELU, loader batch {B} -> {rows} score rows a point")
    torch.manual_seed(0)
    model = FCN(config).to(dev).eval()
    sde, eps = sde_lib.configure_sde(config)
    x = torch.randn(POINTS, D, generator=torch.Generator().manual_seed(1))
    x = (x / x.norm(dim=1, keepdim=True)).contiguous()
    xs = x.to(dev)
    points = [(row, B) for row in x]
    score_fn = mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=True)
    builder = dim_reduction.ScoreMatrixBuilder(score_fn, sde, eps, dev)

    # ---- (b) the layer kernel alone
    P, R, N, K = POINTS, D, H, H
    g = torch.Generator(device=dev).manual_seed(2)
    A = torch.rand(P, R, K, device=dev, generator=g) * 2 - 1
    W = torch.rand(N, K, device=dev, generator=g) * 2 - 1
    act = torch.rand(P, N, device=dev, generator=g) * 1.9 - 0.95
    out = {name: torch.empty(P, R, N, device=dev) for name in ("layer_fused", "layer_batched", "layer_flat", "layer_flat_fp32")}

    def slope_times(c):
        return c.mul_(torch.where(act > 0, 1.0, act + 1.0)[:, None, :])

    def flat_fp32():
        with _lib.thread_option("IDIFF_NO_SPLIT", 1):
            _lib.gemm(A, W, out=out["layer_flat_fp32"], M=P * R, N=N, K=K, lda=K, ldb=K, ldc=N)
        return slope_times(out["layer_flat_fp32"])

    layer = {
        "layer_fused": lambda: _lib.jvp_layer(A, W, act=act, out=out["layer_fused"]),
        "layer_batched": lambda: slope_times(_lib.gemm(A, W, out=out["layer_batched"], M=R, N=N, K=K, lda=K, ldb=K, ldc=N, batch=P,
                                                       stride_a=R * K, stride_b=0, stride_c=R * N)),
        "layer_flat": lambda: slope_times(_lib.gemm(A, W, out=out["layer_flat"], M=P * R, N=N, K=K, lda=K, ldb=K, ldc=N)),
        "layer_flat_fp32": flat_fp32,
    }
    for fn in layer.values():
        fn()
    torch.cuda.synchronize()
    flat_route = lambda: _lib.gemm_route(A, W, out["layer_flat"], P * R, N, K, K, K, N)
    with _lib.thread_option("IDIFF_NO_SPLIT", 1):
        fp32_route = flat_route()
    emit(dict(case=args.case, idiff_gemm_f32_routes=dict(
        layer_batched=_lib.gemm_route(A, W, out["layer_batched"], R, N, K, K, K, N, batch=P, stride_a=R * K, stride_b=0, stride_c=R * N),
        layer_flat=flat_route(), layer_flat_fp32=fp32_route)))
    ref = (A.double() @ W.double().T) * torch.where(act > 0, 1.0, act.double() + 1.0)[:, None, :]
    mag = (A.double().abs() @ W.double().abs().T)
    emit(dict(case=args.case, check="layer routes against fp64: max |C - ref| / (K 2^-24 sum |a w|)",
              **{name: round(float(((c.double() - ref).abs() / (K * 2.0 ** -24 * mag)).max()), 4) for name, c in out.items()}))
    del ref, mag

    # ---- (a) the whole estimate
    whole = {"jacobian": lambda: jacobian.local_dims(model, sde, xs, eps), "sampled": lambda: sampled_dims(config, builder, points)}
    dj, ds = whole["jacobian"](), whole["sampled"]()
    values = sorted(set(dj.tolist()) | set(ds))
    emit(dict(case=args.case, check="dimensions read on random weights (value: points)", jacobian={int(v): int((dj == v).sum()) for v in values},
              sampled={int(v): int(sum(d == v for d in ds)) for v in values}))

    calls = 5
    times = {name: [] for name in list(layer) + list(whole)}
    for rep in range(args.warmup + args.reps):
        for name, fn in layer.items():
            ms = window(fn, calls)
            if rep >= args.warmup:
                times[name].append(ms)
        for name, fn in whole.items():
            ms = wall(fn)
            if rep >= args.warmup:
                times[name].append(ms)
    med = {name: float(np.median(ms)) for name, ms in times.items()}
    layer_flops = 2.0 * P * R * N * K
    # multiply-adds x 2: the tangent path pushes D rows a point through L hidden products and the output one, the sampled path `rows` rows
    # through all L + 2 products
    flops = {"jacobian": 2.0 * P * (D * (L * H * H + H * D) + (D + 1) * H + L * H * H + H * D),
             "sampled": 2.0 * P * rows * ((D + 1) * H + L * H * H + H * D)}
    for name, ms in times.items():
        row = dict(case=args.case, arm=name, points=P, D=D, H=H, median_ms=round(med[name], 3), min_ms=round(min(ms), 3),
                   max_ms=round(max(ms), 3))
        if name in layer:
            row.update(R=R, N=N, K=K, counted_GFLOP=round(layer_flops / 1e9, 2), TFLOPs=round(layer_flops / (med[name] * 1e-3) / 1e12, 2),
                       share_of_fp32_matrix_peak=round(layer_flops / (med[name] * 1e-3) / FP32_MATRIX_PEAK, 3))
        else:
            row.update(counted_GFLOP=round(flops[name] / 1e9, 1), TFLOPs=round(flops[name] / (med[name] * 1e-3) / 1e12, 2))
        emit(row)
    emit(dict(case=args.case, sampled_over_jacobian=round(med["sampled"] / med["jacobian"], 2),
              counted_flops_ratio=round(flops["sampled"] / flops["jacobian"], 1),
              layer_batched_over_fused=round(med["layer_batched"] / med["layer_fused"], 2),
              layer_flat_over_fused=round(med["layer_flat"] / med["layer_fused"], 2),
              layer_flat_fp32_over_fused=round(med["layer_flat_fp32"] / med["layer_fused"], 2),
              unfused_extra_bytes_per_layer=int(2 * 4 * P * R * N)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
