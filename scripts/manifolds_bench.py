"""Time the image-manifold renderers (csrc/manifolds.hip) and the data sets built on them; record the blobs' error.

    python scripts/manifolds_bench.py [--reps 7] [--warmup 2] [--n 500000] [--out profiles/manifolds_bench.txt]

1. Kernels: N = 500,000 images of 32 x 32, K = 10 and 100, both kernels.  Device events around each launch, median of
   --reps after --warmup.  Bytes WRITTEN per second (N S^2 4; the K values read per image are 1 % of that at K = 10,
   10 - 20 % at K = 100) as a fraction of the 6.3 TB/s a streaming kernel achieves on the MI355X.
2. Data sets: the whole ``FixedSquaresManifold(config)`` / ``FixedGaussiansManifold(config)`` construction -- tables,
   Mersenne-Twister stream, upload, rendering in slabs, download into the CPU tensor -- on a host clock, K = 10 and 100
   at N images, per image beside the reference's pixel loops (3.5 ms per squares image and 1.6 ms per blobs image at
   K = 10, measured with the reference's classes on the build machine's CPU).
3. The reference's algorithm on THIS machine's CPU: the reference itself is not part of this repository, so what is timed
   here is a restatement of its per-pixel Python loops (``img[i, j] += c`` on a torch tensor; one meshgrid + exp per blob),
   N = 64 images at K = 10.
4. Blobs: maximum error of the first 16 images of each blobs config against the reference's images
   (tests/golden/synthetic_manifolds.npz) and against the fp64 restatement, beside the bar (K + 4) 2^-24 max / (max - min).
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import id_diff_amd  # noqa: E402,F401
from id_diff_amd import _lib  # noqa: E402
from id_diff_amd.configs.utils import read_config  # noqa: E402
from id_diff_amd.lightning_data_modules import SyntheticDataset as sd  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
PAPER = "configs/dimension_estimation/paper/image_data/"
REFERENCE_MS_PER_IMAGE = {"squares": 3.5, "blobs": 1.6}        # the reference's classes at K = 10 on the build machine's CPU


def config(kind, K, n):
    cfg = read_config(PAPER + ("squares" if kind == "squares" else "gaussian_blobs") + f"/{K}.py")
    cfg.data.data_samples = n
    cfg.device = "cuda"
    return cfg


def tables(cfg, kind, K):
    rng = random.Random()
    if kind == "squares":
        table = sd.square_rects(sd.get_the_squares(cfg.seed, K, list(cfg.data.square_range), 32, rng=rng))
    else:
        table = np.asarray(sd.get_the_gaussian_centers(cfg.seed, K, list(cfg.data.std_range), 32, rng=rng))
    return table, sd.transplanted_stream(rng)


def time_kernel(kind, K, N, reps, warmup):
    cfg = config(kind, K, N)
    table, stream = tables(cfg, kind, K)
    u = stream.random_sample((N, K))
    values = torch.from_numpy(u.astype(np.float32) if kind == "squares" else 1 + 4 * u).to("cuda")
    out = torch.empty(N, 32, 32, device="cuda")
    fn = _lib.render_squares if kind == "squares" else _lib.render_gaussians
    for _ in range(warmup):
        fn(values, table, 32, out=out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(values, table, 32, out=out)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    med = float(np.median(ms))
    written = N * 32 * 32 * 4
    return dict(kernel=kind, N=N, S=32, K=K, median_ms=round(med, 3), ms=[round(m, 3) for m in ms],
                written_GBps=round(written / med / 1e6, 1), frac_of_6p3_TBps=round(written / (med * 1e-3) / HBM_ACHIEVABLE, 3),
                note="upload of the table (K * 12 bytes, synchronous) is inside the timed call")


def time_dataset(kind, K, N):
    cfg = config(kind, K, N)
    cls = sd.FixedSquaresManifold if kind == "squares" else sd.FixedGaussiansManifold
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ds = cls(cfg)
    dt = time.perf_counter() - t0
    assert tuple(ds.data.shape) == (N, 1, 32, 32) and ds.data.device.type == "cpu"
    row = dict(dataset=cls.__name__, N=N, K=K, construction_s=round(dt, 3), us_per_image=round(dt / N * 1e6, 3))
    if K == 10:
        row["reference_ms_per_image_build_machine_cpu"] = REFERENCE_MS_PER_IMAGE[kind]
        row["ratio"] = round(REFERENCE_MS_PER_IMAGE[kind] * 1e-3 / (dt / N), 0)
    return row


def pixel_loops(kind, K, n):
    """The reference's algorithm, restated: seconds per image of Python loops over pixels on this machine's CPU."""
    cfg = config(kind, K, n)
    table, stream = tables(cfg, kind, K)
    u = stream.random_sample((n, K))
    t0 = time.perf_counter()
    for i in range(n):
        img = torch.zeros(32, 32)
        for k in range(K):
            if kind == "squares":
                r0, c0, side = (int(v) for v in table[k])
                c = float(u[i, k])
                for a in range(side):
                    for b in range(side):
                        img[r0 + a, c0 + b] += c
            else:
                std = 1 + 4 * float(u[i, k])
                xx, yy = torch.meshgrid((torch.arange(32), torch.arange(32)), indexing="ij")
                new = np.exp(-1 / (2 * std ** 2) * ((xx - int(table[k][0])) ** 2 + (yy - int(table[k][1])) ** 2))
                new *= 1 / (np.sqrt(2 * np.pi) * std)
                img += new
        if kind == "blobs":
            lo, hi = torch.min(img), torch.max(img)
            img -= lo
            img /= hi - lo
    return (time.perf_counter() - t0) / n


def blobs_error(K):
    from test_hip_manifolds import blobs_bound, ref_blobs_f64
    z = np.load(os.path.join(ROOT, "tests", "golden", "synthetic_manifolds.npz"))
    cfg = config("blobs", K, 16)
    centres, stream = tables(cfg, "blobs", K)
    std = 1 + 4 * stream.random_sample((16, K))
    got = sd.render(cfg)[:, 0].cpu().numpy().astype(np.float64)
    ref, vmin, vmax = ref_blobs_f64(std, centres, 32)
    bar = blobs_bound(K, vmin, vmax)
    e_fix = np.abs(got - z[f"blobs{K}::images"]).reshape(16, -1).max(axis=1)
    e_ref = np.abs(got - ref).reshape(16, -1).max(axis=1)
    return dict(blobs_error=dict(K=K, images=16, max_vs_reference=float(e_fix.max()), max_vs_fp64_restatement=float(e_ref.max()),
                                 bar_min=float(bar.min()), bar_max=float(bar.max()),
                                 worst_ratio_to_bar_vs_reference=round(float(np.max(e_fix / bar)), 3),
                                 worst_ratio_to_bar_vs_fp64=round(float(np.max(e_ref / bar)), 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "manifolds_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "manifolds_bench needs the MI355X"
    lines = []

    def emit(obj):
        line = obj if isinstance(obj, str) else json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    emit(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    for kind in ("squares", "blobs"):
        for K in (10, 100):
            emit(time_kernel(kind, K, args.n, args.reps, args.warmup))
    for kind in ("squares", "blobs"):
        for K in (10, 100):
            emit(time_dataset(kind, K, args.n))
    for kind in ("squares", "blobs"):
        emit(dict(pixel_loop_restatement_on_this_cpu=dict(kind=kind, K=10, N=64, ms_per_image=round(pixel_loops(kind, 10, 64) * 1e3, 3),
                                                         note="the reference's classes are not in this repository: its algorithm restated")))
    for K in (10, 20, 100):
        emit(blobs_error(K))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
