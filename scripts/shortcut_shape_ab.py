"""What one two-source contraction saves against two contractions with the partial product written and read back, at the benchmark's cat
shortcuts whose sources have different widths (B = 2240): one process, HIP events, the forms interleaved.  A shape is ``HW:C1:C2:Cout``.
  split:  gemm(x1, W[:, :C1]) + bias -> part;  gemm(x2, W[:, C1:]) + residual part      (two igemm_pipe_kernel launches)
  fused:  gemm_2src(x1, x2, W) + bias                                                   (one, each source at its own row pitch)
Median and range (min .. max) of the repetitions per form; the spread is the 10th .. 90th percentile range of {first + second GEMM} and of
the fused launch per repetition, the larger of the two; a class is routed only where the fused form's gain is larger than that spread (the
rule of scripts/gn_readers_shape_ab.py).
And what the x2 FIR of an up block's shortcut costs inside Conv_1's tail against the resampler's pass in front of it (``up:HW:Cin:Cout``, at
the end of this file), by the same rule.
  python scripts/shortcut_shape_ab.py [B] [shape ...]
Without shapes: the two cat shortcuts and the three up blocks of the nf = 128 NCSN++ (profiles/shortcut_shape_ab.txt)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import id_diff_amd
from id_diff_amd import _lib

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2240
REPS = 25
SHAPES = [s for s in sys.argv[2:] if not s.startswith("up:")] or ([] if sys.argv[2:] else ["32:256:128:128", "16:256:128:256"])
UP_SHAPES = [s for s in sys.argv[2:] if s.startswith("up:")] or ([] if sys.argv[2:] else ["up:4:256:256", "up:8:256:256", "up:16:256:256"])
dev = "cuda"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    return e0, e1


print(f"B = {B}, {REPS} interleaved repetitions, us per launch: median (min .. max)", flush=True)
for shape in SHAPES:
    H, C1, C2, Cout = (int(v) for v in shape.split(":"))
    M = B * H * H
    g = torch.Generator(device=dev).manual_seed(H + C1 + 3 * C2 + Cout)
    x1, x2 = torch.randn(M, C1, device=dev, generator=g), torch.randn(M, C2, device=dev, generator=g)
    w = torch.randn(Cout, C1 + C2, device=dev, generator=g) / (C1 + C2) ** 0.5
    bias = torch.randn(Cout, device=dev, generator=g)
    w1, w2 = w[:, :C1].contiguous(), w[:, C1:].contiguous()
    part, y, yf = (torch.empty(M, Cout, device=dev) for _ in range(3))
    forms = {
        "gemm1": lambda: _lib.gemm(x1, w1, out=part, epilogue=_lib.make_epilogue(bias=bias)),
        "gemm2": lambda: _lib.gemm(x2, w2, out=y, epilogue=_lib.make_epilogue(residual=part)),
        "fused": lambda: _lib.gemm_2src(x1, x2, w, yf, epilogue=_lib.make_epilogue(bias=bias)),
    }
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    rows = torch.arange(0, M, max(1, M // 4096), device=dev)
    ref = torch.cat([x1[rows], x2[rows]], 1).double() @ w.double().T + bias.double()
    e_split, e_fused = (float((t[rows].double() - ref).norm() / ref.norm()) for t in (y, yf))
    ev = {k_: [] for k_ in forms}
    for _ in range(REPS):
        for k_, fn in forms.items():
            ev[k_].append(timed(fn))
    torch.cuda.synchronize()
    ts = {k_: sorted(a.elapsed_time(b) * 1e3 for a, b in v) for k_, v in ev.items()}
    med = {k_: v[REPS // 2] for k_, v in ts.items()}
    both = sorted(a0.elapsed_time(a1) * 1e3 + b0.elapsed_time(b1) * 1e3 for (a0, a1), (b0, b1) in zip(ev["gemm1"], ev["gemm2"]))
    lo, hi = REPS // 10, REPS - 1 - REPS // 10
    spread = max(both[hi] - both[lo], ts["fused"][hi] - ts["fused"][lo])
    two, one = med["gemm1"] + med["gemm2"], med["fused"]
    fmt = lambda k_: f"{k_} {med[k_]:7.1f} ({ts[k_][0]:7.1f} .. {ts[k_][-1]:7.1f})"
    print(f"{shape:>16s} | {fmt('gemm1')}  {fmt('gemm2')}  = {two:7.1f} | {fmt('fused')} | "
          f"saved {two - one:7.1f} us ({(two - one) / two * 100:5.1f} %), spread {spread:6.1f} | "
          f"rel err vs fp64 on {rows.numel()} rows: split {e_split:.2e} fused {e_fused:.2e}", flush=True)
    del x1, x2, part, y, yf

# ---- an up block's shortcut (``up:HW:Cin:Cout``, HW the LOW-resolution map): the GEMM on the low-resolution rows is common to both forms
#   pass:   upfirdn2d_raw x2 (upfirdn2d_nhwc_up2_block) -> full-resolution shortcut;  Conv_1 (conv2d_wino1d) + residual
#   fused:  Conv_1 with the low-resolution shortcut upsampled in its tail (with_residual_up2)
# Conv_1 is Cout -> Cout at 2 HW x 2 HW with bias, out_scale 2^-1/2 and column sums, as NCSNpp._resblock launches it.
for shape in UP_SHAPES:
    _, HW, Cin, Cout = shape.split(":")
    h, Cin, Cout = int(HW), int(Cin), int(Cout)
    H = 2 * h
    g = torch.Generator(device=dev).manual_seed(h + Cin + Cout)
    x = torch.randn(B, h * h, Cin, device=dev, generator=g)
    w = torch.randn(Cout, Cin, device=dev, generator=g) / Cin ** 0.5
    hin = torch.randn(B, H * H, Cout, device=dev, generator=g)
    wt = torch.randn(Cout, 3, 3, Cout, device=dev, generator=g) / (9 * Cout) ** 0.5
    bias = torch.randn(Cout, device=dev, generator=g)
    k = torch.outer(torch.tensor([1.0, 3.0, 3.0, 1.0]), torch.tensor([1.0, 3.0, 3.0, 1.0]))
    k = k / k.sum() * 4.0
    taps, k = _lib.polyphase_up2(k, 2, 1), k.to(dev)
    u = _lib.wino1d_pack(wt, Cout, Cout)
    ns = _lib.conv2d_wino1d_colstats_split(B, H, H, Cout, Cout)
    cs = torch.empty(B * ns * Cout * 2, device=dev, dtype=torch.float64)
    lo, full = torch.empty(B, h * h, Cout, device=dev), torch.empty(B, H * H, Cout, device=dev)
    y, yf = (torch.empty(B, H * H, Cout, device=dev) for _ in range(2))
    rs = 0.5 ** 0.5
    forms = {
        "gemm": lambda: _lib.gemm(x.view(-1, Cin), w, out=lo.view(-1, Cout), epilogue=_lib.make_epilogue()),
        "fir": lambda: _lib.upfirdn2d_raw(lo, k, full, B, h, h, Cout, 2, 2, 1, 1, 2, 1, 2, 1),
        "conv": lambda: _lib.conv2d_wino1d(hin, u, y, B, H, H, Cout, Cout,
                                           epilogue=_lib.make_epilogue(bias=bias, residual=full, out_scale=rs, colstats=cs, rows_per_group=H * H)),
        "conv_up2": lambda: _lib.conv2d_wino1d(hin, u, yf, B, H, H, Cout, Cout, epilogue=_lib.with_residual_up2(
            _lib.make_epilogue(bias=bias, out_scale=rs, colstats=cs, rows_per_group=H * H), lo, taps)),
    }
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    err = float((y - yf).abs().max())
    ev = {k_: [] for k_ in forms}
    for _ in range(REPS):
        for k_, fn in forms.items():
            ev[k_].append(timed(fn))
    torch.cuda.synchronize()
    ts = {k_: sorted(a.elapsed_time(b) * 1e3 for a, b in v) for k_, v in ev.items()}
    med = {k_: v[REPS // 2] for k_, v in ts.items()}
    both = sorted(a0.elapsed_time(a1) * 1e3 + b0.elapsed_time(b1) * 1e3 for (a0, a1), (b0, b1) in zip(ev["fir"], ev["conv"]))
    lo_, hi_ = REPS // 10, REPS - 1 - REPS // 10
    spread = max(both[hi_] - both[lo_], ts["conv_up2"][hi_] - ts["conv_up2"][lo_])
    two, one = med["fir"] + med["conv"], med["conv_up2"]
    wgs = ((B * H * H + 511) // 512) * (Cout // 64)
    fmt = lambda k_: f"{k_} {med[k_]:7.1f} ({ts[k_][0]:7.1f} .. {ts[k_][-1]:7.1f})"
    print(f"{shape:>16s} | {fmt('gemm')} (common) | {fmt('fir')}  {fmt('conv')}  = {two:7.1f} | {fmt('conv_up2')} | "
          f"saved {two - one:7.1f} us ({(two - one) / two * 100:5.1f} %), spread {spread:6.1f} | tail longer by {med['conv_up2'] - med['conv']:6.1f} us "
          f"over {wgs} workgroups | max |pass - fused| {err:.2e}", flush=True)
    del x, hin, lo, full, y, yf
