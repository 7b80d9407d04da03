"""What the GroupNorm + SiLU applied by the FIR resampler to what it loads costs and saves at the benchmark's up / down blocks (B = 2240):
one process, HIP events, the forms interleaved.  A shape is ``up:HW:C`` or ``down:HW:C`` (the resampler's input map and channels).
  two-launch: groupnorm_apply_colstats (gn_apply_rows_kernel) + upfirdn2d_raw (upfirdn2d_nhwc_up2_block / upfirdn2d_nhwc_rows<0>)
  fused:      groupnorm_reader_coef (gn_coef_kernel) + upfirdn2d_gn (upfirdn2d_nhwc_up2_block_gn / upfirdn2d_nhwc_rows0_gn)
Median and range (min .. max) of the repetitions per form; the spread is the 10th .. 90th percentile range of {pass + FIR} and of
{coefficients + fused FIR} per repetition, the larger of the two; a class is routed only where the fused form's gain is larger than that
spread (the rule of scripts/normload_shape_ab.py).
  python scripts/gn_readers_shape_ab.py [B] [shape ...]
Without shapes: the six of the nf = 128 NCSN++ (profiles/gn_readers_shape_ab.txt)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import id_diff_amd
from id_diff_amd import _lib

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2240
REPS = 25
SHAPES = [s for s in sys.argv[2:] if not s.startswith("sc:")] or ([] if sys.argv[2:] else ["up:16:256", "up:8:256", "up:4:256", "down:32:128", "down:16:256", "down:8:256"])
MODES = {"up": (2, 1, 2, 1, 4.0), "down": (1, 2, 1, 1, 1.0)}
dev = "cuda"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    return e0, e1


def colsums(x):
    return torch.stack([x.double().sum(dim=1), (x.double() ** 2).sum(dim=1)], dim=-1).contiguous().view(-1)


print(f"B = {B}, {REPS} interleaved repetitions, us per launch: median (min .. max)", flush=True)
for shape in SHAPES:
    mode, HW, C = shape.split(":")
    H, C = int(HW), int(C)
    up, down, p0, p1, gain = MODES[mode]
    OH = _lib.upfirdn2d_out_size(H, up, down, p0, p1, 4)
    g = torch.Generator().manual_seed(H + 3 * C + (mode == "up"))
    x = (torch.randn(B, H * H, C, generator=g) + 0.5).to(dev)
    k = torch.outer(torch.tensor([1.0, 3.0, 3.0, 1.0]), torch.tensor([1.0, 3.0, 3.0, 1.0]))
    k = (k / k.sum() * gain).to(dev)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
    n = torch.empty(B, H * H, C, device=dev)
    y, yf = (torch.empty(B, OH * OH, C, device=dev) for _ in range(2))
    cs = colsums(x)
    coef = torch.empty(B * C * 2, device=dev)
    geom = (B, H, H, C, up, up, down, down, p0, p1, p0, p1)
    forms = {
        "apply": lambda: _lib.groupnorm_apply_colstats(x, C, None, 0, B, H * H, 32, cs, 1, None, 0, 1e-6, gamma, beta, "silu", n),
        "fir": lambda: _lib.upfirdn2d_raw(n, k, y, *geom),
        "coef": lambda: _lib.groupnorm_reader_coef(cs, 1, C, B, H * H, 32, 1e-6, gamma, beta, coef),
        "fused": lambda: _lib.upfirdn2d_gn(x, k, coef, "silu", yf, *geom),
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
    per_rep = lambda a, b: sorted(x0.elapsed_time(x1) * 1e3 + y0.elapsed_time(y1) * 1e3 for (x0, x1), (y0, y1) in zip(ev[a], ev[b]))
    lo, hi = REPS // 10, REPS - 1 - REPS // 10
    spread = max(s[hi] - s[lo] for s in (per_rep("apply", "fir"), per_rep("coef", "fused")))
    two, one = med["apply"] + med["fir"], med["coef"] + med["fused"]
    fmt = lambda k_: f"{k_} {med[k_]:7.1f} ({ts[k_][0]:7.1f} .. {ts[k_][-1]:7.1f})"
    print(f"{shape:>12s} | {fmt('apply')}  {fmt('fir')}  = {two:7.1f} | {fmt('coef')}  {fmt('fused')}  = {one:7.1f} | "
          f"saved {two - one:7.1f} us ({(two - one) / two * 100:5.1f} %), spread {spread:6.1f}, FIR slower by {(med['fused'] / med['fir'] - 1) * 100:5.1f} % | "
          f"max |two-launch - fused| {err:.2e}", flush=True)

# ---- an up block's 1x1 shortcut: FIR x2 then the GEMM (the reference's order) against the GEMM then FIR x2 (``sc:HW:Cin:Cout``)
SC_SHAPES = [s for s in sys.argv[2:] if s.startswith("sc:")] or ([] if sys.argv[2:] else ["sc:16:256:128", "sc:8:256:256", "sc:4:256:256"])
for shape in SC_SHAPES:
    _, HW, Cin, Cout = shape.split(":")
    H, Cin, Cout = int(HW), int(Cin), int(Cout)
    up, down, p0, p1, gain = MODES["up"]
    g = torch.Generator().manual_seed(H + Cin + Cout)
    x = torch.randn(B, H * H, Cin, generator=g).to(dev)
    w, bias = (torch.randn(Cout, Cin, generator=g) / Cin ** 0.5).to(dev), torch.randn(Cout, generator=g).to(dev)
    k = torch.outer(torch.tensor([1.0, 3.0, 3.0, 1.0]), torch.tensor([1.0, 3.0, 3.0, 1.0]))
    k = (k / k.sum() * gain).to(dev)
    xu, y = torch.empty(B, 4 * H * H, Cin, device=dev), torch.empty(B, 4 * H * H, Cout, device=dev)
    s, yf = torch.empty(B, H * H, Cout, device=dev), torch.empty(B, 4 * H * H, Cout, device=dev)
    fac = (up, up, down, down, p0, p1, p0, p1)
    forms = {
        "fir": lambda: _lib.upfirdn2d_raw(x, k, xu, B, H, H, Cin, *fac),
        "gemm": lambda: _lib.gemm(xu.view(-1, Cin), w, out=y.view(-1, Cout), epilogue=_lib.make_epilogue(bias=bias)),
        "gemm4": lambda: _lib.gemm(x.view(-1, Cin), w, out=s.view(-1, Cout), epilogue=_lib.make_epilogue()),
        "fir4": lambda: _lib.upfirdn2d_raw(s, k, yf, B, H, H, Cout, *fac),
    }
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    err = float((y - bias - yf).abs().max())
    ev = {k_: [] for k_ in forms}
    for _ in range(REPS):
        for k_, fn in forms.items():
            ev[k_].append(timed(fn))
    torch.cuda.synchronize()
    ts = {k_: sorted(a.elapsed_time(b) * 1e3 for a, b in v) for k_, v in ev.items()}
    med = {k_: v[REPS // 2] for k_, v in ts.items()}
    per_rep = lambda a, b: sorted(x0.elapsed_time(x1) * 1e3 + y0.elapsed_time(y1) * 1e3 for (x0, x1), (y0, y1) in zip(ev[a], ev[b]))
    lo, hi = REPS // 10, REPS - 1 - REPS // 10
    spread = max(q[hi] - q[lo] for q in (per_rep("fir", "gemm"), per_rep("gemm4", "fir4")))
    two, one = med["fir"] + med["gemm"], med["gemm4"] + med["fir4"]
    fmt = lambda k_: f"{k_} {med[k_]:7.1f} ({ts[k_][0]:7.1f} .. {ts[k_][-1]:7.1f})"
    print(f"{shape:>14s} | {fmt('fir')}  {fmt('gemm')}  = {two:7.1f} | {fmt('gemm4')}  {fmt('fir4')}  = {one:7.1f} | "
          f"saved {two - one:7.1f} us ({(two - one) / two * 100:5.1f} %), spread {spread:6.1f} | max |FIR-then-GEMM - GEMM-then-FIR| {err:.2e}", flush=True)
