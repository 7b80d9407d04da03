"""What the GroupNorm + SiLU in the row-wise convolution's LOADER costs and saves at the benchmark's 32 x 32 shapes (B = 2240): one process,
HIP events, the forms interleaved.  A shape is ``Cin->Cout`` (one source) or ``C1+C2->Cout`` (GroupNorm_0 of cat[x1, x2], never made).
  two-launch: groupnorm_apply_colstats (gn_apply_rows_kernel; two sources: writes the concatenated, normalised tensor) + conv2d_wino1d
  loader:     groupnorm_coef (gn_coef_kernel) + conv2d_wino1d with the loader request (wino1d_nl_kernel / wino1d_nl2_kernel)
Median and range (min .. max) of the repetitions per form; the spread is the 10th .. 90th percentile range of {pass + conv} and of
{coefficients + loader} per repetition, the larger of the two; a class is routed (idiff_conv2d_wino1d_normload_ok /
idiff_conv2d_wino1d_normload_2src_ok) only where the loader form's gain is larger than that spread.
  python scripts/normload_shape_ab.py [B] [shape ...]
Without shapes: the one-source table of profiles/normload_shape_ab.txt; profiles/normload2_shape_ab.txt is 128+128->128 256+128->128."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import id_diff_amd
from id_diff_amd import _lib

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2240
REPS = 25
H = 32
SHAPES = sys.argv[2:] or ["128->128", "256->128", "256->256", "384->128"]
dev = "cuda"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    return e0, e1


def colsums(x):
    return torch.stack([x.double().sum(dim=1), (x.double() ** 2).sum(dim=1)], dim=-1).contiguous().view(-1)


print(f"B = {B}, 32 x 32, {REPS} interleaved repetitions, us per launch: median (min .. max)", flush=True)
for shape in SHAPES:
    cin, Cout = shape.split("->")
    C1, C2 = (int(c) for c in (cin + "+0").split("+")[:2])          # C2 = 0: one source
    Cin, Cout = C1 + C2, int(Cout)
    g = torch.Generator().manual_seed(C1 + 3 * C2 + Cout)
    x1 = (torch.randn(B, H * H, C1, generator=g) + 0.5).to(dev)
    x2 = (torch.randn(B, H * H, C2, generator=g) - 0.5).to(dev) if C2 else None
    u = _lib.wino1d_pack((torch.randn(Cout, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5).to(dev), Cin, Cout)
    bias, temb = torch.randn(Cout, generator=g).to(dev), torch.randn(B, Cout, generator=g).to(dev)
    gamma, beta = (torch.rand(Cin, generator=g) + 0.5).to(dev), torch.randn(Cin, generator=g).to(dev)
    n = torch.empty(B, H * H, Cin, device=dev)
    y, yf = (torch.empty(B, H * H, Cout, device=dev) for _ in range(2))
    cs1, (cs2, ns2) = colsums(x1), ((colsums(x2), 1) if C2 else (None, 0))
    coef = torch.empty(B * Cin * 2, device=dev)
    geom = (B, H, H, Cin, Cout)
    ep = dict(bias=bias, rowbias=temb, rows_per_group=H * H)
    forms = {
        "apply": lambda: _lib.groupnorm_apply_colstats(x1, C1, x2, C2, B, H * H, 32, cs1, 1, cs2, ns2, 1e-6, gamma, beta, "silu", n),
        "conv": lambda: _lib.conv2d_wino1d(n, u, y, *geom, epilogue=_lib.make_epilogue(**ep)),
        "coef": lambda: _lib.groupnorm_coef(cs1, 1, C1, cs2, ns2, C2, B, H * H, 32, 1e-6, gamma, beta, coef),
        "loader": lambda: _lib.conv2d_wino1d(x1, u, yf, *geom, epilogue=_lib.with_normload(_lib.make_epilogue(**ep), coef, "silu", x2, C1 if C2 else None)),
    }
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    err = float((y - yf).abs().max())
    ev = {k: [] for k in forms}
    for _ in range(REPS):
        for k, fn in forms.items():
            ev[k].append(timed(fn))
    torch.cuda.synchronize()
    ts = {k: sorted(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in ev.items()}
    med = {k: v[REPS // 2] for k, v in ts.items()}
    per_rep = lambda a, b: sorted(x0.elapsed_time(x1) * 1e3 + y0.elapsed_time(y1) * 1e3 for (x0, x1), (y0, y1) in zip(ev[a], ev[b]))
    lo, hi = REPS // 10, REPS - 1 - REPS // 10
    spread = max(s[hi] - s[lo] for s in (per_rep("apply", "conv"), per_rep("coef", "loader")))
    two, one = med["apply"] + med["conv"], med["coef"] + med["loader"]
    fmt = lambda k: f"{k} {med[k]:7.1f} ({ts[k][0]:7.1f} .. {ts[k][-1]:7.1f})"
    print(f"{shape:>12s} | {fmt('apply')}  {fmt('conv')}  = {two:7.1f} | {fmt('coef')}  {fmt('loader')}  = {one:7.1f} | "
          f"saved {two - one:7.1f} us ({(two - one) / two * 100:5.1f} %), spread {spread:6.1f}, loop slower by {(med['loader'] / med['conv'] - 1) * 100:5.1f} % | "
          f"max |two-launch - loader| {err:.2e}", flush=True)
