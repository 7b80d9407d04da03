"""What the GroupNorm in the row-wise convolution's tail costs and saves, per launch and per workgroup, at the benchmark's Conv_0 shapes
(B = 2240): one process, HIP events, the two forms interleaved.
  two-launch: conv2d_wino1d with column sums (wino1d_kernel) + groupnorm_apply_colstats (gn_apply_rows_kernel)
  fused:      conv2d_wino1d with the GroupNorm request (wino1d_gn_kernel)
and, for the tail alone, the plain convolution without column sums.  A workgroup is 512 pixels x 64 channels; the per-workgroup figure is
(fused - plain conv) x 256 CUs / workgroups, i.e. the launch's difference spread over the rounds of workgroups a CU executes.
Output: profiles/fused_gn_tail_cost.txt."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import id_diff_amd
from id_diff_amd import _lib

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2240
REPS = 30
SHAPES = [(16, 256, 256), (16, 512, 256), (16, 128, 128), (8, 256, 256), (8, 512, 256), (4, 256, 256), (4, 512, 256)]
dev = "cuda"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    return e0, e1


print(f"B = {B}, {REPS} interleaved repetitions, median us per launch; wg = workgroups of the launch, rounds = wg / 256 CUs")
print("shape             wg   rounds |  conv   conv+sums   gn_apply   two-launch |  fused |  saved per launch | fused tail - plain tail, per workgroup")
for H, Cin, Cout in SHAPES:
    g = torch.Generator().manual_seed(H + Cin)
    x = torch.randn(B, H * H, Cin, generator=g).to(dev)
    u = _lib.wino1d_pack((torch.randn(Cout, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5).to(dev), Cin, Cout)
    bias, temb = torch.randn(Cout, generator=g).to(dev), torch.randn(B, Cout, generator=g).to(dev)
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).to(dev), torch.randn(Cout, generator=g).to(dev)
    h, y, yf = (torch.empty(B, H * H, Cout, device=dev) for _ in range(3))
    cs = torch.empty(B * Cout * 2, device=dev, dtype=torch.float64)
    geom = (B, H, H, Cin, Cout)
    assert _lib.conv2d_wino1d_gn_ok(*geom, 32) and _lib.conv2d_wino1d_colstats_split(*geom) == 1
    ep = dict(bias=bias, rowbias=temb, rows_per_group=H * H)
    forms = {
        "conv": lambda: _lib.conv2d_wino1d(x, u, h, *geom, epilogue=_lib.make_epilogue(**ep)),
        "sums": lambda: _lib.conv2d_wino1d(x, u, h, *geom, epilogue=_lib.make_epilogue(colstats=cs, **ep)),
        "apply": lambda: _lib.groupnorm_apply_colstats(h, Cout, None, 0, B, H * H, 32, cs, 1, None, 0, 1e-6, gamma, beta, "silu", y),
        "fused": lambda: _lib.conv2d_wino1d(x, u, yf, *geom, epilogue=_lib.with_groupnorm(_lib.make_epilogue(**ep), 32, gamma, beta, 1e-6, "silu")),
    }
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in forms}
    for _ in range(REPS):
        for k, fn in forms.items():
            ev[k].append(timed(fn))
    torch.cuda.synchronize()
    t = {k: sorted(a.elapsed_time(b) * 1e3 for a, b in v)[REPS // 2] for k, v in ev.items()}
    wg = ((B * H * H + 511) // 512) * (Cout // 64)
    two = t["sums"] + t["apply"]
    print(f"{H:2d}x{H:<2d} {Cin:3d}->{Cout:3d} {wg:6d} {wg / 256:7.2f} | {t['conv']:6.1f} {t['sums']:10.1f} {t['apply']:10.1f} {two:12.1f} | {t['fused']:6.1f} |"
          f" {two - t['fused']:8.1f} ({(two - t['fused']) / two * 100:4.1f} %) | {(t['fused'] - t['conv']) * 256 / wg:6.2f} us"
          f"   (column sums: {(t['sums'] - t['conv']) * 256 / wg:5.2f} us)")
