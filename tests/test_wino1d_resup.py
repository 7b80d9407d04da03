"""The x2 FIR of the residual inside the row-wise convolution's tail (wino1d_kernel<8|16|32>, idiff_conv2d_wino1d_resup_f32,
_lib.with_residual_up2): the shortcut of an up block stays at the low resolution and Conv_1's finishing threads form their 16 pixels' values
from the low-resolution window themselves.  Against an fp64 restatement (fp64 convolution + fp64 upfirdn2d of the low-resolution residual,
then bias, out_scale, column sums) at the bar tests/test_hip_ops.py::test_conv2d_wino1d_vs_cpu sets for the plain-residual form, with the
two-launch path (upfirdn2d_raw, then the plain residual) held to the same bar on the same inputs; the window's edges against NaN-filled
neighbours; the refusals."""
import pytest
import torch
import torch.nn.functional as F

import id_diff_amd
from helpers import rel_err
from id_diff_amd import _lib
from oracle.ops import upfirdn2d_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
# tests/test_hip_ops.py::test_conv2d_wino1d_vs_cpu, the form with every epilogue term (residual included):
#   rel_err(out, ref) < 3e-6;  max |out - ref| < 1e-4 * max |ref|;  column sums: assert_close(rtol=1e-6, atol=1e-6) to those of the stored output
NORM_BAR, ELEM_BAR, SUMS_TOL = 3e-6, 1e-4, 1e-6
# (B, H = W, Cin, Cout): B = 3 leaves a partial last block at W = 8 and 16 (the rows_total guard: 8 / 2 images per block); Cout = 128: the second
# cout tile's channel offset; Cin = 32: the plain kernel's minimum of two K steps; W = 32: half a row per thread, a block is half an image
SHAPES = [(3, 8, 32, 64), (3, 16, 32, 128), (3, 32, 32, 128), (1, 32, 64, 64)]
UP = (2, 2, 1, 1, 2, 1, 2, 1)       # up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1 of NCSNpp._fir(..., "up")
PAD = 4096                          # floats of NaN on either side of the low-resolution residual (a multiple of 4: the buffer stays aligned)
_cache = {}


def _fir_kernel():
    k = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64)
    k = torch.outer(k, k)
    return (k / k.sum() * 4.0).float()


def _case(B, HW, Cin, Cout):
    """Once per shape: the inputs on the device (the low-resolution residual inside a NaN-filled allocation), the filter bank, and the fp64
    restatement conv + bias + FIR x2 of the residual, NHWC."""
    key = (B, HW, Cin, Cout)
    if key in _cache:
        return _cache[key]
    H = W = HW
    g = torch.Generator().manual_seed(1000 * HW + 10 * Cin + Cout + B)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g)
    lo = torch.randn(B, Cout, H // 2, W // 2, generator=g) + 1.0          # mean 1: a tap taken from a wrong place or dropped shows
    k = _fir_kernel()
    up = upfirdn2d_ref(lo.double(), k.double(), *UP)
    assert up.shape == (B, Cout, H, W)
    ref = (F.conv2d(x.double(), w.double(), b.double(), padding=1) + up).permute(0, 2, 3, 1).contiguous()
    n_lo = B * (H // 2) * (W // 2) * Cout
    big = torch.full((PAD + n_lo + PAD,), float("nan"), device=DEV)
    lod = big[PAD:PAD + n_lo]
    lod.copy_(lo.permute(0, 2, 3, 1).contiguous().view(-1).to(DEV))
    wt = w.permute(0, 2, 3, 1).contiguous().to(DEV)
    case = dict(xd=x.permute(0, 2, 3, 1).contiguous().to(DEV), u=_lib.wino1d_pack(wt, Cin, Cout), bd=b.to(DEV), lod=lod, big=big, kd=k.to(DEV),
                taps=_lib.polyphase_up2(k, 2, 1), ref=ref)
    _cache[key] = case
    return case


def _check(tag, out, ref, cs, B, HW, Cout):
    got = out.cpu().double()
    assert bool(torch.isfinite(got).all()), f"{tag}: a NaN from outside the low-resolution image reached the output"
    e_norm, e_elem = rel_err(got, ref), float((got - ref).abs().max()) / float(ref.abs().max())
    print(f"resup {tag}: rel err {e_norm:.3e} (bar {NORM_BAR:.0e}), max elementwise / max |ref| {e_elem:.3e} (bar {ELEM_BAR:.0e})")
    assert e_norm < NORM_BAR
    assert e_elem < ELEM_BAR
    if cs is not None:
        tot = cs.view(B, -1, Cout, 2).sum(1)
        o64 = out.double().reshape(B, HW * HW, Cout)
        torch.testing.assert_close(tot[..., 0], o64.sum(1), rtol=SUMS_TOL, atol=SUMS_TOL)
        torch.testing.assert_close(tot[..., 1], (o64 * o64).sum(1), rtol=SUMS_TOL, atol=SUMS_TOL)


@pytest.mark.parametrize("out_scale", [1.0, 0.5 ** 0.5])
@pytest.mark.parametrize("colstats", [False, True])
@pytest.mark.parametrize("B,HW,Cin,Cout", SHAPES)
def test_resup_vs_fp64_and_two_launch(B, HW, Cin, Cout, colstats, out_scale):
    c = _case(B, HW, Cin, Cout)
    H = W = HW
    assert _lib.conv2d_wino1d_resup_ok(B, H, W, Cin, Cout)
    ref = c["ref"] * out_scale
    ns = _lib.conv2d_wino1d_colstats_split(B, H, W, Cin, Cout)
    assert ns > 0
    sums = lambda: torch.full((B * ns * Cout * 2,), float("nan"), device=DEV, dtype=torch.float64) if colstats else None
    # one launch: the low-resolution residual into the tail
    cs = sums()
    out = torch.full((B, H, W, Cout), float("nan"), device=DEV)                # every output must be written
    ep = _lib.with_residual_up2(_lib.make_epilogue(bias=c["bd"], out_scale=out_scale, colstats=cs), c["lod"], c["taps"])
    _lib.conv2d_wino1d(c["xd"], c["u"], out, B, H, W, Cin, Cout, epilogue=ep)
    _check(f"B={B} {HW}x{HW} {Cin}->{Cout} colstats={int(colstats)} scale={out_scale:.3f} fused", out, ref, cs, B, HW, Cout)
    # two launches on the same inputs: the FIR pass writes the full-resolution residual, the plain tail reads it back
    cs2 = sums()
    full = torch.empty(B, H * W, Cout, device=DEV)
    _lib.upfirdn2d_raw(c["lod"].view(B, (H // 2) * (W // 2), Cout), c["kd"], full, B, H // 2, W // 2, Cout, *UP)
    two = torch.full((B, H, W, Cout), float("nan"), device=DEV)
    _lib.conv2d_wino1d(c["xd"], c["u"], two, B, H, W, Cin, Cout,
                       epilogue=_lib.make_epilogue(bias=c["bd"], residual=full, out_scale=out_scale, colstats=cs2))
    _check(f"B={B} {HW}x{HW} {Cin}->{Cout} colstats={int(colstats)} scale={out_scale:.3f} two-launch", two, ref, cs2, B, HW, Cout)
    torch.cuda.synchronize()
    assert bool(torch.isnan(c["big"][:PAD]).all()) and bool(torch.isnan(c["big"][-PAD:]).all())


def test_resup_refusals_launch_nothing():
    """Every refusal comes before any device call: the output, pre-filled with 7.0, is untouched."""
    B, Cin, Cout = 2, 32, 64
    bank = torch.zeros(_lib.lib().idiff_wino1d_weight_floats(Cin, Cout), device=DEV)
    taps = _lib.polyphase_up2(_fir_kernel(), 2, 1)
    x = torch.zeros(B * 64 * 64 * Cin, device=DEV)
    out = torch.full((B * 64 * 64 * Cout,), 7.0, device=DEV)
    lo_of = lambda H, W: torch.zeros(B * (H // 2) * (W // 2) * Cout, device=DEV)

    def refused(match, H, W, lo=None, ep=None):
        ep = _lib.make_epilogue() if ep is None else ep
        with pytest.raises(RuntimeError, match=match):
            _lib.conv2d_wino1d(x, bank, out, B, H, W, Cin, Cout, epilogue=_lib.with_residual_up2(ep, lo_of(H, W) if lo is None else lo, taps))
    refused("not served", 4, 4)
    refused("not served", 64, 64)
    refused("not served", 15, 16)                                                   # odd H
    refused("16-byte aligned", 16, 16, lo=torch.zeros(B * 64 * Cout + 4, device=DEV)[1:B * 64 * Cout + 1])
    refused("low-resolution residual of", 16, 16, lo=torch.zeros(B * 64 * Cout - 4, device=DEV))
    gamma = torch.ones(Cout, device=DEV)
    refused("cannot be combined", 16, 16, ep=_lib.with_groupnorm(_lib.make_epilogue(rows_per_group=256), 16, gamma, gamma, 1e-6, "silu"))
    with _lib.thread_option("IDIFF_NO_FUSED_RES_UP", 1):
        assert not _lib.conv2d_wino1d_resup_ok(B, 16, 16, Cin, Cout)
        refused("IDIFF_NO_FUSED_RES_UP", 16, 16)
    with pytest.raises(RuntimeError, match="already carries a residual"):
        _lib.with_residual_up2(_lib.make_epilogue(residual=lo_of(32, 32)), lo_of(16, 16), taps)
    ep = _lib.with_residual_up2(_lib.make_epilogue(), lo_of(16, 16), taps)
    with pytest.raises(RuntimeError, match="only conv2d_wino1d serves"):
        _lib.gemm(torch.zeros(64, 128, device=DEV), torch.zeros(128, 128, device=DEV), epilogue=ep)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused request must not launch"
