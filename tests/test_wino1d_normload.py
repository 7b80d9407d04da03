"""GroupNorm (+ SiLU) applied in the LOADER of the row-wise F(4, 3) convolution on 32-pixel rows (wino1d_nl_kernel,
idiff_conv2d_wino1d_normload_f32, coefficients from idiff_groupnorm_coef_f32): the kernel against an fp64 restatement with the two-launch
path (groupnorm_apply_colstats, then the convolution the executor's route table picks) as the yardstick, and the executor step that uses it."""
import warnings

import pytest
import torch
import torch.nn.functional as F

import id_diff_amd
import normfused_cases
import normload_cases
from helpers import fill_from_seed, ncsnpp_config, rel_err
from id_diff_amd import _lib
from id_diff_amd.models import nhwc as hip_nhwc
from id_diff_amd.models import utils as mutils

pytestmark = pytest.mark.gpu
DEV = "cuda"
NET_RTOL = 2e-5                      # tests/test_hip_models.py
EPS = 1e-6
# The loader's path may be at most this many times as far from the fp64 restatement as the two-launch path on the same inputs, in the maximum
# and in the root mean square of the elementwise error: it rounds a x + b once where the pass rounds (x - mean) * s + t three times, and
# evaluates the same v_exp_f32 / v_rcp_f32 SiLU -- two more roundings per element at the most.  Measured: profiles/normload_parity.txt.
FUSED_VS_TWO_LAUNCH = 2.0
B, H, W = 3, 32, 32                  # an odd image count: the row blocks (16 rows) alternate top and bottom halves of an image
# Cin = 16: one K step (the loop is never entered), 48: three; Cout = 64 / 128: one and two tiles staging the same input
CASES = [(cin, cout, act) for cin in (16, 48) for cout in (64, 128) for act in ("silu", None)]
_cache = {}
_tol = {}                            # the absolute, reference-derived bound of tests/normfused_cases.py (the end-to-end chain's), per case


def _case(Cin, Cout, act):
    """Raw input with per-channel means of magnitude ~1.5 (so that a x + b has b != 0 even for beta = 0), beta of magnitude ~1 (silu(beta)
    != 0: a padding pixel that is not forced back to zero shows), the fp64 restatement, and both GPU paths' outputs [B, H, W, Cout]."""
    key = (Cin, Cout, act)
    if key in _cache:
        return _cache[key]
    G = Cin // 4
    g = torch.Generator().manual_seed(77 * Cin + Cout + (act is None))
    x = torch.randn(B, Cin, H, W, generator=g) * 1.3 + (torch.rand(1, Cin, 1, 1, generator=g) + 1.0) * torch.where(
        torch.rand(1, Cin, 1, 1, generator=g) < 0.5, -1.0, 1.0)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g)
    gamma = (torch.rand(Cin, generator=g) + 0.5) * torch.where(torch.rand(Cin, generator=g) < 0.5, -1.0, 1.0) * 1.4
    beta = (torch.rand(Cin, generator=g) * 0.6 + 0.7) * torch.where(torch.rand(Cin, generator=g) < 0.5, -1.0, 1.0)
    n = F.group_norm(x.double(), G, gamma.double(), beta.double(), EPS)
    n = F.silu(n) if act == "silu" else n
    ref = F.conv2d(n, w.double(), b.double(), padding=1).permute(0, 2, 3, 1).contiguous()
    _tol[key] = normfused_cases.chain_bound_conv(x, None, gamma, beta, G, w, b, act)[1]

    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)                      # the raw tensor, NHWC
    cs = normload_cases.colsums(xd.view(B, H * W, Cin))
    wt = w.permute(0, 2, 3, 1).contiguous().to(DEV)
    bd, gd, btd = b.to(DEV), gamma.to(DEV), beta.to(DEV)
    # two launches: the pass, then the 3x3 convolution on the route the executor takes for this geometry behind a GroupNorm
    normed = torch.empty(B, H * W, Cin, device=DEV)
    _lib.groupnorm_apply_colstats(xd.view(B, H * W, Cin), Cin, None, 0, B, H * W, G, cs, 1, None, 0, EPS, gd, btd, act, normed)
    two = torch.empty(B, H * W, Cout, device=DEV)
    route = hip_nhwc.conv3x3_route(B, H, W, Cin, Cout, True, True)
    if route is None:
        _lib.conv2d_nhwc(normed, wt, two, B, H, W, Cin, Cout, 3, 3, 1, 1, epilogue=_lib.make_epilogue(bias=bd))
        name = "igemm"
    else:
        form = route.form(B, H, W, Cin, Cout)
        bank = getattr(_lib, route.pack)(wt, Cin, Cout, **form)
        getattr(_lib, route.launch)(normed, bank, two, B, H, W, Cin, Cout, epilogue=_lib.make_epilogue(bias=bd), **form)
        name = route.name
    # one launch (+ the coefficients): the raw tensor into the loader
    coef = torch.full((B * Cin * 2,), float("nan"), device=DEV)
    _lib.groupnorm_coef(cs, 1, Cin, None, 0, 0, B, H * W, G, EPS, gd, btd, coef)
    fused = torch.full((B, H * W, Cout), float("nan"), device=DEV)       # every output must be written
    ep = _lib.with_normload(_lib.make_epilogue(bias=bd), coef, act)
    _lib.conv2d_wino1d(xd, _lib.wino1d_pack(wt, Cin, Cout), fused, B, H, W, Cin, Cout, epilogue=ep)
    torch.cuda.synchronize()
    out = (ref, two.cpu().double().view(B, H, W, Cout), fused.cpu().double().view(B, H, W, Cout), name)
    _cache[key] = out
    return out


@pytest.fixture
def small_batches(monkeypatch):
    normload_cases.small_batches(monkeypatch)


@pytest.mark.parametrize("Cin,Cout,act", CASES)
def test_normload_vs_fp64_and_two_launch(small_batches, Cin, Cout, act):
    """Every element against the fp64 restatement; the bar is the two-launch path's own error on the same inputs times
    FUSED_VS_TWO_LAUNCH, overall (maximum and rms) and separately on the image's first and last column and on rows 0, 15, 16, 31 (the
    image's edges and the two rows where a workgroup's block meets the other half of the image: the halo rows)."""
    ref, two, fused, name = _case(Cin, Cout, act)
    assert bool(torch.isfinite(fused).all())
    e_two, e_fused = (two - ref).abs(), (fused - ref).abs()
    max_two, max_fused = float(e_two.max()), float(e_fused.max())
    rms_two, rms_fused = float(e_two.pow(2).mean().sqrt()), float(e_fused.pow(2).mean().sqrt())
    print(f"normload_parity B={B} {H}x{W} {Cin}->{Cout} act={act} two-launch conv={name}: two-launch max {max_two:.3e} rms {rms_two:.3e} | "
          f"loader max {max_fused:.3e} rms {rms_fused:.3e} | ratio max {max_fused / max_two:.2f} rms {rms_fused / rms_two:.2f}")
    assert max_two > 0 and rms_two > 0
    # the yardstick itself is sane: fp32 rounding of values of size ~1
    assert max_two < 1e-4 * max(1.0, float(ref.abs().max()))
    assert max_fused <= FUSED_VS_TWO_LAUNCH * max_two
    assert rms_fused <= FUSED_VS_TWO_LAUNCH * rms_two
    # a padding pixel left at silu(b) or a halo row of the wrong image is an error of order 0.1 on these slices alone
    slices = {"col 0": e_fused[:, :, 0], "col 31": e_fused[:, :, 31], "row 0": e_fused[:, 0], "row 15": e_fused[:, 15],
              "row 16": e_fused[:, 16], "row 31": e_fused[:, 31]}
    for what, e in slices.items():
        assert float(e.max()) <= FUSED_VS_TWO_LAUNCH * max_two, what
    # a second view: the absolute, reference-derived bound of tests/normfused_cases.py, element by element
    assert float((e_fused / _tol[(Cin, Cout, act)]).max()) <= 1.0


def test_normload_query_switches_and_refusals():
    assert _lib.conv2d_wino1d_normload_ok(2, 32, 32, 128, 128) and _lib.conv2d_wino1d_normload_ok(2, 32, 32, 384, 128)
    assert not _lib.conv2d_wino1d_normload_ok(2, 32, 32, 256, 256)          # four cout tiles: measured no faster than the pass, not routed
    assert not _lib.conv2d_wino1d_normload_ok(2, 16, 16, 128, 128)          # rows of 16 pixels: the tail fusion's maps
    assert not _lib.conv2d_wino1d_normload_ok(2, 32, 32, 128, 96)
    for switch in ("IDIFF_NO_FUSED_GN_LOAD", "IDIFF_NO_PAIRS", "IDIFF_NO_WINO1D"):
        with _lib.thread_option(switch, 1):
            assert not _lib.conv2d_wino1d_normload_ok(2, 32, 32, 128, 128), switch
    assert _lib.conv2d_wino1d_normload_ok(2, 32, 32, 128, 128)
    x = torch.zeros(2, 256, 128, device=DEV)
    u = _lib.wino1d_pack(torch.zeros(128, 3, 3, 128, device=DEV), 128, 128)
    out = torch.full((2, 256, 128), 7.0, device=DEV)
    ep = _lib.with_normload(_lib.make_epilogue(), torch.zeros(2 * 128 * 2, device=DEV), "silu")
    with pytest.raises(RuntimeError, match="W = 32"):
        _lib.conv2d_wino1d(x, u, out, 2, 16, 16, 128, 128, epilogue=ep)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused request must not launch"
    with pytest.raises(RuntimeError, match="only conv2d_wino1d serves"):
        _lib.gemm(torch.zeros(64, 128, device=DEV), torch.zeros(128, 128, device=DEV), epilogue=ep)


@pytest.fixture
def counted(small_batches, monkeypatch):
    return normload_cases.counted(monkeypatch)


def _small_model():
    """nf = 32, two levels of 64 channels, two residual blocks per level, 32 x 32 input.  At 32 x 32: two blocks down (GroupNorm_0 of one
    source and GroupNorm_1 each: 4 norms read by one 3x3 convolution only), the down block (its GroupNorm_0 is read by the FIR: the pass
    stays; its Conv_0 and GroupNorm_1 are at 16 x 16), three blocks up on cat[h, skip] (GroupNorm_0 of two sources is the two-source form's, on
    under this file's switch too and counted apart as wino1d_nl2 / gn_coef2; GroupNorm_1 goes: 3) and the up block (GroupNorm_0 and the FIR at 16 x 16, Conv_0 -> GroupNorm_1 -> Conv_1 at 32 x 32: 1) -- 8 in all."""
    model = mutils.create_model(ncsnpp_config(**{"model.nf": 32, "model.ch_mult": (2, 2), "model.num_res_blocks": 2, "model.init_scale": 1.0}))
    fill_from_seed(model, 5)
    model.to(DEV)
    model._invalidate()
    g = torch.Generator().manual_seed(3)
    return model, torch.rand(2, 3, 32, 32, generator=g).to(DEV), torch.full((2,), 0.4, device=DEV)


def _on_and_off(model, x, t, calls):
    return normload_cases.on_and_off(model, x, t, calls, "IDIFF_NO_FUSED_GN_LOAD")


def test_small_ncsnpp_with_and_without_normload(counted):
    model, x, t = _small_model()
    on, off, c_on, c_off = _on_and_off(model, x, t, counted)
    print("normload model-level launches on / off:", c_on, c_off)
    assert c_off["wino1d_nl"] == 0 and c_off["gn_coef"] == 0, c_off
    assert c_on["wino1d_nl"] == 8 and c_on["gn_coef"] == 8, c_on
    assert c_off["gn_apply"] - c_on["gn_apply"] == 8, (c_on, c_off)
    assert c_on["wino1d"] == c_off["wino1d"], (c_on, c_off)            # the convolutions' own counters do not change
    assert bool(torch.isfinite(on).all())
    assert rel_err(on.cpu(), off.cpu()) < NET_RTOL


def test_inadmissible_gamma_leaves_the_loader_route(counted):
    """gamma x 500 on one GroupNorm_1 of a 32 x 32 block: sqrt(group size) * |gamma| is beyond the fp16 pairs' range, decided from the
    norm's own record (the tensor in memory is the raw one and says nothing): that layer keeps the pass and the fp32 route, and matches."""
    model, x, t = _small_model()
    blocks = [m for m in model.all_modules if hasattr(m, "GroupNorm_1")]
    with torch.no_grad():
        blocks[1].GroupNorm_1.weight.mul_(500.0)
    model._invalidate()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        on, off, c_on, c_off = _on_and_off(model, x, t, counted)
    print("normload inadmissible-gamma launches on / off:", c_on, c_off)
    assert c_on["wino1d_nl"] == 7 and c_off["wino1d_nl"] == 0, (c_on, c_off)
    assert c_off["gn_apply"] - c_on["gn_apply"] == 7, (c_on, c_off)
    assert c_on["wino1d"] == c_off["wino1d"], (c_on, c_off)
    assert bool(torch.isfinite(on).all())
    assert rel_err(on.cpu(), off.cpu()) < NET_RTOL
