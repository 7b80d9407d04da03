"""GroupNorm (+ SiLU) applied by the two NHWC resampling kernels to what they load (upfirdn2d_nhwc_up2_block_gn / upfirdn2d_nhwc_rows0_gn,
idiff_upfirdn2d_gn_f32, coefficients from idiff_groupnorm_coef_f32): the kernels against an fp64 restatement (F.group_norm -> act -> the
oracle's resampling) with the two-launch path (groupnorm_apply_colstats, then upfirdn2d_raw) as the yardstick, the refusals, and the
executor step of an up / down block that uses it."""
import pytest
import torch
import torch.nn.functional as F

import id_diff_amd
import normfused_cases
import normload_cases
from helpers import fill_from_seed, ncsnpp_config, rel_err
from id_diff_amd import _lib, sde_lib
from id_diff_amd.models import utils as mutils
from oracle import models as omodels, sde as osde
from oracle.ops import upfirdn2d_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
NET_RTOL = 2e-5                      # tests/test_hip_models.py
EPS = 1e-6
# As tests/test_wino1d_normload.py: the fused path may be at most this many times as far from the fp64 restatement as the two-launch path on
# the same inputs, in the maximum and in the root mean square of the elementwise error.  It rounds a x + b once where the pass rounds
# (x - mean) * s + t three times, evaluates the same v_exp_f32 / v_rcp_f32 SiLU, and sums the same taps in the same order.
FUSED_VS_TWO_LAUNCH = 2.0
B = 3
# (up, down, pad0, pad1) of the score networks' resamplers for the 4-tap FIR (models/ncsnpp.py, _fir) and the gain on its taps
MODES = {"up": (2, 1, 2, 1, 4.0), "down": (1, 2, 1, 1, 1.0)}
# maps of 4 x 4 (every pixel on the border) and 8 x 8; C = 8: two channel quads, 32 pixels per workgroup row; C = 64: sixteen quads
CASES = [(hw, c, mode, act) for hw in (4, 8) for c in (8, 64) for mode in ("up", "down") for act in ("silu", None)]
_cache = {}
_tol = {}                            # the absolute, reference-derived bound of tests/normfused_cases.py (the end-to-end chain's), per case


def _fir_taps(gain):
    k = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64)
    k = torch.outer(k, k)
    return (k / k.sum() * gain).float()


def _case(HW, C, mode, act):
    """Raw input with per-channel means of magnitude 1 - 2 and mixed signs, gamma of both signs, |beta| ~ 1 (silu(beta) != 0: a tap outside
    the image that is not an exact zero shows); the fp64 restatement and both GPU paths' outputs [B, OH, OW, C]."""
    key = (HW, C, mode, act)
    if key in _cache:
        return _cache[key]
    up, down, p0, p1, gain = MODES[mode]
    H = W = HW
    G = C // 4
    g = torch.Generator().manual_seed(1000 * HW + 10 * C + 2 * (mode == "up") + (act is None))
    sign = lambda *shape: torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)
    x = torch.randn(B, C, H, W, generator=g) * 1.3 + (torch.rand(1, C, 1, 1, generator=g) + 1.0) * sign(1, C, 1, 1)
    gamma = (torch.rand(C, generator=g) + 0.5) * sign(C) * 1.4
    beta = (torch.rand(C, generator=g) * 0.6 + 0.7) * sign(C)
    k = _fir_taps(gain)
    n = F.group_norm(x.double(), G, gamma.double(), beta.double(), EPS)
    n = F.silu(n) if act == "silu" else n
    ref = upfirdn2d_ref(n, k.double(), up, up, down, down, p0, p1, p0, p1).permute(0, 2, 3, 1).contiguous()
    OH, OW = ref.shape[1], ref.shape[2]
    assert OH == _lib.upfirdn2d_out_size(H, up, down, p0, p1, 4)
    _tol[key] = normfused_cases.chain_bound_fir(x, gamma, beta, G, mode, act)[1]

    xd = x.permute(0, 2, 3, 1).contiguous().view(B, H * W, C).to(DEV)        # the raw tensor, NHWC
    cs = normload_cases.colsums(xd)
    kd, gd, btd = k.to(DEV), gamma.to(DEV), beta.to(DEV)
    geom = (B, H, W, C, up, up, down, down, p0, p1, p0, p1)
    # two launches: the pass, then the resampler
    normed = torch.empty(B, H * W, C, device=DEV)
    _lib.groupnorm_apply_colstats(xd, C, None, 0, B, H * W, G, cs, 1, None, 0, EPS, gd, btd, act, normed)
    two = torch.full((B, OH * OW, C), float("nan"), device=DEV)
    _lib.upfirdn2d_raw(normed, kd, two, *geom)
    # one launch (+ the coefficients): the raw tensor into the resampler
    coef = torch.full((B * C * 2,), float("nan"), device=DEV)
    _lib.groupnorm_reader_coef(cs, 1, C, B, H * W, G, EPS, gd, btd, coef)
    fused = torch.full((B, OH * OW, C), float("nan"), device=DEV)             # every output must be written
    ok = _lib.upfirdn2d_gn_ok(xd, coef, act, fused, B, H, W, C, 4, 4, *geom[4:])
    route = _lib.upfirdn2d_route(xd, fused, B, H, W, C, 4, 4, *geom[4:])
    _lib.upfirdn2d_gn(xd, kd, coef, act, fused, *geom)
    torch.cuda.synchronize()
    out = (ref, two.cpu().double().view(B, OH, OW, C), fused.cpu().double().view(B, OH, OW, C), ok, route)
    _cache[key] = out
    return out


@pytest.mark.parametrize("HW,C,mode,act", CASES)
def test_fir_of_groupnorm_vs_fp64_and_two_launch(HW, C, mode, act):
    """Every element against the fp64 restatement; the bar is the two-launch path's own error on the same inputs times FUSED_VS_TWO_LAUNCH,
    overall (maximum and rms) and separately on the output's four edges, where taps fall outside the image."""
    ref, two, fused, ok, route = _case(HW, C, mode, act)
    # the query routes the measured classes only (up from 8 x 8 maps, down from 16 x 16); the launcher serves these smaller maps as well
    assert ok == (mode == "up" and HW >= 8)
    assert route ==("nhwc_up2_block" if mode == "up" else "nhwc_rows<0>")
    assert bool(torch.isfinite(fused).all())
    e_two, e_fused = (two - ref).abs(), (fused - ref).abs()
    max_two, max_fused = float(e_two.max()), float(e_fused.max())
    rms_two, rms_fused = float(e_two.pow(2).mean().sqrt()), float(e_fused.pow(2).mean().sqrt())
    print(f"fir_gn_parity B={B} {HW}x{HW} C={C} {mode} act={act}: two-launch max {max_two:.3e} rms {rms_two:.3e} | "
          f"fused max {max_fused:.3e} rms {rms_fused:.3e} | ratio max {max_fused / max_two:.2f} rms {rms_fused / rms_two:.2f}")
    assert max_two > 0 and rms_two > 0
    # the yardstick itself is sane: fp32 rounding of values of size ~1
    assert max_two < 1e-4 * max(1.0, float(ref.abs().max()))
    assert max_fused <= FUSED_VS_TWO_LAUNCH * max_two
    assert rms_fused <= FUSED_VS_TWO_LAUNCH * rms_two
    # a tap outside the image left at act(b) is an error of order 0.1 on these slices alone
    for what, e in {"row 0": e_fused[:, 0], "last row": e_fused[:, -1], "col 0": e_fused[:, :, 0], "last col": e_fused[:, :, -1]}.items():
        assert float(e.max()) <= FUSED_VS_TWO_LAUNCH * max_two, what
    # a second view: the absolute, reference-derived bound of tests/normfused_cases.py, element by element
    assert float((e_fused / _tol[(HW, C, mode, act)]).max()) <= 1.0


def test_fir_gn_query_switches_and_refusals():
    Bq, H, W, C = 2, 16, 16, 16
    x = torch.zeros(Bq, H * W, C, device=DEV)
    k = _fir_taps(1.0).to(DEV)
    coef = torch.zeros(Bq * C * 2, device=DEV)
    out_up = torch.full((Bq, 4 * H * W, C), 7.0, device=DEV)
    out_dn = torch.full((Bq, H * W // 4, C), 7.0, device=DEV)
    up, dn = (2, 2, 1, 1, 2, 1, 2, 1), (1, 1, 2, 2, 1, 1, 1, 1)
    ok = lambda x_, c_, act, o_, Bq_, H_, W_, C_, fac: _lib.upfirdn2d_gn_ok(x_, c_, act, o_, Bq_, H_, W_, C_, 4, 4, *fac)
    assert ok(x, coef, "silu", out_up, Bq, H, W, C, up) and ok(x, coef, None, out_dn, Bq, H, W, C, dn)
    with _lib.thread_option("IDIFF_NO_FUSED_GN_FIR", 1):
        assert not ok(x, coef, "silu", out_up, Bq, H, W, C, up) and not ok(x, coef, "silu", out_dn, Bq, H, W, C, dn)
    with _lib.thread_option("IDIFF_UFD_ROWS", 1):                          # the up resampler leaves the block kernel: not served
        assert not ok(x, coef, "silu", out_up, Bq, H, W, C, up)
    assert ok(x, coef, "silu", out_up, Bq, H, W, C, up)
    # the classes measured no faster than the pass are not routed (the launcher serves them: the parity cases above)
    assert ok(x, coef, "silu", out_up, Bq, 8, 8, C, up) and not ok(x, coef, "silu", out_up, Bq, 4, 4, C, up)
    assert not ok(x, coef, "silu", out_dn, Bq, 8, 8, C, dn)

    def refused(match, act, co, o, fac, Bq_=Bq, H_=H, W_=W, C_=C, x_=x):
        assert not ok(x_, co, act, o, Bq_, H_, W_, C_, fac)
        with pytest.raises(RuntimeError, match=match):
            _lib.upfirdn2d_gn(x_, k, co, act, o, Bq_, H_, W_, C_, *fac)

    refused("activation code", "relu", coef, out_up, up)
    refused("16-byte aligned", "silu", torch.zeros(Bq * C * 2 + 1, device=DEV)[1:], out_up, up)
    refused("this geometry takes nhwc_rows<1>", "silu", coef, out_up, (2, 2, 1, 1, 1, 2, 1, 2))        # up 2 with other pads
    refused("this geometry takes nhwc_rows<-1>", "silu", coef, out_up, (3, 3, 1, 1, 2, 1, 2, 1))       # up 3
    refused("with down 1x1", "silu", coef, out_up, (1, 1, 1, 1, 2, 2, 2, 2))                             # the plain FIR: nhwc_rows<0>, no decimation
    # channels that are no multiple of 4, and the NCHW view (minor = 1): no NHWC row kernel
    refused("this geometry takes", "silu", torch.zeros(Bq * 6 * 2, device=DEV), out_dn, dn, C_=6, x_=torch.zeros(Bq, H * W, 6, device=DEV))
    refused("this geometry takes", "silu", torch.zeros(Bq * 2, device=DEV), out_dn, dn, C_=1, x_=torch.zeros(Bq, H * W, 1, device=DEV))
    with pytest.raises(RuntimeError, match="coef holds"):
        _lib.upfirdn2d_gn(x, k, coef[:-2], "silu", out_up, Bq, H, W, C, *up)
    assert not _lib.upfirdn2d_gn_ok(x, 0, "silu", out_up, Bq, H, W, C, 4, 4, *up)                      # null coefficients
    torch.cuda.synchronize()
    assert bool((out_up == 7.0).all()) and bool((out_dn == 7.0).all()), "a refused request must not launch"


# ------------------------------------------------------------------------------------------------ the executor step
@pytest.fixture
def counted(monkeypatch):
    normload_cases.small_batches(monkeypatch)
    calls = {"gn_apply": 0, "fir": 0, "fir_gn": 0, "reader_coef": 0, "loader_coef": 0}
    for key, name in (("gn_apply", "groupnorm_apply_colstats"), ("fir", "upfirdn2d_raw"), ("fir_gn", "upfirdn2d_gn"),
                      ("reader_coef", "groupnorm_reader_coef"), ("loader_coef", "groupnorm_coef")):
        def wrapper(*a, _orig=getattr(_lib, name), _key=key, **kw):
            calls[_key] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(_lib, name, wrapper)
    return calls


def _small_model():
    """nf = 64, two levels of 128 channels, two residual blocks per level, attention at 16 x 16, 32 x 32 input, B = 2: one down block
    (GroupNorm_0 + SiLU at 32 x 32 read by the FIR :2) and one up block (at 16 x 16, read by the FIR x2).  Returns the score function on
    the GPU, the inputs and the CPU oracle's score (computed once)."""
    if "model" in _cache:
        return _cache["model"]
    cfg = ncsnpp_config(**{"model.nf": 64, "model.ch_mult": (2, 2), "model.num_res_blocks": 2, "model.init_scale": 1.0})
    torch.manual_seed(0)
    ref_model = omodels.create_model(cfg)
    fill_from_seed(ref_model, 5)
    g = torch.Generator().manual_seed(11)
    resampling = [m for m in ref_model.all_modules if getattr(m, "up", False) or getattr(m, "down", False)]
    assert len(resampling) == 2
    with torch.no_grad():
        for m in resampling:                  # gamma of both signs, |beta| ~ 1 on the two norms in question
            C = m.GroupNorm_0.weight.numel()
            sign = lambda: torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
            m.GroupNorm_0.weight.copy_((torch.rand(C, generator=g) + 0.5) * sign())
            m.GroupNorm_0.bias.copy_((torch.rand(C, generator=g) * 0.6 + 0.7) * sign())
    model = mutils.create_model(cfg)
    model.load_state_dict(ref_model.state_dict())
    model.to(DEV)
    x, t = torch.rand(2, 3, 32, 32, generator=g), torch.tensor([0.4, 0.05])
    with torch.no_grad():
        ref = osde.get_score_fn(osde.VESDE(0.01, 50, 1000), ref_model)(x, t)
    score = mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)
    _cache["model"] = (score, x.to(DEV), t.to(DEV), ref)
    return _cache["model"]


def test_small_ncsnpp_with_and_without_fir_gn(counted):
    """With the fused form both passes go (two coefficient launches come back, two of the resampler's launches change their kernel); under
    IDIFF_NO_FUSED_GN_FIR neither.  Both against each other and against the CPU oracle."""
    score, x, t, ref = _small_model()
    c0 = dict(counted)
    on = score(x, t)
    c_on = {k: counted[k] - c0[k] for k in counted}
    with _lib.thread_option("IDIFF_NO_FUSED_GN_FIR", 1):
        off = score(x, t)
    c_off = {k: counted[k] - c0[k] - c_on[k] for k in counted}
    print("fir_gn model-level launches on / off:", c_on, c_off)
    assert c_on["fir_gn"] == 2 and c_on["reader_coef"] == 2, c_on
    assert c_off["fir_gn"] == 0 and c_off["reader_coef"] == 0, c_off
    assert c_off["gn_apply"] - c_on["gn_apply"] == 2, (c_on, c_off)
    assert c_off["fir"] - c_on["fir"] == 2, (c_on, c_off)
    assert c_on["loader_coef"] == c_off["loader_coef"], (c_on, c_off)      # the convolution loader's coefficient launches do not change
    assert bool(torch.isfinite(on).all())
    e_on, e_off, e_both = rel_err(on.cpu(), ref), rel_err(off.cpu(), ref), rel_err(on.cpu(), off.cpu())
    print(f"fir_gn model-level rel err vs oracle: on {e_on:.2e} off {e_off:.2e}; on vs off {e_both:.2e}")
    assert e_on < NET_RTOL and e_off < NET_RTOL and e_both < NET_RTOL


def test_small_ncsnpp_shortcut_before_and_after_upsampling(counted, monkeypatch):
    """The up block's 1x1 shortcut before the upsampling (the default: W . x on the 16 x 16 map, then the FIR, the bias behind both in
    Conv_1's) and after it as the reference orders them: the same launches on other rows, both at NET_RTOL from the CPU oracle and from
    each other."""
    from id_diff_amd.models import ncsnpp as hip_ncsnpp
    score, x, t, ref = _small_model()
    assert hip_ncsnpp.SHORTCUT_BEFORE_UPSAMPLE
    c0 = dict(counted)
    on = score(x, t)
    c_on = {k: counted[k] - c0[k] for k in counted}
    monkeypatch.setattr(hip_ncsnpp, "SHORTCUT_BEFORE_UPSAMPLE", False)
    off = score(x, t)
    c_off = {k: counted[k] - c0[k] - c_on[k] for k in counted}
    assert c_on == c_off, (c_on, c_off)
    assert bool(torch.isfinite(on).all())
    e_on, e_off, e_both = rel_err(on.cpu(), ref), rel_err(off.cpu(), ref), rel_err(on.cpu(), off.cpu())
    print(f"early shortcut model-level rel err vs oracle: on {e_on:.2e} off {e_off:.2e}; on vs off {e_both:.2e}")
    assert e_on < NET_RTOL and e_off < NET_RTOL and e_both < NET_RTOL
    assert e_both > 0, "the two orders round differently: identical outputs mean the switch did nothing"
