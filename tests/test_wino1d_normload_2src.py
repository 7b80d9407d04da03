"""GroupNorm (+ SiLU) of cat[x1, x2] applied in the LOADER of the row-wise F(4, 3) convolution from its TWO sources (wino1d_nl2_kernel,
idiff_conv2d_wino1d_normload_2src_f32, coefficients from idiff_groupnorm_coef_f32 with both sources' column sums): the kernel against an
fp64 restatement with the two-launch path (two-source groupnorm_apply_colstats, then the convolution the executor's route table picks) as
the yardstick, the refusals, and the executor step that uses it.  Structure and bars: tests/test_wino1d_normload.py."""
import ctypes
import warnings

import pytest
import torch
import torch.nn.functional as F

import id_diff_amd
import normfused_cases
import normload_cases
from helpers import fill_from_seed, ncsnpp_config, rel_err
from normload_cases import colsums as _colsums
from id_diff_amd import _lib
from id_diff_amd.models import nhwc as hip_nhwc
from id_diff_amd.models import utils as mutils

gpu = pytest.mark.gpu
DEV = "cuda"
NET_RTOL = 2e-5                      # tests/test_hip_models.py
EPS = 1e-6
# tests/test_wino1d_normload.py: the same arithmetic as the one-source loader (a x + b rounded once, the same v_exp_f32 / v_rcp_f32 SiLU)
FUSED_VS_TWO_LAUNCH = 2.0
B, H, W = 3, 32, 32                  # an odd image count: the row blocks (16 rows) alternate top and bottom halves of an image
# (C1, C2) in K steps of 16 channels: 1 + 1 and 1 + 3 (the switch falls in the prologue's request of step 1), 2 + 1 (at the first in-loop
# request; a one-step second source: every clamped request re-reads ITS step), 3 + 2 (inside the loop); pitches 1:1, 1:3, 2:1, 3:2
SOURCES = [(16, 16), (16, 48), (32, 16), (48, 32)]
CASES = [(c1, c2, cout, act) for c1, c2 in SOURCES for cout in (64, 128) for act in ("silu", None)]
_cache = {}
_inputs_cache = {}


def _inputs(C1, C2, Cout, act):
    """CPU only.  Two separate raw sources with per-channel means of magnitude 1 .. 2, POSITIVE in x1 and NEGATIVE in x2 (a read from the
    wrong source, pitch or channel offset is an error of order 1), beta of magnitude ~1 (silu(beta) != 0: a padding pixel that is not forced
    back to zero shows), and the fp64 restatement group_norm(cat[x1, x2]) -> act -> conv2d, NHWC."""
    key = (C1, C2, Cout, act)
    if key in _inputs_cache:
        return _inputs_cache[key]
    Cin = C1 + C2
    G = Cin // 4
    g = torch.Generator().manual_seed(77 * C1 + 13 * C2 + Cout + (act is None))
    x1 = torch.randn(B, C1, H, W, generator=g) * 1.3 + (torch.rand(1, C1, 1, 1, generator=g) + 1.0)
    x2 = torch.randn(B, C2, H, W, generator=g) * 1.3 - (torch.rand(1, C2, 1, 1, generator=g) + 1.0)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g)
    gamma = (torch.rand(Cin, generator=g) + 0.5) * torch.where(torch.rand(Cin, generator=g) < 0.5, -1.0, 1.0) * 1.4
    beta = (torch.rand(Cin, generator=g) * 0.6 + 0.7) * torch.where(torch.rand(Cin, generator=g) < 0.5, -1.0, 1.0)
    n = F.group_norm(torch.cat([x1, x2], dim=1).double(), G, gamma.double(), beta.double(), EPS)
    n = F.silu(n) if act == "silu" else n
    ref = F.conv2d(n, w.double(), b.double(), padding=1).permute(0, 2, 3, 1).contiguous()
    out = (x1, x2, w, b, gamma, beta, G, ref)
    _inputs_cache[key] = out
    return out


def _tol(C1, C2, Cout, act):
    """the absolute, reference-derived bound of tests/normfused_cases.py (the end-to-end chain's), [B, H, W, Cout]"""
    x1, x2, w, b, gamma, beta, G, _ = _inputs(C1, C2, Cout, act)
    return normfused_cases.chain_bound_conv(x1, x2, gamma, beta, G, w, b, act)[1]


def _case(C1, C2, Cout, act):
    key = (C1, C2, Cout, act)
    if key in _cache:
        return _cache[key]
    x1, x2, w, b, gamma, beta, G, ref = _inputs(C1, C2, Cout, act)
    Cin = C1 + C2
    x1d = x1.permute(0, 2, 3, 1).contiguous().view(B, H * W, C1).to(DEV)     # two separate allocations, NHWC
    x2d = x2.permute(0, 2, 3, 1).contiguous().view(B, H * W, C2).to(DEV)
    cs1, cs2 = _colsums(x1d), _colsums(x2d)
    wt = w.permute(0, 2, 3, 1).contiguous().to(DEV)
    bd, gd, btd = b.to(DEV), gamma.to(DEV), beta.to(DEV)
    # two launches: the two-source pass (writes the concatenated, normalised tensor), then the 3x3 convolution on the executor's route
    normed = torch.empty(B, H * W, Cin, device=DEV)
    _lib.groupnorm_apply_colstats(x1d, C1, x2d, C2, B, H * W, G, cs1, 1, cs2, 1, EPS, gd, btd, act, normed)
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
    # one launch (+ the coefficients): the raw sources into the loader
    coef = torch.full((B * Cin * 2,), float("nan"), device=DEV)
    _lib.groupnorm_coef(cs1, 1, C1, cs2, 1, C2, B, H * W, G, EPS, gd, btd, coef)
    fused = torch.full((B, H * W, Cout), float("nan"), device=DEV)       # every output must be written
    ep = _lib.with_normload(_lib.make_epilogue(bias=bd), coef, act, x2d, C1)
    _lib.conv2d_wino1d(x1d, _lib.wino1d_pack(wt, Cin, Cout), fused, B, H, W, Cin, Cout, epilogue=ep)
    torch.cuda.synchronize()
    out = (ref, two.cpu().double().view(B, H, W, Cout), fused.cpu().double().view(B, H, W, Cout), name)
    _cache[key] = out
    return out


@pytest.fixture
def small_batches(monkeypatch):
    normload_cases.small_batches(monkeypatch)


@pytest.mark.parametrize("C1,C2", SOURCES)
def test_case_generator_and_restatement_on_the_cpu(C1, C2):
    """No GPU: the inputs and the fp64 restatement are finite, every channel mean of x1 is above +0.5 and of x2 below -0.5, and the
    restatement is not the one of the sources swapped (a test that could not tell them apart would check nothing)."""
    x1, x2, w, b, gamma, beta, G, ref = _inputs(C1, C2, 64, "silu")
    assert ref.shape == (B, H, W, 64) and bool(torch.isfinite(ref).all())
    assert all(bool(torch.isfinite(t).all()) for t in (x1, x2, w, b, gamma, beta))
    m1, m2 = x1.mean(dim=(0, 2, 3)), x2.mean(dim=(0, 2, 3))
    assert float(m1.min()) > 0.5 and float(m2.max()) < -0.5, (m1, m2)
    assert float(beta.abs().min()) >= 0.7
    if C1 == C2:
        n = F.silu(F.group_norm(torch.cat([x2, x1], dim=1).double(), G, gamma.double(), beta.double(), EPS))
        swapped = F.conv2d(n, w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
        assert float((swapped - ref).abs().max()) > 0.1


@gpu
@pytest.mark.parametrize("C1,C2,Cout,act", CASES)
def test_normload_2src_vs_fp64_and_two_launch(small_batches, C1, C2, Cout, act):
    """Every element against the fp64 restatement; the bar is the two-launch path's own error on the same inputs times
    FUSED_VS_TWO_LAUNCH, overall (maximum and rms) and separately on the image's first and last column and on rows 0, 15, 16, 31."""
    ref, two, fused, name = _case(C1, C2, Cout, act)
    assert bool(torch.isfinite(fused).all())
    e_two, e_fused = (two - ref).abs(), (fused - ref).abs()
    max_two, max_fused = float(e_two.max()), float(e_fused.max())
    rms_two, rms_fused = float(e_two.pow(2).mean().sqrt()), float(e_fused.pow(2).mean().sqrt())
    print(f"normload2_parity B={B} {H}x{W} {C1}+{C2}->{Cout} act={act} two-launch conv={name}: two-launch max {max_two:.3e} rms {rms_two:.3e} | "
          f"loader max {max_fused:.3e} rms {rms_fused:.3e} | ratio max {max_fused / max_two:.2f} rms {rms_fused / rms_two:.2f}")
    assert max_two > 0 and rms_two > 0
    # the yardstick itself is sane: fp32 rounding of values of size ~1
    assert max_two < 1e-4 * max(1.0, float(ref.abs().max()))
    assert max_fused <= FUSED_VS_TWO_LAUNCH * max_two
    assert rms_fused <= FUSED_VS_TWO_LAUNCH * rms_two
    slices = {"col 0": e_fused[:, :, 0], "col 31": e_fused[:, :, 31], "row 0": e_fused[:, 0], "row 15": e_fused[:, 15],
              "row 16": e_fused[:, 16], "row 31": e_fused[:, 31]}
    for what, e in slices.items():
        assert float(e.max()) <= FUSED_VS_TWO_LAUNCH * max_two, what
    # a second view: the absolute bound, element by element
    assert float((e_fused / _tol(C1, C2, Cout, act)).max()) <= 1.0


@gpu
def test_normload_2src_query_and_switches():
    q = _lib.conv2d_wino1d_normload_2src_ok
    base, base2 = q(2, 32, 32, 128, 128, 128), q(2, 32, 32, 256, 128, 128)      # routed class by class where measured faster
    assert not q(2, 32, 32, 128, 128, 256)             # four cout tiles: the one-source form measured no gain there, never routed
    assert not q(2, 16, 16, 128, 128, 128)             # rows of 16 pixels
    assert not q(2, 32, 32, 120, 136, 128) and not q(2, 32, 32, 0, 256, 128) and not q(2, 32, 32, 256, 0, 128)
    for switch in ("IDIFF_NO_FUSED_GN_LOAD_2SRC", "IDIFF_NO_PAIRS", "IDIFF_NO_WINO1D"):
        with _lib.thread_option(switch, 1):
            assert not q(2, 32, 32, 128, 128, 128) and not q(2, 32, 32, 256, 128, 128), switch
    with _lib.thread_option("IDIFF_NO_FUSED_GN_LOAD", 1):               # the one-source form's switch does not bear on this one
        assert q(2, 32, 32, 128, 128, 128) == base and q(2, 32, 32, 256, 128, 128) == base2
        assert not _lib.conv2d_wino1d_normload_ok(2, 32, 32, 128, 128)
    assert q(2, 32, 32, 128, 128, 128) == base


def _request(Bn, C1, C2, Cout, act="silu", x2=None):
    Cin = C1 + C2
    x2 = torch.zeros(2 * 1024 * max(C2, 16), device=DEV) if x2 is None else x2
    return _lib.with_normload(_lib.make_epilogue(), torch.zeros(Bn * Cin * 2, device=DEV), act, x2, C1)


@gpu
def test_normload_2src_refusals_launch_nothing():
    """Every refusal of the launcher comes before any device call: the output, pre-filled with 7.0, is untouched."""
    x1 = torch.zeros(2 * 1024 * 512 + 4, device=DEV)
    out = torch.full((2, 1024, 64), 7.0, device=DEV)
    bank = lambda cin: torch.zeros(_lib.lib().idiff_wino1d_weight_floats(cin, 64), device=DEV)
    refused = [
        ("positive multiples", dict(Bn=2, Hn=32, C1=24, C2=40)),         # C1 % 16
        ("positive multiples", dict(Bn=2, Hn=32, C1=32, C2=24)),         # C2 % 16
        ("positive multiples", dict(Bn=2, Hn=32, C1=0, C2=64)),
        ("positive multiples", dict(Bn=2, Hn=32, C1=64, C2=0)),
        ("W = 32", dict(Bn=2, Hn=16, C1=64, C2=64)),                     # C1 + C2 served, the map is not
        ("not supported", dict(Bn=2, Hn=32, C1=1024, C2=16)),            # C1 + C2 beyond the K loop's 1024 channels
        ("beyond one buffer descriptor", dict(Bn=2240, Hn=32, C1=512, C2=16)),
        ("SiLU or no activation", dict(Bn=2, Hn=32, C1=64, C2=64, act="relu")),
        ("SiLU or no activation", dict(Bn=2, Hn=32, C1=64, C2=64, act="lrelu")),
    ]
    for match, c in refused:
        Cin = c["C1"] + c["C2"]
        with pytest.raises(RuntimeError, match=match):
            _lib.conv2d_wino1d(x1, bank(Cin), out, c["Bn"], c["Hn"], c["Hn"], Cin, 64,
                               epilogue=_request(c["Bn"], c["C1"], c["C2"], 64, c.get("act", "silu")))
    # a misaligned first and second source; a null second source (below the Python wrapper, which cannot express it)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _lib.conv2d_wino1d(x1[1:], bank(128), out, 2, 32, 32, 128, 64, epilogue=_request(2, 64, 64, 64))
    with pytest.raises(RuntimeError, match="x2 is required, 16-byte aligned"):
        _lib.conv2d_wino1d(x1, bank(128), out, 2, 32, 32, 128, 64, epilogue=_request(2, 64, 64, 64, x2=torch.zeros(2 * 1024 * 64 + 4, device=DEV)[1:]))
    ep, coef, u = _lib.make_epilogue(), torch.zeros(2 * 128 * 2, device=DEV), bank(128)
    rc = _lib.lib().idiff_conv2d_wino1d_normload_2src_f32(x1.data_ptr(), 64, None, 64, u.data_ptr(), out.data_ptr(), 2, 32, 32, 64,
                                                          ctypes.byref(ep), coef.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"x2 is required" in _lib.lib().idiff_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused request must not launch"
    # the request is conv2d_wino1d's alone
    ep = _request(2, 64, 64, 64)
    with pytest.raises(RuntimeError, match="only conv2d_wino1d serves"):
        _lib.gemm(torch.zeros(64, 128, device=DEV), torch.zeros(128, 128, device=DEV), epilogue=ep)
    with pytest.raises(RuntimeError, match="only conv2d_wino1d serves"):
        _lib.conv2d_winograd43(x1, torch.zeros(_lib.lib().idiff_winograd43h_weight_floats(128, 64), device=DEV), out, 2, 32, 32, 128, 64,
                               epilogue=ep, pairs=True)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- executor
MEASURED = ((128, 128), (256, 128))      # the benchmark's classes (C1, C2) -> 128 of scripts/normload_shape_ab.py


@pytest.fixture
def counted(small_batches, monkeypatch):
    """Counts the passes, the two-source coefficient launches and the convolutions; the routing query admits every geometry the launcher
    serves with at most two cout tiles (this network's 128 + 64 -> 64 and 64 + 64 -> 64 are not classes of the benchmark) as long as the
    library's own query -- and with it every switch -- admits a measured class."""
    calls, orig_ok = normload_cases.counted(monkeypatch), _lib.conv2d_wino1d_normload_2src_ok

    def admit(B, H, W, C1, C2, Cout):
        return (any(orig_ok(B, 32, 32, c1, c2, 128) for c1, c2 in MEASURED) and W == 32 and H % 16 == 0 and C1 > 0 and C2 > 0
                and C1 % 16 == 0 and C2 % 16 == 0 and Cout in (64, 128))
    monkeypatch.setattr(_lib, "conv2d_wino1d_normload_2src_ok", admit)
    return calls


def _small_model():
    """nf = 64, levels of 64 and 128 channels, one residual block per level, 32 x 32 input.  The up path at 32 x 32 has two blocks on
    cat[h, skip]: 128 + 64 -> 64 (unequal pitch) and 64 + 64 -> 64 (equal pitch); their GroupNorm_0 is the two-source loader's."""
    model = mutils.create_model(ncsnpp_config(**{"model.nf": 64, "model.ch_mult": (1, 2), "model.num_res_blocks": 1, "model.init_scale": 1.0}))
    fill_from_seed(model, 5)
    model.to(DEV)
    model._invalidate()
    g = torch.Generator().manual_seed(3)
    return model, torch.rand(2, 3, 32, 32, generator=g).to(DEV), torch.full((2,), 0.4, device=DEV)


def _on_and_off(model, x, t, calls):
    return normload_cases.on_and_off(model, x, t, calls, "IDIFF_NO_FUSED_GN_LOAD_2SRC")


@gpu
def test_small_ncsnpp_with_and_without_normload_2src(counted):
    model, x, t = _small_model()
    on, off, c_on, c_off = _on_and_off(model, x, t, counted)
    print("normload2 model-level launches on / off:", c_on, c_off)
    assert c_off["wino1d_nl2"] == 0 and c_off["gn_coef2"] == 0, c_off
    assert c_on["wino1d_nl2"] == 2 and c_on["gn_coef2"] == 2, c_on
    assert c_off["gn_apply"] - c_on["gn_apply"] == 2, (c_on, c_off)
    assert c_on["wino1d"] == c_off["wino1d"], (c_on, c_off)            # the convolutions' own counters do not change
    assert bool(torch.isfinite(on).all())
    assert rel_err(on.cpu(), off.cpu()) < NET_RTOL


@gpu
def test_inadmissible_gamma_leaves_the_two_source_loader_route(counted):
    """gamma x 500 on the GroupNorm_0 of the 64 + 64 -> 64 block: beyond the fp16 pairs' range, decided from the norm's own record: that
    block keeps the pass (and the fp32 route), the other keeps the loader, and the outputs match."""
    model, x, t = _small_model()
    blocks = [m for m in model.all_modules if hasattr(m, "GroupNorm_0") and getattr(m, "in_ch", None) == 128 and getattr(m, "out_ch", None) == 64]
    assert len(blocks) == 1
    with torch.no_grad():
        blocks[0].GroupNorm_0.weight.mul_(500.0)
    model._invalidate()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        on, off, c_on, c_off = _on_and_off(model, x, t, counted)
    print("normload2 inadmissible-gamma launches on / off:", c_on, c_off)
    assert c_on["wino1d_nl2"] == 1 and c_off["wino1d_nl2"] == 0, (c_on, c_off)
    assert c_off["gn_apply"] - c_on["gn_apply"] == 1, (c_on, c_off)
    assert bool(torch.isfinite(on).all())
    assert rel_err(on.cpu(), off.cpu()) < NET_RTOL


@gpu
@pytest.mark.parametrize("sources", (1, 2))
def test_conv_makes_the_pass_when_the_loader_no_longer_serves(counted, sources):
    """The deferred norm's way back: _gn_act hands a raw tensor on with a pending record, the form's switch is flipped, and _conv -- whose
    query now answers no -- makes the pass after all, from the record's fields, before it launches.  GroupNorm(8, 32) + SiLU of one raw
    source of 32 channels (the smallest Cin of the plain wino1d route) or of 16 + 16 (one K step each, means +1 .. 2 and -1 .. -2: swapped
    or repeated sources are an error of order 1), B = 2, 32 x 32 -> 64 channels.  Bit-equal to the same two calls made entirely under the
    switch (the same pass and the same convolution launch on the same data), and within the file's bar of the fp64 restatement."""
    Bn, C, Cout = 2, 32, 64
    switch = "IDIFF_NO_FUSED_GN_LOAD" if sources == 1 else "IDIFF_NO_FUSED_GN_LOAD_2SRC"
    model, _, _ = _small_model()
    g = torch.Generator().manual_seed(91 + sources)
    sign = lambda n: torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    widths = (C,) if sources == 1 else (C // 2, C // 2)
    raw = [torch.randn(Bn, c, H, W, generator=g) * 1.3 + s * (torch.rand(1, c, 1, 1, generator=g) + 1.0) for c, s in zip(widths, (1.0, -1.0))]
    w = torch.randn(Cout, C, 3, 3, generator=g) / (C * 9) ** 0.5
    b = torch.randn(Cout, generator=g)
    gn = torch.nn.GroupNorm(8, C, eps=EPS).to(DEV)
    with torch.no_grad():
        gn.weight.copy_((torch.rand(C, generator=g) + 0.5) * sign(C) * 1.4)
        gn.bias.copy_((torch.rand(C, generator=g) * 0.6 + 0.7) * sign(C))
    assert float(gn.bias.detach().abs().min()) >= 0.7
    n = F.silu(F.group_norm(torch.cat(raw, dim=1).double(), 8, gn.weight.detach().cpu().double(), gn.bias.detach().cpu().double(), EPS))
    ref = F.conv2d(n, w.double(), b.double(), padding=1).permute(0, 2, 3, 1).contiguous()
    wt, bd = w.permute(0, 2, 3, 1).contiguous().to(DEV), b.to(DEV)

    def tensors():
        bufs = [r.permute(0, 2, 3, 1).contiguous().view(Bn, H * W, r.shape[1]).to(DEV) for r in raw]
        ts = [hip_nhwc._T(buf, H, W, buf.shape[2], stats=(_colsums(buf), 1)) for buf in bufs]
        return ts[0], (ts[1] if sources == 2 else None)

    with torch.no_grad():
        x, x2 = tensors()
        c0 = dict(counted)
        deferred = model._gn_act(x, gn, "silu", x2, conv_cout=Cout)
        assert deferred.pending is not None and deferred.buf is x.buf and deferred.C == C
        assert counted["gn_apply"] == c0["gn_apply"], "the pass is deferred"
        c1 = dict(counted)
        with _lib.thread_option(switch, 1):
            got = model._conv(deferred, wt, bd, normed=True, rows_per_group=H * W)
        made = {k: counted[k] - c1[k] for k in counted}
        # the whole of it under the switch: the pass at once, no record, the same convolution
        with _lib.thread_option(switch, 1):
            x, x2 = tensors()
            c2 = dict(counted)
            normed = model._gn_act(x, gn, "silu", x2, conv_cout=Cout)
            assert normed.pending is None
            want = model._conv(normed, wt, bd, normed=True, rows_per_group=H * W)
        plain = {k: counted[k] - c2[k] for k in counted}
    torch.cuda.synchronize()
    print(f"rerun sources={sources}: launches of the switched _conv {made}, of both calls under the switch {plain}")
    assert made["gn_apply"] == 1 and plain["gn_apply"] == 1, (made, plain)          # exactly the one pass that was put off
    assert made["wino1d"] == 1 and plain["wino1d"] == 1, (made, plain)
    assert made["wino1d_nl"] == 0 and made["wino1d_nl2"] == 0, made
    assert got.pending is None and (got.H, got.W, got.C) == (H, W, Cout)
    assert torch.equal(got.buf, want.buf)
    e_two = (want.buf.cpu().double().view(Bn, H, W, Cout) - ref).abs()
    e_got = (got.buf.cpu().double().view(Bn, H, W, Cout) - ref).abs()
    max_two, rms_two = float(e_two.max()), float(e_two.pow(2).mean().sqrt())
    print(f"rerun sources={sources}: two-launch max {max_two:.3e} rms {rms_two:.3e} | re-run max {float(e_got.max()):.3e} "
          f"rms {float(e_got.pow(2).mean().sqrt()):.3e}")
    assert max_two > 0 and max_two < 1e-4 * max(1.0, float(ref.abs().max()))
    assert float(e_got.max()) <= FUSED_VS_TWO_LAUNCH * max_two
    assert float(e_got.pow(2).mean().sqrt()) <= FUSED_VS_TWO_LAUNCH * rms_two
