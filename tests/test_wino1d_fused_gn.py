"""GroupNorm + activation applied in the tail of the row-wise F(4, 3) convolution (wino1d_gn_kernel, idiff_conv2d_wino1d_gn_f32): the kernel
against an fp64 oracle with the two-launch path as the yardstick, the refusals, and the executor step that uses it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import id_diff_amd
import normfused_cases
from helpers import fill_from_seed, ncsnpp_config, overrides_from_golden, rel_err
from id_diff_amd import _lib
from id_diff_amd.models import utils as mutils

pytestmark = pytest.mark.gpu
DEV = "cuda"
NET_RTOL = 2e-5                      # tests/test_hip_models.py
EPS = 1e-6
# The fused path may be at most this many times as far from the fp64 oracle as the parent's two-launch path (conv2d_wino1d with column sums,
# then groupnorm_apply_colstats) on the same inputs, per case, in the maximum and in the root mean square of the elementwise error.  Both
# round the same fp32 convolution and differ in how the statistics are summed; measured (profiles/fused_gn_parity.txt): 1.00 x in every case, the two paths' fp64 statistics
# round to the same fp32 mean and rstd.
FUSED_VS_TWO_LAUNCH = 2.0

# (B, H, W, Cin, Cout, groups, offset): 16 x 16, 8 x 8 and 4 x 4 maps, Cin in {128, 256, 512}, Cout in {128, 256} = 4 and 8 channels per group,
# batch sizes that leave the last block partial (a block is 2 / 8 / 32 images), one case whose channels sit 300 standard deviations off zero
CASES = [(5, 16, 16, 128, 128, 32, 0.0), (3, 16, 16, 256, 256, 32, 0.0), (3, 16, 16, 512, 256, 32, 0.0),
         (13, 8, 8, 256, 256, 32, 0.0), (9, 8, 8, 512, 128, 32, 0.0), (11, 8, 8, 128, 256, 32, 0.0),
         (37, 4, 4, 256, 256, 32, 0.0), (33, 4, 4, 512, 256, 32, 0.0), (70, 4, 4, 128, 128, 32, 0.0),
         (5, 16, 16, 256, 256, 32, 300.0), (13, 8, 8, 256, 128, 32, 300.0),
         # group widths 16 and 2 (sixteen lanes' and half a thread's channels), a non-square map of 128 pixels (two waves per image)
         (3, 16, 16, 128, 128, 8, 0.0), (9, 8, 8, 128, 64, 32, 0.0), (5, 8, 16, 128, 128, 32, 0.0),
         # the rest of what the query admits: one channel per group, groups of 32 and 64 channels (eight and all sixteen lanes of a pixel
         # row), maps of 32 pixels (two thread rows per image: one exchange inside the wave), either way round
         (9, 8, 8, 128, 64, 64, 0.0), (3, 16, 16, 128, 128, 4, 0.0), (13, 8, 8, 128, 128, 2, 300.0), (9, 4, 8, 128, 128, 32, 0.0),
         (21, 8, 4, 128, 64, 16, 0.0)]


def _case(B, H, W, Cin, Cout, groups, offset):
    g = torch.Generator().manual_seed(1000 * H + Cin + Cout + B)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g) + offset * (torch.rand(Cout, generator=g) + 0.5)
    temb = torch.randn(B, Cout, generator=g)
    gamma = (torch.rand(Cout, generator=g) + 0.5) * torch.where(torch.rand(Cout, generator=g) < 0.5, -1.0, 1.0) * 1.7    # not near 1
    beta = torch.randn(Cout, generator=g) * 0.8 + 0.6                                                              # not near 0
    h = F.conv2d(x.double(), w.double(), b.double(), padding=1) + temb.double()[:, :, None, None]
    ref = F.silu(F.group_norm(h, groups, gamma.double(), beta.double(), EPS)).permute(0, 2, 3, 1).contiguous()
    return x, w, b, temb, gamma, beta, ref


def _both_paths(B, H, W, Cin, Cout, groups, x, w, b, temb, gamma, beta):
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    u = _lib.wino1d_pack(w.permute(0, 2, 3, 1).contiguous().to(DEV), Cin, Cout)
    bd, td, gd, btd = b.to(DEV), temb.to(DEV), gamma.to(DEV), beta.to(DEV)
    # the parent's path: the convolution writes h and its column sums, the apply kernel reads h and writes y
    ns = _lib.conv2d_wino1d_colstats_split(B, H, W, Cin, Cout)
    assert ns == 1
    cs = torch.full((B * ns * Cout * 2,), float("nan"), device=DEV, dtype=torch.float64)
    h = torch.empty(B, H * W, Cout, device=DEV)
    _lib.conv2d_wino1d(xd, u, h, B, H, W, Cin, Cout, epilogue=_lib.make_epilogue(bias=bd, rowbias=td, rows_per_group=H * W, colstats=cs))
    two = torch.empty(B, H * W, Cout, device=DEV)
    _lib.groupnorm_apply_colstats(h, Cout, None, 0, B, H * W, groups, cs, ns, None, 0, EPS, gd, btd, "silu", two)
    fused = torch.full((B, H * W, Cout), float("nan"), device=DEV)                  # every output must be written
    ep = _lib.with_groupnorm(_lib.make_epilogue(bias=bd, rowbias=td, rows_per_group=H * W), groups, gd, btd, EPS, "silu")
    _lib.conv2d_wino1d(xd, u, fused, B, H, W, Cin, Cout, epilogue=ep)
    torch.cuda.synchronize()
    return two.cpu().double().view(B, H, W, Cout), fused.cpu().double().view(B, H, W, Cout)


@pytest.mark.parametrize("B,H,W,Cin,Cout,groups,offset", CASES)
def test_fused_gn_vs_fp64_oracle(B, H, W, Cin, Cout, groups, offset):
    """conv + bias + per-image bias + GroupNorm + SiLU in one launch against the same chain in fp64 on the CPU, every element compared.  The
    bar is the two-launch path's own error against that oracle on the same inputs, times FUSED_VS_TWO_LAUNCH."""
    assert _lib.conv2d_wino1d_gn_ok(B, H, W, Cin, Cout, groups)
    x, w, b, temb, gamma, beta, ref = _case(B, H, W, Cin, Cout, groups, offset)
    two, fused = _both_paths(B, H, W, Cin, Cout, groups, x, w, b, temb, gamma, beta)
    assert bool(torch.isfinite(fused).all())
    e_two, e_fused = (two - ref).abs(), (fused - ref).abs()
    max_two, max_fused = float(e_two.max()), float(e_fused.max())
    rms_two, rms_fused = float(e_two.pow(2).mean().sqrt()), float(e_fused.pow(2).mean().sqrt())
    print(f"fused_gn_parity B={B} {H}x{W} {Cin}->{Cout} G={groups} offset={offset:g}: two-launch max {max_two:.3e} rms {rms_two:.3e} | "
          f"fused max {max_fused:.3e} rms {rms_fused:.3e} | ratio max {max_fused / max_two:.2f} rms {rms_fused / rms_two:.2f}")
    assert max_two > 0 and rms_two > 0
    assert max_fused <= FUSED_VS_TWO_LAUNCH * max_two
    assert rms_fused <= FUSED_VS_TWO_LAUNCH * rms_two
    # and the two-launch path itself is a sane yardstick: fp32 rounding of values of size 1 + offset, far below the activations' scale
    assert max_two < 1e-4 * max(1.0, float(ref.abs().max())) * (1.0 + offset)
    # a second view: the absolute, reference-derived bound of tests/normfused_cases.py, element by element
    tol = normfused_cases.tail_bound(x, w, b, temb, gamma, beta, groups)[1]
    assert float((e_fused / tol).max()) <= 1.0


def test_fused_gn_refusals():
    """What the tail cannot finish inside one round of one workgroup is refused with a message, by the query and by the launcher, and nothing
    is launched: the output buffer keeps its fill."""
    g = torch.Generator().manual_seed(5)
    gam, bet = torch.ones(256, device=DEV), torch.zeros(256, device=DEV)

    def launch(H, W, Cout, groups, out_fill=7.0, **ep):
        x = torch.randn(2, H * W, 128, generator=g).to(DEV)
        u = _lib.wino1d_pack((torch.randn(Cout, 3, 3, 128, generator=g) / 34.0).to(DEV), 128, Cout)
        out = torch.full((2, H * W, Cout), out_fill, device=DEV)
        ep.setdefault("rows_per_group", H * W)
        epi = _lib.with_groupnorm(_lib.make_epilogue(**ep), groups, gam[:Cout], bet[:Cout], EPS, "silu")
        try:
            _lib.conv2d_wino1d(x, u, out, 2, H, W, 128, Cout, epilogue=epi)
        finally:
            torch.cuda.synchronize()
            assert bool((out == out_fill).all()), "a refused request must not launch"

    assert _lib.conv2d_wino1d_ok(2, 32, 32, 128, 128) and not _lib.conv2d_wino1d_gn_ok(2, 32, 32, 128, 128, 32)
    with pytest.raises(RuntimeError, match="must divide 256"):
        launch(32, 32, 128, 32)                                            # a workgroup is half an image
    with pytest.raises(RuntimeError, match="residual"):
        launch(16, 16, 128, 32, residual=torch.zeros(2, 256, 128, device=DEV))
    with pytest.raises(RuntimeError, match="colstats"):
        launch(16, 16, 128, 32, colstats=torch.zeros(2 * 128 * 2, device=DEV, dtype=torch.float64))
    assert not _lib.conv2d_wino1d_gn_ok(2, 16, 16, 128, 128, 1)            # one group of 128 channels: two tiles
    with pytest.raises(RuntimeError, match="must divide 64"):
        launch(16, 16, 128, 1)
    assert not _lib.conv2d_wino1d_gn_ok(2, 16, 16, 128, 64 * 3, 4)          # groups of 48 channels straddle the tiles
    with pytest.raises(RuntimeError, match="must divide 64"):
        launch(16, 16, 64 * 3, 4)
    with pytest.raises(RuntimeError, match="rows_per_group"):
        launch(16, 16, 128, 32, rows_per_group=64)
    with pytest.raises(RuntimeError, match="no activation, no scale"):
        launch(16, 16, 128, 32, act="silu")
    # the switch: the query answers no, process-wide and per thread
    assert _lib.conv2d_wino1d_gn_ok(2, 16, 16, 128, 128, 32)
    with _lib.thread_option("IDIFF_NO_FUSED_GN", 1):
        assert not _lib.conv2d_wino1d_gn_ok(2, 16, 16, 128, 128, 32)
    prev = _lib.set_option("IDIFF_NO_FUSED_GN", 1)
    try:
        assert not _lib.conv2d_wino1d_gn_ok(2, 16, 16, 128, 128, 32)
    finally:
        _lib.set_option("IDIFF_NO_FUSED_GN", prev)
    assert _lib.conv2d_wino1d_gn_ok(2, 16, 16, 128, 128, 32)
    # a GroupNorm request handed to any other contraction is an error, not dropped
    epi = _lib.with_groupnorm(_lib.make_epilogue(), 32, gam[:128], bet[:128], EPS, "silu")
    a = torch.zeros(64, 128, device=DEV)
    with pytest.raises(RuntimeError, match="only conv2d_wino1d serves"):
        _lib.gemm(a, torch.zeros(128, 128, device=DEV), epilogue=epi)
    with pytest.raises(RuntimeError, match="only conv2d_wino1d serves"):
        _lib.conv2d_nhwc(torch.zeros(1, 8, 8, 128, device=DEV), torch.zeros(128, 3, 3, 128, device=DEV), torch.zeros(1, 8, 8, 128, device=DEV),
                         1, 8, 8, 128, 128, 3, 3, 1, 1, epilogue=epi)
    wt = torch.zeros(128, 3, 3, 128, device=DEV)
    with pytest.raises(RuntimeError, match="only conv2d_wino1d serves"):
        _lib.conv2d_winograd43(torch.zeros(1, 8, 8, 128, device=DEV), _lib.winograd43_pack(wt, 128, 128, pairs=True),
                               torch.zeros(1, 8, 8, 128, device=DEV), 1, 8, 8, 128, 128, epilogue=epi, pairs=True)


@pytest.fixture
def small_batches_on_wino1d(monkeypatch):
    """Test-sized batches through the large-batch kernels, as the existing wino1d network tests do, with the GroupNorm-apply launches counted."""
    from id_diff_amd.models import nhwc as hip_nhwc
    monkeypatch.setattr(hip_nhwc, "WINO1D_MIN_WORKGROUPS", 1)
    monkeypatch.setattr(hip_nhwc, "WINO43_MIN_WORKGROUPS", 1)
    monkeypatch.setattr(hip_nhwc, "WINO43_PAIRS_MIN_WORKGROUPS", 1)
    calls = {"gn_apply": 0, "wino1d": 0, "wino1d_gn": 0}
    orig_gn, orig_conv = _lib.groupnorm_apply_colstats, _lib.conv2d_wino1d

    def counted_gn(*a, **k):
        calls["gn_apply"] += 1
        return orig_gn(*a, **k)

    def counted_conv(x, u, out, B, H, W, Cin, Cout, epilogue=None):
        calls["wino1d"] += 1
        calls["wino1d_gn"] += getattr(epilogue, "groupnorm", None) is not None
        return orig_conv(x, u, out, B, H, W, Cin, Cout, epilogue=epilogue)
    monkeypatch.setattr(_lib, "groupnorm_apply_colstats", counted_gn)
    monkeypatch.setattr(_lib, "conv2d_wino1d", counted_conv)
    return calls


def test_ncsnpp_golden_with_and_without_fused_gn(golden, small_batches_on_wino1d):
    """The nf = 128 golden NCSN++ with the fused step (the default) and under IDIFF_NO_FUSED_GN: both at NET_RTOL from the reference's output
    and from each other, the fused forward with one GroupNorm-apply launch less per residual block, and the consumer of the fused output
    (Conv_1) still admitted to the row-wise pair kernel (the same number of wino1d launches)."""
    calls = small_batches_on_wino1d
    z = golden("ncsnpp_wide.npz")
    model = mutils.create_model(ncsnpp_config(**overrides_from_golden(z)))
    fill_from_seed(model, int(z["seed"]))
    model.to(DEV)
    model._invalidate()
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    fused = model(x, t * 999)
    c_fused = dict(calls)
    assert c_fused["wino1d_gn"] == 5, c_fused                  # one 8 x 8 level: a block down, two in the middle, two up
    with _lib.thread_option("IDIFF_NO_FUSED_GN", 1):
        plain = model(x, t * 999)
    c_plain = {k: calls[k] - c_fused[k] for k in calls}
    assert c_plain["wino1d_gn"] == 0 and c_plain["wino1d"] == c_fused["wino1d"], (c_fused, c_plain)
    assert c_plain["gn_apply"] - c_fused["gn_apply"] == 5, (c_fused, c_plain)
    assert rel_err(fused.cpu(), z["model_out"]) < NET_RTOL
    assert rel_err(plain.cpu(), z["model_out"]) < NET_RTOL
    assert rel_err(fused.cpu(), plain.cpu()) < NET_RTOL        # (in fact equal: both paths' fp64 statistics round to the same fp32 values)


def test_config3_network_makes_34_fewer_groupnorm_launches(small_batches_on_wino1d):
    """The benchmark's network (nf = 128, ch_mult (1, 2, 2, 2), four residual blocks per level, 32 x 32 input) at a test batch: Conv_0 of the
    11 + 11 + 12 residual blocks on the 16 x 16, 8 x 8 and 4 x 4 levels applies GroupNorm_1 itself, the 12 blocks at 32 x 32 do not."""
    calls = small_batches_on_wino1d
    torch.manual_seed(0)
    model = mutils.create_model(ncsnpp_config(**{"model.nf": 128, "model.num_res_blocks": 4, "model.init_scale": 1.0}))
    model.to(DEV)
    model._invalidate()
    g = torch.Generator().manual_seed(11)
    x, t = torch.rand(2, 3, 32, 32, generator=g).to(DEV), torch.full((2,), 0.3, device=DEV)
    fused = model(x, t * 999)
    c_fused = dict(calls)
    with _lib.thread_option("IDIFF_NO_FUSED_GN", 1):
        plain = model(x, t * 999)
    c_plain = {k: calls[k] - c_fused[k] for k in calls}
    assert c_fused["wino1d_gn"] == 34 and c_plain["wino1d_gn"] == 0, (c_fused, c_plain)
    assert c_plain["gn_apply"] - c_fused["gn_apply"] == 34, (c_fused, c_plain)
    assert c_plain["wino1d"] == c_fused["wino1d"], (c_fused, c_plain)
    assert bool(torch.isfinite(fused).all())
    assert rel_err(fused.cpu(), plain.cpu()) < NET_RTOL
