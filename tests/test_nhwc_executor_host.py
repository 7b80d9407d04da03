"""The NHWC executor's host logic that needs no GPU (models/nhwc.py): the NormedBy record against the tuples it replaced, and which
fused attention kernel the one ``_attention`` asks for."""
import numpy as np
import pytest
import torch

from helpers import ncsnpp_config
from id_diff_amd import _lib
from id_diff_amd.models import nhwc, utils as mutils


def test_normed_by_reproduces_the_tuples_it_replaced():
    """(module, elements per normalised group, absolute gain, modulated?) as _gn_act, the fused tail and ncsnpp._fir spelled them out:
    (C // G) * H * W over ALL the norm's channels, gain 1 behind the norm itself, the resamplers multiplying their absolute tap sum in."""
    gn = torch.nn.GroupNorm(32, 128)
    C, G, H, W = 128, 32, 8, 8
    one = nhwc.NormedBy.of(gn, C, H * W)
    assert tuple(one) == (gn, (C // G) * H * W, 1.0, False) and one.group_elems == 256
    gn2 = torch.nn.GroupNorm(32, 64 + 192)
    two = nhwc.NormedBy.of(gn2, 64 + 192, H * W)                                    # cat[x, x2]: the groups run over both sources
    assert tuple(two) == (gn2, ((64 + 192) // 32) * H * W, 1.0, False) and two.group_elems == 512
    mod = nhwc.NormedBy.of(gn, C, H * W, modulated=True)
    assert tuple(mod) == (gn, 256, 1.0, True)
    # the FIR gains of NCSNpp._pack for fir_kernel = [1, 3, 3, 1]: whole tap sum without zero insertion, largest polyphase sum with it
    k = np.outer([1, 3, 3, 1], [1, 3, 3, 1]).astype(np.float32)
    k = k / np.sum(k)
    gains = {"down": float(np.abs(k).sum()), "pre_conv": float(np.abs(k).sum()),
             "up": float(max(np.abs(4.0 * k[py::2, px::2]).sum() for py in (0, 1) for px in (0, 1)))}
    for mode, gain in gains.items():
        assert tuple(one.through(gain)) == (gn, 256, gain, False), mode             # the loader form: the norm, then the resampler
        assert tuple(mod.through(gain)) == (gn, 256, 1.0 * gain, True), mode        # the pass, then the resampler: x.norm[2] * gain
        assert tuple(one.through(gain).through(gain)) == (gn, 256, gain * gain, False), mode
    assert isinstance(one.through(2.0), nhwc.NormedBy) and one.gain == 1.0          # a new record, the old one unchanged


@pytest.mark.parametrize("mode", ("up", "down", "pre_conv"))
def test_fir_passes_the_record_through_its_own_modes_gain(monkeypatch, mode):
    """NCSNpp._fir on a GroupNorm's output: the record with the gain NCSNpp._pack computed for THAT mode multiplied in, nothing else changed
    (fir_kernel = [1, 3, 3, 1]: 1 for down / pre_conv, 1 for up too -- every polyphase of 4 k sums to one -- so a distinct gain is planted)."""
    model = mutils.create_model(ncsnpp_config())
    assert model.fir and model.fir_kernel == [1, 3, 3, 1]
    pk = model._pack()
    assert pk["fir_gain"] == pytest.approx({"down": 1.0, "pre_conv": 1.0, "up": 1.0}, rel=1e-6)
    pk["fir_gain"] = {"down": 2.0, "pre_conv": 3.0, "up": 5.0}
    monkeypatch.setattr(_lib, "upfirdn2d_out_size", lambda size, up, down, p0, p1, n: (size * up + p0 + p1 - n) // down + 1)
    monkeypatch.setattr(_lib, "upfirdn2d_raw", lambda *a, **k: None)
    gn = torch.nn.GroupNorm(2, 8)
    before = nhwc.NormedBy.of(gn, 8, 64, modulated=True).through(1.5)
    y = model._fir(nhwc._T(torch.zeros(1, 64, 8), 8, 8, 8, norm=before), pk, mode)
    assert (y.H, y.W, y.C) == ({"up": 16, "down": 4, "pre_conv": 9}[mode],) * 2 + (8,)
    assert tuple(y.norm) == (gn, 4 * 64, 1.5 * pk["fir_gain"][mode], True)
    assert model._fir(nhwc._T(torch.zeros(1, 64, 8), 8, 8, 8), pk, mode).norm is None


class _Executor(nhwc.NhwcExecutor):
    def __init__(self):
        super().__init__()
        self._packed = {}


@pytest.mark.parametrize("heads", (1, 2, 4))
@pytest.mark.parametrize("served", (True, False))
def test_attention_asks_the_query_of_its_head_count(monkeypatch, heads, served):
    """heads = 1: attention256_ok(B, HW, C) and, served, attention256; more: attention_heads_ok(B, HW, heads, D) and attention_heads.
    Not served: three launches per head (for one head on the whole buffers, K = C) and the plain output projection."""
    B, H, W, C = 2, 4, 4, 64
    HW, D = H * W, C // heads
    calls = []

    def record(name, result=None):
        def fn(*a, **k):
            calls.append((name, tuple(v for v in a if isinstance(v, (int, float, bool))), k))
            return result
        monkeypatch.setattr(_lib, name, fn)

    for name in ("gemm_normed", "gemm_weight_times_normed_t", "attention256", "attention_heads", "gemm", "softmax_rows", "gemm_pairs",
                 "make_epilogue"):
        record(name)
    record("attention256_ok", served)
    record("attention_heads_ok", served)
    record("gemm_pairs_ok", True)
    record("gemm_colstats_split", 0)
    record("pairs_scale_from_rows", "scale")
    record("_pairs_scale_of", "w_scale")
    gn = torch.nn.GroupNorm(16, C)
    x = nhwc._T(torch.zeros(B, HW, C), H, W, C)
    n = nhwc._T(torch.zeros(B, HW, C), H, W, C, norm=nhwc.NormedBy.of(gn, C, HW))
    wqk, bqk, wv, bv, wo, bo = torch.zeros(2 * C, C), torch.zeros(2 * C), torch.zeros(C, C), torch.zeros(C), torch.zeros(C, C), torch.zeros(C)
    cache = {}
    y = _Executor()._attention({}, x, n, wqk, bqk, wv, bv, wo, bo, cache, "scales", heads=heads)
    assert (y.H, y.W, y.C) == (H, W, C)
    names = [c[0] for c in calls if c[0] not in ("make_epilogue", "gemm_colstats_split", "_pairs_scale_of")]
    asked, other = ("attention256_ok", "attention_heads_ok") if heads == 1 else ("attention_heads_ok", "attention256_ok")
    query = next(c for c in calls if c[0] == asked)
    assert query[1] == ((B, HW, C) if heads == 1 else (B, HW, heads, D))
    assert other not in names
    head = ["gemm_normed", "gemm_weight_times_normed_t", asked]
    scale = float(D) ** -0.5
    if served:
        kernel = "attention256" if heads == 1 else "attention_heads"
        assert names == head + ["pairs_scale_from_rows", "pairs_scale_from_rows", kernel, "gemm_pairs_ok", "gemm_pairs"]
        launch = next(c for c in calls if c[0] == kernel)
        assert launch[1] == ((B, C, scale) if heads == 1 else (B, HW, heads, D, scale))
        assert cache == {"scales": ("scale", "scale")}
        assert calls[-1][2]["act_scale"] == "scale"
    else:
        assert names == head + ["gemm", "softmax_rows", "gemm"] * heads + ["gemm"]
        gemms = [c for c in calls if c[0] == "gemm"]
        assert all(g[2]["K"] == D for g in gemms[0:-1:2]) and all(g[2]["N"] == D for g in gemms[1:-1:2])
        assert all(c[1] == (B * HW, HW, scale) for c in calls if c[0] == "softmax_rows")
        assert cache == {}


def test_attention_refuses_narrow_heads_only_with_more_than_one(monkeypatch):
    """A head is a column view of the projections only where its width is a multiple of 4; one head is the whole buffer at any width."""
    for name in ("gemm_normed", "gemm_weight_times_normed_t", "gemm", "softmax_rows", "make_epilogue"):
        monkeypatch.setattr(_lib, name, lambda *a, **k: None)
    monkeypatch.setattr(_lib, "attention256_ok", lambda *a: False)
    monkeypatch.setattr(_lib, "attention_heads_ok", lambda *a: False)
    monkeypatch.setattr(_lib, "gemm_colstats_split", lambda *a: 0)
    C = 6
    gn = torch.nn.GroupNorm(1, C)
    x = nhwc._T(torch.zeros(1, 4, C), 2, 2, C)
    n = nhwc._T(torch.zeros(1, 4, C), 2, 2, C, norm=nhwc.NormedBy.of(gn, C, 4))
    w = (torch.zeros(2 * C, C), torch.zeros(2 * C), torch.zeros(C, C), torch.zeros(C), torch.zeros(C, C), torch.zeros(C))
    assert _Executor()._attention({}, x, n, *w, {}, "k", heads=1).C == C
    with pytest.raises(NotImplementedError):
        _Executor()._attention({}, x, n, *w, {}, "k", heads=3)
