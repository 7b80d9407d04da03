"""Host side of the x2 FIR of an up block's shortcut inside Conv_1's tail (conv2d_wino1d with _lib.with_residual_up2): the 16 polyphase
weights against a brute-force fp64 upfirdn2d, the request and its refusals in front of any launch, and the executor's routing decision with
the library's queries replaced.  No GPU."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import id_diff_amd
from id_diff_amd import _lib
from id_diff_amd.models import nhwc as hip_nhwc


def _fir_kernel():
    """k = outer([1, 3, 3, 1]) normalised and scaled as NCSNpp._pack / _fir(..., "up") do (float32 taps, x 4 for up = 2)"""
    k = np.asarray([1, 3, 3, 1], dtype=np.float32)
    k = np.outer(k, k)
    return (k / np.sum(k)) * np.float32(4.0)


def _upfirdn2d_up2_fp64(x, k, pad0, pad1):
    """zero insertion by 2, padding (pad0, pad1) on both axes, correlation with the flipped kernel: x [H, W] -> [2 H, 2 W], all in fp64"""
    H, W = x.shape
    n = k.shape[0]
    z = np.zeros((2 * H, 2 * W), dtype=np.float64)
    z[::2, ::2] = x
    z = np.pad(z, ((pad0, pad1), (pad0, pad1)))
    kf = k[::-1, ::-1].astype(np.float64)
    OH, OW = z.shape[0] - n + 1, z.shape[1] - n + 1
    out = np.zeros((OH, OW), dtype=np.float64)
    for y in range(OH):
        for xx in range(OW):
            out[y, xx] = np.sum(z[y:y + n, xx:xx + n] * kf)
    return out


def _polyphase_apply(x, taps):
    """out[2 i + a, 2 j + b] = sum_{u, v} x[i - 1 + a + u, j - 1 + b + v] * w[a][b][u][v], zeros outside x: the form the kernel evaluates"""
    H, W = x.shape
    w = np.asarray(taps, dtype=np.float64).reshape(2, 2, 2, 2)
    xp = np.pad(x.astype(np.float64), 1)                 # xp[r + 1, c + 1] = x[r, c]
    out = np.zeros((2 * H, 2 * W), dtype=np.float64)
    for i in range(H):
        for j in range(W):
            for a in (0, 1):
                for b in (0, 1):
                    out[2 * i + a, 2 * j + b] = sum(xp[i + a + u, j + b + v] * w[a, b, u, v] for u in (0, 1) for v in (0, 1))
    return out


@pytest.mark.parametrize("which", ["ramp", "random"])
def test_polyphase_weights_against_brute_force_fp64(which):
    k = _fir_kernel()
    taps = _lib.polyphase_up2(k, 2, 1)
    assert len(taps) == 16 and abs(sum(taps) - 4.0) < 1e-6      # the four phases' weights sum to 1 each
    x = (np.arange(64, dtype=np.float64).reshape(8, 8) + 1.0) if which == "ramp" else np.random.default_rng(5).standard_normal((8, 8))
    ref, got = _upfirdn2d_up2_fp64(x, k, 2, 1), _polyphase_apply(x, taps)
    assert ref.shape == got.shape == (16, 16)
    scale = np.abs(ref).max()
    for a in (0, 1):
        for b in (0, 1):
            err = np.abs(got[a::2, b::2] - ref[a::2, b::2]).max() / scale
            assert err <= 1e-15, (a, b, err)
    # the border outputs see zeros outside the image: with the four weights of their phase they are strictly smaller in magnitude than
    # the same positions of a map continued by its edge values, and equal to the brute force (which pads with zeros)
    edge = np.pad(x, 1, mode="edge")
    cont = _polyphase_apply(edge, taps)[2:-2, 2:-2]
    for sl in ((0, slice(None)), (15, slice(None)), (slice(None), 0), (slice(None), 15)):
        assert np.abs(got[sl] - ref[sl]).max() <= 1e-15 * scale
        if which == "ramp":
            assert np.all(np.abs(got[sl]) < np.abs(cont[sl]))


def test_polyphase_weights_are_the_flipped_kernel_by_phase():
    k = _fir_kernel()
    w = np.asarray(_lib.polyphase_up2(k, 2, 1)).reshape(2, 2, 2, 2)
    for a in (0, 1):
        for b in (0, 1):
            for u in (0, 1):
                for v in (0, 1):
                    assert w[a, b, u, v] == float(k[3 - (a + 2 * u), 3 - (b + 2 * v)])
    with pytest.raises(RuntimeError, match="4 x 4"):
        _lib.polyphase_up2(np.ones((2, 2)), 2, 1)
    with pytest.raises(RuntimeError, match="pads"):
        _lib.polyphase_up2(k, 1, 2)


def test_query_and_switch():
    q = _lib.conv2d_wino1d_resup_ok
    assert q(2, 8, 8, 32, 64) and q(2, 16, 16, 32, 64) and q(2, 32, 32, 64, 128)
    assert not q(2, 4, 4, 32, 64) and not q(2, 64, 64, 32, 64)             # rows of 4 and 64 pixels: not built
    assert not q(2, 16, 16, 24, 64)                                        # what conv2d_wino1d_ok refuses
    for switch in ("IDIFF_NO_FUSED_RES_UP", "IDIFF_NO_WINO1D"):
        with _lib.thread_option(switch, 1):
            assert not q(2, 16, 16, 32, 64), switch
    assert q(2, 16, 16, 32, 64)


def test_entry_point_refuses_before_any_device_call():
    lib, fake = _lib.lib(), 0x10000
    taps = (ctypes.c_float * 16)(*([0.25] * 16))
    call = lambda H=16, W=16, lo=fake, ep=None, t=taps: lib.idiff_conv2d_wino1d_resup_f32(fake, fake, fake, 2, H, W, 32, 64, ep, lo, t, None)
    for kw, text in ((dict(W=4, H=4), b"not served"), (dict(W=64, H=64), b"not served"), (dict(H=15), b"not served"),
                     (dict(lo=fake + 4), b"16-byte aligned"), (dict(lo=None), b"required"), (dict(t=None), b"required")):
        assert call(**kw) != 0 and text in lib.idiff_last_error(), (kw, lib.idiff_last_error())
    ep = _lib.make_epilogue()
    ep.residual = fake
    assert call(ep=ctypes.byref(ep)) != 0 and b"already carries a residual" in lib.idiff_last_error()
    with _lib.thread_option("IDIFF_NO_FUSED_RES_UP", 1):
        assert call() != 0 and b"IDIFF_NO_FUSED_RES_UP" in lib.idiff_last_error()


def test_executor_asks_for_the_request_only_on_the_wino1d_route(monkeypatch):
    """NhwcExecutor._up2_residual_taps with the library's queries replaced: the taps come back only for a GroupNorm's output with no norm
    pending for the loader, on the wino1d route, where the kernel's query says yes."""
    monkeypatch.setattr(hip_nhwc, "WINO1D_MIN_WORKGROUPS", 1)
    asked = []
    monkeypatch.setattr(_lib, "conv2d_wino1d_ok", lambda B, H, W, cin, cout: W in (4, 8, 16, 32, 64))
    monkeypatch.setattr(_lib, "conv2d_wino1d_resup_ok", lambda *g: asked.append(g) or g[2] in (8, 16, 32))
    for name in ("conv2d_winograd43h_ok", "conv2d_winograd43_ok", "conv2d_winograd_ok"):
        monkeypatch.setattr(_lib, name, lambda *g: True)
    admitted = {"ok": True}
    ex = SimpleNamespace(_pairs_ok=lambda norm, transform: admitted["ok"])
    decide = lambda x, cout=64, taps=("t",): hip_nhwc.NhwcExecutor._up2_residual_taps(ex, x, cout, taps)
    t = lambda H, **kw: hip_nhwc._T(torch.empty(2, H * H, 32), H, H, 32, **{"norm": object(), **kw})
    assert decide(t(16)) == ("t",) and decide(t(32)) == ("t",)
    assert asked and asked[0] == (2, 16, 16, 32, 64)
    assert decide(t(8)) is None and len(asked) == 2      # served by the kernel, measured inside the spread: not routed (RESUP_MIN_WIDTH)
    assert decide(t(64)) is None                         # the route is wino1d, the kernel's query says no
    assert decide(t(16), taps=None) is None              # no 4-tap FIR
    assert decide(t(16, norm=None)) is None              # not a GroupNorm's output
    assert decide(t(16, pending=object())) is None       # the loader applies a norm: that kernel form does not take the request
    admitted["ok"] = False                               # not admitted to fp16 pairs: another route
    n = len(asked)
    assert decide(t(16)) is None and len(asked) == n
    admitted["ok"] = True
    monkeypatch.setattr(_lib, "conv2d_wino1d_ok", lambda *g: False)      # the 2-D Winograd route
    assert decide(t(16)) is None and len(asked) == n


def test_request_rides_beside_the_struct_and_other_wrappers_refuse_it():
    lo = torch.zeros(2 * 64 * 64)
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.with_residual_up2(_lib.make_epilogue(), lo, [0.25] * 16)        # a host tensor
    ep = _lib.make_epilogue()
    ep.residual_up2 = _lib.ResidualUp2(lo, tuple([0.25] * 16))
    for what in ("gemm", "conv2d_nhwc", "conv2d_winograd43"):
        with pytest.raises(RuntimeError, match="only conv2d_wino1d serves"):
            _lib._ep_ref(ep, what)
