"""What the loader-norm tests share (tests/test_wino1d_normload.py: one source, tests/test_wino1d_normload_2src.py: cat[x1, x2] from two):
the producers' column sums, the thresholds that send test-sized batches through the large-batch kernels, the counting wrappers, and the
model run with and without a form's switch.  One request (``ep.normload``) serves both forms, so the counters tell them apart themselves:
by the request's second source and by groupnorm_coef's second set of column sums."""
import torch

from id_diff_amd import _lib
from id_diff_amd.models import nhwc as hip_nhwc


def colsums(xd):
    """the producer's column sums of xd [B, HW, C] ([B, nsplit = 1, C, 2] fp64), as a contraction's epilogue would have written them"""
    return torch.stack([xd.double().sum(dim=1), (xd.double() ** 2).sum(dim=1)], dim=-1).contiguous().view(-1)


def small_batches(monkeypatch):
    monkeypatch.setattr(hip_nhwc, "WINO1D_MIN_WORKGROUPS", 1)
    monkeypatch.setattr(hip_nhwc, "WINO43_MIN_WORKGROUPS", 1)
    monkeypatch.setattr(hip_nhwc, "WINO43_PAIRS_MIN_WORKGROUPS", 1)


def counted(monkeypatch):
    """Counts the passes (gn_apply), the coefficient launches of one source (gn_coef) and of two (gn_coef2), the row-wise convolutions
    (wino1d) and among them those with a loader request of one source (wino1d_nl) and of two (wino1d_nl2)."""
    calls = {"gn_apply": 0, "gn_coef": 0, "gn_coef2": 0, "wino1d": 0, "wino1d_nl": 0, "wino1d_nl2": 0}
    orig_gn, orig_coef, orig_conv = _lib.groupnorm_apply_colstats, _lib.groupnorm_coef, _lib.conv2d_wino1d

    def counted_gn(*a, **k):
        calls["gn_apply"] += 1
        return orig_gn(*a, **k)

    def counted_coef(ws1, ns1, C1, ws2, *a, **k):
        calls["gn_coef" if ws2 is None else "gn_coef2"] += 1
        return orig_coef(ws1, ns1, C1, ws2, *a, **k)

    def counted_conv(x, u, out, B, H, W, Cin, Cout, epilogue=None):
        calls["wino1d"] += 1
        nl = getattr(epilogue, "normload", None)
        if nl is not None:
            calls["wino1d_nl" if nl.x2 is None else "wino1d_nl2"] += 1
            assert nl.x2 is None or (isinstance(nl.C1, int) and 0 < nl.C1 < Cin), nl
        return orig_conv(x, u, out, B, H, W, Cin, Cout, epilogue=epilogue)
    monkeypatch.setattr(_lib, "groupnorm_apply_colstats", counted_gn)
    monkeypatch.setattr(_lib, "groupnorm_coef", counted_coef)
    monkeypatch.setattr(_lib, "conv2d_wino1d", counted_conv)
    return calls


def on_and_off(model, x, t, calls, switch):
    """model(x, t) as it is and under ``switch``, with the calls each forward made"""
    c0 = dict(calls)
    on = model(x, t * 999)
    c_on = {k: calls[k] - c0[k] for k in calls}
    with _lib.thread_option(switch, 1):
        off = model(x, t * 999)
    c_off = {k: calls[k] - c0[k] - c_on[k] for k in calls}
    return on, off, c_on, c_off
