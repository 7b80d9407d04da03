"""Every fp32 upfirdn2d kernel route, element by element against an fp64 oracle (python -m pytest -m gpu).

`idiff_upfirdn2d_f32` chooses one of nine kernels (planes_whole and nhwc_rows in three forms each) through a chain of
admission tests; `_lib.upfirdn2d_route` reports the choice for a geometry.  test_hip_ops.py checks about 45 hand-picked
geometries, mostly the score networks' own, with a norm-wise tolerance.  This file adds:

(a) the admission boundaries of every route, at and one step past each limit (pads, alignment, plane and output sizes,
    kernel sizes, `minor`, IDIFF_UFD_ROWS), with the route each case takes written down as data;
(b) a seeded sweep of a few hundred geometries (up / down 1..4, pads -2..8 with some large trailing pads, kernels 1..9,
    planes 1..80, major 1..300) that must reach every route at least 5 times;
(c) the fp16 and fp64 entry points on about 50 of those geometries;
(d) first and second derivatives on 40 geometries, negative derivative pads and dropped samples included;
(e) the NHWC row kernels just past 2^24 workgroups of 256 lanes (the 2^32 work-item limit of one grid dimension);
(f) the routes of every shape the existing tests, the bench and the score networks run, which must not move.

Every element y must satisfy |y - ref| <= (kh kw + 2)(u + 2^-53)(|x| * |k|) + tiny, where ref is the oracle in fp64 on
the same inputs, |x| * |k| the same op on absolute values, and u the unit roundoff of the kernel's accumulation (2^-24 for
fp32 and fp16, 2^-53 for fp64; 2^-53 is the oracle's own rounding).  This holds for any summation order, and a missing,
duplicated or misplaced tap exceeds it: taps are +-U[0.5, 1.5] and inputs are nonzero.  fp16 adds one half-precision ulp for
the final rounding.  Outputs are prefilled with NaN, so an element left unwritten fails.
"""
import os

import numpy as np
import pytest
import torch

from id_diff_amd import _lib, op
from id_diff_amd.op.upfirdn2d import upfirdn2d_xy
from oracle.ops import upfirdn2d_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("planes_fir4", "planes_rowslide", "planes_down2", "planes_whole<0>", "planes_whole<1>", "planes_whole<-1>", "planes_lds",
          "nhwc_up2_block", "nhwc_rows<0>", "nhwc_rows<1>", "nhwc_rows<-1>", "nhwc_vec4", "generic")
ALIGNED = 1 << 16                      # a 16-byte-aligned stand-in address for route queries of production shapes


# ------------------------------------------------------------------ geometry and reference
class Case:
    """One call of idiff_upfirdn2d_f32: [major, in_h, in_w, minor] in, FIR kh x kw, factors and pads per axis; x / out
    shifted by `xoff` / `ooff` elements from their (16-byte aligned) allocation; `rows` sets IDIFF_UFD_ROWS."""

    def __init__(self, major, in_h, in_w, minor, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1, xoff=0, ooff=0, rows=False):
        self.geom = (major, in_h, in_w, minor, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1)
        self.xoff, self.ooff, self.rows = xoff, ooff, rows
        self.major, self.in_h, self.in_w, self.minor, self.kh, self.kw = self.geom[:6]
        self.ux, self.uy, self.dx, self.dy, self.px0, self.px1, self.py0, self.py1 = self.geom[6:]
        self.out_h = _lib.upfirdn2d_out_size(in_h, uy, dy, py0, py1, kh)
        self.out_w = _lib.upfirdn2d_out_size(in_w, ux, dx, px0, px1, kw)

    def raw_args(self):
        return (self.major, self.in_h, self.in_w, self.minor, self.ux, self.uy, self.dx, self.dy, self.px0, self.px1, self.py0, self.py1)

    def route_args(self):
        return (self.major, self.in_h, self.in_w, self.minor, self.kh, self.kw) + self.geom[6:]

    def oracle_cost(self):
        """Multiply-adds of the oracle (its convolution runs over the zero-stuffed, padded planes)."""
        h = self.in_h * self.uy + max(self.py0, 0) + max(self.py1, 0)
        w = self.in_w * self.ux + max(self.px0, 0) + max(self.px1, 0)
        return self.major * self.minor * h * w * self.kh * self.kw

    def __repr__(self):
        extra = "".join([f" xoff={self.xoff}" if self.xoff else "", f" ooff={self.ooff}" if self.ooff else "", " ROWS" if self.rows else ""])
        return f"Case{self.geom}{extra}"


def _taps(kh, kw, g):
    """+-U[0.5, 1.5]: no tap near zero, so a tap that is dropped, doubled or misplaced shows."""
    mag = torch.rand(kh, kw, generator=g, dtype=torch.float64) + 0.5
    return torch.where(torch.rand(kh, kw, generator=g) < 0.5, -mag, mag)


def _inputs(shape, g):
    """+-U[0.25, 2]: no input is zero."""
    mag = torch.rand(*shape, generator=g, dtype=torch.float64) * 1.75 + 0.25
    return torch.where(torch.rand(*shape, generator=g) < 0.5, -mag, mag)


def _oracle_nhwc(x, k, c):
    """The fp64 oracle on [major, H, W, minor] data: value and |x| * |k|."""
    xn = x.permute(0, 3, 1, 2)
    args = (c.ux, c.uy, c.dx, c.dy, c.px0, c.px1, c.py0, c.py1)
    ref = upfirdn2d_ref(xn, k, *args).permute(0, 2, 3, 1)
    mag = upfirdn2d_ref(xn.abs(), k.abs(), *args).permute(0, 2, 3, 1)
    return ref, mag


def _unit(dtype):
    return 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24      # fp16 accumulates in fp32


def _ulp16(v):
    a = v.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def assert_elementwise(y, ref, mag, ntaps, dtype, what):
    """|y - ref| <= (ntaps + 2)(u + 2^-53) |x|*|k| + tiny (+ one half ulp for fp16), every element; NaN fails."""
    y = y.double().cpu()
    bound = (ntaps + 2) * (_unit(dtype) + 2.0 ** -53) * mag + 1e-30
    if dtype == torch.float16:
        bound = bound + _ulp16(ref.abs() + bound)
    err = (y - ref).abs()
    bad = ~(err <= bound)
    if bad.any():
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {y.numel()} elements out of bound; first at {idx}: got {float(y[idx])}, "
                             f"want {float(ref[idx])} +- {float(bound[idx])}")


def _alloc(numel, dtype, off, fill=None):
    buf = torch.empty(numel + 8, device=DEV, dtype=dtype)
    if fill is not None:
        buf.fill_(fill)
    return buf[off:off + numel]


def run_case(c, dtype=torch.float32, seed=0, expect_route=None):
    """One raw call on NHWC-ordered data (minor == 1 is the NCHW view op.upfirdn2d passes), checked element by element."""
    g = torch.Generator().manual_seed(seed)
    x64 = _inputs((c.major, c.in_h, c.in_w, c.minor), g).to(dtype).double()      # exact in the kernel's dtype
    k64 = _taps(c.kh, c.kw, g).to(dtype).double()
    x = _alloc(x64.numel(), dtype, c.xoff)
    x.copy_(x64.reshape(-1).to(dtype))
    out = _alloc(c.major * c.out_h * c.out_w * c.minor, dtype, c.ooff, fill=float("nan"))
    k = k64.to(dtype).to(DEV)
    with _lib.thread_option("IDIFF_UFD_ROWS", int(c.rows)):
        if dtype == torch.float32:
            route = _lib.upfirdn2d_route(x, out, *c.route_args())
            if expect_route is not None:
                assert route == expect_route, f"{c}: route {route}, recorded {expect_route}"
        _lib.upfirdn2d_raw(x, k, out, *c.raw_args())
    ref, mag = _oracle_nhwc(x64, k64, c)
    assert_elementwise(out.reshape(c.major, c.out_h, c.out_w, c.minor), ref, mag, c.kh * c.kw, dtype, repr(c))
    return route if dtype == torch.float32 else None


# ------------------------------------------------------------------ (a) admission boundaries
C = Case
# (case, the route recorded by the admission chain before the frame / grid fixes below)
BOUNDARY = [
    # planes_fir4: up = down = 1, k <= 4x4, 0 <= pad0 <= 4, in_w % 4 == 0, in_h in_w <= 4096, x aligned, not ROWS
    (C(8, 16, 16, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "planes_fir4"),
    (C(8, 16, 16, 1, 4, 4, 1, 1, 1, 1, 4, 1, 4, 1), "planes_fir4"),                # pad0 4
    (C(8, 16, 16, 1, 4, 4, 1, 1, 1, 1, 5, 1, 2, 2), "planes_rowslide"),                # pad_x0 5
    (C(8, 16, 16, 1, 4, 4, 1, 1, 1, 1, 2, 2, 5, 1), "planes_rowslide"),                # pad_y0 5
    (C(8, 16, 16, 1, 4, 4, 1, 1, 1, 1, -1, 4, 2, 2), "planes_rowslide"),               # pad_x0 -1
    (C(8, 16, 16, 1, 4, 4, 1, 1, 1, 1, 2, 2, -1, 4), "planes_rowslide"),               # pad_y0 -1
    (C(8, 16, 17, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "planes_rowslide"),                # in_w % 4 == 1
    (C(3, 64, 64, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "planes_fir4"),                # in_h in_w 4096, out_h 65
    (C(3, 41, 100, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "planes_whole<0>"),               # 4100
    (C(8, 16, 16, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2, xoff=1), "planes_rowslide"),        # x 4 bytes off
    (C(8, 16, 16, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2, ooff=1), "planes_fir4"),        # out 4 bytes off (fir4 stores scalars)
    (C(8, 16, 16, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2, rows=True), "planes_rowslide"),
    (C(8, 16, 16, 1, 4, 5, 1, 1, 1, 1, 2, 2, 2, 2), "planes_whole<-1>"),                # kw 5
    (C(8, 16, 16, 1, 5, 4, 1, 1, 1, 1, 2, 2, 2, 2), "planes_whole<-1>"),                # kh 5
    (C(8, 16, 16, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0), "planes_fir4"),                # 1 x 1 taps, no pads
    (C(1, 4, 4, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "planes_fir4"),                  # single small plane
    # planes_rowslide: up = down = 1, k <= 4x4, out_h <= 128, in_h in_w <= 4096
    (C(6, 64, 64, 1, 4, 4, 1, 1, 1, 1, 5, 5, 5, 5), "planes_rowslide"),                # 4096 with pad0 5, out 71
    (C(6, 17, 241, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "planes_whole<0>"),               # 4097
    (C(4, 127, 31, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "planes_rowslide"),               # out_h 128
    (C(4, 128, 31, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "planes_whole<0>"),               # out_h 129
    (C(5, 9, 7, 1, 3, 2, 1, 1, 1, 1, -2, 3, 6, -1), "planes_rowslide"),                # negative and large pads
    (C(300, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0), "planes_rowslide"),                # 1 x 1 planes
    (C(7, 1, 1, 1, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1), "planes_rowslide"),
    (C(9, 16, 16, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2, xoff=1), "planes_rowslide"),
    # planes_down2: up 1, down 2, k <= 4x4, 0 <= pad0 <= 4, even out_h / out_w, in_w % 4 == 0, in_h in_w <= 4096, x and out aligned
    (C(8, 16, 16, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1), "planes_down2"),
    (C(8, 16, 16, 1, 4, 4, 1, 1, 2, 2, 4, 0, 4, 0), "planes_whole<0>"),                # pad0 4
    (C(8, 16, 16, 1, 4, 4, 1, 1, 2, 2, 5, 1, 1, 1), "planes_whole<0>"),                # pad_x0 5
    (C(8, 16, 16, 1, 4, 4, 1, 1, 2, 2, -1, 3, 1, 1), "planes_whole<0>"),               # pad_x0 -1
    (C(8, 16, 16, 1, 4, 4, 1, 1, 2, 2, 1, 1, 2, 2), "planes_whole<0>"),                # out_h 9 (odd)
    (C(8, 16, 16, 1, 4, 4, 1, 1, 2, 2, 2, 2, 1, 1), "planes_whole<0>"),                # out_w 9 (odd)
    (C(8, 16, 20, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1), "planes_down2"),                # in_w 20, out_w 10
    (C(8, 16, 18, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1), "planes_whole<0>"),                # in_w % 4 == 2
    (C(2, 64, 64, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1), "planes_down2"),                # 4096
    (C(2, 41, 100, 1, 4, 4, 1, 1, 2, 2, 2, 1, 1, 1), "planes_whole<0>"),               # 4100
    (C(8, 16, 16, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1, xoff=1), "planes_whole<0>"),
    (C(8, 16, 16, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1, ooff=1), "planes_whole<0>"),
    (C(8, 16, 16, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1, rows=True), "planes_whole<0>"),
    (C(8, 16, 16, 1, 4, 5, 1, 1, 2, 2, 1, 2, 1, 1), "planes_whole<-1>"),                # kw 5
    (C(300, 4, 4, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1), "planes_down2"),                # 2 x 2 outputs, many planes
    (C(3, 16, 16, 1, 2, 3, 1, 1, 2, 2, 0, 1, 0, 0), "planes_down2"),
    # planes_whole: minor 1, kh kw <= 64, in_h in_w <= 8192, out_h out_w <= 16384; <0> / <1> for up 1 / 2 with k <= 4x4
    (C(3, 64, 128, 1, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1), "planes_whole<0>"),               # 8192
    (C(2, 3, 2731, 1, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1), "planes_lds"),               # 8193
    (C(2, 80, 100, 1, 1, 1, 1, 1, 1, 1, 14, 14, 24, 24), "planes_whole<0>"),           # out 128 x 128 = 16384
    (C(2, 80, 100, 1, 1, 1, 1, 1, 1, 1, 7, 6, 30, 35), "planes_lds"),             # out 145 x 113 = 16385
    (C(2, 64, 64, 1, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1), "planes_whole<1>"),                # up 2: out 128 x 128
    (C(2, 64, 64, 1, 4, 4, 2, 2, 1, 1, 2, 2, 2, 1), "planes_lds"),                # up 2: out 128 x 129
    (C(5, 12, 10, 1, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1), "planes_whole<1>"),
    (C(5, 12, 10, 1, 4, 4, 2, 2, 3, 3, 3, 0, 3, 0), "planes_whole<1>"),
    (C(5, 12, 10, 1, 4, 4, 3, 3, 1, 1, 2, 1, 2, 1), "planes_whole<-1>"),                # up 3
    (C(5, 12, 10, 1, 4, 4, 4, 4, 2, 2, 1, 3, 0, 2), "planes_whole<-1>"),                # up 4
    (C(5, 12, 10, 1, 8, 8, 1, 1, 1, 1, 3, 4, 4, 3), "planes_whole<-1>"),                # kh kw 64
    (C(5, 12, 10, 1, 5, 13, 1, 1, 1, 1, 6, 6, 2, 2), "generic"),               # kh kw 65
    (C(5, 12, 10, 1, 9, 7, 2, 2, 1, 1, 4, 4, 4, 4), "planes_whole<-1>"),                # 63 taps, up 2
    (C(5, 12, 10, 1, 5, 5, 1, 1, 1, 1, 2, 2, 2, 2), "planes_whole<-1>"),
    (C(4, 12, 10, 1, 4, 4, 1, 1, 1, 1, 9, 9, 9, 9), "planes_rowslide"),                # pads far larger than the plane
    (C(4, 12, 10, 1, 4, 4, 1, 1, 3, 3, 1, 1, 1, 1), "planes_whole<0>"),                # down 3
    (C(4, 12, 10, 1, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1, xoff=1, ooff=1), "planes_whole<1>"),
    # planes_lds: minor 1, kh kw <= 64, its own LDS <= 64 KB, grid.y <= 65535
    (C(2, 3, 2731, 1, 3, 3, 1, 1, 1, 1, 2, 0, 1, 1), "planes_lds"),
    (C(2, 96, 96, 1, 8, 8, 1, 1, 8, 8, 0, 0, 0, 0), "planes_lds"),                # 9216 in, down 8
    (C(1, 300, 300, 1, 8, 8, 1, 1, 8, 8, 0, 0, 0, 0), "generic"),              # window past 64 KB
    (C(1, 300, 300, 1, 8, 8, 1, 1, 8, 8, 3, 4, 3, 4), "generic"),
    (C(2, 90, 100, 1, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1), "planes_lds"),
    (C(2, 90, 100, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2, xoff=1, ooff=1), "planes_lds"),
    # NHWC: minor % 4 == 0, minor <= 1024, kh kw <= 64, x and out aligned, major out_h < 2^31
    (C(3, 8, 8, 4, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1), "nhwc_up2_block"),                  # the upsample_2d geometry
    (C(3, 8, 8, 4, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1, rows=True), "nhwc_rows<1>"),
    (C(3, 8, 8, 4, 4, 4, 2, 2, 1, 1, 2, 2, 2, 1), "nhwc_rows<1>"),                  # out_w != 2 in_w
    (C(3, 8, 8, 4, 4, 4, 2, 2, 1, 1, 1, 2, 2, 1), "nhwc_rows<1>"),                  # pad_x0 1
    (C(3, 8, 8, 4, 3, 4, 2, 2, 1, 1, 2, 1, 2, 1), "nhwc_rows<1>"),                  # kh 3
    (C(3, 8, 8, 1028, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1), "nhwc_vec4"),
    (C(3, 8, 8, 4, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1, xoff=1), "generic"),
    (C(3, 8, 8, 4, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1, ooff=1), "generic"),
    (C(3, 12, 10, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "planes_rowslide"),                # minor 1 / 2 / 3 / 4 / 1024 / 1028 / 2048
    (C(3, 12, 10, 2, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "generic"),
    (C(3, 12, 10, 3, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "generic"),
    (C(3, 12, 10, 4, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "nhwc_rows<0>"),
    (C(2, 5, 6, 1024, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "nhwc_rows<0>"),
    (C(2, 5, 6, 1028, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "nhwc_vec4"),
    (C(2, 5, 6, 2048, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "nhwc_vec4"),
    (C(3, 12, 10, 12, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1), "nhwc_rows<0>"),
    (C(3, 12, 10, 12, 4, 4, 2, 2, 2, 2, 1, 2, 1, 2), "nhwc_rows<1>"),
    (C(3, 12, 10, 8, 4, 4, 3, 3, 1, 1, 2, 1, 2, 1), "nhwc_rows<-1>"),
    (C(3, 12, 10, 8, 4, 4, 2, 1, 1, 2, 2, 1, 0, 0), "nhwc_rows<-1>"),                # up_x != up_y
    (C(3, 12, 10, 8, 8, 8, 1, 1, 1, 1, 4, 3, 3, 4), "nhwc_rows<-1>"),                # kh kw 64
    (C(3, 12, 10, 8, 5, 13, 1, 1, 1, 1, 6, 6, 2, 2), "generic"),               # kh kw 65
    (C(3, 12, 10, 8, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2, xoff=1), "generic"),
    (C(3, 12, 10, 8, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2, ooff=1), "generic"),
    (C(3, 12, 10, 8, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2, rows=True), "nhwc_rows<0>"),
    (C(1, 1, 1, 8, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0), "nhwc_rows<0>"),
    (C(2, 9, 7, 4, 3, 2, 1, 1, 1, 1, 9, 9, 9, 9), "nhwc_rows<0>"),                  # pads far larger than the plane
    (C(0, 8, 8, 4, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1), "none"),                  # batch of 0
    (C(0, 16, 16, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2), "none"),
]

# The oversized-frame geometries: one plane's copy in LDS needs more than 64 KB.  These kernels were launched with that LDS
# and no hipFuncSetAttribute; they are now admitted only when one plane fits 64 KB.  (NCHW through op.upfirdn2d.)
OVERSIZED = [
    ((1, 1, 64, 64), 4, 1, (2, 70), "planes_lds"),        # was planes_fir4: frame 76,160 B
    ((1, 1, 63, 63), 4, 1, (2, 60), "planes_whole<0>"),   # was planes_rowslide: 75,728 B
    ((1, 1, 64, 64), 3, 1, (5, 55), "planes_whole<0>"),   # was planes_rowslide: 76,240 B
    ((1, 1, 64, 64), 4, 2, (2, 72), "planes_whole<0>"),   # was planes_down2: frame 77,280 B
]

# upfirdn2d_xy with different factors / pads per axis on every plane route
XY = [
    ((2, 3, 16, 16), 4, 4, 1, 1, 1, 1, 1, 3, 2, 0, "planes_fir4"),
    ((2, 3, 12, 13), 4, 3, 1, 1, 1, 1, 0, 3, 2, 5, "planes_rowslide"),
    ((2, 3, 16, 16), 4, 4, 1, 1, 2, 2, 2, 2, 1, 1, "planes_whole<0>"),
    ((2, 3, 12, 10), 4, 4, 2, 1, 1, 2, 2, 1, 0, 0, "planes_whole<-1>"),
    ((2, 3, 12, 10), 4, 4, 2, 2, 1, 3, 2, 1, 3, 0, "planes_whole<1>"),
    ((2, 3, 12, 10), 3, 5, 1, 3, 2, 1, 0, 2, 1, 1, "planes_whole<-1>"),
    ((1, 2, 100, 90), 4, 4, 1, 3, 1, 1, 1, 2, 2, 1, "planes_lds"),
]


@pytest.mark.parametrize("case,route", BOUNDARY, ids=[repr(c) for c, _ in BOUNDARY])
def test_admission_boundary(case, route):
    got = run_case(case, seed=sum(case.geom) + case.xoff + case.ooff, expect_route=route)
    assert got == route


@pytest.mark.parametrize("shape,ksz,down,pad,route", OVERSIZED)
def test_oversized_frame_nchw(shape, ksz, down, pad, route):
    g = torch.Generator().manual_seed(ksz + down)
    x, k = _inputs(shape, g).float(), _taps(ksz, ksz, g).float()
    c = Case(shape[0] * shape[1], shape[2], shape[3], 1, ksz, ksz, 1, 1, down, down, pad[0], pad[1], pad[0], pad[1])
    assert _lib.upfirdn2d_route(ALIGNED, ALIGNED, *c.route_args()) == route
    y = op.upfirdn2d(x.to(DEV), k.to(DEV), up=1, down=down, pad=pad)
    ref = upfirdn2d_ref(x.double(), k.double(), 1, 1, down, down, pad[0], pad[1], pad[0], pad[1])
    mag = upfirdn2d_ref(x.double().abs(), k.double().abs(), 1, 1, down, down, pad[0], pad[1], pad[0], pad[1])
    assert_elementwise(y, ref, mag, ksz * ksz, torch.float32, f"{shape} k{ksz} down {down} pad {pad}")


@pytest.mark.parametrize("shape,kh,kw,ux,uy,dx,dy,px0,px1,py0,py1,route", XY)
def test_upfirdn2d_xy_plane_routes(shape, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1, route):
    g = torch.Generator().manual_seed(kh * 7 + kw + ux + 3 * dy)
    x, k = _inputs(shape, g).float(), _taps(kh, kw, g).float()
    args = (ux, uy, dx, dy, px0, px1, py0, py1)
    c = Case(shape[0] * shape[1], shape[2], shape[3], 1, kh, kw, *args)
    assert _lib.upfirdn2d_route(ALIGNED, ALIGNED, *c.route_args()) == route
    y = upfirdn2d_xy(x.to(DEV), k.to(DEV), *args)
    ref = upfirdn2d_ref(x.double(), k.double(), *args)
    mag = upfirdn2d_ref(x.double().abs(), k.double().abs(), *args)
    assert_elementwise(y, ref, mag, kh * kw, torch.float32, f"xy {shape} {args}")


def test_batch_of_zero_and_refused_geometries():
    k = torch.ones(4, 4, device=DEV)
    for dtype in (torch.float32, torch.float16, torch.float64):      # an empty tensor's data_ptr() is null: nothing is launched
        y = op.upfirdn2d(torch.empty(0, 3, 16, 16, device=DEV, dtype=dtype), k, up=1, down=2, pad=(1, 1))
        assert y.shape == (0, 3, 8, 8) and y.dtype == dtype
    assert _lib.upfirdn2d_route(0, 0, 0, 16, 16, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1) == "none"
    assert _lib.upfirdn2d_route(ALIGNED, ALIGNED, 4, 2, 2, 1, 5, 5, 1, 1, 1, 1, 0, 0, 0, 0) is None     # kernel > padded input
    assert _lib.upfirdn2d_route(ALIGNED, ALIGNED, 4, 8, 8, 1, 4, 4, 0, 1, 1, 1, 0, 0, 0, 0) is None     # up 0
    assert _lib.upfirdn2d_route(0, ALIGNED, 4, 8, 8, 1, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0) is None           # null input
    with pytest.raises(RuntimeError):
        op.upfirdn2d(torch.zeros(1, 1, 4, 4, device=DEV), torch.ones(3, 3, device=DEV), down=2, pad=(-2, 0))


# ------------------------------------------------------------------ (b) seeded random sweep
def sweep_cases(n=300, seed=20261016):
    """Deterministic list of random geometries.  Every fifth case is drawn free; the others are tilted towards one route
    family in turn (plain FIR, decimation / upsampling by 2, large outputs, NHWC), so that the narrow routes are reached too."""
    rng = np.random.default_rng(seed)
    cases = []
    r = lambda a, b: int(rng.integers(a, b + 1))

    def pad1():
        return r(20, 60) if rng.random() < 0.08 else r(-2, 8)

    while len(cases) < n:
        fam = len(cases) % 5
        minor, xoff, ooff = 1, 0, 0
        px0, px1, py0, py1 = r(-2, 8), pad1(), r(-2, 8), pad1()
        if fam == 0:                                          # free
            ux, uy, dx, dy = r(1, 4), r(1, 4), r(1, 4), r(1, 4)
            kh, kw = r(1, 9), r(1, 9)
            h, w = r(1, 80), r(1, 80)
            minor = int(rng.choice([1, 1, 1, 2, 3, 4, 8, 12]))
        elif fam == 1:                                        # plain FIR, small planes
            ux = uy = dx = dy = 1
            kh, kw = r(1, 5), r(1, 5)
            h, w = r(1, 60), 4 * r(1, 16) if rng.random() < 0.8 else r(1, 60)
            px0, py0 = r(0, 5), r(0, 5)
        elif fam == 2:                                        # decimation by 2 / upsampling by 2
            ux, uy, dx, dy = (1, 1, 2, 2) if rng.random() < 0.7 else (2, 2, 1, 1)
            kh, kw = r(1, 5), r(1, 4)
            h, w = r(1, 64), 4 * r(1, 16) if rng.random() < 0.8 else r(1, 64)
            px0, py0 = r(0, 5), r(-1, 4)
            if rng.random() < 0.8:                            # an even output, as planes_down2 needs
                sx, sy = w * ux + px0 + px1 - kw, h * uy + py0 + py1 - kh
                px1 += dx if sx >= 0 and sx // dx % 2 == 0 else 0
                py1 += dy if sy >= 0 and sy // dy % 2 == 0 else 0
        elif fam == 3:                                        # large planes or outputs
            ux = uy = r(1, 4)
            dx, dy = r(1, 2), r(1, 2)
            kh, kw = r(1, 8), r(1, 8)
            h, w = r(40, 80), r(40, 80)
        else:                                                 # NHWC
            minor = int(rng.choice([4, 8, 16, 64, 256, 1028]))
            u = rng.random()
            ux, uy = (1, 1) if u < 0.3 else (2, 2) if u < 0.75 else (r(1, 3), r(1, 3))
            dx = dy = 1 if rng.random() < 0.6 else r(1, 3)
            u = rng.random()
            kh, kw = (4, 4) if u < 0.5 else (r(1, 4), r(1, 4)) if u < 0.75 else (r(1, 9), r(1, 9))
            h, w = r(1, 24), r(1, 24)
            if rng.random() < 0.25:                           # the upsample_2d geometry
                ux, uy, dx, dy, kh, kw, px0, px1, py0, py1 = 2, 2, 1, 1, 4, 4, 2, 1, 2, 1
        if rng.random() < 0.1:
            xoff = 1
        if rng.random() < 0.05:
            ooff = 1
        rows = bool(rng.random() < 0.1)
        major = r(1, 300)
        c = Case(major, h, w, minor, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1, xoff, ooff, rows)
        # keep the oracle's work per case bounded (~2e6 multiply-adds): fewer planes for the big geometries
        if c.out_h > 0 and c.out_w > 0:
            per_plane = max(1, c.oracle_cost() // major)
            major = max(1, min(major, 2_000_000 // per_plane))
            c = Case(major, h, w, minor, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1, xoff, ooff, rows)
        cases.append(c)
    return cases


SWEEP = sweep_cases()


def test_random_sweep_every_route():
    counts = {}
    for i, c in enumerate(SWEEP):
        if c.out_h <= 0 or c.out_w <= 0:
            # an empty output is refused, as the reference's op refuses it
            x = torch.ones(1, c.minor, c.in_h, c.in_w, device=DEV)
            with pytest.raises(RuntimeError):
                upfirdn2d_xy(x, torch.ones(c.kh, c.kw, device=DEV), c.ux, c.uy, c.dx, c.dy, c.px0, c.px1, c.py0, c.py1)
            assert _lib.upfirdn2d_route(ALIGNED, ALIGNED, *c.route_args()) is None
            counts["refused"] = counts.get("refused", 0) + 1
            continue
        route = run_case(c, seed=i)
        counts[route] = counts.get(route, 0) + 1
    few = {r: counts.get(r, 0) for r in ROUTES if counts.get(r, 0) < 5}
    assert not few, f"the sweep reaches these routes fewer than 5 times: {few} (all: {counts})"


# ------------------------------------------------------------------ (c) fp16 and fp64
def _other_dtype_cases():
    small = [c for c, _ in BOUNDARY if c.major > 0 and c.out_h > 0 and c.oracle_cost() < 2_000_000]
    drawn = [c for c in SWEEP if c.out_h > 0 and c.out_w > 0 and c.oracle_cost() < 1_000_000]
    return small[::2][:30] + drawn[::3][:30]


OTHER = _other_dtype_cases()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
def test_other_dtypes_elementwise(dtype):
    assert len(OTHER) >= 45
    for i, c in enumerate(OTHER):
        run_case(c, dtype=dtype, seed=1000 + i)


# ------------------------------------------------------------------ (d) backward and double backward
def _grad_geometries():
    rng = np.random.default_rng(77)
    r = lambda a, b: int(rng.integers(a, b + 1))
    geo = [
        ((2, 3, 9, 10), 4, 4, 1, 2, (1, 1, 1, 1)), ((2, 3, 9, 10), 4, 4, 2, 1, (2, 1, 2, 1)),
        ((2, 3, 16, 16), 4, 4, 1, 1, (2, 2, 2, 2)), ((2, 3, 9, 10), 4, 4, 1, 1, (5, 1, 4, 0)),     # pad0 >= kw
        ((2, 2, 8, 8), 3, 3, 1, 1, (6, -1, 3, 2)), ((2, 2, 12, 11), 4, 4, 1, 3, (0, -2, 1, -1)),   # down > up, dropped samples
        ((2, 2, 12, 11), 2, 5, 2, 4, (1, 3, -1, 0)), ((1, 2, 16, 16), 4, 4, 1, 2, (1, 40, 1, 40)),
    ]
    while len(geo) < 40:
        kh, kw = r(1, 6), r(1, 6)
        up, down = r(1, 3), r(1, 4)
        shape = (r(1, 2), r(1, 3), r(4, 20), r(4, 20))
        pad = (r(-2, 8), r(-2, 8), r(-2, 8), r(-2, 8))
        if len(geo) % 3 == 0:
            pad = (kw + r(0, 2), pad[1], kh + r(0, 2), pad[3])                                     # negative derivative pads
        oh = _lib.upfirdn2d_out_size(shape[2], up, down, pad[2], pad[3], kh)
        ow = _lib.upfirdn2d_out_size(shape[3], up, down, pad[0], pad[1], kw)
        if oh > 0 and ow > 0:
            geo.append((shape, kh, kw, up, down, pad))
    return geo


GRAD = _grad_geometries()


@pytest.mark.parametrize("shape,kh,kw,up,down,pad", GRAD)
def test_backward_and_double_backward_elementwise(shape, kh, kw, up, down, pad):
    """op.upfirdn2d's derivatives (the same HIP kernel with swapped factors and complementary pads) against torch.autograd
    through the fp64 oracle; the bound's magnitude term is the same derivative with |k| and |grad_output|."""
    g = torch.Generator().manual_seed(sum(shape) * 31 + kh * 7 + kw + up * 3 + down)
    x, k = _inputs(shape, g).float(), _taps(kh, kw, g).float()
    px0, px1, py0, py1 = pad
    args = (up, up, down, down, px0, px1, py0, py1)

    def oracle_grad(kk, go):
        xc = x.double().clone().requires_grad_(True)
        gi, = torch.autograd.grad(upfirdn2d_ref(xc, kk, *args), xc, go)
        return gi

    oh = _lib.upfirdn2d_out_size(shape[2], up, down, py0, py1, kh)
    ow = _lib.upfirdn2d_out_size(shape[3], up, down, px0, px1, kw)
    go = _inputs((shape[0], shape[1], oh, ow), g).float()
    xd = x.to(DEV).requires_grad_(True)
    yd = upfirdn2d_xy(xd, k.to(DEV), *args)
    god = go.to(DEV).requires_grad_(True)
    gi, = torch.autograd.grad(yd, xd, god, create_graph=True)
    assert gi.shape == x.shape
    assert_elementwise(gi.detach(), oracle_grad(k.double(), go.double()), oracle_grad(k.double().abs(), go.double().abs()),
                       kh * kw, torch.float32, f"d/dx {shape} k{kh}x{kw} up {up} down {down} pad {pad}")
    # double backward: d(gi . probe)/d(grad_output) is the forward op applied to probe
    probe = _inputs(x.shape, g).float()
    gg, = torch.autograd.grad(gi, god, probe.to(DEV))
    assert_elementwise(gg, upfirdn2d_ref(probe.double(), k.double(), *args), upfirdn2d_ref(probe.double().abs(), k.double().abs(), *args),
                       kh * kw, torch.float32, f"d2 {shape} k{kh}x{kw} up {up} down {down} pad {pad}")


# ------------------------------------------------------------------ (e) grid limits of the NHWC row kernels
MAJOR_E = (1 << 20) + 1     # 16 rows per plane: 2^24 + 16 rows (or input rows) in all


@pytest.mark.parametrize("name,geom,route", [
    ("nhwc_rows", (MAJOR_E, 16, 1, 4, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1), "nhwc_vec4"),        # was nhwc_rows<0>
    ("nhwc_up2_block", (MAJOR_E, 16, 1, 4, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1), "nhwc_vec4"),   # was nhwc_up2_block
])
def test_nhwc_rows_past_2_pow_24_workgroups(name, geom, route):
    c = Case(*geom)
    g = torch.Generator(device=DEV).manual_seed(5)
    x = (torch.rand(c.major, c.in_h, c.in_w, c.minor, device=DEV, generator=g) * 1.75 + 0.25)
    x = torch.where(torch.rand(x.shape, device=DEV, generator=g) < 0.5, -x, x)
    k64 = _taps(c.kh, c.kw, torch.Generator().manual_seed(6)).float().double()
    out = torch.full((c.major, c.out_h, c.out_w, c.minor), float("nan"), device=DEV)
    assert _lib.upfirdn2d_route(x, out, *c.route_args()) == route
    _lib.upfirdn2d_raw(x, k64.float().to(DEV), out, *c.raw_args())
    assert not bool(torch.isnan(out).any()), f"{name}: outputs left unwritten"
    # planes are independent: the oracle on the first, the last and the planes around (input or output) row 2^24
    pivot = (1 << 24) // 16
    for lo, hi in ((0, 2), (pivot - 2, pivot + 1)):
        sub = Case(hi - lo, *geom[1:])
        ref, mag = _oracle_nhwc(x[lo:hi].double().cpu(), k64, sub)
        assert_elementwise(out[lo:hi], ref, mag, c.kh * c.kw, torch.float32, f"{name} planes {lo}..{hi - 1}")


# ------------------------------------------------------------------ (f) production shapes keep their routes
def _production():
    """(description, Case, route recorded before the fixes): the shapes of test_hip_ops.py's upfirdn2d tests (their
    derivative calls included), the goldens, and the NHWC calls of the score networks at B = 128."""
    out = []

    def nchw(tag, shape, k, up, down, pad, rows=False):
        n, ch, h, w = shape
        px0, px1, py0, py1 = pad if len(pad) == 4 else (pad[0], pad[1], pad[0], pad[1])
        ux, uy, dx, dy = (up, up, down, down) if isinstance(up, int) else up + down
        out.append((tag, Case(n * ch, h, w, 1, k[0], k[1], ux, uy, dx, dy, px0, px1, py0, py1, rows=rows)))

    for s, up, down, pad in [((128, 128, 32, 32), 1, 2, (1, 1)), ((128, 256, 16, 16), 2, 1, (2, 1)), ((128, 3, 32, 32), 1, 1, (2, 2)),
                             ((3, 5, 70, 130), 1, 2, (1, 1)), ((2, 3, 37, 129), 2, 3, (3, 0)), ((16, 256, 16, 16), 2, 1, (2, 1))]:
        nchw("nchw_vs_oracle", s, (4, 4), up, down, pad)
    for s, pad, ksz in [((128, 256, 16, 16), (1, 1), 4), ((128, 256, 8, 8), (1, 1), 4), ((5, 7, 32, 32), (1, 1), 4),
                        ((3, 33, 16, 24), (1, 1), 4), ((2, 9, 16, 16), (2, 2), 4), ((2, 9, 16, 16), (3, 1), 4), ((2, 9, 12, 16), (0, 0), 2),
                        ((2, 5, 16, 16), (1, 2), 3)]:
        nchw("down2_block", s, (ksz, ksz), 1, 2, pad)
        nchw("down2_block ROWS", s, (ksz, ksz), 1, 2, pad, rows=True)
    for s, pad, ksz in [((128, 128, 16, 16), (2, 2), 4), ((128, 256, 8, 8), (2, 2), 4), ((128, 3, 32, 32), (2, 2), 4),
                        ((3, 33, 16, 24), (2, 2), 4), ((2, 9, 16, 16), (1, 2), 4), ((2, 9, 12, 16), (0, 0), 3), ((2, 5, 16, 16), (3, 0), 2),
                        ((1, 1, 4, 4), (2, 2), 4)]:
        nchw("fir_strip", s, (ksz, ksz), 1, 1, pad)
        nchw("fir_strip ROWS", s, (ksz, ksz), 1, 1, pad, rows=True)
    for up, down, pad in [(1, 2, (1, 1)), (2, 1, (2, 1)), (1, 1, (2, 2)), (2, 3, (3, 0)), (1, 1, (0, 0))]:
        n, ch, h, w, kh, kw = 2, 3, 9, 10, 4, 4
        nchw("backward fwd", (n, ch, h, w), (kh, kw), up, down, pad)
        oh = _lib.upfirdn2d_out_size(h, up, down, pad[0], pad[1], kh)
        ow = _lib.upfirdn2d_out_size(w, up, down, pad[0], pad[1], kw)
        gp = (kw - pad[0] - 1, w * up - ow * down + pad[0] - up + 1, kh - pad[0] - 1, h * up - oh * down + pad[0] - up + 1)
        nchw("backward grad", (n, ch, oh, ow), (kh, kw), down, up, gp)
    for mode in [(1, 2, 1, 1), (2, 1, 2, 1), (1, 1, 2, 2)]:
        up, down, p0, p1 = mode
        for ch in (4, 8, 128, 3):
            out.append(("nhwc_minor", Case(3, 12, 10, ch, 4, 4, up, up, down, down, p0, p1, p0, p1)))
    z = np.load(os.path.join(ROOT, "tests", "golden", "upfirdn2d.npz"))
    for i in range(int(z["n_cases"])):
        up, down, p0, p1 = (int(v) for v in z[f"c{i}::params"])
        nchw(f"golden c{i}", z[f"c{i}::x"].shape, z[f"c{i}::k"].shape, up, down, (p0, p1))
    ux, uy, dx, dy, px0, px1, py0, py1 = (int(v) for v in z["xy::params"])
    nchw("golden xy", z["xy::x"].shape, z["xy::k"].shape, (ux, uy), (dx, dy), (px0, px1, py0, py1))
    # the score networks' FIR calls, NHWC (models/ncsnpp.py _fir), B = 128
    for hw, ch in [(32, 128), (16, 256), (8, 256)]:
        out.append((f"net down2 {hw}", Case(128, hw, hw, ch, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)))
    for hw, ch in [(32, 3), (16, 128), (8, 256)]:
        out.append((f"net fir {hw}", Case(128, hw, hw, ch, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)))
    for hw in (4, 8, 16):
        out.append((f"net up2 {hw}", Case(128, hw, hw, 256, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)))
    return out


PRODUCTION = _production()
PRODUCTION_ROUTES = {   # repr(Case) -> route, recorded before the frame and grid fixes
    'Case(16384, 32, 32, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'planes_down2',
    'Case(32768, 16, 16, 1, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)': 'planes_whole<1>',
    'Case(384, 32, 32, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'planes_fir4',
    'Case(15, 70, 130, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'planes_lds',
    'Case(6, 37, 129, 1, 4, 4, 2, 2, 3, 3, 3, 0, 3, 0)': 'planes_whole<1>',
    'Case(4096, 16, 16, 1, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)': 'planes_whole<1>',
    'Case(32768, 16, 16, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'planes_down2',
    'Case(32768, 16, 16, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1) ROWS': 'planes_whole<0>',
    'Case(32768, 8, 8, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'planes_down2',
    'Case(32768, 8, 8, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1) ROWS': 'planes_whole<0>',
    'Case(35, 32, 32, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'planes_down2',
    'Case(35, 32, 32, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1) ROWS': 'planes_whole<0>',
    'Case(99, 16, 24, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'planes_down2',
    'Case(99, 16, 24, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1) ROWS': 'planes_whole<0>',
    'Case(18, 16, 16, 1, 4, 4, 1, 1, 2, 2, 2, 2, 2, 2)': 'planes_whole<0>',
    'Case(18, 16, 16, 1, 4, 4, 1, 1, 2, 2, 2, 2, 2, 2) ROWS': 'planes_whole<0>',
    'Case(18, 16, 16, 1, 4, 4, 1, 1, 2, 2, 3, 1, 3, 1)': 'planes_whole<0>',
    'Case(18, 16, 16, 1, 4, 4, 1, 1, 2, 2, 3, 1, 3, 1) ROWS': 'planes_whole<0>',
    'Case(18, 12, 16, 1, 2, 2, 1, 1, 2, 2, 0, 0, 0, 0)': 'planes_down2',
    'Case(18, 12, 16, 1, 2, 2, 1, 1, 2, 2, 0, 0, 0, 0) ROWS': 'planes_whole<0>',
    'Case(10, 16, 16, 1, 3, 3, 1, 1, 2, 2, 1, 2, 1, 2)': 'planes_whole<0>',
    'Case(10, 16, 16, 1, 3, 3, 1, 1, 2, 2, 1, 2, 1, 2) ROWS': 'planes_whole<0>',
    'Case(16384, 16, 16, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'planes_fir4',
    'Case(16384, 16, 16, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2) ROWS': 'planes_rowslide',
    'Case(32768, 8, 8, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'planes_fir4',
    'Case(32768, 8, 8, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2) ROWS': 'planes_rowslide',
    'Case(384, 32, 32, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2) ROWS': 'planes_rowslide',
    'Case(99, 16, 24, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'planes_fir4',
    'Case(99, 16, 24, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2) ROWS': 'planes_rowslide',
    'Case(18, 16, 16, 1, 4, 4, 1, 1, 1, 1, 1, 2, 1, 2)': 'planes_fir4',
    'Case(18, 16, 16, 1, 4, 4, 1, 1, 1, 1, 1, 2, 1, 2) ROWS': 'planes_rowslide',
    'Case(18, 12, 16, 1, 3, 3, 1, 1, 1, 1, 0, 0, 0, 0)': 'planes_fir4',
    'Case(18, 12, 16, 1, 3, 3, 1, 1, 1, 1, 0, 0, 0, 0) ROWS': 'planes_rowslide',
    'Case(10, 16, 16, 1, 2, 2, 1, 1, 1, 1, 3, 0, 3, 0)': 'planes_fir4',
    'Case(10, 16, 16, 1, 2, 2, 1, 1, 1, 1, 3, 0, 3, 0) ROWS': 'planes_rowslide',
    'Case(1, 4, 4, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'planes_fir4',
    'Case(1, 4, 4, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2) ROWS': 'planes_rowslide',
    'Case(6, 9, 10, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'planes_whole<0>',
    'Case(6, 4, 5, 1, 4, 4, 2, 2, 1, 1, 2, 1, 2, 2)': 'planes_whole<1>',
    'Case(6, 9, 10, 1, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)': 'planes_whole<1>',
    'Case(6, 18, 20, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'planes_whole<0>',
    'Case(6, 9, 10, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'planes_rowslide',
    'Case(6, 10, 11, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1)': 'planes_rowslide',
    'Case(6, 9, 10, 1, 4, 4, 2, 2, 3, 3, 3, 0, 3, 0)': 'planes_whole<1>',
    'Case(6, 6, 7, 1, 4, 4, 3, 3, 2, 2, 0, 1, 0, 2)': 'planes_whole<-1>',
    'Case(6, 9, 10, 1, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0)': 'planes_rowslide',
    'Case(6, 6, 7, 1, 4, 4, 1, 1, 1, 1, 3, 3, 3, 3)': 'planes_rowslide',
    'Case(3, 12, 10, 4, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'nhwc_rows<0>',
    'Case(3, 12, 10, 8, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'nhwc_rows<0>',
    'Case(3, 12, 10, 128, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'nhwc_rows<0>',
    'Case(3, 12, 10, 3, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'generic',
    'Case(3, 12, 10, 4, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)': 'nhwc_up2_block',
    'Case(3, 12, 10, 8, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)': 'nhwc_up2_block',
    'Case(3, 12, 10, 128, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)': 'nhwc_up2_block',
    'Case(3, 12, 10, 3, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)': 'generic',
    'Case(3, 12, 10, 4, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'nhwc_rows<0>',
    'Case(3, 12, 10, 8, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'nhwc_rows<0>',
    'Case(3, 12, 10, 128, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'nhwc_rows<0>',
    'Case(3, 12, 10, 3, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'generic',
    'Case(6, 8, 8, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'planes_down2',
    'Case(6, 8, 8, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'planes_fir4',
    'Case(6, 4, 4, 1, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)': 'planes_whole<1>',
    'Case(2, 7, 5, 1, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0)': 'planes_rowslide',
    'Case(2, 7, 5, 1, 3, 3, 2, 2, 1, 1, 1, 1, 1, 1)': 'planes_whole<1>',
    'Case(2, 9, 6, 1, 3, 3, 1, 1, 2, 2, 0, 1, 0, 1)': 'planes_whole<0>',
    'Case(4, 5, 7, 1, 4, 4, 2, 2, 2, 2, 2, 1, 2, 1)': 'planes_whole<1>',
    'Case(3, 6, 6, 1, 4, 4, 3, 3, 2, 2, 1, 2, 1, 2)': 'planes_whole<-1>',
    'Case(2, 8, 9, 1, 3, 3, 1, 1, 1, 1, -1, -2, -1, -2)': 'planes_rowslide',
    'Case(2, 8, 9, 1, 4, 4, 2, 2, 1, 1, -1, 3, -1, 3)': 'planes_whole<1>',
    'Case(1, 5, 5, 1, 2, 3, 1, 1, 1, 1, 1, 1, 1, 1)': 'planes_rowslide',
    'Case(3, 4, 4, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0)': 'planes_fir4',
    'Case(1, 1, 1, 1, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)': 'planes_whole<1>',
    'Case(4, 16, 16, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'planes_down2',
    'Case(4, 33, 17, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'planes_whole<0>',
    'Case(4, 16, 16, 1, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)': 'planes_whole<1>',
    'Case(4, 6, 7, 1, 2, 3, 2, 1, 1, 2, 1, 0, 0, 2)': 'planes_whole<-1>',
    'Case(128, 32, 32, 128, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'nhwc_rows<0>',
    'Case(128, 16, 16, 256, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'nhwc_rows<0>',
    'Case(128, 8, 8, 256, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)': 'nhwc_rows<0>',
    'Case(128, 32, 32, 3, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'generic',
    'Case(128, 16, 16, 128, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'nhwc_rows<0>',
    'Case(128, 8, 8, 256, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2)': 'nhwc_rows<0>',
    'Case(128, 4, 4, 256, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)': 'nhwc_up2_block',
    'Case(128, 8, 8, 256, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)': 'nhwc_up2_block',
    'Case(128, 16, 16, 256, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1)': 'nhwc_up2_block',
}


def test_production_routes_unchanged():
    moved = []
    for tag, c in PRODUCTION:
        with _lib.thread_option("IDIFF_UFD_ROWS", int(c.rows)):
            got = _lib.upfirdn2d_route(ALIGNED, ALIGNED, *c.route_args())
        want = PRODUCTION_ROUTES[repr(c)]
        if got != want:
            moved.append(f"{tag} {c}: {want} -> {got}")
    assert not moved, "production shapes changed kernel:\n" + "\n".join(moved)
