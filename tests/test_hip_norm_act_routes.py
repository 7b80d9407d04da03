"""Every kernel route of the memory-bound passes (csrc/norm_act.hip, csrc/rng.hip), element by element against fp64 (python -m pytest -m gpu).

Each launch writes into a NaN-filled output that sits between two guard regions of 64 sentinel floats; afterwards the guards must be untouched
and no NaN left (a vec4 tail that runs over, a skipped row), every element must satisfy |out - ref| <= tol, and the route the launcher's
query reports (idiff_*_route: the admission code the launcher itself runs) must be the expected one.  A failure reports the worst flat index
and err / tol.  test_every_route_has_cases asserts that the cases below reach every name the queries can return.

References and bounds (tests/norm_act_cases.py; u = 2^-24; k counts fp32 roundings, each on the magnitude it rounds; device libm and
v_exp_f32 / v_rcp_f32 are allowed 2 u each; nothing is fitted to a kernel's output; tests/test_norm_act_host.py holds a numpy float32 replay
of each expression to the same bounds and shows that ten mutations leave them):
  bit-equal to the fp32 expression on the CPU: concat_cols, nhwc_to_nchw (with rowscale: one product), resample2x up, add_scale ((a + b) s:
      an add then a product cannot contract), nchw_to_nhwc at alpha = 1, beta = 0, affine_act with act none, alpha = 1, beta = 0.
  k u (sum of the terms' magnitudes): nchw_to_nhwc with alpha, beta (k = 2: product and add, or one fma), perturb and the arithmetic of
      perturb_randn on the z_out it returns (k = 2), resample2x down (k = 3: three adds, the product by 1/4 is exact), affine_act's
      v = a alpha + beta (k = 2), and one more rounding u |y| for its product by rowscale.
  activations, on top of the bound on v:  silu u |silu v| (6 + 1.5 |v|) + 1.1 x (exponent -v log2e: one rounding and log2e_f32's 0.22 u =
      1.22 |v| u, counted 1.5; v_exp 2, add 1, v_rcp 2, product 1; slope <= 1.0998);  elu below 0 u (4 |expm1 v| + 1) (expf(v) - 1 cancels);
      lrelu one rounding; relu none.
  GroupNorm, y = act(((x - mean) rstd gamma + beta)(1 + m1) + m2): k u ((|x| + |mean|) rstd |gamma| |1 + m1| + |beta (1 + m1)| + |m2|), k = 6
      without mod (mean and rstd stored in fp32 2, x - mean 1, two products 2, + beta 1), 9 with (1 + m1, the product, + m2), plus the one-pass
      fp64 variance's cancellation, c64 = 1.5 (n + 8) 2^-53 E x^2 / (var + eps) relative on rstd (1e-13 for randn inputs, 131 u at mean 100 /
      std 0.01, where it dominates).  groupnorm_coef: a to 2 u |a|, b to u (|beta| + 2 |mean a|).
  softmax: tol_i = y_i u (A + 3 (|s x_i| + max_j |s x_j|)) + 2^-125, A = exp 2 + per-lane sum (max(ceil(cols / 64), 4 ceil(cols / 256)) terms: the
      vec kernels add four columns per run) + 6 shuffle steps + reciprocal 2 + product 1; entries at -inf are exactly 0.
  positional_embed: tol = |arg| u (r |e| + 4) + 4 u, e the exponent handed to expf, r = 1 in mode 0 and 2 in mode 1 (its division rounds
      e once more).  fourier_embed: 3 u |arg| + 4 u.
  Philox stream: z_out against fp64 Box-Muller on the integers of a numpy Philox4x32-10 that reproduces Random123's known answers;
      tol = u r (4 pi + 8), r = sqrt(-2 ln u01).  A wrong counter or key moves z by O(1).

Measured on the MI355X (launches compared, largest err / tol; "bits": equal bits asked and found on every launch):
    op                               route        launches   max err / tol
    groupnorm stats + apply          rows            27        0.466
    groupnorm stats + apply          flat            15        0.438
    groupnorm_apply_colstats         rows             4        0.388      (and the bits of finalize + apply)
    groupnorm_apply_colstats         rows, G > 256    4        0.391      (and the bits of finalize + apply)
    groupnorm_coef                   -                4        0.976  (*)
    softmax_rows                     vec<1>          48        0.351
    softmax_rows                     vec<2>          33        0.438
    softmax_rows                     vec<4>          44        0.342
    softmax_rows                     regs           329        0.308
    softmax_rows                     stream         120        0.265
    affine_act                       vec4 / scalar   21 / 73   0.554 / 0.567  (*)
    affine_act silu on [-20, 20]     scalar           1        0.600  (*)
    affine_act, add_scale, concat_cols, nchw_to_nhwc, nhwc_to_nchw, resample2x up (bits)   26 + 18 + 24 + 5 + 10 + 4 launches, all equal
    nchw_to_nhwc alpha, beta         -                5        0.500
    resample2x down                  -                4        0.714  (*)
    perturb                          -                6        0.499
    perturb_randn z_out              -               36        0.335
    perturb_randn arithmetic         -               36        0.920  (*)
    positional_embed                 mode 0 / 1       3 / 3    0.342 / 0.247
    fourier_embed                    -                3        0.537  (*)
(*) above 0.5, all of them bounds of one to three roundings that correct rounding alone comes close to.  groupnorm_coef: b is ONE rounding
of an fp64 value and u |b| is half a last place just above a power of two (the worst element: b = -0.12530, err 7.3e-9 of the 7.45e-9 half-place
of [1/8, 1/4)).  perturb_randn arithmetic: three roundings (two products, one add) under 2 u (|m x| + |std z|); 0.92 is the worst of 8192
elements, reached where the terms do not cancel.  resample2x down: three adds under 3 u of the magnitudes, 0.71 the worst of 132,000.
affine_act 0.55 / 0.57: act none with rowscale, the add and the product under 2 u + 1 u.  fourier_embed: two roundings of an argument of 65 under 3 u.
No bound was missed and no guard or NaN check failed: the module exposed no kernel bug.  SiLU on the grid: 0.60, at the
large |v|, where the rounded exponent -v log2e contributes 1.22 |v| u of the 1.5 |v| u counted.  Its largest |err| / |silu v| is 1.4e-7 over
|v| <= 2 and 9.8e-7 over |v| >= 10: the error grows with |v| as derived, and the comment in csrc/common.h, which said 3e-7 for all v, now
states the derived bound (2.1e-6 |silu v| at |v| = 20).
"""
import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd import _lib

import norm_act_cases as nc

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENTINEL = -7777.0
REPORT = {}          # (op, route) -> [launches, largest err / tol]
F32 = np.float32


class Out:
    """n floats of NaN between two guards of sentinels; `offset` floats shift the view off 16-byte alignment."""

    def __init__(self, n, offset=0, init=None):
        self.buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL, device=DEV)
        self.lo, self.n = GUARD + offset, n
        self.view = self.buf[self.lo:self.lo + n]
        if init is None:
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)))
        assert (self.view.data_ptr() % 16 == 0) == (offset % 4 == 0)

    def result(self, what):
        host = self.buf.cpu().numpy()
        assert np.all(host[:self.lo] == SENTINEL) and np.all(host[self.lo + self.n:] == SENTINEL), f"{what}: a guard region was written"
        out = host[self.lo:self.lo + self.n]
        assert not np.isnan(out).any(), f"{what}: {int(np.isnan(out).sum())} elements were never written (first: {int(np.isnan(out).argmax())})"
        return out


def dev(a, offset=0):
    """numpy -> device tensor (flat view of the same shape), `offset` floats off a fresh allocation's alignment."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.to(DEV)
    flat = torch.empty(a.size + offset, device=DEV, dtype=t.dtype)
    flat[offset:].copy_(t.reshape(-1))
    return flat[offset:].view(a.shape)


def check(op, route, out, ref, tol, what):
    ratio, i = nc.worst(out, ref, tol)
    rec = REPORT.setdefault((op, route), [0, 0.0])
    rec[0] += 1
    rec[1] = max(rec[1], ratio)
    print(f"[norm_act] {op:28s} {str(route):8s} {what}: err/tol = {ratio:.3f}")
    assert ratio <= 1.0, f"{op} ({route}) {what}: err / tol = {ratio:.3g} at flat index {i}: got {np.ravel(out)[i]!r}, reference {np.ravel(ref)[i]!r}"


# ---------------------------------------------------------------------------------------------- GroupNorm
def gn_device(d):
    return dict(x=dev(d["x"]), x2=dev(d["x2"]), gamma=dev(d["gamma"]), beta=dev(d["beta"]),
                mod=None if d["mod"] is None else dev(d["mod_wide"])[:, nc.MOD_COL0:nc.MOD_COL0 + 2 * (d["C"] + d["C2"])])


def gn_stats_apply(d, act, expect, what):
    B, HW, C, C2, G = d["B"], d["HW"], d["C"], d["C2"], d["G"]
    Ctot = C + C2
    t = gn_device(d)
    if t["mod"] is not None:
        assert t["mod"].stride(0) > 2 * Ctot and (t["mod"].data_ptr() // 4) % 4 != 0
    nsplit = _lib.groupnorm_nsplit(B, HW, Ctot)
    ws = torch.full((B * nsplit * Ctot * 2,), float("nan"), device=DEV, dtype=torch.float64)
    stats = torch.full((B * G * 2,), float("nan"), device=DEV)
    _lib.groupnorm_stats(t["x"], C, t["x2"], C2, B, HW, G, nc.EPS, ws, stats)
    y = Out(B * HW * Ctot)
    route = _lib.groupnorm_apply_route(t["x"], C, t["x2"], C2, B, HW, G, stats, t["gamma"], t["beta"], y.view)
    assert route == expect, f"{what}: route {route}, expected {expect}"
    _lib.groupnorm_apply(t["x"], C, t["x2"], C2, B, HW, G, stats, t["gamma"], t["beta"], act, y.view, mod=t["mod"])
    ref, tol = nc.gn_ref(d, act)
    check("groupnorm stats + apply", route, y.result(what), ref, tol, what)
    return nsplit


@pytest.mark.parametrize("shape", nc.GN_CASES, ids=str)
def test_groupnorm_rows(shape):
    B, HW, C, C2, G = shape
    big = B * HW * (C + C2) > 1 << 20
    d = nc.gn_inputs(*shape, seed=1)
    for act in (("silu",) if big else ("none", "silu")):
        nsplit = gn_stats_apply(d, act, "rows", f"{shape} {act}")
    if shape == (1, 6401, 8, 0, 2):
        assert nsplit == 100 and 99 * -(-HW // nsplit) >= HW            # the last split is empty
    if B == 2048:                                                     # the shapes on the boundary of the four-loads-in-flight loop
        RP, rpb, xblocks = nc.gn_launch_numbers(B, HW, C + C2)
        assert (RP, xblocks) == (4, 1) and HW - 16 in (-1, 0, 1) and rpb >= HW


@pytest.mark.parametrize("shape", nc.GN_FLAT_CASES, ids=str)
def test_groupnorm_flat(shape):
    d = nc.gn_inputs(*shape, seed=1)
    gn_stats_apply(d, "silu", "flat", f"{shape} silu")


@pytest.mark.parametrize("shape,route", list(zip(nc.GN_ACT_SHAPES, ("rows", "flat"))), ids=str)
@pytest.mark.parametrize("mod", [False, True], ids=["plain", "mod"])
def test_groupnorm_every_activation_with_and_without_mod(shape, route, mod):
    d = nc.gn_inputs(*shape, seed=2, mod=mod)
    for act in nc.ACTS:
        gn_stats_apply(d, act, route, f"{shape} {act} mod={mod}")


@pytest.mark.parametrize("shape,route", list(zip(nc.GN_ACT_SHAPES, ("rows", "flat"))), ids=str)
@pytest.mark.parametrize("kind", ["const", "offset"])
def test_groupnorm_zero_variance_and_large_mean(shape, route, kind):
    """const: the variance is exactly 0 (rstd = eps^-1/2).  offset: mean 100, std 0.01."""
    gn_stats_apply(nc.gn_inputs(*shape, seed=3, kind=kind), "silu", route, f"{shape} {kind}")


@pytest.mark.parametrize("case", nc.GN_COLSTATS_CASES, ids=str)
def test_groupnorm_from_column_sums(case):
    """Statistics from [B][ns][C][2] fp64 column sums the test writes itself: against fp64, bit-equal to finalize + apply, and the coefficient
    pair of groupnorm_coef.  G = 512: every thread finishes the groups of its own four channels."""
    B, HW, C, C2, G, ns1, ns2 = case
    Ctot = C + C2
    d = nc.gn_inputs(B, HW, C, C2, G, seed=4)
    t = gn_device(d)
    ws1 = dev(nc.gn_colsums(d["x"], ns1))
    ws2 = dev(nc.gn_colsums(d["x2"], ns2)) if C2 else None
    for act in ("none", "silu"):
        what = f"{case} {act}"
        y = Out(B * HW * Ctot)
        route = _lib.groupnorm_apply_colstats_route(t["x"], C, t["x2"], C2, B, HW, G, ws1, ns1, ws2, ns2, t["gamma"], t["beta"], y.view)
        assert route == "rows"
        _lib.groupnorm_apply_colstats(t["x"], C, t["x2"], C2, B, HW, G, ws1, ns1, ws2, ns2, nc.EPS, t["gamma"], t["beta"], act, y.view)
        out = y.result(what)
        check("groupnorm_apply_colstats", route + (" G>256" if G > 256 else ""), out, *nc.gn_ref(d, act), what)
        stats = torch.full((B * G * 2,), float("nan"), device=DEV)
        _lib.groupnorm_finalize(ws1, ns1, C, ws2, ns2, C2, B, HW, G, nc.EPS, stats)
        y2 = Out(B * HW * Ctot)
        _lib.groupnorm_apply(t["x"], C, t["x2"], C2, B, HW, G, stats, t["gamma"], t["beta"], act, y2.view)
        assert np.array_equal(out, y2.result(what)), f"{what}: not the bits of finalize + apply"
    coef = Out(B * Ctot * 2)
    _lib.groupnorm_coef(ws1, ns1, C, ws2, ns2, C2, B, HW, G, nc.EPS, t["gamma"], t["beta"], coef.view)
    ref, tol = nc.gn_coef_ref(d)
    check("groupnorm_coef", "-", coef.result(str(case)), ref, tol, str(case))


def test_groupnorm_refusals():
    B, HW, C, G = 2, 6, 8, 2
    x, y, ga, be = (torch.zeros(n + 4, device=DEV) for n in (B * HW * C, B * HW * C, C, C))
    stats = torch.zeros(B * G * 2, device=DEV)
    ws = torch.zeros(B * C * 2, device=DEV, dtype=torch.float64)
    ok = (x, C, None, 0, B, HW, G, stats, ga, be, y)
    assert _lib.groupnorm_apply_route(*ok) == "rows"
    bad = {
        "C % 4 != 0": (x, 6, None, 0, B, HW, G, stats, ga, be, y),
        "Ctot % G != 0": (x, C, None, 0, B, HW, 3, stats, ga, be, y),
        "misaligned x": (x[1:], C, None, 0, B, HW, G, stats, ga, be, y),
        "misaligned y": (x, C, None, 0, B, HW, G, stats, ga, be, y[1:]),
        "misaligned gamma": (x, C, None, 0, B, HW, G, stats, ga[1:], be, y),
    }
    for why, a in bad.items():
        assert _lib.groupnorm_apply_route(*a) is None, why
        with pytest.raises(RuntimeError, match="groupnorm_apply"):
            _lib.groupnorm_apply(*a[:10], "none", a[10])
    # column sums: more than 1024 channels; a second source without its sums
    wide = 1032
    xw, yw, gw = torch.zeros(B * HW * wide, device=DEV), torch.zeros(B * HW * wide, device=DEV), torch.zeros(wide, device=DEV)
    wsw = torch.zeros(B * wide * 2, device=DEV, dtype=torch.float64)
    assert _lib.groupnorm_apply_colstats_route(xw, wide, None, 0, B, HW, 8, wsw, 1, None, 0, gw, gw, yw) is None
    with pytest.raises(RuntimeError, match="more than 1024 channels"):
        _lib.groupnorm_apply_colstats(xw, wide, None, 0, B, HW, 8, wsw, 1, None, 0, nc.EPS, gw, gw, "none", yw)
    x2 = torch.zeros(B * HW * 4, device=DEV)
    g12 = torch.zeros(12, device=DEV)
    y12 = torch.zeros(B * HW * 12, device=DEV)
    assert _lib.groupnorm_apply_colstats_route(x, C, x2, 4, B, HW, G, ws, 1, None, 0, g12, g12, y12) is None
    with pytest.raises(RuntimeError, match="second source needs its column sums"):
        _lib.groupnorm_apply_colstats(x, C, x2, 4, B, HW, G, ws, 1, None, 0, nc.EPS, g12, g12, "none", y12)


# ---------------------------------------------------------------------------------------------- softmax
def softmax_launch(x, scale, expect, what, in_place=False, offset=0):
    rows, cols = x.shape
    if in_place:
        y = Out(x.size, offset, init=x)
        src = y.view
    else:
        y = Out(x.size)
        src = dev(x, offset)
    route = _lib.softmax_rows_route(src, y.view, rows, cols, scale)
    assert route == expect, f"{what}: route {route}, expected {expect}"
    _lib.softmax_rows(src, y.view, rows, cols, scale)
    out = y.result(what).reshape(rows, cols)
    ref, tol = nc.softmax_ref(x, scale)
    check("softmax_rows", route, out, ref, tol, what)
    return out


@pytest.mark.parametrize("cols", list(nc.SOFTMAX_COLS))
def test_softmax_every_route(cols):
    for rows in nc.SOFTMAX_ROWS:
        x = nc.softmax_inputs(rows, cols)
        for scale in nc.SOFTMAX_SCALES:
            vec = nc.SOFTMAX_COLS[cols] if scale > 0 else nc.general_route(cols)
            softmax_launch(x, scale, vec, f"{rows} x {cols} scale {scale}")
            softmax_launch(x, scale, vec, f"{rows} x {cols} scale {scale} in place", in_place=True)
            # one float off 16-byte alignment: never a vec kernel, also where cols % 4 == 0
            general = nc.general_route(cols)
            assert not general.startswith("vec")
            softmax_launch(x, scale, general, f"{rows} x {cols} scale {scale} offset input", offset=1)
            softmax_launch(x, scale, general, f"{rows} x {cols} scale {scale} offset in place", in_place=True, offset=1)


@pytest.mark.parametrize("rows,cols", nc.SOFTMAX_WRAP)
def test_softmax_vec_row_loop_wraps(rows, cols):
    """16387 rows: 4097 workgroups of four rows on a grid of 4096, so the first workgroup walks two rows (prefetch, then no prefetch)."""
    x = nc.softmax_inputs(rows, cols)
    softmax_launch(x, 0.25, "vec<1>", f"{rows} x {cols}")
    softmax_launch(x, 0.25, "vec<1>", f"{rows} x {cols} in place", in_place=True)
    softmax_launch(x, 0.25, "regs", f"{rows} x {cols} offset", offset=1)


@pytest.mark.parametrize("kind", ["big", "equal", "masked"])
def test_softmax_edge_inputs(kind):
    """Logits of magnitude 80; a row of equal values; rows with entries at -inf, which must come out exactly 0."""
    for cols in nc.SOFTMAX_COLS:
        if kind == "masked" and cols < 3:
            continue
        x = nc.softmax_inputs(5, cols, kind=kind)
        for offset in (0, 1):
            out = softmax_launch(x, 1.0, nc.SOFTMAX_COLS[cols] if offset == 0 else nc.general_route(cols), f"{kind} 5 x {cols} offset {offset}",
                                 offset=offset)
            if kind == "masked":
                assert np.all(out[~np.isfinite(x)] == 0)
            if kind == "equal":
                assert np.all(out[0] == out[0, 0])


def test_softmax_no_rows_and_refusals():
    e = torch.empty(0, device=DEV)
    assert _lib.softmax_rows_route(e, e, 0, 4, 1.0) == "none"
    _lib.softmax_rows(e, e, 0, 4, 1.0)
    assert _lib.softmax_rows_route(4096, 4096, 3, 0, 1.0) is None and _lib.softmax_rows_route(0, 4096, 3, 4, 1.0) is None


# ---------------------------------------------------------------------------------------------- pointwise maps
def fp32_cpu(expr):
    return np.asarray(expr, F32)


def affine_launch(a, alpha, beta, act, expect, what, offset=0, rowscale=None, inner=0, exact=False):
    src, y = dev(a, offset), Out(a.size, offset)
    rs = dev(rowscale)
    route = _lib.affine_act_route(src, y.view, a.size, rs, inner)
    assert route == expect, f"{what}: route {route}, expected {expect}"
    _lib.affine_act(src, y.view, a.size, alpha, beta, act, rs, inner)
    out = y.result(what)
    if exact:        # act none, alpha = 1, beta = 0: at most the product by rowscale
        ref = a if rowscale is None else fp32_cpu(a * rowscale[np.arange(a.size) // inner])
        check("affine_act (bits)", route, out, ref, 0.0, what)
    else:
        check("affine_act", route, out, *nc.affine_ref(a, alpha, beta, act, rowscale, inner), what)


@pytest.mark.parametrize("n", nc.POINTWISE_N + (nc.WRAP_VEC4_N, nc.WRAP_SCALAR_N))
def test_affine_act_and_add_scale(n):
    g = nc.rng(20 + n)
    a, b = nc.randn32(g, n), nc.randn32(g, n)
    for offset in (0, 1):
        expect = "vec4" if n % 4 == 0 and offset == 0 else "scalar"
        for act in (nc.ACTS if n < 1 << 19 else ("silu",)):
            affine_launch(a, nc.ALPHA, nc.BETA, act, expect, f"n = {n} {act} offset {offset}", offset)
        affine_launch(a, 1.0, 0.0, "none", expect, f"n = {n} identity offset {offset}", offset, exact=True)
        what = f"n = {n} offset {offset}"
        ad, bd, y = dev(a, offset), dev(b, offset), Out(n, offset)
        assert _lib.add_scale_route(ad, bd, y.view, n) == expect
        _lib.add_scale(ad, bd, y.view, n, 0.7071)
        check("add_scale (bits)", expect, y.result(what), fp32_cpu((a + b) * F32(0.7071)), 0.0, what)
    if n % 4 == 0:               # one misaligned operand is enough to leave the vec4 kernel
        assert _lib.add_scale_route(dev(a), dev(b, 1), Out(n).view, n) == "scalar"


def test_silu_error_grows_with_v():
    """act_apply's SiLU on v in [-20, 20] (a alpha + beta is exact at alpha = 1, beta = 0, so v carries no error): u |silu v| (6 + 1.5 |v|).
    Prints the largest relative error over |v| <= 2 and over |v| >= 10 (what csrc/common.h states about it)."""
    a = nc.SILU_GRID
    src, y = dev(a), Out(a.size)
    assert _lib.affine_act_route(src, y.view, a.size) == "scalar"        # 4001 elements
    _lib.affine_act(src, y.view, a.size, 1.0, 0.0, "silu")
    out = y.result("silu grid")
    ref, tol = nc.act_ref("silu", a), nc.act_tol("silu", a, 0.0)
    rel = np.abs(out - ref) / np.maximum(np.abs(ref), 1e-300)
    print(f"[norm_act] silu: max |err| / |silu v| = {rel[np.abs(a) <= 2].max():.3g} over |v| <= 2, {rel[np.abs(a) >= 10].max():.3g} over |v| >= 10")
    check("affine_act silu on [-20, 20]", "scalar", out, ref, tol, "4001 points")


@pytest.mark.parametrize("inner", list(nc.AFFINE_INNER))
def test_affine_act_rowscale(inner):
    rows = 37
    g = nc.rng(30 + inner)
    a, rs = nc.randn32(g, rows * inner), -(g.random(rows).astype(F32) + F32(0.5))
    for act in nc.ACTS:
        affine_launch(a, nc.ALPHA, nc.BETA, act, nc.AFFINE_INNER[inner], f"inner = {inner} {act}", rowscale=rs, inner=inner)
    affine_launch(a, 1.0, 0.0, "none", nc.AFFINE_INNER[inner], f"inner = {inner} identity", rowscale=rs, inner=inner, exact=True)
    affine_launch(a, 1.0, 0.0, "none", "scalar", f"inner = {inner} identity, offset", offset=1, rowscale=rs, inner=inner, exact=True)


def test_pointwise_empty_and_refusals():
    e = torch.empty(0, device=DEV)
    assert _lib.affine_act_route(e, e, 0) == "none" and _lib.add_scale_route(e, e, e, 0) == "none" and _lib.concat_cols_route(e, 4, e, 4, e, 0) == "none"
    _lib.affine_act(e, e, 0)
    _lib.add_scale(e, e, e, 0, 1.0)
    _lib.concat_cols(e, 4, e, 4, e, 0)
    assert _lib.affine_act_route(4096, 4096, -1) is None and _lib.affine_act_route(4096, 4096, 8, 4096, 0) is None
    assert _lib.add_scale_route(4096, 0, 4096, 8) is None and _lib.concat_cols_route(4096, 0, 4096, 4, 4096, 1) is None


CONCAT_WRAPS = [((4, 8), 174764), ((3, 5), 65537)]       # 524292 float4 / 524296 floats: one trip of the grid-stride loop and a few more


@pytest.mark.parametrize("widths,rows", [(w, r) for w in nc.CONCAT_CASES for r in nc.CONCAT_ROWS] + CONCAT_WRAPS, ids=str)
def test_concat_cols(widths, rows):
    Ca, Cb = widths
    g = nc.rng(40 + Ca + rows)
    a, b = nc.randn32(g, rows, Ca), nc.randn32(g, rows, Cb)
    for offset in (0, 1):
        expect = nc.CONCAT_CASES[widths] if offset == 0 else "scalar"
        what = f"{widths} x {rows} offset {offset}"
        ad, bd, y = dev(a, offset), dev(b), Out(rows * (Ca + Cb))
        assert _lib.concat_cols_route(ad, Ca, bd, Cb, y.view, rows) == expect
        _lib.concat_cols(ad, Ca, bd, Cb, y.view, rows)
        check("concat_cols (bits)", expect, y.result(what), np.concatenate([a, b], 1), 0.0, what)


# ---------------------------------------------------------------------------------------------- layout, resampling, perturbation
@pytest.mark.parametrize("shape", nc.LAYOUT_CASES + [nc.LAYOUT_WRAP], ids=str)
def test_layout_changes(shape):
    B, C, HW, Cpad = shape
    g = nc.rng(50 + HW)
    x = nc.randn32(g, B, C, HW)
    xd = dev(x)
    y = Out(B * HW * Cpad)
    _lib.nchw_to_nhwc(xd, y.view, B, C, HW, Cpad)
    nhwc = np.zeros((B, HW, Cpad), F32)
    nhwc[..., :C] = x.transpose(0, 2, 1)
    check("nchw_to_nhwc (bits)", "-", y.result(str(shape)), nhwc, 0.0, str(shape))
    y = Out(B * HW * Cpad)
    _lib.nchw_to_nhwc(xd, y.view, B, C, HW, Cpad, nc.ALPHA, nc.BETA)
    check("nchw_to_nhwc alpha, beta", "-", y.result(str(shape)), *nc.nchw_to_nhwc_ref(x, Cpad, nc.ALPHA, nc.BETA), str(shape))
    src = nc.randn32(g, B, HW, Cpad)                      # the pad channels hold values too: they must not be read into the output
    rs = -(g.random(B).astype(F32) + F32(0.5))
    for scale in (None, rs):
        what = f"{shape} rowscale {'on' if scale is not None else 'off'}"
        y = Out(B * C * HW)
        _lib.nhwc_to_nchw(dev(src), y.view, B, C, HW, Cpad, dev(scale))
        ref = src[..., :C].transpose(0, 2, 1)
        check("nhwc_to_nchw (bits)", "-", y.result(what), ref if scale is None else fp32_cpu(ref * scale[:, None, None]), 0.0, what)


@pytest.mark.parametrize("shape", nc.RESAMPLE_CASES + [nc.RESAMPLE_WRAP], ids=str)
def test_resample2x(shape):
    B, H, W, C = shape
    x = nc.randn32(nc.rng(60 + W), *shape)
    xd = dev(x)
    y = Out(B * 2 * H * 2 * W * C)
    _lib.resample2x_nhwc(xd, y.view, B, H, W, C, 1)
    check("resample2x up (bits)", "-", y.result(str(shape)), x.repeat(2, 1).repeat(2, 2), 0.0, str(shape))
    y = Out(B * (H // 2) * (W // 2) * C)
    _lib.resample2x_nhwc(xd, y.view, B, H, W, C, 0)
    check("resample2x down", "-", y.result(str(shape)), *nc.resample_down_ref(x), str(shape))


def test_resample2x_refusals():
    x, y = torch.zeros(3 * 4 * 8 + 4, device=DEV), torch.zeros(4 * 3 * 4 * 8, device=DEV)
    for args, why in (((1, 3, 4, 8, 0), "even"), ((1, 4, 4, 6, 1), "bad arguments"), ((1, 4, 4, 6, 0), "bad arguments")):
        with pytest.raises(RuntimeError, match=why):
            _lib.resample2x_nhwc(x, y, *args)
    with pytest.raises(RuntimeError, match="aligned"):
        _lib.resample2x_nhwc(x[1:], y, 1, 2, 2, 8, 1)


@pytest.mark.parametrize("D", nc.PERTURB_D)
def test_perturb(D):
    g = nc.rng(70 + D)
    rows = 9
    x, z, std, mc = nc.randn32(g, D), nc.randn32(g, rows, D), g.random(rows).astype(F32), g.random(rows).astype(F32)
    for coeff in (None, mc):
        what = f"D = {D} mean_coeff {'on' if coeff is not None else 'off'}"
        y = Out(rows * D)
        _lib.perturb(dev(x), dev(z), dev(std), dev(coeff), y.view, rows, D)
        check("perturb", "-", y.result(what), *nc.perturb_ref(x, z, std, coeff), what)


# ---------------------------------------------------------------------------------------------- embeddings
@pytest.mark.parametrize("dim", nc.POS_DIMS)
@pytest.mark.parametrize("mode", [0, 1])
def test_positional_embed(dim, mode):
    t = np.array(nc.POS_T, F32)
    y = Out(t.size * dim)
    _lib.positional_embed(dev(t), y.view, t.size, dim, nc.MAX_POSITIONS, mode)
    what = f"dim {dim} mode {mode}"
    check("positional_embed", f"mode {mode}", y.result(what).reshape(t.size, dim), *nc.positional_ref(t, dim, mode), what)


def test_positional_embed_refusals():
    t, y = torch.zeros(3, device=DEV), torch.zeros(64, device=DEV)
    for dim, mode in ((5, 0), (2, 0), (8, 2)):
        with pytest.raises(RuntimeError, match="positional_embed"):
            _lib.positional_embed(t, y, 3, dim, nc.MAX_POSITIONS, mode)


@pytest.mark.parametrize("half", nc.FOURIER_HALF)
def test_fourier_embed(half):
    """t = log sigma over the models' range; B = 17, so B * half = 17, 272 (crossing one workgroup of 256) and 5100."""
    g = nc.rng(80 + half)
    B = 17
    t, W = (g.random(B) * 8.5 - 4.6).astype(F32), (F32(16) * nc.randn32(g, half)).astype(F32)
    y = Out(B * 2 * half)
    _lib.fourier_embed(dev(t), dev(W), y.view, B, half)
    check("fourier_embed", "-", y.result(f"half {half}").reshape(B, 2 * half), *nc.fourier_ref(t, W), f"half {half}")


# ---------------------------------------------------------------------------------------------- the Philox stream
@pytest.mark.parametrize("rows,D", nc.PHILOX_SHAPES)
def test_normal_stream_is_philox4x32_10(rows, D):
    g = nc.rng(90 + rows)
    x, std, mc = nc.randn32(g, D), g.random(rows).astype(F32), g.random(rows).astype(F32)
    for seed in nc.PHILOX_SEEDS:
        for row0 in nc.PHILOX_ROW0:
            for coeff in (None, mc):
                what = f"{rows} x {D} seed {seed} row0 {row0} mean_coeff {'on' if coeff is not None else 'off'}"
                out, z = Out(rows * D), Out(rows * D)
                _lib.perturb_randn(dev(x), dev(std), dev(coeff), out.view, rows, D, row0, seed, z.view)
                zk = z.result(what).reshape(rows, D)
                check("perturb_randn z_out", "-", zk, *nc.normal_stream_ref(rows, D, row0, seed), what)
                check("perturb_randn arithmetic", "-", out.result(what).reshape(rows, D), *nc.perturb_ref(x, zk, std, coeff), what)


def test_perturb_randn_refusals():
    x, std, out = torch.zeros(12, device=DEV), torch.zeros(2, device=DEV), torch.zeros(28, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        _lib.perturb_randn(x, std, None, out, 2, 6, 0, 1)
    with pytest.raises(RuntimeError, match="aligned"):
        _lib.perturb_randn(x, std, None, out[1:], 2, 8, 0, 1)


# ---------------------------------------------------------------------------------------------- coverage and the record
def test_every_route_has_cases():
    """The routes the cases above take, asked of the queries with the cases' own geometry (addresses stand for alignment only), are all the
    names the queries can return."""
    assert nc.routes_reached(_lib) == nc.ALL_ROUTES


def test_zz_report():
    """Prints what the module measured (pytest -s): op, route, launches, largest err / tol."""
    print("\n[norm_act] op                              route      launches   max err/tol")
    for (op, route), (n, ratio) in sorted(REPORT.items()):
        print(f"[norm_act] {op:32s} {route:10s} {n:8d}   {ratio:.3f}")
