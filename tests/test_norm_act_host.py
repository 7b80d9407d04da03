"""CPU-side checks of the bounds tests/test_hip_norm_act_routes.py holds the memory-bound kernels to (tests/norm_act_cases.py).

The bounds hold for the reference arithmetic alone: a numpy float32 replay of each kernel's expression (same order of operations, exp2 for
the hardware exponential, statistics rounded to fp32) stays inside the bound on every case of the GPU module that replays in a second
or two -- every element, nothing excluded.  And the bounds have teeth: each mutated replay (a wrong group index, a dropped modulation term,
a wrong pitch, a row missing from the statistics, a dropped softmax tail, a wrong rowscale index, swapped halves of an embedding, a wrong
Philox key or counter) leaves the bound on at least one element.  The numpy Philox4x32-10 reproduces Random123's known answers.
"""
import numpy as np
import pytest

import norm_act_cases as nc

REPLAY_MAX = 1 << 20          # elements: the larger cases (the 8M-float row-loop shapes, the flat wrap) are left to the GPU


def inside(out, ref, tol, what):
    ratio, i = nc.worst(out, ref, tol)
    assert ratio <= 1.0, f"{what}: err / tol = {ratio:.3g} at flat index {i}"
    return ratio


def outside(out, ref, tol, what):
    ratio, i = nc.worst(out, ref, tol)
    assert ratio > 1.0, f"{what}: the mutation stays inside the bound (largest err / tol = {ratio:.3g})"


def gn_route(C, C2, B):
    return "rows" if (C + C2) // 4 <= 256 and B <= 65535 else "flat"


def test_philox_known_answers():
    for ctr, key, want in nc.PHILOX_KAT:
        got = nc.philox4x32_10([np.array([c], np.uint64) for c in ctr], key)
        assert tuple(int(g[0]) for g in got) == want


@pytest.mark.parametrize("shape", [s for s in nc.GN_CASES + nc.GN_FLAT_CASES if s[0] * s[1] * (s[2] + s[3]) <= REPLAY_MAX], ids=str)
def test_groupnorm_replay_inside_the_bound(shape):
    B, HW, C, C2, G = shape
    d = nc.gn_inputs(*shape, seed=1)
    for act in ("none", "silu"):
        inside(nc.gn_replay(d, act, gn_route(C, C2, B)), *nc.gn_ref(d, act), f"groupnorm {shape} {act}")


@pytest.mark.parametrize("shape", nc.GN_ACT_SHAPES, ids=str)
@pytest.mark.parametrize("mod", [False, True], ids=["plain", "mod"])
@pytest.mark.parametrize("act", nc.ACTS)
def test_groupnorm_activation_and_mod_replay_inside_the_bound(shape, mod, act):
    d = nc.gn_inputs(*shape, seed=2, mod=mod)
    for route in ("rows", "flat"):           # both expressions at both shapes: the bound does not depend on the route
        inside(nc.gn_replay(d, act, route), *nc.gn_ref(d, act), f"groupnorm {shape} {act} mod={mod} as {route}")


@pytest.mark.parametrize("kind", ["const", "offset"])
@pytest.mark.parametrize("shape", nc.GN_ACT_SHAPES, ids=str)
def test_groupnorm_zero_variance_and_large_mean_replay(shape, kind):
    d = nc.gn_inputs(*shape, seed=3, kind=kind)
    inside(nc.gn_replay(d, "silu", gn_route(shape[2], shape[3], shape[0])), *nc.gn_ref(d, "silu"), f"groupnorm {shape} {kind}")


@pytest.mark.parametrize("shape", nc.GN_COLSTATS_CASES, ids=str)
def test_groupnorm_colstats_and_coef_replay(shape):
    B, HW, C, C2, G, ns1, ns2 = shape
    d = nc.gn_inputs(B, HW, C, C2, G, seed=4)
    inside(nc.gn_replay(d, "silu", "rows"), *nc.gn_ref(d, "silu"), f"groupnorm colstats {shape}")
    # the coefficient pair formed in fp64 from the one-pass moments of the column sums and rounded once
    full = nc.gn_full(d)
    ws = nc.gn_colsums(full, ns1 if not C2 else 1).sum(1)                     # [B, Ctot, 2]
    n = HW * ((C + C2) // G)
    s, q = (ws[..., k].reshape(B, G, -1).sum(2) for k in (0, 1))
    mean = s / n
    rstd = 1.0 / np.sqrt(np.maximum(q / n - mean * mean, 0) + nc.EPS)
    a = np.repeat(rstd, (C + C2) // G, 1) * d["gamma"].astype(np.float64)
    b = d["beta"].astype(np.float64) - np.repeat(mean, (C + C2) // G, 1) * a
    inside(np.stack([a, b], -1).astype(np.float32), *nc.gn_coef_ref(d), f"groupnorm_coef {shape}")


def test_groupnorm_mutations_leave_the_bound():
    # the group of the float4's first channel for all four lanes, cpg = 3
    d = nc.gn_inputs(2, 5, 12, 0, 4, seed=5)
    for route in ("rows", "flat"):
        inside(nc.gn_replay(d, "none", route), *nc.gn_ref(d, "none"), "cpg = 3")
        outside(nc.gn_replay(d, "none", route, mutation="group_of_lane0"), *nc.gn_ref(d, "none"), f"group of lane 0, {route}")
    # the modulation: shift dropped; 1 + m1 on the scale but not on beta
    d = nc.gn_inputs(2, 70, 8, 4, 2, seed=6, mod=True)
    for route in ("rows", "flat"):
        for mutation in ("no_shift", "scale_only"):
            outside(nc.gn_replay(d, "silu", route, mutation=mutation), *nc.gn_ref(d, "silu"), f"{mutation}, {route}")
    # x2 read with C as its pitch
    d = nc.gn_inputs(2, 70, 16, 8, 6, seed=7)
    outside(nc.gn_replay(d, "none", "rows", mutation="x2_pitch"), *nc.gn_ref(d, "none"), "x2 pitch")
    # the last row of a split left out of the statistics (nsplit = 100, rows_per = 65; split 3)
    d = nc.gn_inputs(1, 6401, 8, 0, 2, seed=8)
    outside(nc.gn_replay(d, "none", "rows", mutation=("stats_skip", 100, 3)), *nc.gn_ref(d, "none"), "row missing from the statistics")


def softmax_cases():
    for cols, route in nc.SOFTMAX_COLS.items():
        for rows in nc.SOFTMAX_ROWS:
            yield rows, cols, route
    for rows, cols in nc.SOFTMAX_WRAP:
        yield rows, cols, "vec<1>"


@pytest.mark.parametrize("scale", nc.SOFTMAX_SCALES)
def test_softmax_replay_inside_the_bound(scale):
    worst = 0.0
    for rows, cols, route in softmax_cases():
        x = nc.softmax_inputs(rows, cols)
        routes = {route, nc.general_route(cols)} if scale > 0 else {nc.general_route(cols)}      # unaligned pointers take the general kernel
        for r in sorted(routes):
            worst = max(worst, inside(nc.softmax_replay(x, scale, r), *nc.softmax_ref(x, scale), f"softmax {rows} x {cols} scale {scale} {r}"))
    assert worst > 0


@pytest.mark.parametrize("kind", ["big", "equal", "masked"])
def test_softmax_edge_inputs_replay(kind):
    for cols, route in nc.SOFTMAX_COLS.items():
        x = nc.softmax_inputs(5, cols, kind=kind)
        if kind == "masked" and cols < 3:
            continue
        for r in sorted({route, nc.general_route(cols)}):
            y = nc.softmax_replay(x, 1.0, r)
            ref, tol = nc.softmax_ref(x, 1.0)
            inside(y, ref, tol, f"softmax {kind} cols {cols} {r}")
            if kind == "masked":
                assert np.all(y[~np.isfinite(x)] == 0)


def test_softmax_mutation_leaves_the_bound():
    for cols in (260, 516, 768 + 4, 1020):
        x = nc.softmax_inputs(5, cols)
        outside(nc.softmax_replay(x, 0.25, nc.SOFTMAX_COLS.get(cols, "vec<4>"), mutation="skip_tail"), *nc.softmax_ref(x, 0.25), f"skip tail {cols}")


def test_pointwise_replays_inside_the_bound():
    g = nc.rng(9)
    for n in nc.POINTWISE_N + (nc.WRAP_SCALAR_N, nc.WRAP_VEC4_N):
        a = nc.randn32(g, n)
        for act in (nc.ACTS if n < 1 << 19 else ("silu",)):
            inside(nc.affine_replay(a, nc.ALPHA, nc.BETA, act), *nc.affine_ref(a, nc.ALPHA, nc.BETA, act), f"affine_act n = {n} {act}")
    inside(nc.act_f32("silu", nc.SILU_GRID), nc.act_ref("silu", nc.SILU_GRID), nc.act_tol("silu", nc.SILU_GRID, 0.0), "silu on [-20, 20], v exact")
    for inner in nc.AFFINE_INNER:
        rows = 37
        a, rs = nc.randn32(g, rows * inner), -(g.random(rows).astype(np.float32) + np.float32(0.5))
        for act in nc.ACTS:
            inside(nc.affine_replay(a, nc.ALPHA, nc.BETA, act, rs, inner), *nc.affine_ref(a, nc.ALPHA, nc.BETA, act, rs, inner),
                   f"affine_act rowscale inner = {inner} {act}")
    a, rs = nc.randn32(g, 37 * 10), -(g.random(37).astype(np.float32) + np.float32(0.5))
    outside(nc.affine_replay(a, 1.0, 0.0, "none", rs, 10, mutation="inner_down4"), *nc.affine_ref(a, 1.0, 0.0, "none", rs, 10), "rowscale index")
    for B, C, HW, Cpad in nc.LAYOUT_CASES + [nc.LAYOUT_WRAP]:
        x = nc.randn32(g, B, C, HW)
        out = np.zeros((B, HW, Cpad), np.float32)
        out[..., :C] = (x * np.float32(nc.ALPHA) + np.float32(nc.BETA)).transpose(0, 2, 1)
        inside(out, *nc.nchw_to_nhwc_ref(x, Cpad, nc.ALPHA, nc.BETA), f"nchw_to_nhwc {(B, C, HW, Cpad)}")
    for shape in nc.RESAMPLE_CASES + [nc.RESAMPLE_WRAP]:
        x = nc.randn32(g, *shape)
        inside(nc.resample_down_replay(x), *nc.resample_down_ref(x), f"resample2x down {shape}")
    for D in nc.PERTURB_D:
        x, z, std, mc = nc.randn32(g, D), nc.randn32(g, 9, D), g.random(9).astype(np.float32), g.random(9).astype(np.float32)
        for coeff in (None, mc):
            inside(nc.perturb_replay(x, z, std, coeff), *nc.perturb_ref(x, z, std, coeff), f"perturb D = {D}")


def test_embedding_replays_inside_the_bound_and_swapped_halves_leave_it():
    t = np.array(nc.POS_T, np.float32)
    for dim in nc.POS_DIMS:
        for mode in (0, 1):
            inside(nc.positional_replay(t, dim, mode), *nc.positional_ref(t, dim, mode), f"positional_embed dim {dim} mode {mode}")
        outside(nc.positional_replay(t, dim, 1, mutation="sincos"), *nc.positional_ref(t, dim, 1), f"positional_embed dim {dim} [sin, cos] in mode 1")
    g = nc.rng(10)
    for half in nc.FOURIER_HALF:
        tt, W = (g.random(5) * 8.5 - 4.6).astype(np.float32), (np.float32(16) * nc.randn32(g, half)).astype(np.float32)
        inside(nc.fourier_replay(tt, W), *nc.fourier_ref(tt, W), f"fourier_embed half {half}")


@pytest.mark.parametrize("rows,D", nc.PHILOX_SHAPES)
def test_normal_stream_replay_and_mutations(rows, D):
    for seed in nc.PHILOX_SEEDS:
        for row0 in nc.PHILOX_ROW0:
            z = nc.normal_stream_replay(rows, D, row0, seed)
            inside(z, *nc.normal_stream_ref(rows, D, row0, seed), f"normal stream {(rows, D)} seed {seed} row0 {row0}")
            if seed >> 32 != seed & 0xFFFFFFFF:
                outside(z, *nc.normal_stream_ref(rows, D, row0, seed, mutation="key_swapped"), "key halves swapped")
            if (row0 * D) >> 34:                   # the counter's high word is nonzero
                outside(z, *nc.normal_stream_ref(rows, D, row0, seed, mutation="ctr_low_only"), "counter's high word dropped")
    assert (nc.PHILOX_ROW0[1] * 8) >> 34         # D = 8 at row0 = 2^38 reaches it


# ---------------------------------------------------------------------------------------------- the route queries, without a GPU
def test_route_queries_name_every_kernel_and_refuse_what_the_launchers_refuse():
    """The queries run the launchers' own admission code on the host (nothing is launched, addresses stand for alignment only)."""
    from id_diff_amd import _lib
    assert nc.routes_reached(_lib) == nc.ALL_ROUTES
    AL, OFF = 1 << 20, (1 << 20) + 4
    for cols, route in nc.SOFTMAX_COLS.items():                      # the thresholds, pinned: 256 / 512 / 1024 columns, alignment, scale > 0
        assert _lib.softmax_rows_route(AL, AL, 5, cols, 0.25) == route
        for x, y, scale in ((OFF, AL, 0.25), (AL, OFF, 0.25), (AL, AL, -0.5), (AL, AL, 0.0)):
            assert _lib.softmax_rows_route(x, y, 5, cols, scale) == nc.general_route(cols)
    gn = lambda **k: _lib.groupnorm_apply_route(*[{**dict(x=AL, C=8, x2=None, C2=0, B=2, HW=6, G=2, stats=AL, gamma=AL, beta=AL, y=AL), **k}[n]
                                                  for n in ("x", "C", "x2", "C2", "B", "HW", "G", "stats", "gamma", "beta", "y")])
    assert gn() == "rows" and gn(C=1024) == "rows" and gn(C=1024, x2=AL, C2=4, G=4) == "flat" and gn(B=65535) == "rows" and gn(B=65536) == "flat"
    for bad in (dict(C=6), dict(G=3), dict(x=OFF), dict(y=OFF), dict(gamma=OFF), dict(beta=OFF), dict(x2=OFF, C2=4), dict(stats=None), dict(x=None)):
        assert gn(**bad) is None, bad
        assert _lib.lib().idiff_last_error().decode().startswith("groupnorm_apply: ")
    cs = lambda C=8, x2=None, C2=0, B=2, ws2=None, ns2=0, ws1=AL, ns1=1: _lib.groupnorm_apply_colstats_route(AL, C, x2, C2, B, 6, 2, ws1, ns1, ws2, ns2, AL, AL, AL)
    assert cs() == "rows" and cs(x2=AL, C2=4, ws2=AL, ns2=1) == "rows" and cs(C=1024) == "rows"
    for bad in (dict(C=1028), dict(C=1024, x2=AL, C2=4, ws2=AL, ns2=1), dict(B=65536), dict(x2=AL, C2=4), dict(x2=AL, C2=4, ws2=AL), dict(ws1=None), dict(ns1=0)):
        assert cs(**bad) is None, bad
        assert _lib.lib().idiff_last_error().decode().startswith("groupnorm_apply_colstats: ")
    assert _lib.affine_act_route(AL, AL, 8, AL, 0) is None and _lib.affine_act_route(AL, AL, -1) is None and _lib.affine_act_route(None, AL, 8) is None
    assert _lib.affine_act_route(AL, AL, 8, AL, 4) == "vec4" and _lib.affine_act_route(AL, AL, 8, AL, 2) == "scalar" and _lib.affine_act_route(AL, OFF, 8) == "scalar"
    assert _lib.add_scale_route(AL, AL, AL, 8) == "vec4" and _lib.add_scale_route(AL, OFF, AL, 8) == "scalar" and _lib.add_scale_route(AL, AL, AL, 6) == "scalar"
    assert _lib.add_scale_route(AL, None, AL, 8) is None and _lib.concat_cols_route(AL, 0, AL, 4, AL, 1) is None
    assert _lib.concat_cols_route(AL, 4, AL, 8, AL, 3) == "vec4" and _lib.concat_cols_route(AL, 4, AL, 8, OFF, 3) == "scalar"
    assert _lib.softmax_rows_route(AL, AL, 3, 0, 1.0) is None and _lib.softmax_rows_route(None, AL, 3, 4, 1.0) is None and _lib.softmax_rows_route(AL, AL, 2 ** 34, 4, 1.0) is None
