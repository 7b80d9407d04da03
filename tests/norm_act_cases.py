"""What tests/test_norm_act_host.py and tests/test_hip_norm_act_routes.py share: the cases of the memory-bound passes (csrc/norm_act.hip,
csrc/rng.hip), an fp64 reference of each op on the fp32 inputs, a per-element bound derived from the kernel's own expression, and a numpy
float32 replay of that expression (same order of operations), which the host test holds to the bound -- and mutated, must leave it.

Every bound counts roundings: u = 2^-24 per fp32 operation, on the magnitude it rounds.  Device libm (expf, sinf, cosf, logf, sincosf) and
the hardware v_exp_f32 / v_rcp_f32 are allowed 2 u each, relative.  No figure here comes from what a kernel returned.  Inputs are O(1)
(randn; gamma, beta randn; mod 0.5 randn; rowscale = -(rand + 0.5)), so a dropped, doubled or shifted term or index moves elements by O(1).
The derivations are next to each bound and collected in the docstring of tests/test_hip_norm_act_routes.py.
"""
import numpy as np

U = 2.0 ** -24
F32_MIN = 2.0 ** -126          # below it v_exp_f32 / a product may flush to zero: the absolute floor of the softmax bound
ACTS = ("none", "silu", "elu", "relu", "lrelu")
LOG2E_F32 = np.float32(1.44269504088896340736)
EPS = float(np.float32(1e-6))  # the GroupNorm eps as the launcher receives it (a float argument)
f32 = np.float32


def _fn32(fn, x):
    """A libm function of a float32 argument, rounded once to float32 (numpy's own float32 exp / sin are SIMD routines of up to 2.5 ulp,
    a worse libm than the bounds allow a device: the replays take the correctly rounded one)."""
    return fn(np.asarray(x, f32).astype(np.float64)).astype(f32)


def rng(seed):
    return np.random.default_rng(seed)


def randn32(g, *shape):
    return g.standard_normal(shape).astype(f32)


# ---------------------------------------------------------------------------------------------- activations
def act_ref(name, v):
    v = np.asarray(v, np.float64)
    if name == "silu":
        return v / (1.0 + np.exp(-v))
    if name == "elu":
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0)))
    if name == "relu":
        return np.maximum(v, 0)
    if name == "lrelu":
        return np.where(v > 0, v, 0.2 * v)
    return v


def act_tol(name, v, tol_v):
    """Bound on |act_kernel(v_kernel) - act(v)| given |v_kernel - v| <= tol_v (v: the fp64 pre-activation).
    silu = v * rcp(1 + exp2(fl(-v log2e))): the product -v log2e rounds once and log2e_f32 is off by 0.22 u, an error of 1.22 |v| u in the
        exponent (counted 1.5 |v| u); v_exp_f32 2 u, the add 1 u, v_rcp_f32 2 u, the product 1 u: k = 6.  d silu / dv <= 1.0998.
    elu below 0 = fl(expf(v) - 1): the subtraction cancels, so expf's error (its last place is u on [0.5, 1), up to 4 u |exp v| below) stays
        absolute: u (4 |expm1 v| + 1) covers it and the subtraction's rounding u |expm1 v|.  d elu / dv <= 1.
    relu: none.  lrelu below 0: the product 0.2 v, k = 1.  Both have slope <= 1."""
    v = np.asarray(v, np.float64)
    y = np.abs(act_ref(name, v))
    if name == "silu":
        return U * y * (6 + 1.5 * np.abs(v)) + 1.1 * tol_v
    if name == "elu":
        return np.where(v > 0, 0.0, U * (4 * y + 1)) + tol_v
    if name == "lrelu":
        return U * y + tol_v
    return tol_v


def act_f32(name, v):
    """The kernel's act_apply on a float32 array, operation by operation."""
    v = np.asarray(v, f32)
    if name == "silu":
        return v * (f32(1) / (f32(1) + _fn32(np.exp2, -v * LOG2E_F32)))
    if name == "elu":
        return np.where(v > 0, v, _fn32(np.exp, np.minimum(v, f32(0))) - f32(1)).astype(f32)
    if name == "relu":
        return np.where(v > 0, v, f32(0)).astype(f32)
    if name == "lrelu":
        return np.where(v > 0, v, f32(0.2) * v).astype(f32)
    return v


# ---------------------------------------------------------------------------------------------- GroupNorm
# (B, HW, C, C2, G) of the stats + apply cases, and what each is there for
def gn_launch_numbers(B, HW, Ctot):
    """RP, rows_per_block, xblocks of the row-structured apply: the launcher's formula (groupnorm_apply_launch)."""
    cd = lambda a, b: -(-a // b)
    RP = 256 // (Ctot // 4)
    xblocks = max(1, min(cd(HW, RP), cd(2048, B)))
    rpb = cd(cd(HW, xblocks), RP) * RP
    return RP, rpb, cd(HW, rpb)


GN_CASES = [
    (2, 5, 8, 0, 2),          # fewer rows than RP = 128
    (3, 67, 24, 0, 6),        # CVt = 6 does not divide 256 (threads 252..255 idle)
    (2, 130, 1024, 0, 32),    # RP = 1
    (2, 70, 16, 8, 6),        # two sources
    (2, 70, 8, 4, 2),         # cpg = 6: a group straddles a float4 and the x / x2 boundary
    (1, 6401, 8, 0, 2),       # nsplit = 100 with rows_per = 65: the last split starts at 6435 > HW and is empty
    # the four-loads-in-flight loop takes 4 RP rows per trip and runs only where a workgroup has at least that many rows, i.e. where the cap of
    # ~2048 workgroups binds: B = 2048 gives xblocks = 1, one workgroup per sample with the row range [0, HW).  C = 256: RP = 4, so
    # HW = 16 = 4 RP, 17 = 4 RP + 1, 15 = 4 RP - 1 (rows_per_block = 16, 20, 16).  8M floats each: the smallest that reaches the loop
    (2048, 16, 256, 0, 32), (2048, 17, 256, 0, 32), (2048, 15, 256, 0, 32),
]
GN_FLAT_CASES = [
    (2, 9, 1024, 8, 8),       # Ctot = 1032 > 1024, cpg = 129
    (65536, 2, 8, 0, 2),      # B > 65535
    # the flat kernel has no row loop; its grid-stride loop takes 256 x 2048 float4 per trip: Ctot = 1032 (258 float4 per pixel), B HW =
    # 2033 pixels = 524514 float4 = one trip + 226: the wrap
    (19, 107, 1024, 8, 8),
]
GN_ACT_SHAPES = [(2, 70, 8, 4, 2), (2, 9, 1024, 8, 8)]     # all five activations x mod {off, column slice}, one per apply route
GN_COLSTATS_CASES = [      # (B, HW, C, C2, G, ns1, ns2)
    (3, 12, 24, 0, 6, 3, 0), (2, 12, 16, 8, 6, 3, 1), (2, 3, 1024, 0, 512, 1, 0), (2, 6, 512, 512, 512, 3, 1),
]
MOD_COL0 = 3               # the mod slice starts at a column that is no multiple of 4 ...
MOD_EXTRA = 11             # ... of a tensor 2 Ctot + 11 wide


def gn_inputs(B, HW, C, C2, G, seed=0, kind="randn", mod=False):
    g = rng(1000 + seed)
    Ctot = C + C2
    full = randn32(g, B, HW, Ctot)
    if kind == "const":
        full[:] = f32(3.25)
    elif kind == "offset":
        full = (f32(100) + f32(0.01) * full).astype(f32)
    d = dict(B=B, HW=HW, C=C, C2=C2, G=G, x=np.ascontiguousarray(full[..., :C]), x2=np.ascontiguousarray(full[..., C:]) if C2 else None,
             gamma=randn32(g, Ctot), beta=randn32(g, Ctot), mod=None)
    if mod:
        d["mod_wide"] = (f32(0.5) * randn32(g, B, 2 * Ctot + MOD_EXTRA)).astype(f32)
        d["mod"] = d["mod_wide"][:, MOD_COL0:MOD_COL0 + 2 * Ctot]          # a view: ld_mod = 2 Ctot + 11
    return d


def gn_full(d):
    return d["x"] if d["x2"] is None else np.concatenate([d["x"], d["x2"]], -1)


def gn_stats64(full, G, eps=EPS, skip_last_row_of_split=None):
    """Two-pass fp64 mean and rstd per (sample, group): [B, G] each, and the one-pass moments the kernels form (for the fp64 term of the
    bound and for the replay).  skip_last_row_of_split = (nsplit, split): the mutation that leaves that row out of the sums."""
    B, HW, Ctot = full.shape
    x = full.astype(np.float64).reshape(B, HW, G, Ctot // G)
    if skip_last_row_of_split is not None:
        ns, sp = skip_last_row_of_split
        rows_per = -(-HW // ns)
        keep = np.ones(HW, bool)
        keep[min(HW, (sp + 1) * rows_per) - 1] = False
        n_all = HW * (Ctot // G)
        s, q = x[:, keep].sum((1, 3)), (x[:, keep] ** 2).sum((1, 3))
        mean1 = s / n_all
        return None, None, mean1, 1.0 / np.sqrt(np.maximum(q / n_all - mean1 * mean1, 0) + eps), None
    mean = x.mean((1, 3))
    var = ((x - mean[:, None, :, None]) ** 2).mean((1, 3))
    n = HW * (Ctot // G)
    mean1 = x.sum((1, 3)) / n
    ex2 = (x ** 2).sum((1, 3)) / n
    rstd1 = 1.0 / np.sqrt(np.maximum(ex2 - mean1 * mean1, 0) + eps)
    # the kernels' fp64: sums of n terms in any order are off by <= (n + 8) 2^-53 sum |terms|; var = E x^2 - mean^2 cancels, so rstd is off
    # by c64 = 1.5 (n + 8) 2^-53 E x^2 / (var + eps) relative, the mean by (n + 8) 2^-53 E |x| absolute (E |x| <= sqrt(E x^2))
    e64 = (n + 8) * 2.0 ** -53
    c64 = 1.5 * e64 * ex2 / (var + eps)
    return mean, 1.0 / np.sqrt(var + eps), mean1, rstd1, (c64, e64 * np.sqrt(ex2))


def _per_channel(a, B, G, Ctot):
    """[B, G] -> [B, 1, Ctot]"""
    return np.repeat(a, Ctot // G, axis=1)[:, None, :]


def gn_ref(d, act, eps=EPS):
    """(reference, bound) of act(((x - mean) rstd gamma + beta)(1 + m1) + m2), fp64, [B, HW, Ctot].
    Pre-activation bound k u (T1 + T2 + T3) with T1 = (|x| + |mean|) rstd |gamma| |1 + m1|, T2 = |beta (1 + m1)|, T3 = |m2|.  Roundings on
    T1, the flat kernel (the longer chain): mean stored in fp32 1, x - mean 1, rstd stored in fp32 1, the products by rstd and gamma 2, + beta 1,
    and with mod: 1 + m1 1, the product 1, + m2 1: k = 6 without mod, 9 with.  The row kernel folds the same factors into s and t first
    (rstd gamma (1 + m1): 4, x - mean: 2, the product and the add: 2; t: 3 and the add) and stays within the same k.  The fp64 statistics
    add c64 T1 and rstd |gamma| |1 + m1| dmean (gn_stats64).  1.001 covers the products of (1 + u) factors."""
    B, HW, C, C2, G = d["B"], d["HW"], d["C"], d["C2"], d["G"]
    Ctot = C + C2
    full = gn_full(d).astype(np.float64)
    mean, rstd, _, _, (c64, dmean) = gn_stats64(gn_full(d), G, eps)
    mean, rstd, c64, dmean = (_per_channel(a, B, G, Ctot) for a in (mean, rstd, c64, dmean))
    ga, be = d["gamma"].astype(np.float64), d["beta"].astype(np.float64)
    one_m1, m2, k = 1.0, 0.0, 6
    if d["mod"] is not None:
        m = d["mod"].astype(np.float64)
        one_m1, m2, k = 1.0 + m[:, None, :Ctot], m[:, None, Ctot:], 9
    v = ((full - mean) * rstd * ga + be) * one_m1 + m2
    scale = rstd * np.abs(ga) * np.abs(one_m1)
    T1 = (np.abs(full) + np.abs(mean)) * scale
    tol_v = 1.001 * (k * U * (T1 + np.abs(be * one_m1) + np.abs(m2)) + c64 * T1 + scale * dmean)
    return act_ref(act, v), act_tol(act, v, tol_v)


def gn_replay(d, act, route, eps=EPS, mutation=None):
    """float32 replay of gn_apply_rows_kernel ("rows") / gn_apply_kernel ("flat") on statistics rounded to fp32.  Mutations (each a bug the
    bound must catch): "group_of_lane0", "no_shift", "scale_only", "x2_pitch", ("stats_skip", nsplit, split)."""
    B, HW, C, C2, G = d["B"], d["HW"], d["C"], d["C2"], d["G"]
    Ctot, cpg = C + C2, (C + C2) // G
    full = gn_full(d)
    if mutation == "x2_pitch" and C2:          # x2 addressed with C as its row pitch (reads run into the next rows; wraps inside the sample set)
        flat2 = d["x2"].reshape(-1)
        idx = (np.arange(B * HW)[:, None] * C + np.arange(C2)[None, :]) % flat2.size
        full = np.concatenate([d["x"], flat2[idx].reshape(B, HW, C2)], -1)
    skip = (mutation[1], mutation[2]) if isinstance(mutation, tuple) else None
    _, _, mean1, rstd1, _ = gn_stats64(gn_full(d), G, eps, skip_last_row_of_split=skip)
    gidx = np.arange(Ctot) // cpg
    if mutation == "group_of_lane0":
        gidx = (np.arange(Ctot) // 4 * 4) // cpg
    mu, rs = mean1.astype(f32)[:, gidx][:, None, :], rstd1.astype(f32)[:, gidx][:, None, :]
    ga, be = d["gamma"][None, None, :], d["beta"][None, None, :]
    m = d["mod"]
    if route == "rows":
        sc, sh = rs * ga, np.broadcast_to(be, (B, 1, Ctot)).astype(f32)
        if m is not None:
            m1 = f32(1) + m[:, None, :Ctot]
            sc = sc * m1
            sh = sh if mutation == "scale_only" else sh * m1
            if mutation != "no_shift":
                sh = sh + m[:, None, Ctot:]
        v = (full - mu) * sc + sh
    else:
        v = (full - mu) * rs * ga + be
        if m is not None:
            m1 = f32(1) + m[:, None, :Ctot]
            v = (v - be) * m1 + be if mutation == "scale_only" else v * m1
            if mutation != "no_shift":
                v = v + m[:, None, Ctot:]
    assert v.dtype == f32
    return act_f32(act, v)


def gn_colsums(t, ns):
    """[B, ns, C, 2] fp64: sums and sums of squares over ns equal row ranges (HW % ns == 0), as a producing contraction's epilogue writes them."""
    B, HW, C = t.shape
    parts = t.astype(np.float64).reshape(B, ns, HW // ns, C)
    return np.ascontiguousarray(np.stack([parts.sum(2), (parts ** 2).sum(2)], -1))


def gn_coef_ref(d, eps=EPS):
    """coef [B, Ctot, 2] = (a, b) = (rstd gamma, beta - mean a), formed in fp64 by the kernel and rounded once: a to 2 u |a| (the rounding and
    c64, which the caller's inputs keep below u), b to u (|beta| + 2 |mean a|) (the rounding of b, c64 |mean a| and the mean's fp64 error)."""
    B, G, Ctot = d["B"], d["G"], d["C"] + d["C2"]
    mean, rstd, _, _, (c64, _) = gn_stats64(gn_full(d), G, eps)
    assert c64.max() < U
    mean, rstd = np.repeat(mean, Ctot // G, 1), np.repeat(rstd, Ctot // G, 1)
    a = rstd * d["gamma"].astype(np.float64)
    b = d["beta"].astype(np.float64) - mean * a
    return np.stack([a, b], -1), np.stack([2 * U * np.abs(a), U * (np.abs(d["beta"].astype(np.float64)) + 2 * np.abs(mean * a))], -1)


# ---------------------------------------------------------------------------------------------- softmax
SOFTMAX_COLS = {1: "regs", 3: "regs", 4: "vec<1>", 63: "regs", 64: "vec<1>", 65: "regs", 252: "vec<1>", 256: "vec<1>", 260: "vec<2>",
                508: "vec<2>", 512: "vec<2>", 516: "vec<4>", 768: "vec<4>", 1020: "vec<4>", 1024: "vec<4>", 1025: "stream", 1028: "stream",
                1500: "stream", 2051: "stream"}        # cols -> route for aligned pointers and scale > 0
SOFTMAX_ROWS = (1, 5)
SOFTMAX_WRAP = ((16387, 4), (16387, 8))                 # 4097 workgroups of work on the vec kernels' 4096: the row loop wraps, the prefetch ends
SOFTMAX_SCALES = (0.25, 1.0, -0.5)


def general_route(cols):
    return "regs" if cols <= 1024 else "stream"


def softmax_inputs(rows, cols, seed=0, kind="randn"):
    g = rng(2000 + seed + 7 * cols + rows)
    x = (f32(5) * randn32(g, rows, cols)).astype(f32)
    if kind == "big":
        x = (f32(80) * randn32(g, rows, cols)).astype(f32)
    elif kind == "equal":
        x[0, :] = f32(1.7)
    elif kind == "masked":           # every third entry of each row at -inf, never the whole row
        x[:, 1::3] = -np.inf
    return x


def softmax_ref(x, scale):
    """tol_i = y_i u (A + 3 (|s x_i| + max_j |s x_j|)) + 2 F32_MIN.  A: the exponential 2, the per-lane sum (ceil(cols / 64) terms in the
    general kernel; the vec kernels add four columns per run, 4 ceil(cols / 256) terms) plus 6 shuffle steps, the reciprocal 2, the product 1.
    The scaled logit is rounded (once; in the vec kernels by scale log2e, itself rounded) before the subtraction of the maximum, which rounds
    again: errors of the exponent proportional to |s x_i| + max |s x_j|, for element i and, through the sum, for the elements that carry the
    sum.  An entry at -inf is exactly 0 (bound 0) and takes no part in the maximum.  2 F32_MIN: results below the normal range may flush."""
    rows, cols = x.shape
    sx = float(scale) * x.astype(np.float64)
    finite = np.isfinite(sx)
    m = np.where(finite, sx, -np.inf).max(1, keepdims=True)
    e = np.where(finite, np.exp(np.where(finite, sx, 0) - m), 0.0)
    y = e / e.sum(1, keepdims=True)
    amax = np.where(finite, np.abs(sx), 0).max(1, keepdims=True)
    A = 2 + max(-(-cols // 64), 4 * -(-cols // 256)) + 6 + 2 + 1
    tol = y * U * (A + 3 * (np.where(finite, np.abs(sx), 0) + amax)) + 2 * F32_MIN
    return y, np.where(finite, tol, 0.0)


def _wave_sum(lane_sums):
    """[rows, 64] -> [rows]: the xor-shuffle butterfly of wave_sum, float32."""
    s = lane_sums.astype(f32)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, np.arange(64) ^ o]
    return s[:, 0]


def softmax_replay(x, scale, route, mutation=None):
    """float32 replay of softmax_rows_kernel ("regs" / "stream": libm expf) or softmax_rows_vec_kernel ("vec<R>": exp2 of x (scale log2e)).
    mutation "skip_tail": columns >= 4 * 64 * floor(cols / 256) are not read and not written (a vec kernel that drops its partly filled run)."""
    rows, cols = x.shape
    x = x.astype(f32)
    live = cols if mutation != "skip_tail" else 256 * (cols // 256)
    with np.errstate(invalid="ignore", over="ignore"):
        if route.startswith("vec"):
            k = f32(scale) * LOG2E_F32
            v = x * k
        else:
            v = x * f32(scale)
        v[:, live:] = -np.inf
        m = v.max(1, keepdims=True)
        e = _fn32(np.exp2 if route.startswith("vec") else np.exp, v - m)
        lanes = np.zeros((rows, 64), f32)
        if route.startswith("vec"):
            R = int(route[4])
            pad = np.zeros((rows, 256 * R), f32)
            pad[:, :cols] = e
            q = pad.reshape(rows, R, 64, 4)
            for i in range(R):
                lanes = lanes + ((q[:, i, :, 0] + q[:, i, :, 1]) + (q[:, i, :, 2] + q[:, i, :, 3]))
        else:
            n = -(-cols // 64)
            pad = np.zeros((rows, 64 * n), f32)
            pad[:, :cols] = e
            q = pad.reshape(rows, n, 64)
            for i in range(n):
                lanes = lanes + q[:, i]
        inv = f32(1) / _wave_sum(lanes)
        y = e * inv[:, None]
    y[:, live:] = np.nan           # never written
    return y


# ---------------------------------------------------------------------------------------------- pointwise and layout
POINTWISE_N = (1, 3, 4, 5, 1023, 1024, 1025)
WRAP_VEC4_N = 4 * 524288 + 8       # 2048 workgroups x 256 float4 per trip, + 2 float4
WRAP_SCALAR_N = 524288 + 3
AFFINE_INNER = {4: "vec4", 12: "vec4", 3: "scalar", 10: "scalar"}
CONCAT_CASES = {(4, 8): "vec4", (8, 4): "vec4", (3, 5): "scalar", (4, 3): "scalar", (1, 1): "scalar"}
CONCAT_ROWS = (1, 7)
LAYOUT_CASES = [(3, 3, 64, 4), (2, 1, 5, 4), (2, 5, 7, 5), (1, 3, 1, 8)]      # (B, C, HW, Cpad)
LAYOUT_WRAP = (2, 3, 87382, 4)      # B HW Cpad = 699056 > 524288 elements: the scalar loop wraps
RESAMPLE_CASES = [(2, 6, 6, 8), (1, 2, 2, 4), (3, 2, 10, 12)]                  # (B, H, W, C)
RESAMPLE_WRAP = (1, 182, 182, 16)   # up: 529984 float4 of output > 524288, the loop wraps (down would need a 33 MB input: not built)
PERTURB_D = (1, 3, 8)
ALPHA, BETA = 2.0, -1.0             # the `2 x - 1` of the models' input scaling
SILU_GRID = np.linspace(-20.0, 20.0, 4001).astype(np.float32)      # where the error of act_apply's SiLU grows with |v| (alpha = 1, beta = 0: v = a)


def affine_ref(a, alpha, beta, act, rowscale=None, inner=0):
    """y = act(a alpha + beta) rowscale[i // inner].  v = fl(fl(a alpha) + beta) (or one fma): k = 2 on |a alpha| + |beta|; then the
    activation's bound; the product by rowscale rounds once more: u |y|.  alpha = 1, beta = 0, act none: at most the one product, and the
    caller asks for equal bits instead."""
    a64 = a.astype(np.float64)
    v = a64 * float(f32(alpha)) + float(f32(beta))
    y, tol = act_ref(act, v), act_tol(act, v, 2 * U * (np.abs(a64 * float(f32(alpha))) + abs(float(f32(beta)))))
    if rowscale is not None:
        rs = rowscale.astype(np.float64)[np.arange(a.size) // inner]
        y, tol = y * rs, np.abs(rs) * tol + U * np.abs(y * rs)
    return y, tol


def affine_replay(a, alpha, beta, act, rowscale=None, inner=0, mutation=None):
    """mutation "inner_down4": the vec4 kernel's rowscale[(4 v) / inner] with inner rounded down to a multiple of 4."""
    y = act_f32(act, a * f32(alpha) + f32(beta))
    if rowscale is not None:
        i = np.arange(a.size)
        idx = i // inner if mutation is None else np.minimum((i // 4 * 4) // (inner // 4 * 4), rowscale.size - 1)
        y = y * rowscale[idx]
    return y.astype(f32)


def nchw_to_nhwc_ref(x, Cpad, alpha, beta):
    """x [B, C, HW] -> [B, HW, Cpad], pad channels 0.  fl(fl(x alpha) + beta) or one fma: k = 2 on |x alpha| + |beta|."""
    B, C, HW = x.shape
    y, tol = np.zeros((B, HW, Cpad)), np.zeros((B, HW, Cpad))
    x64 = x.astype(np.float64).transpose(0, 2, 1)
    y[..., :C] = x64 * float(f32(alpha)) + float(f32(beta))
    tol[..., :C] = 2 * U * (np.abs(x64 * float(f32(alpha))) + abs(float(f32(beta))))
    return y, tol


def resample_down_ref(x):
    """2 x 2 mean of x [B, H, W, C]: three adds in fp32, the product by 0.25 exact: k = 3 on 0.25 (|p00| + |p01| + |p10| + |p11|)."""
    B, H, W, C = x.shape
    q = x.astype(np.float64).reshape(B, H // 2, 2, W // 2, 2, C)
    return q.sum((2, 4)) * 0.25, 3 * U * 0.25 * np.abs(q).sum((2, 4))


def resample_down_replay(x):
    B, H, W, C = x.shape
    q = x.reshape(B, H // 2, 2, W // 2, 2, C)
    return (q[:, :, 0, :, 0] + q[:, :, 0, :, 1] + q[:, :, 1, :, 0] + q[:, :, 1, :, 1]) * f32(0.25)


def perturb_ref(x, z, std, mean_coeff):
    """out[r] = mean_coeff[r] x + std[r] z[r]: each product rounds once and the add once, or one of them folds into an fma: k = 2 on
    |mean_coeff x| + |std z| (without mean_coeff the first term is exact: the same k bounds it)."""
    m = x.astype(np.float64)[None, :] * (1.0 if mean_coeff is None else mean_coeff.astype(np.float64)[:, None])
    n = std.astype(np.float64)[:, None] * z.astype(np.float64)
    return m + n, 2 * U * (np.abs(m) + np.abs(n))


def perturb_replay(x, z, std, mean_coeff):
    m = x[None, :] if mean_coeff is None else mean_coeff[:, None] * x[None, :]
    return (m + std[:, None] * z).astype(f32)


# ---------------------------------------------------------------------------------------------- embeddings
POS_DIMS = (4, 6, 128)
POS_T = (0.0, 1e-5 * 999, 999.0)
MAX_POSITIONS = 10000.0
FOURIER_HALF = (1, 16, 300)


def positional_ref(t, dim, mode, max_positions=MAX_POSITIONS, swap=False):
    """The real-valued embedding in fp64 from the fp32 t and the launcher's fp32 constants.  The exponent e handed to expf is j (-c0) (mode 0:
    one rounding, u |e|) or c1 j / half (mode 1: the product and the division, 2 u |e| -- one rounding more than mode 0, the division); expf
    2 u; arg = fl(t freq) 1 u: arg is off by |arg| u (r |e| + 3), r = 1 or 2.  sin and cos have slope <= 1 and sinf / cosf are allowed 2 u of
    a value <= 1, counted 4 u with the last place of values in [0.5, 1]:  tol = |arg| u (r |e| + 4) + 4 u."""
    half = dim // 2
    j = np.arange(half, dtype=np.float64)
    if mode == 0:
        e, r = j * -float(f32(np.log(max_positions) / (half - 1))), 1
    else:
        e, r = float(f32(-np.log(max_positions))) * j / half, 2
    arg = t.astype(np.float64)[:, None] * np.exp(e)[None, :]
    tol = np.abs(arg) * U * (r * np.abs(e)[None, :] + 4) + 4 * U
    first, second = (np.sin, np.cos) if (mode == 0) != swap else (np.cos, np.sin)
    return np.concatenate([first(arg), second(arg)], 1), np.concatenate([tol, tol], 1)


def positional_replay(t, dim, mode, max_positions=MAX_POSITIONS, mutation=None):
    """mutation "sincos": mode 1 written in mode 0's [sin, cos] order."""
    half = dim // 2
    j = np.arange(half, dtype=f32)
    if mode == 0:
        freq = _fn32(np.exp, j * -f32(np.log(max_positions) / (half - 1)))
    else:
        freq = _fn32(np.exp, f32(-np.log(max_positions)) * j / f32(half))
    arg = (t[:, None] * freq[None, :]).astype(f32)
    s, c = _fn32(np.sin, arg), _fn32(np.cos, arg)
    return np.concatenate([s, c] if (mode == 0 or mutation == "sincos") else [c, s], 1).astype(f32)


TWO_PI_F32 = f32(6.2831854820251465)


def fourier_ref(t, W):
    """[sin, cos] of arg = t W 2pi_f32 in fp64; the kernel rounds both products: 2 u |arg|, counted 3 as the issue does; sinf / cosf: 4 u."""
    arg = t.astype(np.float64)[:, None] * W.astype(np.float64)[None, :] * float(TWO_PI_F32)
    tol = 3 * U * np.abs(arg) + 4 * U
    return np.concatenate([np.sin(arg), np.cos(arg)], 1), np.concatenate([tol, tol], 1)


def fourier_replay(t, W):
    arg = ((t[:, None] * W[None, :]).astype(f32) * TWO_PI_F32).astype(f32)
    return np.concatenate([_fn32(np.sin, arg), _fn32(np.cos, arg)], 1)


# ---------------------------------------------------------------------------------------------- Philox4x32-10 and the normal stream
PHILOX_KAT = [      # Random123's known answers (counter, key, output)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
PHILOX_SHAPES = ((3, 4), (5, 12), (1024, 8))
PHILOX_SEEDS = (0, 12345, 2 ** 63 + 5)
PHILOX_ROW0 = (0, 2 ** 38)

_M0, _M1, _W0, _W1, _MASK = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))


def philox4x32_10(ctr, key):
    """Salmon et al., SC'11.  ctr: four uint64 arrays holding 32-bit words, key: two 32-bit words.  Returns four uint64 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in ctr)
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                         # 32 x 32 -> 64 bits, no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def normal_stream_ref(rows, D, row0, seed, mutation=None):
    """(z, tol) [rows, D] fp64: Box-Muller on the reference integers.  Element (r, c) belongs to the group of four with counter
    ((row0 + r) D + c) >> 2 in words 0, 1 (zeros in 2, 3), key (seed & 0xffffffff, seed >> 32); the group's words (x, y, z, w) give
    (r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1), r0 = sqrt(-2 ln u01(x)), a0 = 2 pi u01(y), r1 from z, a1 from w, u01(v) = ((v >> 8) + 1) 2^-24.
    tol = u r (4 pi + 8): the angle 2pi_f32 u01 rounds once and 2pi_f32 is off by 0.47 u (1.47 x 2 pi u r), sincosf 4 u, logf 2 u halved by
    the root, the root and the product 1 u each.  mutation: "key_swapped", "ctr_low_only"."""
    idx = [(int(row0) + r) * D + c for r in range(rows) for c in range(0, D, 4)]
    ctr = [i >> 2 for i in idx]
    lo = np.array([c & 0xFFFFFFFF for c in ctr], np.uint64)
    hi = np.array([0 if mutation == "ctr_low_only" else c >> 32 for c in ctr], np.uint64)
    zero = np.zeros_like(lo)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (seed & 0xFFFFFFFF, seed >> 32)
    if mutation == "key_swapped":
        key = key[::-1]
    w = philox4x32_10((lo, hi, zero, zero), key)
    u01 = [((v >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24 for v in w]
    r0, r1 = np.sqrt(-2.0 * np.log(u01[0])), np.sqrt(-2.0 * np.log(u01[2]))
    a0, a1 = 2.0 * np.pi * u01[1], 2.0 * np.pi * u01[3]
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], 1).reshape(rows, D)
    rr = np.stack([r0, r0, r1, r1], 1).reshape(rows, D)
    return z, U * rr * (4 * np.pi + 8)


def normal_stream_replay(rows, D, row0, seed):
    """The kernel's float32 Box-Muller on the reference integers."""
    idx = [((int(row0) + r) * D + c) >> 2 for r in range(rows) for c in range(0, D, 4)]
    lo, hi = np.array([c & 0xFFFFFFFF for c in idx], np.uint64), np.array([c >> 32 for c in idx], np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((lo, hi, np.zeros_like(lo), np.zeros_like(lo)), (seed & 0xFFFFFFFF, seed >> 32))
    u01 = [((v >> np.uint64(8)).astype(f32) + f32(1)) * f32(2.0 ** -24) for v in w]
    r0, r1 = np.sqrt(f32(-2) * _fn32(np.log, u01[0])), np.sqrt(f32(-2) * _fn32(np.log, u01[2]))
    a0, a1 = f32(6.2831853071795864) * u01[1], f32(6.2831853071795864) * u01[3]
    return np.stack([r0 * _fn32(np.cos, a0), r0 * _fn32(np.sin, a0), r1 * _fn32(np.cos, a1), r1 * _fn32(np.sin, a1)], 1).reshape(rows, D).astype(f32)


# ---------------------------------------------------------------------------------------------- routes
ALL_ROUTES = {"groupnorm_apply": {"rows", "flat"}, "groupnorm_apply_colstats": {"rows"},
              "softmax_rows": {"vec<1>", "vec<2>", "vec<4>", "regs", "stream", "none"},
              "affine_act": {"vec4", "scalar", "none"}, "add_scale": {"vec4", "scalar", "none"}, "concat_cols": {"vec4", "scalar", "none"}}


def routes_reached(lib):
    """op -> the set of names the route queries of ``lib`` (id_diff_amd._lib) return over the geometry of the cases above; the addresses
    stand for alignment only (nothing is launched, so this runs without a GPU)."""
    AL, OFF = 1 << 20, (1 << 20) + 4
    ns = POINTWISE_N + (WRAP_VEC4_N, WRAP_SCALAR_N, 0)
    return {
        "groupnorm_apply": {lib.groupnorm_apply_route(AL, C, AL if C2 else None, C2, B, HW, G, AL, AL, AL, AL)
                            for B, HW, C, C2, G in GN_CASES + GN_FLAT_CASES},
        "groupnorm_apply_colstats": {lib.groupnorm_apply_colstats_route(AL, C, AL if C2 else None, C2, B, HW, G, AL, n1, AL if C2 else None, n2, AL, AL, AL)
                                     for B, HW, C, C2, G, n1, n2 in GN_COLSTATS_CASES},
        "softmax_rows": {lib.softmax_rows_route(a, a, rows, cols, s) for cols in SOFTMAX_COLS for rows in SOFTMAX_ROWS + (0,)
                         for s in SOFTMAX_SCALES for a in (AL, OFF)},
        "affine_act": {lib.affine_act_route(a, a, n) for n in ns for a in (AL, OFF)} | {lib.affine_act_route(AL, AL, 37 * i, AL, i) for i in AFFINE_INNER},
        "add_scale": {lib.add_scale_route(a, a, a, n) for n in ns for a in (AL, OFF)},
        "concat_cols": {lib.concat_cols_route(a, Ca, AL, Cb, AL, r) for Ca, Cb in CONCAT_CASES for r in CONCAT_ROWS + (0,) for a in (AL, OFF)},
    }


# ---------------------------------------------------------------------------------------------- comparison
def worst(out, ref, tol):
    """(largest err / tol, its flat index): element by element; where tol == 0 the values must be equal (ratio inf otherwise).  A NaN in
    `out` counts as inf."""
    out, ref, tol = (np.asarray(a, np.float64).reshape(-1) for a in (out, ref, np.broadcast_to(tol, np.shape(ref))))
    err = np.abs(out - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, np.where(tol > 0, err / tol, np.inf))
    ratio = np.where(np.isnan(out) | np.isnan(ratio), np.inf, ratio)
    i = int(ratio.argmax()) if ratio.size else 0
    return (float(ratio[i]) if ratio.size else 0.0), i
