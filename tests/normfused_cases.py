"""What tests/test_normfused_host.py and tests/test_hip_normfused_matrix.py share: the cases of the four kernels that apply a GroupNorm
(+ SiLU) themselves (csrc/wino1d.hip: in the tail, in the loader of one source, in the loader of cat[x1, x2]; csrc/upfirdn2d.hip: in the
loader of the two FIR resamplers), their inputs, an fp64 reference of each, a per-element bound derived from the arithmetic and from the
reference alone, and an fp32 CPU replay of each form that the host test holds to the bound -- and mutated, must leave it.  No GPU here.

Isolated consumer (the default).  The test forms the coefficient pair itself, a = rstd gamma, b = beta - mean rstd gamma from fp64
statistics, rounded once to fp32, and hands it to the kernel: groupnorm_coef is not part of the run (its own bound:
tests/test_hip_norm_act_routes.py).  The reference is fp64 ON THE FP32 COEFFICIENT VALUES:
    z = a32 x + b32,   n = act(z) (zero outside the image),   the convolution or FIR of n,   the header's epilogue.
Input side, u = 2^-24: the loader is ONE fmaf, so dz = u |z| -- whatever the size of a and b: a loader must be within one fma rounding of
what its coefficients say; dn = act_tol(act, z, dz), the project's SiLU bound u |silu z| (6 + 1.5 |z|) + 1.1 dz.
Convolution: D = conv(dn, |w|), A = conv(|n|, |w|) and the bound of tests/test_hip_epilogue_matrix.py with A replaced by A + D / E:
    tol = |s| (1.1 (E (A + |bias| + |rowbias|) + D) + 8 u (|act(pre)| + |residual|)).
FIR: tol = sum_t |k_t| dn_t + 17 u sum_t |k_t n_t| (sixteen taps multiplied and added in fp32, and the store).
Tail norm: pre = conv + bias + rowbias with e = 1.1 E (A + |bias| + |rowbias|); the kernel forms mean and variance (about the mean) in
fp64 on chip, so to first order, e_mean and e_rms the group's mean and rms of e,
    dnhat <= rstd (e + e_mean) + |nhat| rstd e_rms,
    dy = act_tol(act, y_pre, 1.1 (|gamma| dnhat + 6 u ((|pre| + |mean|) rstd |gamma| + |beta|)))      (6 u: the GroupNorm pass's own count).
The 300-sigma bias offset makes e large (e ~ E 450): that is what an fp16-pair contraction next to a bias of 450 gives, and it is not capped.

E, the contraction's own error relative to A, is not taken from a kernel.  ``wino1d_emulate`` is a CPU emulation of the row-wise F(4, 3)
on fp16 pairs (hi = fp16(v), lo = fp16(v - hi) on both operands, U = G g in fp64 scaled by a power of two to [2^11, 2^12) and rounded once,
three partial products, fp32 accumulation, the transforms of csrc/winograd43_shared.h restated in numpy: points 0, +-2/3, +-3/2, inf).  On
this module's own inputs -- SiLU of normalised values, where an output below 0.25 carries an absolute 2^-25 instead of a relative 2^-22 --
it measures (test_normfused_host.py::test_emulated_contraction_error, printed as EMUL)
    max |err| / A = 3.9e-7  (loader cases, silu and none, every statistics kind),   4.1e-7  (the tail-norm inputs, Gaussian)
so 4 x that = 1.6e-6 stays below the class's E_F4 = 4.5e-6 and   E = max(E_F4, 4 x measured) = 4.5e-6   is what every wino1d bound here uses
(the 4 x: the kernels' up to 2 x larger norm errors and the tail of ~1e5 elements, as in tests/test_hip_epilogue_matrix.py).  The
emulation sums in torch's order, not the kernel's: it bounds the arithmetic class, not the bits.  The replays contract directly in fp32
and take the direct class's E_DIRECT = 1e-6.

The coefficient form a x + b rounds a and b separately: against the EXACT GroupNorm its error is u (|a x| + |b|), which grows with
|mean| rstd.  On the CPU (3 x 32 x 32, 32 -> 128 channels, test_normfused_host.py::test_coefficient_form_on_ill_conditioned_groups, printed as
COEF): a group of constant value 2.5 has |a| up to 1773 and |b| up to 4434, u (|a x| + |b|) = 5e-4 on z, and rounding the coefficients
alone moves the convolution's output by 0.12 x the isolated bound (four channels of 32 carry it; a wider constant group or unluckier
roundings reach the bound itself: up to 2 x by the estimate 9 taps x 4 channels x |w| x 5e-4 against E A); at |mean| / std = 30 by 0.096 x
(|b| up to 64); on benign statistics by 0.004 x.  The isolated-consumer bound does not carry that term (the reference uses the fp32
coefficients), the end-to-end chain's does: conv(1.1 (da |x| + db), |w|) with (da, db) of gn_coef_ref, plus the fp64 statistics' own
cancellation term where the variance is tiny (coef_tolerance) -- next to E A it is 0.2 x (benign), 4 - 5 x (|mean| / std = 30) and 1e3 x (a
constant group) (printed as CHAIN by the host test and by the GPU module).  The executor can hand such a group to the loader (it routes
by shape, not by statistics): a known property, stated in DESIGN.md.
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import norm_act_cases as nc
from epilogue_cases import E_DIRECT, E_F4, OUT_SCALE, SLICE_PAD, act64, combos, epilogue_ref  # noqa: F401
from norm_act_cases import EPS, U, act_ref, act_tol, f32, gn_coef_ref, gn_colsums, gn_stats64  # noqa: F401

E_EMULATED = 4.1e-7                       # the largest max |err| / A of wino1d_emulate on this module's inputs (docstring)
E_W1D = max(E_F4, 4 * E_EMULATED)
W32 = 32
NL_ACTS = ("silu", "none")
TAIL_ACTS = ("none", "silu", "elu", "relu", "lrelu")

# ---------------------------------------------------------------------------------------------- cases
# loader forms: (B, H, C1, C2, Cout), W = 32.  C2 = 0: one source
LOADER_1SRC = [(3, 32, 32, 0, 128),       # odd image count, two cout tiles, ns = 2
               (3, 16, 16, 0, 64),        # a block is a whole image, a single K step, ns = 1
               (1, 48, 48, 0, 64)]        # three blocks per image, ns = 3
LOADER_2SRC = [(3, 32, 16, 16, 64),
               (2, 32, 32, 48, 128),
               (1, 64, 48, 16, 64)]       # interior blocks with both halo rows inside the image
LOADER_CASES = LOADER_1SRC + LOADER_2SRC
# statistics kinds on two shapes: (shape, kind, channels per group); 0: one group of all Cin channels
KIND_SHAPES = [(3, 32, 32, 0, 128), (2, 32, 32, 48, 128)]
KIND_CASES = ([(s, k, 4) for s in KIND_SHAPES for k in ("mean30", "constgroup")] +
              [(s, "benign", cpg) for s in KIND_SHAPES for cpg in (4, 16, 0)] +      # G = Cin / 4, Cin / 16, 1
              [((2, 32, 48, 0, 64), "benign", 12)])                                  # G = 4: groups of 12, one source
# end-to-end chains: (B, H, C1, C2, Cout, G, kind); 32 + 64 in 8 groups of 12: groups straddle a K step and the two sources
CHAIN_CASES = [((2, 32, 64, 0, 64), 16, "benign"), ((2, 32, 32, 64, 64), 8, "benign"), ((2, 32, 64, 0, 64), 16, "mean30"),
               ((2, 32, 32, 64, 64), 8, "mean30"), ((2, 32, 64, 0, 64), 16, "constgroup")]
# the production epilogues of the executor (models/nhwc.py): Conv_0 bias + rowbias, Conv_1 bias + residual + 1 / sqrt 2; and bias alone
BIAS_ONLY = (True, False, "none", "off", 1.0, False)
PRODUCTION = [(True, True, "none", "off", 1.0, False), (True, False, "none", "dense", OUT_SCALE, False)]
# tail-norm form: (B, H, W, Cin, Cout, groups, offset)
TAIL_CASES = [(3, 16, 16, 32, 64, 16, 0.0), (9, 8, 8, 32, 128, 32, 0.0),
              (37, 4, 4, 32, 64, 64, 0.0),        # one channel per group, partial last block
              (5, 8, 16, 32, 64, 2, 0.0),         # groups of 32, a 128-pixel map
              (3, 4, 8, 32, 64, 1, 0.0),          # one group per tile
              (5, 16, 16, 32, 64, 16, 300.0)]     # the 300-sigma bias offset
# FIR forms: (B, H, W, C)
FIR_MODES = {"up": (2, 1, 2, 1, 4.0), "down": (1, 2, 1, 1, 1.0)}           # up, down, pad0, pad1, gain on the taps (models/ncsnpp.py, _fir)
FIR_CASES = {"up": [(3, 8, 8, 8), (2, 5, 7, 12),          # cv = 3: idle lanes
                    (1, 16, 16, 64), (1, 4, 300, 4),      # rows wider than col_step
                    (1, 4, 4, 1024)],
             "down": [(3, 8, 8, 8), (2, 6, 10, 12),       # out 3 x 5, both odd
                      (1, 16, 16, 64),                    # the routed class
                      (1, 4, 600, 4), (1, 4, 4, 1024)]}
FIR_ROUTE = {"up": "nhwc_up2_block", "down": "nhwc_rows<0>"}
FIR_KINDS = ("benign", "mean30")


def tail_instantiations():
    """(NL, two sources, act != none, residual, scaled, stats) over the loader cases x the product with and without column sums."""
    seen = set()
    for (B, H, C1, C2, Cout), nl in itertools.product(LOADER_CASES, NL_ACTS):
        for stats in (False, True):
            for hb, hrb, act, rk, osc, hrs in combos():
                seen.add((nl, C2 > 0, act != "none", rk != "off", osc != 1.0 or hrs, stats))
    return seen


# ---------------------------------------------------------------------------------------------- inputs
def _sign(g, *shape):
    return np.where(g.random(shape) < 0.5, -1.0, 1.0).astype(f32)


def raw_inputs(B, HW, C1, C2, G, kind="benign", seed=0):
    """Two raw sources [B, HW, C1], [B, HW, C2] (x2 None when C2 == 0), gamma of both signs and magnitude 0.7 .. 2.1, |beta| in [0.7, 1.3]
    (silu(beta) != 0: padding that is not forced back to zero shows).  Channel means of magnitude 1 .. 2, POSITIVE in x1 and NEGATIVE in
    x2 (a read from the wrong source, pitch or channel offset is an error of order 1).  kind "mean30": every channel at +-30 standard
    deviations, the same offset across a source's channels (|mean| / std = 30 for the groups inside one source); "constgroup": group 1 of
    every image holds the constant 2.5 (variance exactly zero: rstd = eps^-1/2 = 1000)."""
    g = nc.rng(5000 + seed + 7 * C1 + 13 * C2 + HW)
    Cin = C1 + C2
    x = (f32(1.3) * nc.randn32(g, B, HW, Cin)).astype(f32)
    off = (g.random(Cin) + 1.0).astype(f32)
    if kind == "mean30":
        off[:] = f32(30 * 1.3)
    off[C1:] *= f32(-1)
    x = (x + off[None, None, :]).astype(f32)
    if kind == "constgroup":
        cpg = Cin // G
        x[:, :, cpg:2 * cpg] = f32(2.5)
    gamma = ((g.random(Cin) + 0.5) * 1.4).astype(f32) * _sign(g, Cin)
    beta = (g.random(Cin) * 0.6 + 0.7).astype(f32) * _sign(g, Cin)
    return dict(B=B, HW=HW, C=C1, C2=C2, G=G, kind=kind, x=np.ascontiguousarray(x[..., :C1]),
                x2=np.ascontiguousarray(x[..., C1:]) if C2 else None, gamma=gamma, beta=beta)


def exact_coef(d):
    """(a, b) [B, Cin, 2] in fp64 from two-pass fp64 statistics of cat[x, x2]."""
    Cin, G = d["C"] + d["C2"], d["G"]
    mean, rstd, _, _, _ = gn_stats64(nc.gn_full(d), G)
    a = np.repeat(rstd, Cin // G, 1) * d["gamma"].astype(np.float64)
    b = d["beta"].astype(np.float64) - np.repeat(mean, Cin // G, 1) * a
    return np.stack([a, b], -1)


def coef_from_colsums(ws, d, first_slot_only=False):
    """What groupnorm_coef forms: one-pass fp64 moments from the producers' column sums ws [B, ns, Cin, 2], rounded once to fp32.
    first_slot_only: the mutation that reads slot 0 of nsplit alone."""
    B, ns, Cin, _ = ws.shape
    G, n = d["G"], d["HW"] * (Cin // d["G"])
    tot = ws[:, 0] if first_slot_only else ws.sum(1)
    s, q = (tot[..., k].reshape(B, G, -1).sum(2) for k in (0, 1))
    mean = s / n
    rstd = 1.0 / np.sqrt(np.maximum(q / n - mean * mean, 0) + EPS)
    a = np.repeat(rstd, Cin // G, 1) * d["gamma"].astype(np.float64)
    b = d["beta"].astype(np.float64) - np.repeat(mean, Cin // G, 1) * a
    return np.stack([a, b], -1).astype(f32)


def coef_tolerance(d):
    """(da, db) [B, Cin] of gn_coef_ref, with the fp64 statistics' own term kept where the group's variance is tiny (gn_coef_ref asserts it
    below u and drops it; the same derivation, not dropped)."""
    Cin, G = d["C"] + d["C2"], d["G"]
    mean, rstd, _, _, (c64, dmean) = gn_stats64(nc.gn_full(d), G)
    rep = lambda t: np.repeat(t, Cin // G, 1)
    a = rep(rstd) * d["gamma"].astype(np.float64)
    ma = rep(mean) * a
    c = rep(np.maximum(c64, 0))
    return (2 * U + c) * np.abs(a), U * np.abs(d["beta"].astype(np.float64)) + (2 * U + c) * np.abs(ma) + rep(dmean) * np.abs(a)


def conv_weights(Cin, Cout, seed=0):
    g = nc.rng(7000 + seed + Cin + 3 * Cout)
    return (nc.randn32(g, Cout, Cin, 3, 3) / f32((Cin * 9) ** 0.5)).astype(f32)


# ---------------------------------------------------------------------------------------------- references
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _nchw(a, H):
    """[B, H W, C] numpy -> [B, C, H, W] torch (same dtype)"""
    B, HW, C = a.shape
    return _t(a).reshape(B, H, HW // H, C).permute(0, 3, 1, 2).contiguous()


def _rows(t):
    """[B, Cout, H, W] torch -> [B H W, Cout]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def normed64(d, coef, act, extra_dz=None):
    """z, n, dn [B, HW, Cin] fp64 for the coefficient VALUES coef [B, Cin, 2] (any dtype): dz = u |z| (+ extra_dz)."""
    c = coef.astype(np.float64)
    x = nc.gn_full(d).astype(np.float64)
    z = c[:, None, :, 0] * x + c[:, None, :, 1]
    dz = U * np.abs(z) + (0.0 if extra_dz is None else extra_dz)
    return z, act_ref(act, z), act_tol(act, z, dz)


def conv_terms(n, dn, w, H):
    """acc, A, D [M, Cout] torch fp64: the 3 x 3 / pad 1 convolution of n, of |n| with |w| and of dn with |w|."""
    w64 = _t(w).double()
    conv = lambda a, ww: _rows(F.conv2d(_nchw(a, H), ww, padding=1))
    return conv(n, w64), conv(np.abs(n), w64.abs()), conv(dn, w64.abs())


def loader_reference(d, H, w, coef, act, extra_dz=None, E=E_W1D):
    """(acc64, A + D / E) of the loader forms for tests/test_hip_epilogue_matrix.py's epilogue_ref: 1.1 E (A + D / E + ...) = 1.1 (E A_terms + D)."""
    _, n, dn = normed64(d, coef, act, extra_dz)
    acc, A, D = conv_terms(n, dn, w, H)
    return acc, A + D / E


def chain_extra_dz(d):
    """da |x| + db [B, HW, Cin]: what the device's coefficients may differ by from the exact ones, on z."""
    da, db = coef_tolerance(d)
    return da[:, None, :] * np.abs(nc.gn_full(d).astype(np.float64)) + db[:, None, :]


def epilogue_operands(M, N, G, seed=0):
    """The operands run_matrix draws (the same generator and order): bias [N], rowbias [G, N], res [M, N], wide [M, N + 32], rowscale [G]."""
    g = torch.Generator().manual_seed(1000 + seed)
    bias, rowbias = torch.randn(N, generator=g), torch.randn(G, N, generator=g)
    res = torch.randn(M, N, generator=g)
    wide = torch.randn(M, N + 32, generator=g)
    rsc = -(torch.rand(G, generator=g) + 0.5)
    return dict(bias=bias, rowbias=rowbias, res=res, wide=wide, rsc=rsc)


def epilogue_terms(ops, combo, rpg, N):
    hb, hrb, act, rk, osc, hrs = combo
    res = {"off": None, "dense": ops["res"].double(), "slice": ops["wide"][:, 16:16 + N].double()}[rk]
    return dict(bias=ops["bias"].double() if hb else None, rowbias=ops["rowbias"].double() if hrb else None, rows_per_group=rpg, act=act,
                residual=res, out_scale=osc, rowscale=ops["rsc"].double() if hrs else None)


def act32(name, v):
    """torch fp32 activations of the replays"""
    if name == "silu":
        return F.silu(v)
    if name == "elu":
        return F.elu(v)
    if name == "relu":
        return F.relu(v)
    if name == "lrelu":
        return F.leaky_relu(v, 0.2)
    return v


def epilogue_replay(acc32, ops, combo, rpg, mutation=None):
    """The header's epilogue in fp32 on an fp32 contraction [M, N].  Mutations: "rowbias_wrong_image", "residual_before_act",
    "scale_residual_only"."""
    hb, hrb, act, rk, osc, hrs = combo
    M, N = acc32.shape
    grp = torch.arange(M) // rpg
    v = acc32
    if hb:
        v = v + ops["bias"]
    if hrb:
        rb = ops["rowbias"].roll(1, 0) if mutation == "rowbias_wrong_image" else ops["rowbias"]
        v = v + rb[grp]
    res = {"off": None, "dense": ops["res"], "slice": ops["wide"][:, 16:16 + N]}[rk]
    s = torch.full((M, 1), osc, dtype=torch.float32)
    if hrs:
        s = s * ops["rsc"][grp][:, None]
    if res is not None and mutation == "residual_before_act":
        return act32(act, v + res) * s
    v = act32(act, v)
    if res is not None and mutation == "scale_residual_only":
        return v + res * s
    if res is not None:
        v = v + res
    return v * s


# ---------------------------------------------------------------------------------------------- loader replay
LOADER_MUTATIONS = ("pad_act_b", "coef_next_image", "x2_offset_dropped", "sources_swapped", "halo_other_image", "ab_swapped",
                    "silu_skipped", "silu_twice")


def loader_replay(d, H, w, coef32, act, mutation=None):
    """fp32 replay of the loader forms' contraction [M, Cout]: z rounded to fp32 from the fp64 fma of the fp32 operands, torch fp32 SiLU,
    torch fp32 direct convolution.  Mutations: LOADER_MUTATIONS."""
    B, HW, C1, C2 = d["B"], d["HW"], d["C"], d["C2"]
    x1, x2 = d["x"], d["x2"]
    if mutation == "sources_swapped" and C2:
        full = np.concatenate([x2, x1], -1)
    elif mutation == "x2_offset_dropped" and C2:                     # x2 read at channel c instead of c - C1 (wrapping inside its row)
        full = np.concatenate([x1, x2[..., (np.arange(C2) + C1) % C2]], -1)
    else:
        full = nc.gn_full(d)
    c = coef32.astype(np.float64)
    if mutation == "coef_next_image":
        c = np.roll(c, -1, 0)
    a, b = (c[..., 1], c[..., 0]) if mutation == "ab_swapped" else (c[..., 0], c[..., 1])
    z = _t((a[:, None, :] * full.astype(np.float64) + b[:, None, :]).astype(f32))
    n = z if (act == "none" or mutation == "silu_skipped") else F.silu(z)
    if mutation == "silu_twice":
        n = F.silu(n)
    n = n.reshape(B, H, HW // H, C1 + C2).permute(0, 3, 1, 2).contiguous()
    w32 = _t(w)
    if mutation == "pad_act_b":                                       # the padding left at act(b)
        pb = act32(act, _t(b.astype(f32)))[:, :, None, None].expand(B, C1 + C2, H + 2, HW // H + 2).clone()
        pb[:, :, 1:-1, 1:-1] = n
        return _rows(F.conv2d(pb, w32))
    if mutation == "halo_other_image":                                # the images stacked: a block's halo row comes from the neighbour image
        tall = n.permute(1, 0, 2, 3).reshape(1, C1 + C2, B * H, HW // H)
        out = F.conv2d(tall, w32, padding=1)
        return _rows(out.reshape(-1, B, H, HW // H).permute(1, 0, 2, 3))
    return _rows(F.conv2d(n, w32, padding=1))


# ---------------------------------------------------------------------------------------------- tail-norm form
def tail_inputs(B, H, W, Cin, Cout, groups, offset, seed=0):
    g = nc.rng(9000 + seed + 1000 * H + Cin + Cout + B)
    x = nc.randn32(g, B, H * W, Cin)
    w = conv_weights(Cin, Cout, seed)
    bias = (nc.randn32(g, Cout) + f32(offset) * (g.random(Cout) + 0.5).astype(f32)).astype(f32)
    rowbias = nc.randn32(g, B, Cout)
    gamma = ((g.random(Cout) + 0.5) * 1.7).astype(f32) * _sign(g, Cout)          # not near 1
    beta = (nc.randn32(g, Cout) * f32(0.8) + f32(0.6)).astype(f32)              # not near 0
    return dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, G=groups, x=x, w=w, bias=bias, rowbias=rowbias, gamma=gamma, beta=beta)


def tail_contraction(t):
    """acc, A [B, HW, Cout] numpy fp64, computed once per case"""
    x, w64 = t["x"].astype(np.float64), _t(t["w"]).double()
    shp = (t["B"], t["H"] * t["W"], t["Cout"])
    conv = lambda a, ww: _rows(F.conv2d(_nchw(a, t["H"]), ww, padding=1)).numpy().reshape(shp)
    return conv(x, w64), conv(np.abs(x), w64.abs())


def tail_ref(t, acc, A, has_bias, has_rowbias, act, E=E_W1D):
    """(reference, bound) [B, HW, Cout] of act(GroupNorm(conv + bias + rowbias)): the module docstring's first-order bound."""
    B, HW, Cout, G = t["B"], t["H"] * t["W"], t["Cout"], t["G"]
    cpg = Cout // G
    pre, mag = acc, A
    if has_bias:
        pre, mag = pre + t["bias"].astype(np.float64), mag + np.abs(t["bias"].astype(np.float64))
    if has_rowbias:
        pre, mag = pre + t["rowbias"].astype(np.float64)[:, None, :], mag + np.abs(t["rowbias"].astype(np.float64))[:, None, :]
    e = 1.1 * E * mag
    grp = lambda a: a.reshape(B, HW, G, cpg)
    mean = grp(pre).mean((1, 3), keepdims=True)
    var = ((grp(pre) - mean) ** 2).mean((1, 3), keepdims=True)
    rstd = 1.0 / np.sqrt(var + EPS)
    nhat = (grp(pre) - mean) * rstd
    e_mean, e_rms = grp(e).mean((1, 3), keepdims=True), np.sqrt((grp(e) ** 2).mean((1, 3), keepdims=True))
    dnhat = rstd * (grp(e) + e_mean) + np.abs(nhat) * rstd * e_rms
    ga, be = t["gamma"].astype(np.float64).reshape(1, 1, G, cpg), t["beta"].astype(np.float64).reshape(1, 1, G, cpg)
    y_pre = nhat * ga + be
    tol_pre = 1.1 * (np.abs(ga) * dnhat + 6 * U * ((np.abs(grp(pre)) + np.abs(mean)) * rstd * np.abs(ga) + np.abs(be)))
    return act_ref(act, y_pre).reshape(B, HW, Cout), act_tol(act, y_pre, tol_pre).reshape(B, HW, Cout)


def tail_replay(t, has_bias, has_rowbias, act, mutation=None):
    """fp32 replay: torch fp32 direct convolution, + bias + rowbias in fp32, fp64 mean and variance about the mean of those fp32 values,
    rounded to fp32, y = act((v - mu) * (rstd gamma) + beta) as the kernel writes it.  Mutations: "var_about_zero", "group_width_x2"."""
    B, H, HW, Cout, G = t["B"], t["H"], t["H"] * t["W"], t["Cout"], t["G"]
    v = _rows(F.conv2d(_nchw(t["x"], H), _t(t["w"]), padding=1)).reshape(B, HW, Cout)
    if has_bias:
        v = v + _t(t["bias"])
    if has_rowbias:
        v = v + _t(t["rowbias"])[:, None, :]
    v = v.numpy()
    if mutation == "group_width_x2":
        G = G // 2 if G > 1 else 2
    cpg = Cout // G
    g64 = v.astype(np.float64).reshape(B, HW, G, cpg)
    mean = g64.mean((1, 3), keepdims=True)
    var = (g64 ** 2).mean((1, 3), keepdims=True) if mutation == "var_about_zero" else ((g64 - mean) ** 2).mean((1, 3), keepdims=True)
    mu = np.broadcast_to(mean.astype(f32), g64.shape).reshape(B, HW, Cout)
    sc = np.broadcast_to((1.0 / np.sqrt(var + EPS)).astype(f32), g64.shape).reshape(B, HW, Cout) * t["gamma"]
    y = ((v - mu) * sc + t["beta"]).astype(f32)
    return nc.act_f32(act, y)


# ---------------------------------------------------------------------------------------------- FIR forms
def fir_taps(gain):
    k = np.outer([1.0, 3.0, 3.0, 1.0], [1.0, 3.0, 3.0, 1.0])
    return (k / k.sum() * gain).astype(f32)


def fir_out_size(n, up, down, p0, p1):
    return (n * up + p0 + p1 - 4) // down + 1


def upfirdn(x, k, up, down, p0, p1, dtype=np.float64):
    """upfirdn2d of x [B, H, W, C] with the 4 x 4 taps k: zero insertion, padding, correlation with the flipped taps, decimation.  The
    sixteen taps are multiplied and added one after the other in ``dtype`` (float32: the replay's tap loop)."""
    B, H, W, C = x.shape
    q0, q1 = max(p0, 0), max(p1, 0)                                # a negative pad crops
    xu = np.zeros((B, H * up + q0 + q1, W * up + q0 + q1, C), dtype)
    xu[:, q0:q0 + H * up:up, q0:q0 + W * up:up] = x
    xu = xu[:, q0 - p0:xu.shape[1] - (q1 - p1), q0 - p0:xu.shape[2] - (q1 - p1)]
    OH, OW = fir_out_size(H, up, down, p0, p1), fir_out_size(W, up, down, p0, p1)
    kf = k[::-1, ::-1].astype(dtype)
    out = np.zeros((B, OH, OW, C), dtype)
    for i in range(4):
        for j in range(4):
            out = (out + xu[:, i:i + (OH - 1) * down + 1:down, j:j + (OW - 1) * down + 1:down] * kf[i, j]).astype(dtype)
    return out


def fir_inputs(B, H, W, C, kind, seed=0):
    d = raw_inputs(B, H * W, C, 0, max(1, C // 4), kind, seed=seed + 31 * H + W)
    sg = np.repeat(_sign(nc.rng(seed + C), max(1, C // 4)), min(4, C))           # mixed signs of the channel means, one per group
    d["x"] = (d["x"] * sg[None, None, :]).astype(f32)
    return d


def fir_ref(d, H, coef, mode, act, extra_dz=None):
    """(reference, bound) [B, OH, OW, C]: tol = sum |k_t| dn_t + 17 u sum |k_t n_t|."""
    up, down, p0, p1, gain = FIR_MODES[mode]
    k = fir_taps(gain)
    _, n, dn = normed64(d, coef, act, extra_dz)
    img = lambda a: a.reshape(d["B"], H, d["HW"] // H, -1)
    return (upfirdn(img(n), k, up, down, p0, p1),
            upfirdn(img(dn), np.abs(k), up, down, p0, p1) + 17 * U * upfirdn(np.abs(img(n)), np.abs(k), up, down, p0, p1))


FIR_MUTATIONS = ("pad_act_b", "coef_next_image", "ab_swapped", "silu_skipped", "silu_twice")


def fir_replay(d, H, coef32, mode, act, mutation=None):
    up, down, p0, p1, gain = FIR_MODES[mode]
    B, HW, C = d["B"], d["HW"], d["C"]
    W = HW // H
    c = coef32.astype(np.float64)
    if mutation == "coef_next_image":
        c = np.roll(c, -1, 0)
    a, b = (c[..., 1], c[..., 0]) if mutation == "ab_swapped" else (c[..., 0], c[..., 1])
    z = _t((a[:, None, :] * d["x"].astype(np.float64) + b[:, None, :]).astype(f32))
    n = z if (act == "none" or mutation == "silu_skipped") else F.silu(z)
    if mutation == "silu_twice":
        n = F.silu(n)
    n = n.numpy().reshape(B, H, W, C)
    k = fir_taps(gain)
    if mutation == "pad_act_b":          # every tap outside the image reads act(b): a frame of act(b) pixels around the image, the pads shrunk
        fr = 1
        pb = act32(act, _t(b.astype(f32))).numpy()[:, None, None, :]
        big = np.broadcast_to(pb, (B, H + 2 * fr, W + 2 * fr, C)).copy()
        big[:, fr:-fr, fr:-fr] = n
        return upfirdn(big, k, up, down, p0 - fr * up, p1 - fr * up, f32)
    return upfirdn(n, k, up, down, p0, p1, f32)


# ---------------------------------------------------------------------------------------------- the row-wise F(4, 3) on fp16 pairs, emulated
_A, _B = 2.0 / 3.0, 1.5
F43_BT = np.array([[1, 0, -(_A * _A + _B * _B), 0, 1, 0],
                   [0, -_A * _B * _B, -_B * _B, _A, 1, 0], [0, _A * _B * _B, -_B * _B, -_A, 1, 0],
                   [0, -_B * _A * _A, -_A * _A, _B, 1, 0], [0, _B * _A * _A, -_A * _A, -_B, 1, 0],
                   [0, 1, 0, -(_A * _A + _B * _B), 0, 1]], np.float64)
_na, _nb, _n0 = 1 / (2 * _A * _A * (_A * _A - _B * _B)), 1 / (2 * _B * _B * (_B * _B - _A * _A)), 1 / (_A * _A * _B * _B)
F43_G = np.array([[_n0, 0, 0], [_na, _A * _na, _A * _A * _na], [_na, -_A * _na, _A * _A * _na], [_nb, _B * _nb, _B * _B * _nb],
                  [_nb, -_B * _nb, _B * _B * _nb], [0, 0, 1]], np.float64)
F43_AT = np.array([[1, 1, 1, 1, 1, 0], [0, _A, -_A, _B, -_B, 0], [0, _A ** 2, _A ** 2, _B ** 2, _B ** 2, 0],
                   [0, _A ** 3, -_A ** 3, _B ** 3, -_B ** 3, 1]], np.float64)


def f43_identity_error():
    """max |A^T ((G g) . (B^T d)) - correlation| on random data in fp64: the restated matrices are F(4, 3)'s."""
    g = nc.rng(0)
    dd, gg = g.standard_normal(6), g.standard_normal(3)
    y = F43_AT @ ((F43_G @ gg) * (F43_BT @ dd))
    return float(np.abs(y - np.array([sum(gg[k] * dd[i + k] for k in range(3)) for i in range(4)])).max())


def _pairs(v):
    hi = v.half().float()
    return hi, (v - hi).half().float()


def wino1d_emulate(n32, w, H):
    """The row-wise F(4, 3) convolution of n32 [B, H W, Cin] fp32 (W % 4 == 0) with w [Cout, Cin, 3, 3] on fp16 pairs: [B H W, Cout] fp32."""
    B, HW, Cin = n32.shape
    W, Cout = HW // H, w.shape[0]
    T = W // 4
    x = _t(n32).reshape(B, H, W, Cin)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))                                               # one zero row above and below, one zero pixel left and right
    d = xp.unfold(2, 6, 4)                                                           # [B, H + 2, T, Cin, 6]
    V = torch.einsum("ik,brtck->brtic", _t(F43_BT).float(), d)                       # fp32 transform, [B, H + 2, T, 6, Cin]
    Uw = torch.einsum("ik,ocyk->iyoc", _t(F43_G), _t(w).double())                    # [6, 3 (ky), Cout, Cin] fp64
    e = int(np.frexp(float(Uw.abs().max()))[1])
    k = 12 - e
    Us = (Uw * 2.0 ** k).float()
    Vh, Vl = _pairs(V)
    Uh, Ul = _pairs(Us)
    M = torch.zeros(B, H, T, 6, Cout)
    for ky in range(3):
        vh, vl = Vh[:, ky:ky + H], Vl[:, ky:ky + H]
        for a_, b_ in ((vh, Uh), (vh, Ul), (vl, Uh)):
            M = M + torch.einsum("brtic,ioc->brtio", a_, b_[:, ky])
    Y = torch.einsum("ai,brtio->brtao", _t(F43_AT).float(), M) * f32(2.0 ** -k)     # [B, H, T, 4, Cout]
    return Y.reshape(B * H * W, Cout)


# ---------------------------------------------------------------------------------------------- the absolute bounds for the earlier modules
def _nhwc_np(x):
    """[B, C, H, W] torch -> [B, H W, C] numpy fp32"""
    B, C, H, W = x.shape
    return np.ascontiguousarray(x.permute(0, 2, 3, 1).reshape(B, H * W, C).float().numpy())


def _raw_dict(x1, x2, gamma, beta, G):
    a, b = _nhwc_np(x1), (None if x2 is None else _nhwc_np(x2))
    return dict(B=a.shape[0], HW=a.shape[1], C=a.shape[2], C2=0 if b is None else b.shape[2], G=G, x=a, x2=b,
                gamma=gamma.float().numpy(), beta=beta.float().numpy())


def chain_bound_conv(x1, x2, gamma, beta, G, w, bias, act):
    """The end-to-end chain's bound for tests that hold their own NCHW torch operands (tests/test_wino1d_normload*.py): per-element
    tolerance [B, H, W, Cout] of conv(act(GroupNorm(cat[x1, x2]))) + bias against the EXACT fp64 GroupNorm, coefficients formed on the
    device from column sums (coef_tolerance) and the loader's one fma."""
    d, H = _raw_dict(x1, x2, gamma, beta, G), x1.shape[2]
    acc, A = loader_reference(d, H, w.float().numpy(), exact_coef(d), act or "none", chain_extra_dz(d))
    terms = dict(bias=bias.double(), rowbias=None, rows_per_group=d["HW"], act="none", residual=None, out_scale=1.0, rowscale=None)
    ref, tol = epilogue_ref(acc, A, terms, E_W1D)
    shape = (d["B"], H, d["HW"] // H, w.shape[0])
    return ref.reshape(shape), tol.reshape(shape)


def chain_bound_fir(x, gamma, beta, G, mode, act):
    """The same for the FIR resamplers (tests/test_upfirdn2d_gn.py): (reference, tolerance) [B, OH, OW, C]."""
    d, H = _raw_dict(x, None, gamma, beta, G), x.shape[2]
    ref, tol = fir_ref(d, H, exact_coef(d), mode, act or "none", chain_extra_dz(d))
    return _t(ref), _t(tol)


def tail_bound(x, w, bias, rowbias, gamma, beta, groups, act="silu"):
    """The tail-norm form's bound for tests/test_wino1d_fused_gn.py: (reference, tolerance) [B, H, W, Cout] from NCHW torch operands."""
    B, Cin, H, W = x.shape
    t = dict(B=B, H=H, W=W, Cin=Cin, Cout=w.shape[0], G=groups, x=_nhwc_np(x), w=w.float().numpy(), bias=bias.float().numpy(),
             rowbias=rowbias.float().numpy(), gamma=gamma.float().numpy(), beta=beta.float().numpy())
    acc, A = tail_contraction(t)
    ref, tol = tail_ref(t, acc, A, True, True, act)
    return _t(ref).reshape(B, H, W, -1), _t(tol).reshape(B, H, W, -1)


# ---------------------------------------------------------------------------------------------- comparison
def worst(out, ref, tol):
    """largest err / tol (NaN in `out` counts as inf); torch or numpy"""
    as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return nc.worst(as_np(out), as_np(ref), as_np(tol))[0]
