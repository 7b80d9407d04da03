"""The four kernels that apply a GroupNorm (+ SiLU) themselves, element-wise against fp64 (python -m pytest -m gpu):

    form                                   entry point                               kernel
    norm in the tail of the row-wise conv  idiff_conv2d_wino1d_gn_f32                wino1d_gn_kernel<4 / 8 / 16>
    norm in the loader, one source         idiff_conv2d_wino1d_normload_f32          wino1d_nl_kernel<1 / 2>
    norm in the loader of cat[x1, x2]      idiff_conv2d_wino1d_normload_2src_f32     wino1d_nl2_kernel<1 / 2>
    norm in the loader of the resamplers   idiff_upfirdn2d_gn_f32                    upfirdn2d_nhwc_up2_block_gn, upfirdn2d_nhwc_down2_block_gn

References, bounds, the E that is used (4.5e-6, behind it an emulated 4.1e-7) and the coefficient form's own error are derived in
tests/normfused_cases.py from the arithmetic and a CPU reference alone; tests/test_normfused_host.py shows on the CPU that the bounds hold
for an fp32 replay of every case and that thirteen mutations leave them by a factor above 10.  Nothing in a bound is a kernel's output.

Isolated consumer (every matrix): the test hands the kernel its own fp32 coefficients, and the reference is fp64 on those values.
  Loader forms: one pytest case is one shape and one loader activation; inside it tests/test_hip_epilogue_matrix.py's run_matrix launches
  the product of 240 epilogue combinations, and again with the fp64 column sums (checked slot by slot), into a NaN-filled output that is
  followed by NaN guard rows; the raw sources lie inside larger buffers filled with 1e3.  r1_body<32, false, NL, S2> compiles the plain
  kernel's tail 16 times per (NL, sources): the cases reach all 64 (test_loader_tail_instantiations_are_enumerated), with the executor's two
  production epilogues (Conv_0: bias + rowbias + column sums; Conv_1: bias + residual + 1 / sqrt 2 + column sums).
  Statistics kinds: |mean| / std = 30, a group of zero variance (|a| ~ 1.8e3, |b| ~ 4.4e3), G in {Cin / 4, Cin / 16, 1}, groups of 12 --
  bias-only and the two production epilogues with column sums, against the same isolated bound (dz = u |z| whatever the coefficients' size).
  Tail norm: bias {off, on} x rowbias {off, on} x five activations per shape; widths 4, 8 and 16; one channel per group up to one group per tile.
  FIR: act {silu, none} x statistics {benign, |mean| / std = 30} per shape, the route asserted, every edge row and column compared.
End-to-end chain: a producing conv2d_wino1d writes x and its column sums at nsplit = H / 16 = 2 (two producers for two sources),
groupnorm_coef forms the coefficients on the device, the loader form consumes them; the reference is the EXACT fp64 GroupNorm of the stored
x and the bound gains conv(1.1 (da |x| + db), |w|) (normfused_cases.coef_tolerance).  32 + 64 channels in 8 groups of 12 straddle both a K
step and the two sources.  Next to E A the coefficient term is 0.24 - 0.26 x on benign statistics, 4.6 - 4.7 x at |mean| / std = 30, and
1.1e3 x with a zero-variance group (channels 4 .. 7 of the producer have zero weights and the bias 2.5), where the fp64 one-pass variance's
own cancellation enters the coefficients (printed as CHAIN).  The same chain feeds both resamplers (groupnorm_reader_coef, [2, 32, 32, 64]).

Found by this module: the loader forms admit a single K step (Cin = 16) but the launcher asked the plain kernel's query -- which needs two --
whether column sums may be written, and refused them with "switched off"; fixed in the launcher (csrc/wino1d.hip, r1_run).

Measured on the MI355X (launches compared, largest err / tol; a ratio above 0.5 is called out):
    form                                   cases   launches   max err / tol
    loader, one source                        6      2880        0.071
    loader, two sources                       6      2880        0.084
    loader, statistics kinds                 22        66        0.068
    loader, end-to-end chains                 5        30        0.061
    tail norm                                 6       120        0.028
    FIR up / down                           5 / 5    20 / 20     0.174 / 0.201
    FIR, end-to-end chains                    4         8        0.389
6,024 launches compared element by element; no ratio above 0.5.  The largest, 0.389, is the up resampler behind device-formed coefficients:
there the bound is the coefficients' own tolerance and the kernel's coefficients use a good part of it.  No combination failed once the
launcher served the single-K-step column sums: the matrix exposed no kernel bug.
"""
import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
import norm_act_cases as nc
import normfused_cases as fc
from id_diff_amd import _lib
from test_hip_epilogue_matrix import DEV, Form, run_matrix

pytestmark = pytest.mark.gpu
GUARD = 64            # NaN rows behind every output
BURY = 4096           # floats of 1e3 in front of and behind every raw input
EPS = fc.EPS


def buried(a):
    """a (numpy fp32) on the device as a view into a larger buffer whose surroundings hold 1e3: a read outside the tensor is an O(100) error"""
    flat = torch.full((a.size + 2 * BURY,), 1e3, device=DEV)
    flat[BURY:BURY + a.size] = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1).to(DEV)
    return flat[BURY:BURY + a.size].view(a.shape)


def guarded(M, N):
    """(out [M, N] view, check) of a NaN buffer with GUARD rows behind the view: check() is True while they are all still NaN and the
    view holds none"""
    full = torch.full((M + GUARD, N), float("nan"), device=DEV)
    return full[:M], lambda: int(torch.isnan(full).sum()) == GUARD * N


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bank(w, Cin, Cout):
    return _lib.wino1d_pack(dev(w).permute(0, 2, 3, 1).contiguous(), Cin, Cout)


def test_loader_tail_instantiations_are_enumerated():
    """The loader cases x {silu, none} x run_matrix's product with and without column sums reach all 4 x 16 = 64 instantiations of the
    tail the loader kernels share with wino1d_kernel, the production ones included (tests/test_normfused_host.py asserts the same set)."""
    seen = fc.tail_instantiations()
    assert len(seen) == 64
    assert {(nl, two) for nl, two, *_ in seen} == {(nl, two) for nl in fc.NL_ACTS for two in (False, True)}
    for nl in fc.NL_ACTS:
        for two in (False, True):
            assert (nl, two, False, True, True, True) in seen and (nl, two, False, False, False, True) in seen


def loader_form(name, shape, act, d, w, coefd, acc, A):
    """The Form of a loader case: d's raw sources buried in 1e3, a guarded NaN output, the launch with the loader request."""
    B, H, C1, C2, Cout = shape
    Cin, M = C1 + C2, B * H * fc.W32
    x1d, x2d = buried(d["x"]), (buried(d["x2"]) if C2 else None)
    u = bank(w, Cin, Cout)
    out, check = guarded(M, Cout)
    ns = _lib.conv2d_wino1d_colstats_split(B, H, fc.W32, max(Cin, 32), Cout)      # (the query is the plain kernel's: two K steps at least)
    assert ns == H // 16 and H * fc.W32 // ns == 512

    def launch(ep):
        _lib.with_normload(ep, coefd, act, x2d, C1 if C2 else None)
        _lib.conv2d_wino1d(x1d, u, out, B, H, fc.W32, Cin, Cout, epilogue=ep)

    return Form(name, shape + (act,), M, Cout, H * fc.W32, acc, A, fc.E_W1D, out, launch, stats_rows=512, outside_nan=check)


def isolated(shape, act, kind="benign", cpg=4):
    B, H, C1, C2, Cout = shape
    Cin = C1 + C2
    d = fc.raw_inputs(B, H * fc.W32, C1, C2, 1 if cpg == 0 else Cin // cpg, kind)
    w = fc.conv_weights(Cin, Cout)
    coef = fc.exact_coef(d).astype(np.float32)
    acc, A = fc.loader_reference(d, H, w, coef, act)
    name = "normload" + ("_2src" if C2 else "") + ("" if kind == "benign" and cpg == 4 else f"[{kind}, groups of {cpg or Cin}]")
    return loader_form(name, shape, act, d, w, dev(coef).reshape(-1), acc, A)


@pytest.mark.parametrize("act", fc.NL_ACTS)
@pytest.mark.parametrize("shape", fc.LOADER_CASES, ids=str)
def test_loader_matrix(shape, act):
    B, H, C1, C2, Cout = shape
    assert (_lib.conv2d_wino1d_normload_2src_ok(B, H, fc.W32, C1, C2, Cout) if C2 else _lib.conv2d_wino1d_normload_ok(B, H, fc.W32, C1, Cout))
    count, _ = run_matrix(isolated(shape, act))
    assert count == 480


@pytest.mark.parametrize("act", fc.NL_ACTS)
@pytest.mark.parametrize("shape,kind,cpg", fc.KIND_CASES, ids=str)
def test_loader_statistics_kinds(shape, kind, cpg, act):
    wanted = [fc.BIAS_ONLY] + fc.PRODUCTION
    count, _ = run_matrix(isolated(shape, act, kind, cpg), only=lambda combo, stats: stats and combo in wanted)
    assert count == 3


# ---------------------------------------------------------------------------------------------- end-to-end chains
def produce(B, H, Cout, sign, kind, seed):
    """A producing conv2d_wino1d (32 -> Cout channels, 32-pixel rows): its stored output [B, HW, Cout] and the column sums it wrote
    [B, ns, Cout, 2] on the device.  Channel means +-(1 .. 2), or +-30 output standard deviations ("mean30"); "constgroup": channels
    4 .. 7 have zero weights and the bias 2.5 (a group of exactly zero variance)."""
    g = nc.rng(11000 + seed)
    Cin, HW = 32, H * fc.W32
    xin = nc.randn32(g, B, HW, Cin)
    w = fc.conv_weights(Cin, Cout, seed + 1)
    bias = (sign * (g.random(Cout) + 1.0)).astype(np.float32)
    if kind == "mean30":
        bias[:] = np.float32(sign * 30.0)
    if kind == "constgroup":
        w[4:8] = 0
        bias[4:8] = np.float32(2.5)
    ns = _lib.conv2d_wino1d_colstats_split(B, H, fc.W32, Cin, Cout)
    assert ns == H // 16 and ns > 1
    cs = torch.full((B, ns, Cout, 2), float("nan"), device=DEV, dtype=torch.float64)
    out = torch.full((B, HW, Cout), float("nan"), device=DEV)
    _lib.conv2d_wino1d(dev(xin), bank(w, Cin, Cout), out, B, H, fc.W32, Cin, Cout, epilogue=_lib.make_epilogue(bias=dev(bias), colstats=cs))
    return out, cs, ns


@pytest.mark.parametrize("shape,G,kind", fc.CHAIN_CASES, ids=str)
def test_chain_producer_coefficients_consumer(shape, G, kind):
    B, H, C1, C2, Cout = shape
    Cin, HW = C1 + C2, H * fc.W32
    x1, cs1, ns = produce(B, H, 64, 1.0, kind, 1)
    if C1 < 64:                                    # the first C1 channels of a 64-channel producer, as a tensor and column sums of their own
        x1, cs1 = x1[..., :C1].contiguous(), cs1[:, :, :C1].contiguous()
    x2 = cs2 = None
    if C2:
        x2, cs2, _ = produce(B, H, C2, -1.0, "benign" if kind == "constgroup" else kind, 2)
    d = fc.raw_inputs(B, HW, C1, C2, G, "benign")                        # gamma and beta; the sources are the producers' stored outputs
    d["x"], d["x2"] = x1.cpu().numpy(), (x2.cpu().numpy() if C2 else None)
    assert bool(np.isfinite(nc.gn_full(d)).all())
    if kind == "constgroup":
        assert float(d["x"][..., 4:8].var()) == 0.0 and G == Cin // 4
    gd, bd = dev(d["gamma"]), dev(d["beta"])
    coefd = torch.full((B * Cin * 2,), float("nan"), device=DEV)
    _lib.groupnorm_coef(cs1, ns, C1, cs2, ns if C2 else 0, C2, B, HW, G, EPS, gd, bd, coefd)
    w = fc.conv_weights(Cin, Cout)
    extra = fc.chain_extra_dz(d)
    acc, A = fc.loader_reference(d, H, w, fc.exact_coef(d), "silu", extra)
    _, n, _ = fc.normed64(d, fc.exact_coef(d), "silu")
    _, A0, Dc = fc.conv_terms(n, 1.1 * extra, w, H)
    print(f"\nCHAIN {shape} G={G} {kind}: coefficient term / (E A) = {float((Dc / (fc.E_W1D * A0)).max()):.3g}")
    wanted = [fc.BIAS_ONLY] + fc.PRODUCTION
    f = loader_form("chain normload" + ("_2src" if C2 else "") + f"[{kind}, G={G}]", shape, "silu", d, w, coefd, acc, A)
    count, _ = run_matrix(f, only=lambda combo, stats: combo in wanted)
    assert count == 6


# ---------------------------------------------------------------------------------------------- tail-norm form
@pytest.mark.parametrize("case", fc.TAIL_CASES, ids=str)
def test_tail_norm_matrix(case):
    B, H, W, Cin, Cout, groups, offset = case
    assert _lib.conv2d_wino1d_gn_ok(B, H, W, Cin, Cout, groups)
    t = fc.tail_inputs(*case)
    acc, A = fc.tail_contraction(t)
    xd, u = buried(t["x"]), bank(t["w"], Cin, Cout)
    bd, rbd, gd, btd = dev(t["bias"]), dev(t["rowbias"]), dev(t["gamma"]), dev(t["beta"])
    out, check = guarded(B * H * W, Cout)
    failures, worst, count = [], 0.0, 0
    for hb in (False, True):
        for hrb in (False, True):
            for act in fc.TAIL_ACTS:
                kw = dict(rows_per_group=H * W)
                if hb:
                    kw["bias"] = bd
                if hrb:
                    kw["rowbias"] = rbd
                ep = _lib.with_groupnorm(_lib.make_epilogue(**kw), groups, gd, btd, EPS, act)
                out.fill_(float("nan"))
                _lib.conv2d_wino1d(xd, u, out, B, H, W, Cin, Cout, epilogue=ep)
                ref, tol = fc.tail_ref(t, acc, A, hb, hrb, act)
                r = fc.worst(out.cpu().view(B, H * W, Cout), ref, tol)
                count += 1
                tag = f"conv2d_wino1d_gn {case} bias={int(hb)} rowbias={int(hrb)} act={act}"
                if r > 1.0:
                    failures.append(f"{tag}: err / tol = {r:.3g}")
                else:
                    worst = max(worst, r)
                if not check():
                    failures.append(f"{tag}: wrote outside its [M, N] block")
    print(f"\nMATRIX conv2d_wino1d_gn {case}: {count} combinations, max err / tol = {worst:.3f}, {len(failures)} failures")
    assert not failures, "\n".join(failures)


def test_tail_norm_widths_are_all_covered():
    assert {c[2] for c in fc.TAIL_CASES} == {4, 8, 16}          # wino1d_gn_kernel<4 / 8 / 16>


# ---------------------------------------------------------------------------------------------- FIR forms
@pytest.mark.parametrize("mode,shape", [(m, s) for m in fc.FIR_CASES for s in fc.FIR_CASES[m]], ids=str)
def test_fir_matrix(mode, shape):
    B, H, W, C = shape
    up, down, p0, p1, gain = fc.FIR_MODES[mode]
    geom = (B, H, W, C, up, up, down, down, p0, p1, p0, p1)
    OH, OW = fc.fir_out_size(H, up, down, p0, p1), fc.fir_out_size(W, up, down, p0, p1)
    assert OH == _lib.upfirdn2d_out_size(H, up, down, p0, p1, 4)
    kd = dev(fc.fir_taps(gain))
    out, check = guarded(B * OH * OW, C)
    failures, worst, count = [], 0.0, 0
    for kind in fc.FIR_KINDS:
        d = fc.fir_inputs(B, H, W, C, kind)
        coef = fc.exact_coef(d).astype(np.float32)
        xd, coefd = buried(d["x"]), dev(coef).reshape(-1)
        assert _lib.upfirdn2d_route(xd, out, B, H, W, C, 4, 4, *geom[4:]) == fc.FIR_ROUTE[mode]
        for act in fc.NL_ACTS:
            out.fill_(float("nan"))
            _lib.upfirdn2d_gn(xd, kd, coefd, act, out, *geom)
            ref, tol = fc.fir_ref(d, H, coef, mode, act)
            r = fc.worst(out.cpu().view(B, OH, OW, C), ref, tol)              # every element, the edge rows and columns included
            count += 1
            tag = f"upfirdn2d_gn {mode} {shape} {kind} act={act}"
            if r > 1.0:
                failures.append(f"{tag}: err / tol = {r:.3g}")
            else:
                worst = max(worst, r)
            if not check():
                failures.append(f"{tag}: wrote outside its output")
    print(f"\nMATRIX upfirdn2d_gn {mode} {shape}: {count} combinations, max err / tol = {worst:.3f}, {len(failures)} failures")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind", fc.FIR_KINDS)
@pytest.mark.parametrize("mode", list(fc.FIR_CASES))
def test_fir_chain_producer_coefficients_consumer(mode, kind):
    """A producing conv2d_wino1d writes x [2, 32, 32, 64] and its column sums at nsplit = 2, groupnorm_reader_coef forms the coefficients on
    the device, the resampler consumes them; against the EXACT fp64 GroupNorm of the stored x, the bound with the coefficient term."""
    B, H, W, C, G = 2, 32, fc.W32, 64, 16
    up, down, p0, p1, gain = fc.FIR_MODES[mode]
    geom = (B, H, W, C, up, up, down, down, p0, p1, p0, p1)
    OH, OW = fc.fir_out_size(H, up, down, p0, p1), fc.fir_out_size(W, up, down, p0, p1)
    x, cs, ns = produce(B, H, C, 1.0, kind, 3)
    d = fc.raw_inputs(B, H * W, C, 0, G, "benign")
    d["x"] = x.cpu().numpy()
    assert bool(np.isfinite(d["x"]).all())
    coefd = torch.full((B * C * 2,), float("nan"), device=DEV)
    _lib.groupnorm_reader_coef(cs, ns, C, B, H * W, G, EPS, dev(d["gamma"]), dev(d["beta"]), coefd)
    out, check = guarded(B * OH * OW, C)
    assert _lib.upfirdn2d_route(x, out, B, H, W, C, 4, 4, *geom[4:]) == fc.FIR_ROUTE[mode]
    assert _lib.upfirdn2d_gn_ok(x, coefd, "silu", out, B, H, W, C, 4, 4, *geom[4:])          # a routed class in both modes
    worst = 0.0
    for act in fc.NL_ACTS:
        out.fill_(float("nan"))
        _lib.upfirdn2d_gn(x, dev(fc.fir_taps(gain)), coefd, act, out, *geom)
        ref, tol = fc.fir_ref(d, H, fc.exact_coef(d), mode, act, fc.chain_extra_dz(d))
        worst = max(worst, fc.worst(out.cpu().view(B, OH, OW, C), ref, tol))
        assert check(), f"{mode} {kind} {act}: wrote outside its output"
    print(f"\nMATRIX chain upfirdn2d_gn {mode} {kind}: 2 combinations, max err / tol = {worst:.3f}")
    assert worst <= 1.0
