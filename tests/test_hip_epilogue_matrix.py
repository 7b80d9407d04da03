"""Every combination of epilogue terms of every contraction launcher, element-wise against fp64 (python -m pytest -m gpu).

    out = (act(acc + bias + rowbias[g]) + residual) * out_scale * rowscale[g],   g = m // rows_per_group      (include/idiff_hip.h)

One pytest case is one launcher form at one shape.  Inside it the full product bias {off, on} x rowbias {off, on} x act {none, silu, elu,
relu, lrelu} x residual {off, dense, a column slice of a wider tensor} x out_scale {1, 0.7071} x rowscale {off, on} = 240 launches runs
into a NaN-filled output, and once more with the fp64 column sums wherever the launcher's *_colstats_split offers them.  The terms a form
does not take (a per-row-group term on the per-image kernels, column sums without whole tiles) are asserted to be REFUSED instead.

Reference and bound (``epilogue_ref``): the formula above in fp64 on the fp64 contraction `acc64` of the fp32 operands, and per element
    tol = |s| (1.1 E (A + |bias| + |rowbias|) + 8 u (|act(pre)| + |residual|)),   s = out_scale rowscale[g],  u = 2^-24,
A the same contraction of the operands' absolute values, 1.1 the Lipschitz constant of SiLU (the other activations: <= 1).  E is the
contraction's own error relative to A and is NOT taken from the kernels under test: scripts/f43_emulation.py (the project's CPU
emulation of the Winograd arithmetic, points 0, +-2/3, +-3/2, inf) against fp64 on Gaussian inputs at (5, 8, 8, 32->128), (3, 32, 32, 32->64),
(2, 16, 16, 128->64), (3, 8, 8, 8->64) gives max |err| / A = 1.8e-7 (fp32 direct), 1.4e-7 (F(2x2) fp32), 7.5e-7 (F(4x4) fp32), 1.08e-6 (F(4x4)
fp16 pairs); four times that, for the kernels' up to 2x larger norm errors and the tail of ~1e5 elements:
    E = 1e-6 for gemm*, conv2d_nhwc and F(2x2);   E = 4.5e-6 for F(4x4) fp32 / pairs and wino1d.
The split-bf16 contraction, the pair GEMM and the 1-D transform were not emulated and take their class's E.  Operands are all O(1)
(weights randn / sqrt(K), bias / rowbias / residual randn, rowscale = -(rand + 0.5) as the score function's -1 / std), so a dropped,
doubled or misordered term moves elements by O(1).  Column sums: |sum - sum_ref| <= n 2^-52 sum |v| against fp64 sums of the STORED
fp32 outputs (n rows per slot), the same for the squares, every slot of a NaN-filled buffer written.

Routes: every implicit-GEMM launch asserts the kernel and tail form `_lib.gemm_route` / `_lib.conv2d_route` report for it (the same
chooser the launcher calls); the tail forms reached over the module are asserted to be {buf-block, buf-row, vec64, scalar}
(test_every_epilogue_form_of_the_pipelined_kernel_has_cases).  wino1d_kernel compiles its tail 16 times over (act != none, residual, scaled, stats): the product
above with and without column sums enumerates all 16 (test_wino1d_instantiations_are_enumerated).

Measured on the MI355X (combinations run, largest err / tol; a ratio above 0.5 is called out):
    launcher form                                          cases   combinations   max err / tol
    conv2d_wino1d                                              4        1920          0.071
    conv2d_winograd43, fp32 contraction                        2         960          0.277
    conv2d_winograd43, fp16 pairs                              2         960          0.132
    conv2d_winograd, fp32                                      3         960          0.128
    conv2d_nhwc, default / IDIFF_NO_SPLIT / IDIFF_NO_PIPE    3 each   960 / 960 / 720   0.200 / 0.213 / 0.213
    conv2d_nhwc narrow head, the same three                  3 each     720 each      0.175 / 0.141 / 0.117
    gemm (routes of GEMM_CASES)                                9        2880          0.235
    gemm, column block of a NaN buffer                         1         240          0.184
    gemm, 64-bit tail (ldc = 2^20)                             2         720          0.168
    gemm, batched x 3, shared epilogue                         1         720          0.231
    gemm, 128-row tiles (TILE_CASES)                           7         872          0.296
    gemm_2src                                                  1         240          0.184
    gemm_pairs / weight_is_a batched / gemm_pairs_2src         3     240 / 336 / 240  0.143 / 0.178 / 0.143
16,088 launches compared element by element; no ratio above 0.5, the largest 0.296 (gemm (4096, 64, 32) on the 128 x 64 split tile).  The
bias-only combination stays within the bound on every launcher.  No combination failed: the matrix exposed no kernel bug.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

import id_diff_amd  # noqa: F401
from epilogue_cases import ACTS, E_DIRECT, E_F4, OUT_SCALE, RESIDUALS, SLICE_PAD, U32, act64, combos, epilogue_ref  # noqa: F401
from id_diff_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Form:
    """One launcher form at one shape: the fp64 contraction, the device buffers, and `launch(ep)` into the NaN-filled `out_view`."""

    def __init__(self, name, shape, M, N, rpg, acc64, A, E, out, launch, stats_rows=0, route=None, outside_nan=None):
        self.name, self.shape, self.M, self.N, self.rpg, self.acc64, self.A, self.E = name, shape, M, N, rpg, acc64, A, E
        self.out, self.launch, self.stats_rows, self.route, self.outside_nan = out, launch, stats_rows, route, outside_nan
        self.G = (M + rpg - 1) // rpg


def run_matrix(f, seed=0, only=None):
    """The 240 combinations (and again with column sums when f.stats_rows > 0).  f.out: [M, N] device view the launcher writes;
    f.route: None or callable(ep, combo) asserting the route; f.outside_nan: None or callable() -> bool, checked on the device after
    every launch."""
    g = torch.Generator().manual_seed(1000 + seed)
    M, N, G = f.M, f.N, f.G
    bias, rowbias = torch.randn(N, generator=g), torch.randn(G, N, generator=g)
    res = torch.randn(M, N, generator=g)
    wide = torch.randn(M, N + SLICE_PAD, generator=g)
    rsc = -(torch.rand(G, generator=g) + 0.5)
    d = dict(bias=bias.to(DEV), rowbias=rowbias.to(DEV), res=res.to(DEV), wide=wide.to(DEV), rsc=rsc.to(DEV))
    res_of = {"off": None, "dense": res.double(), "slice": wide[:, 16:16 + N].double()}
    cs = None
    if f.stats_rows:
        assert M % f.stats_rows == 0
        cs = torch.empty(M // f.stats_rows, N, 2, device=DEV, dtype=torch.float64)
    failures, worst_ratio, count = [], 0.0, 0
    for stats in ((False, True) if f.stats_rows else (False,)):
        for combo in combos():
            if only is not None and not only(combo, stats):
                continue
            hb, hrb, act, rk, osc, hrs = combo
            kw = dict(rows_per_group=f.rpg, act=act, out_scale=osc)
            if hb:
                kw["bias"] = d["bias"]
            if hrb:
                kw["rowbias"] = d["rowbias"]
            if rk == "dense":
                kw["residual"] = d["res"]
            elif rk == "slice":
                kw["residual"], kw["ld_residual"] = d["wide"][:, 16:16 + N], N + SLICE_PAD
            if hrs:
                kw["rowscale"] = d["rsc"]
            if stats:
                cs.fill_(float("nan"))
                kw["colstats"] = cs
            ep = _lib.make_epilogue(**kw)
            tag = f"{f.name} {f.shape} bias={int(hb)} rowbias={int(hrb)} act={act} residual={rk} out_scale={osc} rowscale={int(hrs)} colstats={int(stats)}"
            if f.route is not None:
                f.route(ep, combo, stats, tag)
            f.out.fill_(float("nan"))
            f.launch(ep)
            got = f.out.cpu().double()
            ref, tol = epilogue_ref(f.acc64, f.A, dict(bias=bias.double() if hb else None, rowbias=rowbias.double() if hrb else None,
                                                        rows_per_group=f.rpg, act=act, residual=res_of[rk], out_scale=osc,
                                                        rowscale=rsc.double() if hrs else None), f.E)
            ratio = (got - ref).abs() / tol
            ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)   # an unwritten element is a failure
            w = int(ratio.argmax())
            r = float(ratio.reshape(-1)[w])
            count += 1
            if r > 1.0:
                failures.append(f"{tag}: element (m={w // N}, n={w % N}) got {float(got.reshape(-1)[w])!r} want {float(ref.reshape(-1)[w])!r}: "
                                f"err / tol = {r:.3g}, {int((ratio > 1).sum())} of {ratio.numel()} elements beyond the bound")
            else:
                worst_ratio = max(worst_ratio, r)
            if f.outside_nan is not None and not f.outside_nan():
                failures.append(f"{tag}: wrote outside its [M, N] block")
            if stats:
                c = cs.cpu()
                v = got.reshape(M // f.stats_rows, f.stats_rows, N)
                for k, (sums, vals) in enumerate(((c[..., 0], v), (c[..., 1], v * v))):
                    want, bound = vals.sum(1), f.stats_rows * 2.0 ** -52 * vals.abs().sum(1)
                    bad = ~((sums - want).abs() <= bound)
                    if bool(bad.any()):
                        i = int(bad.reshape(-1).nonzero()[0])
                        failures.append(f"{tag}: column {'sum' if k == 0 else 'sum of squares'} slot {i // N} column {i % N}: got "
                                        f"{float(sums.reshape(-1)[i])!r} want {float(want.reshape(-1)[i])!r} (bound {float(bound.reshape(-1)[i]):.3g})")
    print(f"\nMATRIX {f.name} {f.shape}: {count} combinations, max err / tol = {worst_ratio:.3f}, {len(failures)} failures")
    assert not failures, f"{len(failures)} of {count} combinations fail:\n" + "\n".join(failures[:40])
    return count, worst_ratio


# ------------------------------------------------------------------------------------------- operands
def conv_operands(B, H, W, Cin, Cout, k=3, stride=1, pad=1, pad_hi=None, seed=0):
    """x NHWC and the [Cout, k, k, Cin] panel on the device; acc64 and A as [M, N] fp64 (the fp64 convolution of the fp32 operands and of
    their absolute values), computed once per shape."""
    g = torch.Generator().manual_seed(B * H * W + Cin + Cout + seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    hi = pad if pad_hi is None else pad_hi
    conv = lambda a, b: F.conv2d(F.pad(a.double(), (pad, hi, pad, hi)), b.double(), stride=stride).permute(0, 2, 3, 1)
    acc = conv(x, w)
    OH, OW = acc.shape[1:3]
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wt = w.permute(0, 2, 3, 1).contiguous().to(DEV)
    return xd, wt, acc.reshape(-1, Cout).contiguous(), conv(x.abs(), w.abs()).reshape(-1, Cout).contiguous(), OH, OW


def gemm_operands(M, N, K, seed=0):
    g = torch.Generator().manual_seed(M + N + K + seed)
    a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    return a, w, a.double() @ w.double().T, a.double().abs() @ w.double().abs().T


def note_route(route):
    assert route is not None, _lib.lib().idiff_last_error().decode()
    return route


# ------------------------------------------------------------------------------------------- the Winograd forms
WINO1D_SHAPES = [(3, 8, 8, 32, 128),      # eight images per block, a partial last block, two output-channel tiles
                 (3, 32, 32, 32, 64),     # half an image per block, ns = 2
                 (37, 4, 4, 32, 64),      # 32 images per block, partial
                 (1, 64, 64, 32, 64)]     # halo rows on both sides, ns = 8


def test_wino1d_instantiations_are_enumerated():
    """wino1d_kernel's tail is compiled for ACT {none, any} x RES x SCALED x STATS (csrc/wino1d.hip, finish_round): the loop of run_matrix
    with and without column sums visits all 16, the production one (none, res, scaled, +-stats) of (x + Conv_1(h)) / sqrt(2) included."""
    seen = set()
    for stats in (False, True):
        for hb, hrb, act, rk, osc, hrs in combos():
            seen.add((act != "none", rk != "off", osc != 1.0 or hrs, stats))
    assert len(seen) == 16 and (False, True, True, False) in seen and (False, True, True, True) in seen


@pytest.mark.parametrize("B,H,W,Cin,Cout", WINO1D_SHAPES)
def test_wino1d_matrix(B, H, W, Cin, Cout):
    assert _lib.conv2d_wino1d_ok(B, H, W, Cin, Cout)
    xd, wt, acc, A, _, _ = conv_operands(B, H, W, Cin, Cout)
    u = _lib.wino1d_pack(wt, Cin, Cout)
    out = torch.empty(B * H * W, Cout, device=DEV)
    ns = _lib.conv2d_wino1d_colstats_split(B, H, W, Cin, Cout)
    assert ns == max(1, H * W // 512)
    f = Form("conv2d_wino1d", (B, H, W, Cin, Cout), B * H * W, Cout, H * W, acc, A, E_F4, out,
             lambda ep: _lib.conv2d_wino1d(xd, u, out, B, H, W, Cin, Cout, epilogue=ep), stats_rows=H * W // ns)
    run_matrix(f)


@pytest.mark.parametrize("pairs", [False, True], ids=["fp32", "pairs"])
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(5, 8, 8, 32, 128), (3, 32, 32, 32, 64)])
def test_winograd43_matrix(B, H, W, Cin, Cout, pairs):
    assert (_lib.conv2d_winograd43h_ok if pairs else _lib.conv2d_winograd43_ok)(B, H, W, Cin, Cout)
    xd, wt, acc, A, _, _ = conv_operands(B, H, W, Cin, Cout)
    u = _lib.winograd43_pack(wt, Cin, Cout, pairs=pairs)
    out = torch.empty(B * H * W, Cout, device=DEV)
    ns = _lib.conv2d_winograd43_colstats_split(B, H, W, Cin, Cout)
    assert ns == max(1, H * W // 512)
    f = Form("conv2d_winograd43" + ("h" if pairs else ""), (B, H, W, Cin, Cout), B * H * W, Cout, H * W, acc, A, E_F4, out,
             lambda ep: _lib.conv2d_winograd43(xd, u, out, B, H, W, Cin, Cout, epilogue=ep, pairs=pairs), stats_rows=H * W // ns)
    run_matrix(f)


WINO22_MATRIX_CASES = [(3, 6, 10, 32, 64, "image"), (3, 6, 10, 32, 64, "row"), (2, 16, 16, 32, 128, "image")]


@pytest.mark.parametrize("B,H,W,Cin,Cout,rows", WINO22_MATRIX_CASES, ids=["-".join(map(str, c)) + "-fp32" for c in WINO22_MATRIX_CASES])
def test_winograd_matrix(B, H, W, Cin, Cout, rows):
    assert _lib.conv2d_winograd_ok(B, H, W, Cin, Cout)
    xd, wt, acc, A, _, _ = conv_operands(B, H, W, Cin, Cout)
    u = _lib.winograd_pack(wt, Cin, Cout)
    out = torch.empty(B * H * W, Cout, device=DEV)
    rpg = H * W if rows == "image" else W
    ns = _lib.conv2d_winograd_colstats_split(B, H, W, Cin, Cout)
    assert (ns > 0) == ((H, W) == (16, 16))                # 15 tiles of 2 x 2 per image: no whole workgroups, no whole samples
    f = Form("conv2d_winograd", (B, H, W, Cin, Cout, f"rows_per_group={rpg}"), B * H * W, Cout, rpg, acc, A,
             E_DIRECT, out, lambda ep: _lib.conv2d_winograd(xd, u, out, B, H, W, Cin, Cout, epilogue=ep),
             stats_rows=H * W // ns if ns else 0)
    run_matrix(f)
    if not ns:
        cs = torch.zeros(B * Cout * 2, device=DEV, dtype=torch.float64)
        with pytest.raises(RuntimeError, match="colstats"):
            _lib.conv2d_winograd(xd, u, out, B, H, W, Cin, Cout, epilogue=_lib.make_epilogue(colstats=cs))


# ------------------------------------------------------------------------------------------- conv2d_nhwc
MODES = {"default": (), "no_split": ("IDIFF_NO_SPLIT",), "no_pipe": ("IDIFF_NO_PIPE",)}


class options:
    def __init__(self, *names):
        self.ctx = [_lib.thread_option(n, 1) for n in names]

    def __enter__(self):
        for c in self.ctx:
            c.__enter__()

    def __exit__(self, *exc):
        for c in reversed(self.ctx):
            c.__exit__(*exc)
        return False


CONV_SHAPES = [
    # B, H, W, Cin, Cout, k, stride, pad, pad_hi, rows_per_group, expected pipe tail
    (3, 8, 8, 32, 64, 3, 1, 1, None, 64, "buf-block"),      # rows_per_group 64: the block-folded groups, column sums offered
    (2, 9, 7, 8, 12, 3, 2, 0, 1, 12, None),                 # Cin = 8: the general kernel; OH * OW = 12, M and N tails
    (5, 4, 4, 64, 32, 1, 1, 0, None, 16, "buf-row"),        # 1 x 1, groups of 16 rows: per-row group terms
]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride,pad,pad_hi,rpg,tail", CONV_SHAPES)
def test_conv2d_nhwc_matrix(B, H, W, Cin, Cout, k, stride, pad, pad_hi, rpg, tail, mode):
    xd, wt, acc, A, OH, OW = conv_operands(B, H, W, Cin, Cout, k, stride, pad, pad_hi)
    M = B * OH * OW
    assert rpg == OH * OW
    out = torch.empty(M, Cout, device=DEV)
    arith = "fp32" if mode == "no_split" else "split"
    want = f"pipe 64x64 {arith} {tail}" if (tail and mode != "no_pipe") else "direct-vec 64x64 fp32 scalar"

    def route(ep, combo, stats, tag):
        assert note_route(_lib.conv2d_route(xd, wt, out, B, H, W, Cin, Cout, k, k, stride, pad, epilogue=ep, pad_hi=pad_hi)) == want, tag

    with options(*MODES[mode]):
        ns = _lib.conv2d_colstats_split(B, H, W, Cin, Cout, k, k, stride, pad, pad_hi)
        assert ns == (1 if (Cout == 64 and mode != "no_pipe") else 0)
        f = Form(f"conv2d_nhwc[{mode}]", (B, H, W, Cin, Cout, k, stride, pad, pad_hi), M, Cout, rpg, acc, A, E_DIRECT, out,
                 lambda ep: _lib.conv2d_nhwc(xd, wt, out, B, H, W, Cin, Cout, k, k, stride, pad, epilogue=ep, pad_hi=pad_hi),
                 stats_rows=rpg // ns if ns else 0, route=route)
        run_matrix(f)
        if not ns:      # column sums this call cannot produce are refused (general kernel; 80 rows in tiles of 64), never dropped
            cs = torch.zeros(2 * Cout * 2, device=DEV, dtype=torch.float64)
            with pytest.raises(RuntimeError, match="colstats"):
                _lib.conv2d_nhwc(xd, wt, out, B, H, W, Cin, Cout, k, k, stride, pad, epilogue=_lib.make_epilogue(colstats=cs), pad_hi=pad_hi)
            assert _lib.conv2d_route(xd, wt, out, B, H, W, Cin, Cout, k, k, stride, pad, epilogue=_lib.make_epilogue(colstats=cs), pad_hi=pad_hi) is None


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B,H,W,Cout,rpg", [(2, 5, 28, 3, 140), (2, 5, 28, 3, 35), (1, 2, 2, 1, 4)])
def test_conv2d_narrow_head_matrix(B, H, W, Cout, rpg, mode):
    """The 128 -> 3 / 128 -> 1 image heads: the narrow kernel folds the per-group scale per image row (a group never ends inside a row:
    rows_per_group 140, 4) or applies it per element (35); a rowbias or a residual sends the call to the implicit GEMM (N % 4 != 0: its scalar
    tail), which must be right as well; column sums are not offered for these and refused."""
    Cin = 128
    xd, wt, acc, A, _, _ = conv_operands(B, H, W, Cin, Cout)
    M = B * H * W
    out = torch.empty(M, Cout, device=DEV)
    arith = "fp32" if mode == "no_split" else "split"

    def route(ep, combo, stats, tag):
        hb, hrb, act, rk, osc, hrs = combo
        if mode == "no_pipe":
            want = "direct-vec 64x64 fp32 scalar"
        elif hrb or rk != "off":
            want = f"pipe 64x64 {arith} scalar"
        else:
            want = f"narrow c{Cout} fp32 " + ("none" if not hrs else "row" if rpg % W == 0 else "elem")
        assert note_route(_lib.conv2d_route(xd, wt, out, B, H, W, Cin, Cout, 3, 3, 1, 1, epilogue=ep)) == want, tag

    with options(*MODES[mode]):
        assert _lib.conv2d_colstats_split(B, H, W, Cin, Cout, 3, 3, 1, 1) == 0
        f = Form(f"conv2d_nhwc narrow head[{mode}]", (B, H, W, Cin, Cout, f"rows_per_group={rpg}"), M, Cout, rpg, acc, A, E_DIRECT, out,
                 lambda ep: _lib.conv2d_nhwc(xd, wt, out, B, H, W, Cin, Cout, 3, 3, 1, 1, epilogue=ep), route=route)
        run_matrix(f)
        cs = torch.zeros(8 * Cout * 2, device=DEV, dtype=torch.float64)
        with pytest.raises(RuntimeError, match="colstats"):
            _lib.conv2d_nhwc(xd, wt, out, B, H, W, Cin, Cout, 3, 3, 1, 1, epilogue=_lib.make_epilogue(colstats=cs))


# ------------------------------------------------------------------------------------------- gemm
def _gemm_case(M, N, K, rpg, want, opts=(), ldc=None, rows_extra=0, col0=0, stats=False, misaligned_bias=False):
    a, w, acc, A = gemm_operands(M, N, K)
    ad, wd = a.to(DEV), w.to(DEV)
    ldc = N if ldc is None else ldc
    full = torch.full((M + rows_extra, ldc), float("nan"), device=DEV)
    out = full[:M, col0:col0 + N]
    n_in = M * N

    def outside_nan():          # on the device: everything but the [M, N] block is still NaN
        return int(torch.isnan(full).sum()) == full.numel() - n_in

    def route(ep, combo, stats_, tag):
        assert note_route(_lib.gemm_route(ad, wd, out, M, N, K, K, K, ldc, epilogue=ep)) == want, tag

    with options(*opts):
        ns = _lib.gemm_colstats_split(M, N, K, K, K, rpg) if M % rpg == 0 else 0
        assert bool(ns) == stats
        f = Form("gemm" + (f"[{','.join(opts)}]" if opts else ""), (M, N, K, f"rows_per_group={rpg}", f"ldc={ldc}"), M, N, rpg, acc, A, E_DIRECT, out,
                 lambda ep: _lib.gemm(ad, wd, out=out, M=M, N=N, K=K, lda=K, ldb=K, ldc=ldc, epilogue=ep),
                 stats_rows=rpg // ns if ns else 0, route=route, outside_nan=outside_nan if (ldc != N or rows_extra) else None)
        return run_matrix(f)


GEMM_CASES = [
    (300, 72, 64, 100, "pipe 64x64 split buf-row", (), False),                       # per-row groups, M and N tails
    (300, 72, 64, 64, "pipe 64x64 split buf-block", (), False),                      # block groups, the last group partial
    (256, 64, 64, 64, "pipe 64x64 split buf-block", (), True),                       # whole tiles: column sums offered
    (256, 64, 64, 64, "pipe 64x64 fp32 buf-block", ("IDIFF_NO_SPLIT",), True),
    (300, 72, 64, 100, "pipe 64x64 split scalar", ("IDIFF_SCALAR_EPILOGUE",), False),
    (256, 64, 64, 64, "pipe 64x64 split scalar", ("IDIFF_SCALAR_EPILOGUE",), True),  # the scalar tail's column sums
    (300, 65, 64, 100, "pipe 64x64 split scalar", (), False),                        # N = 65: no 16-byte runs
    (300, 72, 101, 100, "direct-scalar 64x64 fp32 scalar", (), False),               # K = 101: the general kernel, 4-byte loads
    (300, 72, 64, 100, "direct-vec 64x64 fp32 scalar", ("IDIFF_NO_PIPE",), False),
]
VEC64_CASES = [(70, 64, 64, 32, "pipe 64x64 split vec64", False), (128, 64, 64, 64, "pipe 64x64 split vec64", True)]


@pytest.mark.parametrize("M,N,K,rpg,want,opts,stats", GEMM_CASES)
def test_gemm_matrix(M, N, K, rpg, want, opts, stats):
    _gemm_case(M, N, K, rpg, want, opts=opts, stats=stats)


def test_gemm_matrix_column_block_of_a_nan_buffer():
    """C is the column block [24, 24 + 72) of a buffer 140 rows taller and 48 columns wider that must stay NaN outside [M, N]."""
    _gemm_case(300, 72, 64, 100, "pipe 64x64 split buf-row", ldc=72 + 48, rows_extra=140, col0=24)


def test_gemm_matrix_vec64_tail():
    """igemm_pipe_kernel's 64-bit-address tail (vec_ep && !buf_ep) without gigabytes: C is a column block with ldc = 2^20 and M = 70, so the
    64 rows of a tile span 2^28 bytes >= 0x0FFFFFF0 -- a 294 MB NaN-filled buffer that must stay NaN outside the block (counted on the
    device), with residual and group terms; then M = 128, rows_per_group 64, where column sums are offered."""
    for M, N, K, rpg, want, stats in VEC64_CASES:
        _gemm_case(M, N, K, rpg, want, ldc=1 << 20, col0=64, stats=stats)
        torch.cuda.empty_cache()


def test_gemm_matrix_misaligned_bias_takes_the_scalar_tail():
    """A bias that is a view one float into its buffer: the route reports the scalar tail, and the terms are right through it."""
    M, N, K, rpg = 300, 72, 64, 100
    a, w, acc, A = gemm_operands(M, N, K)
    ad, wd = a.to(DEV), w.to(DEV)
    out = torch.empty(M, N, device=DEV)
    g = torch.Generator().manual_seed(3)
    buf = torch.randn(N + 1, generator=g)
    bufd = buf.to(DEV)
    bias = bufd[1:]
    assert bias.data_ptr() % 16 == 4
    rowbias, rsc, res = torch.randn(3, N, generator=g), -(torch.rand(3, generator=g) + 0.5), torch.randn(M, N, generator=g)
    failures = []
    for act, hres in itertools.product(ACTS, (False, True)):
        ep = _lib.make_epilogue(bias=bias, rowbias=rowbias.to(DEV), rows_per_group=rpg, act=act, residual=res.to(DEV) if hres else None,
                                out_scale=OUT_SCALE, rowscale=rsc.to(DEV))
        assert note_route(_lib.gemm_route(ad, wd, out, M, N, K, K, K, N, epilogue=ep)) == "pipe 64x64 split scalar"
        out.fill_(float("nan"))
        _lib.gemm(ad, wd, out=out, epilogue=ep)
        ref, tol = epilogue_ref(acc, A, dict(bias=buf[1:].double(), rowbias=rowbias.double(), rows_per_group=rpg, act=act,
                                             residual=res.double() if hres else None, out_scale=OUT_SCALE, rowscale=rsc.double()), E_DIRECT)
        ratio = (out.cpu().double() - ref).abs() / tol
        if not bool((ratio <= 1).all()):
            failures.append((act, hres, float(ratio.nan_to_num(float("inf")).max())))
    assert not failures, failures


def test_gemm_matrix_batched_shared_epilogue():
    """Batched x 3 with the epilogue pointers shared by the batch entries (include/idiff_hip.h): every entry gets the same bias, rowbias, residual
    and scales, each its own contraction."""
    B, M, N, K, rpg = 3, 300, 72, 64, 100
    ops = [gemm_operands(M, N, K, seed=s) for s in range(B)]
    ad = torch.stack([o[0] for o in ops]).to(DEV)
    wd = torch.stack([o[1] for o in ops]).to(DEV)
    out = torch.empty(B, M, N, device=DEV)
    failures, worst, count = [], 0.0, 0
    g = torch.Generator().manual_seed(17)
    bias, rowbias, res = torch.randn(N, generator=g), torch.randn(3, N, generator=g), torch.randn(M, N, generator=g)
    wide, rsc = torch.randn(M, N + SLICE_PAD, generator=g), -(torch.rand(3, generator=g) + 0.5)
    d = dict(bias=bias.to(DEV), rowbias=rowbias.to(DEV), res=res.to(DEV), wide=wide.to(DEV), rsc=rsc.to(DEV))
    for hb, hrb, act, rk, osc, hrs in combos():
        kw = dict(rows_per_group=rpg, act=act, out_scale=osc)
        if hb:
            kw["bias"] = d["bias"]
        if hrb:
            kw["rowbias"] = d["rowbias"]
        if rk == "dense":
            kw["residual"] = d["res"]
        elif rk == "slice":
            kw["residual"], kw["ld_residual"] = d["wide"][:, 16:16 + N], N + SLICE_PAD
        if hrs:
            kw["rowscale"] = d["rsc"]
        ep = _lib.make_epilogue(**kw)
        geom = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, batch=B, stride_a=M * K, stride_b=N * K, stride_c=M * N)
        assert note_route(_lib.gemm_route(ad, wd, out, epilogue=ep, **geom)) == "pipe 64x64 split buf-row"
        out.fill_(float("nan"))
        _lib.gemm(ad, wd, out=out, epilogue=ep, **geom)
        got = out.cpu().double()
        terms = dict(bias=bias.double() if hb else None, rowbias=rowbias.double() if hrb else None, rows_per_group=rpg, act=act,
                     residual={"off": None, "dense": res.double(), "slice": wide[:, 16:16 + N].double()}[rk], out_scale=osc,
                     rowscale=rsc.double() if hrs else None)
        for b in range(B):
            ref, tol = epilogue_ref(ops[b][2], ops[b][3], terms, E_DIRECT)
            ratio = ((got[b] - ref).abs() / tol).nan_to_num(float("inf"))
            count += 1
            r = float(ratio.max())
            if r > 1:
                w_ = int(ratio.argmax())
                failures.append(f"gemm batched entry {b} bias={int(hb)} rowbias={int(hrb)} act={act} residual={rk} out_scale={osc} rowscale={int(hrs)}: "
                                f"element (m={w_ // N}, n={w_ % N}) err / tol = {r:.3g}")
            else:
                worst = max(worst, r)
    print(f"\nMATRIX gemm batched x3 {(M, N, K)}: {count} comparisons, max err / tol = {worst:.3f}")
    assert not failures, "\n".join(failures[:40])


def test_gemm_2src_matrix():
    M, N, K1, K2, rpg = 300, 72, 32, 32, 100
    a, w, acc, A = gemm_operands(M, N, K1 + K2)
    both = a.to(DEV)
    a1, a2, wd = both[:, :K1], both[:, K1:], w.to(DEV)          # two column blocks of one matrix: equal row pitch
    out = torch.empty(M, N, device=DEV)

    def route(ep, combo, stats, tag):   # the two-source call takes the route of the one-source call with A = A1
        assert note_route(_lib.gemm_route(a1, wd, out, M, N, K1 + K2, K1 + K2, K1 + K2, N, epilogue=ep)) == "pipe 64x64 split buf-row", tag

    def launch(ep):
        _lib._check(_lib.lib().idiff_gemm_2src_f32(a1.data_ptr(), a2.data_ptr(), K1 + K2, K1, wd.data_ptr(), K1 + K2, out.data_ptr(), N, M, N,
                                                   K1 + K2, _lib._ep_ref(ep, "gemm_2src"), _lib._stream()), "idiff_gemm_2src_f32")

    run_matrix(Form("gemm_2src", (M, f"{K1}+{K2}", N), M, N, rpg, acc, A, E_DIRECT, out, launch, route=route))


@pytest.mark.parametrize("form", ["pairs", "pairs_weight_is_a_batched", "pairs_2src"])
def test_gemm_pairs_matrix(form):
    """The fp16-pair contraction (one 128 x 128 tile shape), served at a small size under IDIFF_PAIRS_MIN_TILES = 1: (300, 128, 64), per-row
    groups.  Gaussian activations of order one and N(0, 1 / K) weights."""
    M, N, K, rpg = 300, 128, 64, 100
    with _lib.thread_option("IDIFF_PAIRS_MIN_TILES", 1):
        assert _lib.gemm_pairs_ok(M, N, K)
        if form == "pairs_weight_is_a_batched":
            # out[b] = W [M, K] x X[b] [N, K]^T: the weight on the left, broadcast; one activation per batch entry; shared epilogue
            B = 2
            g = torch.Generator().manual_seed(5)
            wl = torch.randn(M, K, generator=g) / K ** 0.5
            xs = torch.randn(B, N, K, generator=g)
            wd, xd = wl.to(DEV), xs.to(DEV)
            sc = _lib.gemm_pairs_scale(wd)
            out = torch.empty(B, M, N, device=DEV)
            geom = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, batch=B, stride_a=0, stride_b=N * K, stride_c=M * N)
            for b in range(B):
                acc, A = wl.double() @ xs[b].double().T, wl.double().abs() @ xs[b].double().abs().T
                view = out[b]

                def route(ep, combo, stats, tag):
                    assert note_route(_lib.gemm_route(wd, xd, out, epilogue=ep, pairs=True, **geom)) == "pipe 128x128 pairs buf-row", tag

                run_matrix(Form(f"gemm_pairs weight_is_a batch entry {b} of {B}", (M, N, K), M, N, rpg, acc, A, E_DIRECT, view,
                                lambda ep: _lib.gemm_pairs(wd, xd, sc, out, epilogue=ep, weight_is_a=True, **geom), route=route),
                           only=(lambda combo, stats: True) if b == 0 else (lambda combo, stats: combo[2] in ("none", "silu")))
            return
        a, w, acc, A = gemm_operands(M, N, K)
        ad, wd = a.to(DEV), w.to(DEV)
        sc = _lib.gemm_pairs_scale(wd)
        out = torch.empty(M, N, device=DEV)

        def route(ep, combo, stats, tag):
            assert note_route(_lib.gemm_route(ad, wd, out, M, N, K, K, K, N, epilogue=ep, pairs=True)) == "pipe 128x128 pairs buf-row", tag

        if form == "pairs":
            launch = lambda ep: _lib.gemm_pairs(ad, wd, sc, out, epilogue=ep)
        else:
            one = torch.tensor([1.0, 1.0, 0, 0, 0, 0, 0, 0], device=DEV)          # act_scale {s, 1 / s} = 1: the activations are of order one
            a1, a2 = ad[:, :32], ad[:, 32:]

            def launch(ep):
                _lib._check(_lib.lib().idiff_gemm_pairs_2src_f32(a1.data_ptr(), a2.data_ptr(), K, 32, one.data_ptr(), wd.data_ptr(), K, sc.data_ptr(),
                                                                 out.data_ptr(), N, M, N, K, _lib._ep_ref(ep, "gemm_pairs_2src"), _lib._stream()),
                            "idiff_gemm_pairs_2src_f32")
        run_matrix(Form("gemm_" + form, (M, N, K), M, N, rpg, acc, A, E_DIRECT, out, launch, route=route))


# ------------------------------------------------------------------------------------------- refusals
def test_terms_a_launcher_does_not_take_are_refused():
    """Nothing is dropped silently: a per-row-group term with rows_per_group != H * W on the per-image kernels, column sums where the split is
    0, a bias / rowbias the Winograd tails cannot read 16 bytes at a time (refusal only: nothing misaligned is launched)."""
    B, H, W, Cin, Cout = 2, 8, 8, 32, 64
    x = torch.zeros(B, H, W, Cin, device=DEV)
    out = torch.zeros(B, H, W, Cout, device=DEV)
    wt = torch.randn(Cout, 3, 3, Cin, device=DEV)
    rowb, rsc = torch.zeros(B * H, Cout, device=DEV), torch.ones(B * H, device=DEV)
    pad = torch.zeros(Cout + 4, device=DEV)
    forms = [("conv2d_wino1d", _lib.wino1d_pack(wt, Cin, Cout), lambda u, ep: _lib.conv2d_wino1d(x, u, out, B, H, W, Cin, Cout, epilogue=ep), True),
             ("conv2d_winograd43", _lib.winograd43_pack(wt, Cin, Cout), lambda u, ep: _lib.conv2d_winograd43(x, u, out, B, H, W, Cin, Cout, epilogue=ep), True),
             ("conv2d_winograd43h", _lib.winograd43_pack(wt, Cin, Cout, pairs=True),
              lambda u, ep: _lib.conv2d_winograd43(x, u, out, B, H, W, Cin, Cout, epilogue=ep, pairs=True), True),
             ("conv2d_winograd", _lib.winograd_pack(wt, Cin, Cout), lambda u, ep: _lib.conv2d_winograd(x, u, out, B, H, W, Cin, Cout, epilogue=ep), False)]
    for name, u, call, per_image_only in forms:
        if per_image_only:
            with pytest.raises(RuntimeError, match="per image"):
                call(u, _lib.make_epilogue(rowbias=rowb, rows_per_group=W))
            with pytest.raises(RuntimeError, match="per image"):
                call(u, _lib.make_epilogue(rowscale=rsc, rows_per_group=W))
        with pytest.raises(RuntimeError, match="bias must be 16-byte aligned"):
            call(u, _lib.make_epilogue(bias=pad[1:]))
        with pytest.raises(RuntimeError, match="rowbias must be 16-byte aligned"):
            call(u, _lib.make_epilogue(rowbias=rowb.reshape(-1)[2:], ld_rowbias=Cout, rows_per_group=H * W))
        with pytest.raises(RuntimeError, match="rowbias must be 16-byte aligned"):
            call(u, _lib.make_epilogue(rowbias=rowb, ld_rowbias=Cout + 2, rows_per_group=H * W))
        if per_image_only:                                         # (the F(2x2) launcher refuses by geometry: test_winograd_matrix)
            with _lib.thread_option("IDIFF_NO_COLSTATS", 1):       # the splits answer 0
                with pytest.raises(RuntimeError, match="colstats"):
                    call(u, _lib.make_epilogue(colstats=torch.zeros(B * Cout * 2, device=DEV, dtype=torch.float64)))
    # F(4x4): 3 x 3 = 9 tiles of 4 x 4 per image divide no workgroup of 32
    x12, out12 = torch.zeros(B, 12, 12, Cin, device=DEV), torch.zeros(B, 12, 12, Cout, device=DEV)
    assert _lib.conv2d_winograd43_ok(B, 12, 12, Cin, Cout) and _lib.conv2d_winograd43_colstats_split(B, 12, 12, Cin, Cout) == 0
    for pairs in (False, True):
        with pytest.raises(RuntimeError, match="colstats"):
            _lib.conv2d_winograd43(x12, _lib.winograd43_pack(wt, Cin, Cout, pairs=pairs), out12, B, 12, 12, Cin, Cout, pairs=pairs,
                                   epilogue=_lib.make_epilogue(colstats=torch.zeros(B * Cout * 2, device=DEV, dtype=torch.float64)))
    # gemm: 300 rows in tiles of 64 are no whole tiles; the general kernel (K = 101) has no column sums
    a, w, c = torch.zeros(300, 64, device=DEV), torch.zeros(72, 64, device=DEV), torch.zeros(300, 72, device=DEV)
    cs = torch.zeros(5 * 72 * 2, device=DEV, dtype=torch.float64)
    assert _lib.gemm_colstats_split(300, 72, 64, 64, 64, 100) == 0
    with pytest.raises(RuntimeError, match="colstats"):
        _lib.gemm(a, w, out=c, epilogue=_lib.make_epilogue(colstats=cs, rows_per_group=100))
    assert _lib.gemm_route(a, w, c, 300, 72, 64, 64, 64, 72, epilogue=_lib.make_epilogue(colstats=cs, rows_per_group=100)) is None
    with pytest.raises(RuntimeError, match="colstats"):
        _lib.gemm(torch.zeros(256, 101, device=DEV), torch.zeros(64, 101, device=DEV), out=torch.zeros(256, 64, device=DEV),
                  epilogue=_lib.make_epilogue(colstats=cs, rows_per_group=64))


# ------------------------------------------------------------------------------------------- every tile the chooser picks at small sizes
TILE_CASES = [
    (4096, 64, 32, (), "pipe 128x64 split buf-block"),
    (4096, 32, 32, (), "pipe 128x32 split buf-block"),
    (4096, 64, 32, ("IDIFF_NO_SPLIT",), "pipe 128x64 fp32 buf-block"),
    (4096, 32, 32, ("IDIFF_NO_SPLIT",), "pipe 128x32 fp32 buf-block"),
    (4096, 72, 32, ("IDIFF_NO_PIPE",), "direct-vec 128x64 fp32 scalar"),
    (16384, 256, 32, (), "pipe 128x128 split buf-block"),
    (16384, 256, 32, ("IDIFF_NO_SPLIT",), "pipe 128x128 fp32 buf-block"),
]


@pytest.mark.parametrize("M,N,K,opts,want", TILE_CASES)
def test_gemm_tiles_of_128_rows(M, N, K, opts, want):
    """The 128-row tiles the chooser picks from M = 4096, and 128 x 128 from 256 workgroups (M = 16384, N = 256; the single-buffer fp32 form
    starts at 1024 workgroups and stays with the large-shape tests): groups of 128 rows, column sums per 128-row tile.  A part of the
    product keeps these larger cases within seconds: act {none, silu} at M = 4096, and at M = 16384 the production tail (none, residual,
    scaled) and the all-terms one."""
    a, w, acc, A = gemm_operands(M, N, K)
    ad, wd = a.to(DEV), w.to(DEV)
    out = torch.empty(M, N, device=DEV)
    rpg = 128

    def route(ep, combo, stats, tag):
        assert note_route(_lib.gemm_route(ad, wd, out, M, N, K, K, K, N, epilogue=ep)) == want, tag

    with options(*opts):
        ns = _lib.gemm_colstats_split(M, N, K, K, K, rpg)
        assert ns == (0 if "IDIFF_NO_PIPE" in opts else 1)
        f = Form(f"gemm[{','.join(opts)}]", (M, N, K), M, N, rpg, acc, A, E_DIRECT, out, lambda ep: _lib.gemm(ad, wd, out=out, epilogue=ep),
                 stats_rows=rpg if ns else 0, route=route)
        if M == 4096:
            run_matrix(f, only=lambda c, stats: c[2] in ("none", "silu"))
        else:
            run_matrix(f, only=lambda c, stats: c in ((True, False, "none", "dense", OUT_SCALE, False), (True, True, "silu", "slice", OUT_SCALE, True)))


def test_every_epilogue_form_of_the_pipelined_kernel_has_cases():
    """The tails the cases of this module are routed to (each launch asserts its route): all four forms of igemm_pipe_kernel."""
    wants = [c[4] for c in GEMM_CASES] + [c[4] for c in VEC64_CASES] + [c[4] for c in TILE_CASES]
    wants += [f"pipe 64x64 split {c[10]}" for c in CONV_SHAPES if c[10]]
    forms = {w.split()[3] for w in wants if w.startswith("pipe ")}
    assert forms == {"buf-block", "buf-row", "vec64", "scalar"}
