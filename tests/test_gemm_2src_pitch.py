"""The two-source contraction with a row pitch per source (idiff_gemm_2src_ld_f32, _lib.gemm_2src): [A1 | A2] @ W^T for sources of different
widths -- the shortcut of a residual block on cat[h, skip] with 256 + 128 channels, which used to take two contractions with the partial
product written and read back.  Against fp64 at the bar of tests/test_hip_ops.py::test_gemm_two_sources, bit-equal to idiff_gemm_2src_f32
where the pitches are equal, the host cut with both sources shifted, the refusals, and the executor step with and without its switch."""
import ctypes

import pytest
import torch

import id_diff_amd
import normload_cases
from helpers import fill_from_seed, ncsnpp_config, rel_err
from id_diff_amd import _lib, sde_lib
from id_diff_amd.models import utils as mutils
from oracle import models as omodels, sde as osde

gpu = pytest.mark.gpu
DEV = "cuda"
GEMM_RTOL = 2e-6                     # tests/test_hip_ops.py::test_gemm_two_sources: rel_err(out, fp64) < 2e-6
NET_RTOL = 2e-5                      # tests/test_hip_models.py
# (K1, K2): the flagship's 256 + 128, the wide source second, and the narrowest second source a 16-byte load allows (one k-tile of which
# only the first float4 column is inside K); M = 300: a partial row tile at every tile height, M = 385 = 3 * 128 + 1: a tile of one row
WIDTHS = [(256, 128), (128, 256), (32, 4)]
_cache = {}


def _operands(M, K1, K2, N):
    """CPU, once per shape: sources of mean +1.5 and -1.5 (a read at the other source's pitch or from the other source is an error of order
    1), the weight, bias, residual, and the fp64 product of the concatenation."""
    key = (M, K1, K2, N)
    if key not in _cache:
        g = torch.Generator().manual_seed(M + 7 * K1 + 3 * K2 + N)
        a1 = torch.randn(M, K1, generator=g) + 1.5
        a2 = torch.randn(M, K2, generator=g) - 1.5
        w = torch.randn(N, K1 + K2, generator=g) / (K1 + K2) ** 0.5
        b, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        acc = torch.cat([a1, a2], 1).double() @ w.double().T
        _cache[key] = (a1, a2, w, b, res, acc)
    return _cache[key]


def test_query_switch_and_refusals_on_the_host():
    """No GPU: the routing query, its switch, and the refusals of the new entry point, all before any device call."""
    q = _lib.gemm_2src_ld_ok
    assert q(256, 128) and q(128, 256) and q(32, 4)
    assert not q(48, 16) and not q(32, 6) and not q(0, 32) and not q(32, 0)
    for switch in ("IDIFF_NO_2SRC_PITCH", "IDIFF_NO_PIPE"):
        with _lib.thread_option(switch, 1):
            assert not q(256, 128), switch
    assert q(256, 128)
    lib, fake = _lib.lib(), 0x10000
    call = lambda a2=fake, lda1=64, lda2=32, K1=64, K=96, M=256: lib.idiff_gemm_2src_ld_f32(fake, lda1, a2, lda2, K1, fake, K, fake, 64, M, 64, K,
                                                                                            None, None)
    for kw, text in ((dict(lda2=28), b"leading dimension smaller than the row length"), (dict(lda1=60), b"leading dimension smaller"),
                     (dict(K1=48), b"must be a multiple of 32"), (dict(K1=96), b"bad sizes"), (dict(a2=None), b"null pointer"),
                     (dict(lda2=34), b"16-byte aligned"), (dict(a2=fake + 4), b"16-byte aligned")):
        assert call(**kw) != 0 and text in lib.idiff_last_error(), (kw, lib.idiff_last_error())
    assert call(M=0) == 0


@gpu
@pytest.mark.parametrize("N", [128, 192])
@pytest.mark.parametrize("K1,K2", WIDTHS)
@pytest.mark.parametrize("M", [300, 385])
def test_gemm_2src_pitch_vs_fp64(M, K1, K2, N):
    """Bias alone, and bias + residual + out_scale, into a NaN-filled output (every element must be written)."""
    a1, a2, w, b, res, acc = _operands(M, K1, K2, N)
    a1d, a2d, wd, bd, resd = (t.to(DEV) for t in (a1, a2, w, b, res))
    for ep, ref in ((dict(bias=bd), acc + b.double()),
                    (dict(bias=bd, residual=resd, out_scale=0.5 ** 0.5), (acc + b.double() + res.double()) * 0.5 ** 0.5)):
        out = torch.full((M, N), float("nan"), device=DEV)
        _lib.gemm_2src(a1d, a2d, wd, out, epilogue=_lib.make_epilogue(**ep))
        err = rel_err(out.cpu(), ref)
        print(f"gemm_2src pitch M={M} {K1}+{K2} N={N} {sorted(ep)}: rel err {err:.3e}")
        assert bool(torch.isfinite(out).all())
        assert err < GEMM_RTOL


@gpu
@pytest.mark.parametrize("N", [128, 192])
@pytest.mark.parametrize("K1,K2", WIDTHS)
def test_gemm_2src_pitch_colstats(K1, K2, N):
    """Bias + residual + the fp64 column sums per row tile.  The sums are per WHOLE row tile (idiff_gemm_colstats_split), so this case takes
    M = 512; with M = 300 the request is refused in the words of the one-source call.  Sums against those of the output itself at
    rows * 2^-52 * sum |v| (tests/test_hip_epilogue_matrix.py)."""
    M = 512
    a1, a2, w, b, res, acc = _operands(M, K1, K2, N)
    a1d, a2d, wd, bd, resd = (t.to(DEV) for t in (a1, a2, w, b, res))
    ns = _lib.gemm_colstats_split(M, N, K1 + K2, K1, K1 + K2, M)
    assert ns > 0
    cs = torch.full((ns, N, 2), float("nan"), device=DEV, dtype=torch.float64)
    out = torch.full((M, N), float("nan"), device=DEV)
    _lib.gemm_2src(a1d, a2d, wd, out, epilogue=_lib.make_epilogue(bias=bd, residual=resd, colstats=cs, rows_per_group=M))
    got = out.cpu().double()
    assert rel_err(got, acc + b.double() + res.double()) < GEMM_RTOL
    v, c = got.reshape(ns, M // ns, N), cs.cpu()
    for sums, vals in ((c[..., 0], v), (c[..., 1], v * v)):
        assert bool(((sums - vals.sum(1)).abs() <= (M // ns) * 2.0 ** -52 * vals.abs().sum(1)).all())
    with pytest.raises(RuntimeError, match="colstats with M = 300"):
        _lib.gemm_2src(a1d[:300], a2d[:300], wd, out[:300], epilogue=_lib.make_epilogue(colstats=cs, rows_per_group=300))


@gpu
@pytest.mark.parametrize("M,K1,K2,N", [(1000, 128, 128, 128), (4100, 256, 256, 64), (77, 32, 32, 200)])
def test_equal_pitches_are_bit_identical_to_the_one_pitch_entry_point(M, K1, K2, N):
    """The shapes of tests/test_hip_ops.py::test_gemm_two_sources: gemm_2src (the new entry point) against idiff_gemm_2src_f32 via ctypes."""
    a1, a2, w, b, res, _ = _operands(M, K1, K2, N)
    a1d, a2d, wd, bd, resd = (t.to(DEV) for t in (a1, a2, w, b, res))
    new, old = torch.full((M, N), float("nan"), device=DEV), torch.full((M, N), float("nan"), device=DEV)
    ep = _lib.make_epilogue(bias=bd, residual=resd)
    _lib.gemm_2src(a1d, a2d, wd, new, epilogue=ep)
    _lib._check(_lib.lib().idiff_gemm_2src_f32(a1d.data_ptr(), a2d.data_ptr(), K1, K1, wd.data_ptr(), K1 + K2, old.data_ptr(), N, M, N, K1 + K2,
                                               ctypes.byref(ep), _lib._stream()), "idiff_gemm_2src_f32")
    assert bool(torch.isfinite(new).all()) and torch.equal(new, old)


@gpu
def test_gemm_2src_pitch_beyond_4gib():
    """The first source past one buffer descriptor (4.4 GB at 256 columns), the second inside one (2.2 GB at 128): the rows are cut on the
    host and BOTH sources shift, each by its own pitch.  The allocation pattern of test_gemm_two_sources_beyond_4gib."""
    g = torch.Generator(device=DEV).manual_seed(2)
    M, K1, K2, N, grp = 4_300_000, 256, 128, 64, 1000
    a1 = torch.randn(M, K1, device=DEV, generator=g)
    a2 = torch.randn(M, K2, device=DEV, generator=g)
    w = torch.randn(N, K1 + K2, device=DEV, generator=g) / 20
    rb = torch.randn(M // grp, N, device=DEV, generator=g)
    out = torch.empty(M, N, device=DEV)
    _lib.gemm_2src(a1, a2, w, out, epilogue=_lib.make_epilogue(rowbias=rb, rows_per_group=grp))
    rows = torch.tensor([0, 1, M // 2 - 1, M // 2, M // 2 + 1, 3_000_000, M - 1], device=DEV)
    ref = torch.cat([a1[rows], a2[rows]], 1).double().cpu() @ w.double().cpu().T + rb[rows // grp].double().cpu()
    assert rel_err(out[rows].cpu(), ref) < GEMM_RTOL
    del a1, a2, out
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- executor
@gpu
def test_small_ncsnpp_with_and_without_both_shortcut_forms(monkeypatch):
    """nf = 64, levels of 64, 128 and 128 channels at 32, 16 and 8 pixels, one residual block per level, B = 2, the launch thresholds of
    the row-wise convolution lowered to test-sized batches.  The up path has blocks on cat[h, skip] of 128 + 64 channels -- each one
    gemm_2src with the form and two gemm calls under IDIFF_NO_2SRC_PITCH -- and up blocks whose shortcut Conv_1's tail upsamples (the
    8 -> 16 block: rows of 16 pixels, no norm pending for the loader) -- each one FIR launch fewer than under IDIFF_NO_FUSED_RES_UP, the
    convolutions' count unchanged.  Nothing else changes, and every combination is at NET_RTOL from the CPU oracle and from the others."""
    normload_cases.small_batches(monkeypatch)
    cfg = ncsnpp_config(**{"model.nf": 64, "model.ch_mult": (1, 2, 2), "model.num_res_blocks": 1, "model.init_scale": 1.0})
    torch.manual_seed(0)
    ref_model = omodels.create_model(cfg)
    fill_from_seed(ref_model, 5)
    model = mutils.create_model(cfg)
    model.load_state_dict(ref_model.state_dict())
    model.to(DEV)
    g = torch.Generator().manual_seed(3)
    x, t = torch.rand(2, 3, 32, 32, generator=g), torch.tensor([0.4, 0.05])
    with torch.no_grad():
        ref = osde.get_score_fn(osde.VESDE(0.01, 50, 1000), ref_model)(x, t)
    score = mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)
    calls, unequal = {"gemm": 0, "gemm_2src": 0, "upfirdn2d_raw": 0, "upfirdn2d_gn": 0, "conv2d_wino1d": 0, "resup": 0}, []
    for name in calls:
        if name == "resup":
            continue

        def wrapper(*a, _name=name, _orig=getattr(_lib, name), **k):
            calls[_name] += 1
            if _name == "conv2d_wino1d" and getattr(k.get("epilogue"), "residual_up2", None) is not None:
                calls["resup"] += 1
            return _orig(*a, **k)
        monkeypatch.setattr(_lib, name, wrapper)
    orig_block = model._resblock

    def block(idx, x, temb_all, pk, x2=None):
        mod = model.all_modules[idx]
        if x2 is not None and x.C != x2.C and (hasattr(mod, "Conv_2") or hasattr(mod, "NIN_0")):
            unequal.append((x.C, x2.C))
        return orig_block(idx, x, temb_all, pk, x2=x2)
    monkeypatch.setattr(model, "_resblock", block)
    xd, td = x.to(DEV), t.to(DEV)

    def run(*switches):
        c0 = dict(calls)
        if not switches:
            out = score(xd, td)
        elif len(switches) == 1:
            with _lib.thread_option(switches[0], 1):
                out = score(xd, td)
        else:
            with _lib.thread_option(switches[0], 1), _lib.thread_option(switches[1], 1):
                out = score(xd, td)
        return out, {k: calls[k] - c0[k] for k in calls}
    on, c_on = run()
    n = len(unequal)
    no_pitch, c_np = run("IDIFF_NO_2SRC_PITCH")
    no_up, c_nu = run("IDIFF_NO_FUSED_RES_UP")
    off, c_off = run("IDIFF_NO_2SRC_PITCH", "IDIFF_NO_FUSED_RES_UP")
    print(f"shortcut forms: blocks on cat of unequal widths {unequal[:n]}; launches on {c_on} | no 2src pitch {c_np} | no res up {c_nu} | "
          f"neither {c_off}")
    assert n >= 1 and all(c1 % 32 == 0 and c2 % 4 == 0 for c1, c2 in unequal)
    n_up = c_on["resup"]
    assert n_up >= 1 and c_np["resup"] == n_up and c_nu["resup"] == 0 and c_off["resup"] == 0
    for with_form, without in ((c_on, c_np), (c_nu, c_off)):                # the two-pitch GEMM: one launch for two, whatever the other switch
        assert with_form["gemm_2src"] - without["gemm_2src"] == n, (with_form, without)
        assert without["gemm"] - with_form["gemm"] == 2 * n, (with_form, without)
        assert all(with_form[k] == without[k] for k in ("upfirdn2d_raw", "upfirdn2d_gn", "conv2d_wino1d", "resup"))
    for with_form, without in ((c_on, c_nu), (c_np, c_off)):                # the tail's FIR: one resampler launch fewer per up block
        assert without["upfirdn2d_raw"] - with_form["upfirdn2d_raw"] == n_up, (with_form, without)
        assert all(with_form[k] == without[k] for k in ("gemm", "gemm_2src", "upfirdn2d_gn", "conv2d_wino1d"))
    assert bool(torch.isfinite(on).all())
    errs = {name: rel_err(o.cpu(), ref) for name, o in (("on", on), ("no 2src pitch", no_pitch), ("no res up", no_up), ("neither", off))}
    e_both = rel_err(on.cpu(), off.cpu())
    print(f"shortcut forms model-level rel err vs oracle: {errs}; on vs neither {e_both:.2e}")
    assert all(e < NET_RTOL for e in errs.values()) and e_both < NET_RTOL
