"""GPU parity of the streaming multi-head attention kernel (idiff_attention_heads_f32) and of the multi-head BeatGANs U-Nets that
run on it (python -m pytest -m gpu).  The kernel's bar is the single-head kernel's own (tests/test_hip_ops.py::test_attention256_vs_fp64):
its error against fp64 beside the per-head three-launch form's on the same operands."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import (beatgans_config, fill_from_seed, overrides_from_golden, rel_err, state_dict_from_golden, weight_abs_sums)
from id_diff_amd import _lib, sde_lib
from id_diff_amd.models import utils as mutils
from oracle import models as omodels, sde as osde

pytestmark = pytest.mark.gpu
DEV = "cuda"
NET_RTOL = 2e-5                                  # tests/test_hip_models.py


def make_operands(B, T, H, D, qk_gain, seed):
    """q | k and V^T as the executors produce them: projections of a GroupNorm's output, the scales from the projections' row norms."""
    C = H * D
    g = torch.Generator().manual_seed(seed)
    n = F.group_norm(torch.randn(B, C, T, generator=g) * 3 + 1, 32, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2)
    n = n.permute(0, 2, 1).contiguous()                                                   # [B, T, C]
    wqk = torch.randn(2 * C, C, generator=g) * (qk_gain / C ** 0.5)
    bqk = torch.randn(2 * C, generator=g) * 0.1
    wv, bv = torch.randn(C, C, generator=g) * (0.7 / C ** 0.5), torch.randn(C, generator=g) * 0.1
    qk = (n.reshape(-1, C) @ wqk.T + bqk).contiguous()
    vt = torch.einsum("oc,bpc->bop", wv, n).contiguous()                                  # [B, C, T], bias deferred
    gam = float(torch.sqrt((n.double() ** 2).mean()))
    s_qk, s_v = _lib.pairs_scale_from_rows(wqk.to(DEV), bqk.to(DEV), gam), _lib.pairs_scale_from_rows(wv.to(DEV), bv.to(DEV), gam)
    return qk, vt, bv, s_qk, s_v


def reference_f64(qk, vt, bv, B, T, H, D):
    C = H * D
    q = qk[:, :C].double().reshape(B, T, H, D)
    k = qk[:, C:].double().reshape(B, T, H, D)
    logits = torch.einsum("bihc,bjhc->bhij", q, k) * D ** -0.5
    v = vt.double().reshape(B, H, D, T)
    ref = torch.einsum("bhij,bhcj->bihc", torch.softmax(logits, dim=-1), v).reshape(B, T, C)
    return (ref + bv.double() if bv is not None else ref), logits


def three_launches_per_head(qkd, vtd, bvd, B, T, H, D):
    """The form the executor falls back to, on the library's gemm / softmax_rows: not code under test."""
    C = H * D
    lg = torch.empty(B, T, T, device=DEV)
    out = torch.empty(B, T, C, device=DEV)
    for h in range(H):
        _lib.gemm(qkd[:, h * D:], qkd[:, C + h * D:], out=lg, M=T, N=T, K=D, lda=2 * C, ldb=2 * C, ldc=T, batch=B,
                  stride_a=T * 2 * C, stride_b=T * 2 * C, stride_c=T * T)
        _lib.softmax_rows(lg, lg, B * T, T, D ** -0.5)
        _lib.gemm(lg, vtd[:, h * D:(h + 1) * D], out=out[..., h * D:], M=T, N=D, K=T, lda=T, ldb=T, ldc=C, batch=B,
                  stride_a=T * T, stride_b=C * T, stride_c=T * C,
                  epilogue=_lib.make_epilogue(bias=bvd[h * D:(h + 1) * D]) if bvd is not None else None)
    return out


def check_against_fp64(qk, vt, bv, s_qk, s_v, B, T, H, D, what):
    C = H * D
    ref, logits = reference_f64(qk, vt, bv, B, T, H, D)
    qkd, vtd, bvd = qk.to(DEV), vt.to(DEV), bv.to(DEV)
    big = torch.full((B * T + 8, C), float("nan"), device=DEV)          # over-allocated: the rows past B T must stay untouched
    out = big[:B * T]
    _lib.attention_heads(qkd, vtd, out, B, T, H, D, s_qk, s_v, D ** -0.5, bias_v=bvd)
    assert bool(torch.isnan(big[B * T:]).all()), "rows past B * tokens were written"
    assert bool(torch.isfinite(out).all())
    three = three_launches_per_head(qkd, vtd, bvd, B, T, H, D)
    got = out.cpu().reshape(B, T, C)
    e_fused, e_three = rel_err(got, ref), rel_err(three.cpu(), ref)
    print(f"attention_heads {what} B={B} T={T} H={H} D={D}: fused {e_fused:.2e}, three launches per head {e_three:.2e}, "
          f"max |logit| {float(logits.abs().max()):.1f}")
    for h in range(H):                                                  # every head in its own columns (a head written elsewhere fails here)
        assert rel_err(got[..., h * D:(h + 1) * D], ref[..., h * D:(h + 1) * D]) < 1e-4, h
    assert e_fused < max(2e-6, 1.2 * e_three) and e_fused < 3 * e_three + 2e-7, (e_fused, e_three)
    big.fill_(float("nan"))
    _lib.attention_heads(qkd, vtd, out, B, T, H, D, s_qk, s_v, D ** -0.5)
    assert rel_err(out.cpu().reshape(B, T, C), ref - bv.double()) < 3e-6
    assert bool(torch.isnan(big[B * T:]).all())


# every T in {64, 192, 256, 1024, 4096}, every D in {32, 64, 128}, every H in {1, 2, 4, 8}; qk_gain 6: peaked rows, 0.05: nearly uniform
CASES = [
    (2, 64, 4, 64, 1.0), (3, 64, 8, 32, 6.0), (2, 64, 2, 128, 1.0), (2, 64, 1, 32, 0.05),
    (2, 192, 2, 64, 1.0), (1, 192, 4, 32, 6.0), (2, 192, 1, 128, 0.05),
    (2, 256, 4, 64, 1.0), (2, 256, 2, 128, 6.0), (2, 256, 8, 32, 1.0), (1, 256, 1, 64, 0.05), (1, 256, 8, 128, 1.0),
    (1, 1024, 2, 64, 1.0), (1, 1024, 4, 32, 6.0), (1, 1024, 1, 128, 1.0), (1, 1024, 8, 64, 0.05),
    (1, 4096, 1, 32, 1.0), (1, 4096, 2, 64, 1.0), (1, 4096, 1, 128, 6.0), (1, 4096, 2, 32, 0.05),
]


@pytest.mark.parametrize("B,T,H,D,qk_gain", CASES)
def test_attention_heads_vs_fp64(B, T, H, D, qk_gain):
    """idiff_attention_heads_f32 against fp64 of the same fp32 q, k, v, beside the three-launch form per head (BeatGANsblocks.py:466-526).
    Operands as test_attention256_vs_fp64 builds them: a head's logits sum D products of order qk_gain^2 and are scaled by D^-1/2, so
    their spread is the single-head test's (gain 6: up to +-60)."""
    assert _lib.attention_heads_ok(B, T, H, D)
    qk, vt, bv, s_qk, s_v = make_operands(B, T, H, D, qk_gain, seed=int(100 * qk_gain) + T + 7 * H + D)
    for sc in (s_qk, s_v):
        a, b_ = sc.cpu().tolist()
        assert a * b_ == 1.0 and np.log2(a) == round(np.log2(a))
    check_against_fp64(qk, vt, bv, s_qk, s_v, B, T, H, D, f"gain={qk_gain}")


@pytest.mark.parametrize("B,T,H,D", [(2, 256, 2, 64), (1, 1024, 2, 32), (1, 192, 1, 128)])
def test_attention_heads_running_maximum_moves_in_the_last_chunk(B, T, H, D):
    """One key of the LAST chunk of 64 leads every query's logits by more than 100: the running maximum moves after all other chunks
    have been accumulated, and what they accumulated is rescaled by exp(-100 or less)."""
    C = H * D
    qk, vt, bv, s_qk, s_v = make_operands(B, T, H, D, 1.0, seed=T + D)
    g = torch.Generator().manual_seed(5)
    lead = T - 3
    qk = qk.reshape(B, T, 2 * C).clone()
    amp = (200.0 * D ** 0.5) ** 0.5                                     # (amp u) . (amp u) D^-1/2 = 200
    for h in range(H):
        u = F.normalize(torch.randn(D, generator=g), dim=0)
        qk[:, :, h * D:(h + 1) * D] += amp * u                          # every query of the head gets the component
        qk[:, lead, C + h * D:C + (h + 1) * D] = amp * u                # and one key is that direction
    qk = qk.reshape(B * T, 2 * C).contiguous()
    _, logits = reference_f64(qk, vt, bv, B, T, H, D)
    top2 = logits.topk(2, dim=-1)
    assert bool((top2.indices[..., 0] == lead).all()) and float((top2.values[..., 0] - top2.values[..., 1]).min()) > 100
    assert float(qk.abs().max()) * float(s_qk[0]) < 65504
    check_against_fp64(qk, vt, bv, s_qk, s_v, B, T, H, D, "peaked in the last chunk")


def test_attention_heads_limits():
    """What the streaming kernel refuses (the executor then runs the three-launch form per head), its switches, the entry point's
    errors, and its documented failure: operands beyond the fp16 range give non-finite outputs, never finite wrong numbers."""
    assert _lib.attention_heads_ok(7, 256, 4, 64) and _lib.attention_heads_ok(7, 64, 8, 128) and _lib.attention_heads_ok(1, 4096, 1, 32)
    assert not _lib.attention_heads_ok(7, 16, 4, 64) and not _lib.attention_heads_ok(7, 96, 4, 64)
    assert not _lib.attention_heads_ok(7, 256, 4, 48) and not _lib.attention_heads_ok(7, 256, 1, 256)
    assert not _lib.attention_heads_ok(7, 8192, 1, 64) and not _lib.attention_heads_ok(7, 256, 16, 128)            # H D > 1024
    assert not _lib.attention_heads_ok(1 << 19, 256, 4, 64) and not _lib.attention_heads_ok(0, 256, 4, 64)         # B H > 2^20
    for name in ("IDIFF_NO_FUSED_ATTN", "IDIFF_NO_PAIRS", "IDIFF_NO_SPLIT"):
        with _lib.thread_option(name, 1):
            assert not _lib.attention_heads_ok(7, 256, 4, 64)
    assert _lib.attention_heads_ok(7, 256, 4, 64)
    B, T, H, D = 2, 256, 2, 64
    C = H * D
    g = torch.Generator().manual_seed(0)
    qk, vt = torch.randn(B * T, 2 * C, generator=g).to(DEV), torch.randn(B, C, T, generator=g).to(DEV)
    one = torch.tensor([1.0, 1.0], device=DEV)
    out = torch.full((B * T, C), float("nan"), device=DEV)
    with pytest.raises(RuntimeError, match="shapes"):
        _lib.attention_heads(qk[:, :C].contiguous(), vt, out, B, T, H, D, one, one, 1 / 8)
    with pytest.raises(RuntimeError, match="shapes"):
        _lib.attention_heads(qk, vt, out, B, T, H, D, one, one, 1 / 8, bias_v=torch.zeros(D, device=DEV))
    with pytest.raises(RuntimeError, match="cuda"):
        _lib.attention_heads(qk.cpu(), vt, out, B, T, H, D, one, one, 1 / 8)
    # shapes the binding accepts and the library refuses: nothing is launched, the output stays as it was
    for (t2, h2, d2) in ((96, 2, 64), (256, 2, 48), (16, 2, 64), (256, 1, 256)):
        c2 = h2 * d2
        with pytest.raises(RuntimeError, match="attention_heads"):
            _lib.attention_heads(torch.zeros(B * t2, 2 * c2, device=DEV), torch.zeros(B, c2, t2, device=DEV),
                                 torch.empty(B * t2, c2, device=DEV), B, t2, h2, d2, one, one, 1 / 8)
    with pytest.raises(RuntimeError, match="aligned"):
        _lib.attention_heads(qk, vt, out, B, T, H, D, one, one, 1 / 8, bias_v=torch.zeros(C + 1, device=DEV)[1:])
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    _lib.attention_heads(qk, vt * 1e6, out, B, T, H, D, one, one, 1 / 8)                              # s |v| beyond 65504
    assert not bool(torch.isfinite(out).all())
    _lib.attention_heads(qk, vt * 1e6, out, B, T, H, D, one, torch.tensor([2.0 ** -20, 2.0 ** 20], device=DEV), 1 / 8)   # the same values with their scale
    ref, _ = reference_f64(qk.cpu(), (vt * 1e6).cpu(), None, B, T, H, D)
    assert rel_err(out.cpu().reshape(B, T, C), ref) < 3e-6
    _lib.attention_heads(qk * 1e6, vt, out, B, T, H, D, one, one, 1 / 8)                              # s |q|, s |k| beyond 65504
    assert not bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------------------ networks
@pytest.fixture
def launches(monkeypatch):
    """Counts the launches of the attention forms by wrapping the bindings the executor looks up on _lib at each call."""
    n = {"attention_heads": 0, "attention256": 0, "softmax_rows": 0, "fused_tokens": []}
    for name in ("attention_heads", "attention256", "softmax_rows"):
        orig = getattr(_lib, name)

        def counted(*a, _orig=orig, _name=name, **k):
            n[_name] += 1
            if _name == "attention_heads":
                n["fused_tokens"].append(a[4])
            return _orig(*a, **k)
        monkeypatch.setattr(_lib, name, counted)
    return n


def heads_model(z):
    model = mutils.create_model(beatgans_config(**overrides_from_golden(z)))
    fill_from_seed(model, int(z["seed"]))
    np.testing.assert_allclose(weight_abs_sums(model), z["weight_abs_sums"], rtol=1e-12)
    model.to(DEV)
    model._invalidate()
    return model


@pytest.mark.parametrize("name", ["beatgans_heads_legacy.npz", "beatgans_heads_new_order.npz"])
def test_multi_head_beatgans_golden(golden, launches, name):
    """Both head orders against the REFERENCE's outputs: the 256- and 64-token blocks on the streaming kernel (three of each), the
    16-token middle block (4 heads) on the three-launch form per head."""
    z = golden(name)
    model = heads_model(z)
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    raw = model(x, t * 999)
    assert launches["attention_heads"] == 6 and sorted(launches["fused_tokens"]) == [64] * 3 + [256] * 3, launches
    assert launches["softmax_rows"] == 4 and launches["attention256"] == 0, launches
    e_raw = rel_err(raw.cpu(), z["model_out"])
    y = mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)(x, t)
    e_score = rel_err(y.cpu(), z["score"])
    print(f"{name}: model_out {e_raw:.2e}, score {e_score:.2e}")
    assert e_raw < NET_RTOL and e_score < NET_RTOL
    assert launches["attention_heads"] == 12 and launches["softmax_rows"] == 8


@pytest.mark.parametrize("switch", ["IDIFF_NO_PAIRS", "IDIFF_NO_FUSED_ATTN"])
@pytest.mark.parametrize("name", ["beatgans_heads_legacy.npz", "beatgans_heads_new_order.npz"])
def test_multi_head_beatgans_golden_on_the_per_head_fallback(golden, launches, name, switch):
    """The safe route (IDIFF_NO_PAIRS: what ScoreMatrixBuilder.build(safe=True) runs under) and IDIFF_NO_FUSED_ATTN: every block on
    the three-launch form per head, no launch of the streaming kernel, the same bar."""
    z = golden(name)
    model = heads_model(z)
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    with _lib.thread_option(switch, 1):
        raw = model(x, t * 999)
        y = mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)(x, t)
    assert launches["attention_heads"] == 0 and launches["attention256"] == 0, launches
    heads_total = (2 * 3 + 4 * 4) if "legacy" in name else (4 + 4 + 4 + 2 + 2 + 2 + 2)
    assert launches["softmax_rows"] == 2 * heads_total, launches
    e_raw, e_score = rel_err(raw.cpu(), z["model_out"]), rel_err(y.cpu(), z["score"])
    print(f"{name} under {switch}: model_out {e_raw:.2e}, score {e_score:.2e}")
    assert e_raw < NET_RTOL and e_score < NET_RTOL


def test_multi_head_beatgans_1024_tokens_vs_oracle(launches):
    """Attention at 32 x 32 (1024 tokens, 2 heads of 32) and in the 16 x 16 middle block (256 tokens, 4 heads of 32) of a random-weight
    network at B = 2 against the oracle: the streaming path (16 and 4 key chunks) inside a network."""
    cfg = beatgans_config(**{"model.model_channels": 64, "model.channel_mult": (1, 2), "model.embed_channels": 32,
                             "model.attention_resolutions": (32,), "model.num_head_channels": 32, "data.image_size": 32,
                             "data.effective_image_size": 32, "data.shape": [3, 32, 32], "model.image_size": 32})
    torch.manual_seed(0)
    ref_model = omodels.create_model(cfg)
    fill_from_seed(ref_model, 77)
    ref_model.eval()
    model = mutils.create_model(cfg)
    model.load_state_dict(ref_model.state_dict())
    model.to(DEV)
    x, t = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)), torch.tensor([1e-5, 0.4])
    with torch.no_grad():
        ref = ref_model(x, t * 999)
        ref_score = osde.get_score_fn(osde.VESDE(0.01, 50, 1000), ref_model)(x, t)
    raw = model(x.to(DEV), (t * 999).to(DEV))
    assert sorted(launches["fused_tokens"]) == [256] + [1024] * 3 and launches["softmax_rows"] == 0, launches
    e_raw = rel_err(raw.cpu(), ref)
    y = mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)(x.to(DEV), t.to(DEV))
    e_score = rel_err(y.cpu(), ref_score)
    print(f"1024-token multi-head network: model_out {e_raw:.2e}, score {e_score:.2e}")
    assert e_raw < NET_RTOL and e_score < NET_RTOL


def test_single_head_networks_do_not_reach_the_new_kernel(golden, launches):
    """Unchanged ground: the single-head fixtures still load and pass (the assertions of tests/test_hip_models.py, repeated), and
    their attention launches nothing of the streaming kernel."""
    z = golden("beatgans_wide.npz")
    model = mutils.create_model(beatgans_config(**overrides_from_golden(z)))
    fill_from_seed(model, int(z["seed"]))
    np.testing.assert_allclose(weight_abs_sums(model), z["weight_abs_sums"], rtol=1e-12)
    model.to(DEV)
    model._invalidate()
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    assert rel_err(model(x, t * 999).cpu(), z["model_out"]) < NET_RTOL
    assert rel_err(mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)(x, t).cpu(), z["score"]) < NET_RTOL
    z = golden("beatgans_paper_like.npz")
    model = mutils.create_model(beatgans_config(**overrides_from_golden(z)))
    model.load_state_dict(state_dict_from_golden(z))
    model.to(DEV)
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    assert rel_err(model(x, t * 999).cpu(), z["model_out"]) < NET_RTOL
    assert rel_err(mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)(x, t).cpu(), z["score"]) < NET_RTOL
    assert launches["attention_heads"] == 0 and launches["softmax_rows"] + launches["attention256"] > 0, launches
