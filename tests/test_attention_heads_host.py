"""Multi-head BeatGANs attention, the part that needs no GPU: the model builds with the reference's head settings and keeps its
``state_dict`` layout, and the pack-time row permutation (``models.beatgans.pack_qkv_heads``) turns both head orders of the
reference (BeatGANsblocks.py:466-526) into the executor's head-contiguous q | k, v."""
import numpy as np
import pytest
import torch

from helpers import beatgans_config, fill_from_seed, overrides_from_golden, rel_err, weight_abs_sums
from id_diff_amd.models import beatgans as hip_beatgans, utils as mutils
from oracle import beatgans as obeatgans, models as omodels, sde as osde

FIXTURES = ("beatgans_heads_legacy.npz", "beatgans_heads_new_order.npz")


@pytest.mark.parametrize("name", FIXTURES)
def test_model_builds_with_heads_and_keeps_the_state_dict_layout(golden, name):
    z = golden(name)
    cfg = beatgans_config(**overrides_from_golden(z))
    model = mutils.create_model(cfg)
    ref = omodels.create_model(cfg)
    sd, rsd = model.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd)
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in rsd.values()]
    heads = [(m.channels, m.num_heads, m.use_new_attention_order) for m in model.modules() if isinstance(m, hip_beatgans.AttentionBlock)]
    want = [m.num_heads for m in ref.modules() if isinstance(m, obeatgans.AttentionBlock)]
    assert [h for _, h, _ in heads] == want and max(want) > 1
    if "legacy" in name:
        assert heads == [(128, 2, False), (256, 4, False), (256, 4, False), (256, 4, False), (256, 4, False), (128, 2, False), (128, 2, False)]
    else:                                                   # 4 heads on the way down and in the middle, 2 on the way up
        assert heads == [(128, 4, True), (256, 4, True), (256, 4, True), (256, 2, True), (256, 2, True), (128, 2, True), (128, 2, True)]
    fill_from_seed(model, int(z["seed"]))
    np.testing.assert_allclose(weight_abs_sums(model), z["weight_abs_sums"], rtol=1e-12)


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_the_reference_outputs(golden, name):
    """The yardstick of the GPU tests: oracle.beatgans on the fixture's weights against what the reference computed."""
    z = golden(name)
    model = omodels.create_model(beatgans_config(**overrides_from_golden(z)))
    fill_from_seed(model, int(z["seed"]))
    x, t = torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    with torch.no_grad():
        raw = model.eval()(x, t * 999)
        y = osde.get_score_fn(osde.VESDE(0.01, 50, 1000), model)(x, t)
    assert rel_err(raw, z["model_out"]) < 2e-6
    assert rel_err(y, z["score"]) < 2e-6


def canonical_attention_f64(x, norm, wqk, bqk, wv, bv, wo, bo, heads):
    """The executor's arithmetic restated in float64 on the PACKED weights: q | k and v projections of the normalised input,
    softmax(q_h k_h^T D^-1/2) v_h per head on column ranges [h D, (h + 1) D), heads concatenated in that order, output projection."""
    b, c, hh, ww = x.shape
    n = norm(x.reshape(b, c, -1)).permute(0, 2, 1)                               # [B, T, C]
    qk = n @ wqk.T + bqk
    v = n @ wv.T + bv
    D = c // heads
    out = torch.empty_like(v)
    for h in range(heads):
        q, k = qk[..., h * D:(h + 1) * D], qk[..., c + h * D:c + (h + 1) * D]
        w = torch.softmax(q @ k.transpose(1, 2) * D ** -0.5, dim=-1)
        out[..., h * D:(h + 1) * D] = w @ v[..., h * D:(h + 1) * D]
    y = out @ wo.T + bo
    return (x.reshape(b, c, -1) + y.permute(0, 2, 1)).reshape(b, c, hh, ww)


@pytest.mark.parametrize("new_order", [False, True])
@pytest.mark.parametrize("heads", [1, 2, 4, 8])
def test_packed_weights_reproduce_the_reference_head_order(heads, new_order):
    g = torch.Generator().manual_seed(10 * heads + int(new_order))
    C = 64
    blk = obeatgans.AttentionBlock(C, num_heads=heads, new_order=new_order).double()
    with torch.no_grad():
        for prm in blk.parameters():
            prm.copy_(torch.randn(prm.shape, generator=g, dtype=torch.float64) * (0.3 if prm.ndim > 1 else 0.1) + (1.0 if prm.ndim == 1 and prm is blk.norm.weight else 0.0))
    x = torch.randn(2, C, 4, 6, generator=g, dtype=torch.float64)
    w, b = blk.qkv.weight.detach().view(3 * C, C), blk.qkv.bias.detach()
    wqk, bqk, wv, bv = hip_beatgans.pack_qkv_heads(w, b, heads, new_order)
    assert wqk.shape == (2 * C, C) and bqk.shape == (2 * C,) and wv.shape == (C, C) and bv.shape == (C,)
    assert all(t.is_contiguous() for t in (wqk, bqk, wv, bv))
    # a permutation of the projection's rows: nothing dropped, nothing duplicated
    assert torch.equal(torch.sort(torch.cat([bqk, bv])).values, torch.sort(b).values)
    with torch.no_grad():
        ref = blk(x)
        got = canonical_attention_f64(x, blk.norm, wqk, bqk, wv, bv, blk.proj_out.weight.view(C, C), blk.proj_out.bias, heads)
    assert float((got - ref).abs().max()) < 1e-12 * max(1.0, float(ref.abs().max()))
    if heads > 1:                                           # the other order on the same weights is another function
        wrong = hip_beatgans.pack_qkv_heads(w, b, heads, not new_order)
        with torch.no_grad():
            other = canonical_attention_f64(x, blk.norm, *wrong, blk.proj_out.weight.view(C, C), blk.proj_out.bias, heads)
        assert float((other - ref).abs().max()) > 1e-3


@pytest.mark.parametrize("new_order", [False, True])
def test_one_head_packs_the_plain_thirds_bit_for_bit(new_order):
    g = torch.Generator().manual_seed(3)
    C = 32
    w, b = torch.randn(3 * C, C, generator=g), torch.randn(3 * C, generator=g)
    wqk, bqk, wv, bv = hip_beatgans.pack_qkv_heads(w, b, 1, new_order)
    assert torch.equal(wqk, w[:2 * C].contiguous()) and torch.equal(bqk, b[:2 * C].contiguous())
    assert torch.equal(wv, w[2 * C:].contiguous()) and torch.equal(bv, b[2 * C:].contiguous())


def test_channels_that_do_not_split_into_heads_are_refused_at_construction():
    with pytest.raises(ValueError):
        hip_beatgans.AttentionBlock(96, num_heads=5)
    with pytest.raises(ValueError):
        hip_beatgans.AttentionBlock(96, num_heads=1, num_head_channels=64)
    with pytest.raises(ValueError):
        hip_beatgans.pack_qkv_heads(torch.zeros(3 * 96, 96), torch.zeros(3 * 96), 5, False)
    with pytest.raises(ValueError):
        mutils.create_model(beatgans_config(**{"model.num_heads": 3}))          # 32 channels, 3 heads
    blk = hip_beatgans.AttentionBlock(96, num_heads=1, num_head_channels=32, use_new_attention_order=True)
    assert blk.num_heads == 3 and blk.use_new_attention_order
