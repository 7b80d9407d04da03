"""Generate tests/golden/beatgans_heads_legacy.npz and beatgans_heads_new_order.npz: multi-head BeatGANs U-Nets RUN by the reference.

Run once, in the build container only (``/root/reference`` does not exist on the GPU box)::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_beatgans_heads.py

The reference is imported read-only through make_golden.py's stand-ins and helpers (``beatgans_config``, ``fill_from_seed``,
``save``); nothing of it is copied.  No weights are stored (the ``beatgans_wide.npz`` scheme): a test rebuilds them from ``seed``
and checks ``weight_abs_sums``.  Both fixtures: 16 x 16 images, model_channels 128, channel_mult (1, 2, 2), attention at the
16 x 16 and 8 x 8 levels (256 and 64 tokens) and in the 4 x 4 middle block (16 tokens), every parameter drawn by
``fill_from_seed`` so that the zero-initialised projections contribute.
    legacy     num_head_channels = 64, QKVAttentionLegacy: 2 heads of 64 over 256 tokens, 4 heads of 64 over 64 and over 16 tokens
    new_order  num_heads = 4, num_heads_upsample = 2, QKVAttention: heads of 32 and 64 on the way down, of 128 and 64 on the way up
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (installs the stand-ins, puts the reference on sys.path)

HEADS_SEED = 20300
COMMON = {"model.model_channels": 128, "model.channel_mult": (1, 2, 2), "model.embed_channels": 64,
          "model.attention_resolutions": (16, 8), "data.image_size": 16, "data.effective_image_size": 16,
          "data.shape": [3, 16, 16], "model.image_size": 16}
VARIANTS = {
    "legacy": {"model.num_head_channels": 64},
    "new_order": {"model.num_heads": 4, "model.num_heads_upsample": 2, "model.use_new_attention_order": True},
}


def gen(name, extra, seed):
    from models import BeatGANsUNET  # reference: registers the model
    torch.manual_seed(0)
    over = dict(COMMON, **extra)
    heads_up = over.get("model.num_heads_upsample", -1)
    if heads_up != -1:
        # BeatGANsUNET.py:24-25 sets self.num_heads_upsample only when the config says -1 and reads it at :185 either way, so any
        # other value dies in the constructor with an AttributeError.  The value it evidently means to read is the config's: hand
        # it over as a class attribute for the duration of the construction (the reference's own code builds and runs the model).
        BeatGANsUNET.BeatGANsUNetModel.num_heads_upsample = heads_up
    try:
        model = mg.mutils.create_model(mg.beatgans_config(**over))
    finally:
        if heads_up != -1:
            del BeatGANsUNET.BeatGANsUNetModel.num_heads_upsample
    if heads_up != -1:
        model.num_heads_upsample = heads_up
        assert [m.attention.n_heads for m in model.output_blocks.modules() if hasattr(m, "attention")] and \
            all(m.attention.n_heads == heads_up for m in model.output_blocks.modules() if hasattr(m, "attention"))
    mg.fill_from_seed(model, seed)
    sde = mg.sde_lib.VESDE(sigma_min=0.01, sigma_max=50, N=1000)
    score_fn = mg.mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=True)
    x = torch.rand(3, 3, 16, 16, generator=torch.Generator().manual_seed(seed + 7))
    t = torch.tensor([1e-5, 0.2, 0.9])
    with torch.no_grad():
        y = score_fn(x, t)
        raw = model.eval()(x, t * 999)
    ks = sorted(over)
    chk = np.array([float(v.double().abs().sum()) for v in model.state_dict().values() if v.dtype.is_floating_point])
    mg.save(f"beatgans_heads_{name}.npz", x=x.numpy(), t=t.numpy(), score=y.numpy(), model_out=raw.numpy(), weight_abs_sums=chk,
            seed=np.array(seed), override_keys=np.array(ks, dtype="U64"),
            override_vals=np.array([repr(over[k]) for k in ks], dtype="U64"))


if __name__ == "__main__":
    torch.set_num_threads(8)
    for i, (name, extra) in enumerate(VARIANTS.items()):
        gen(name, extra, HEADS_SEED + i)
