"""Generate tests/golden/ksphere_variants.npz by RUNNING the reference's KSphereDataset on the CPU (run once, where the reference
checkout is present; see make_golden.py for how the reference is imported).  Nothing of the reference is copied: the file holds the
arrays it produced, keyed by the config values that produced them.

    uniform::<embedding>::noise<noise_std>            two spheres of dimension 3 and 10, radii [1, 2], in R^48, 64 samples each
    polar::std<angle_std>::k<k>::noise<noise_std>     two k-spheres, radii [1, 2], 'first' embedding in R^16, 64 samples each

Every array is drawn after torch.manual_seed(SEED).
"""
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
SEED = 20240611
UNIFORM = dict(n_spheres=2, ambient_dim=48, manifold_dim=[3, 10], radii=[1, 2], data_samples=64)
POLAR = dict(n_spheres=2, ambient_dim=16, radii=[1, 2], data_samples=64, embedding_type='first')


def main():
    pl = types.ModuleType("pytorch_lightning")
    pl.LightningDataModule = object
    sys.modules["pytorch_lightning"] = pl
    _orig = torch.from_numpy                          # numpy >= 2: np.linalg.qr(Tensor) hands back a Tensor (KSphereDataset.py:42-43)
    torch.from_numpy = lambda a: a if isinstance(a, torch.Tensor) else _orig(a)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REPO, "id-diff_amd", "configs"))
    from config_dict import ConfigDict
    from lightning_data_modules.KSphereDataset import KSphereDataset

    def run(**data):
        cfg = ConfigDict()
        cfg.data = ConfigDict(**data)
        torch.manual_seed(SEED)
        return KSphereDataset(cfg).data.numpy()

    out = {"seed": np.int64(SEED)}
    for noise in (0.0, 0.01):
        for emb in ("separating", "along_axis", "first"):
            out[f"uniform::{emb}::noise{noise}"] = run(noise_std=noise, embedding_type=emb, **UNIFORM)
        for std in (0.5, 1.0):
            for k in (1, 3, 10):
                out[f"polar::std{std}::k{k}::noise{noise}"] = run(noise_std=noise, angle_std=std, manifold_dim=k, **POLAR)
    path = os.path.join(HERE, "ksphere_variants.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
