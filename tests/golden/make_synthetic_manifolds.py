"""Generate tests/golden/synthetic_manifolds.npz by RUNNING the reference's synthetic data modules on the CPU.

Run once, where a checkout of the reference (GBATZOLIS/ID-diff) is at hand -- not on the GPU box::

    ID_DIFF_REFERENCE=/path/to/ID-diff PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_synthetic_manifolds.py

The reference is imported read-only.  Packages it imports at module level that are not installed here (pytorch_lightning,
torchvision, cv2, ml_collections) get in-memory stand-ins, as in make_golden.py; its top-level ``utils`` (imported for one
helper the fixed manifolds never call) is a stand-in too.  Nothing of the reference is copied: the file holds arrays and scalars.

Per image config (prefixes squares10 / squares20 / squares100 / blobs10 / blobs20 / blobs100):
    <p>::table      the reference's own table: [K, 3] (x, y, side) of get_the_squares, or [K, 2] centres
    <p>::images     [16, S, S] fp32: the data set at data_samples = 16 (the stream is sequential: the first 16 of any larger set)
    <p>::cfg_keys / <p>::cfg_vals   every scalar / list setting of the reference's config, dotted key and repr
and for the line config:
    line::rows      the first 32 rows of LineDataset under torch.manual_seed(42)
    line::cfg_keys / line::cfg_vals
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("ID_DIFF_REFERENCE", "/root/reference")
PAPER = "configs/dimension_estimation/paper"
IMAGE_CONFIGS = {"squares10": "image_data/squares/10.py", "squares20": "image_data/squares/20.py",
                 "squares100": "image_data/squares/100.py", "blobs10": "image_data/gaussian_blobs/10.py",
                 "blobs20": "image_data/gaussian_blobs/20.py", "blobs100": "image_data/gaussian_blobs/100.py"}
LINE_CONFIG = "euclidean_data/line/config.py"
N_IMAGES, N_ROWS = 16, 32


def _install_standins():
    sys.path.insert(0, os.path.join(REPO, "id-diff_amd", "configs"))
    from config_dict import ConfigDict            # plain attribute dict, ours
    pl = types.ModuleType("pytorch_lightning")
    pl.LightningModule = torch.nn.Module
    pl.LightningDataModule = object
    tv, tvt, tvf = (types.ModuleType(n) for n in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional"))
    tvf.normalize = None
    tvt.functional = tvf
    tv.transforms = tvt
    ml = types.ModuleType("ml_collections")
    ml.ConfigDict = ConfigDict
    ut = types.ModuleType("utils")
    ut.compute_grad = None
    sys.modules.update({"pytorch_lightning": pl, "torchvision": tv, "torchvision.transforms": tvt,
                        "torchvision.transforms.functional": tvf, "ml_collections": ml, "utils": ut})
    try:
        __import__("cv2")
    except Exception:
        sys.modules["cv2"] = types.ModuleType("cv2")
    import torch.utils.cpp_extension as ce
    ce.load = lambda *a, **k: None
    import matplotlib
    matplotlib.use("Agg")
    return ConfigDict


def flatten(cfg, ConfigDict, prefix=""):
    """Dotted key -> repr for every leaf that is a plain scalar or a list / tuple of them."""
    out = {}
    for k, v in cfg.items():
        if isinstance(v, ConfigDict):
            out.update(flatten(v, ConfigDict, f"{prefix}{k}."))
        elif v is None or isinstance(v, (bool, int, float, str)) or (
                isinstance(v, (list, tuple)) and all(isinstance(e, (bool, int, float, str)) for e in v)):
            out[f"{prefix}{k}"] = repr(list(v) if isinstance(v, tuple) else v)
    return out


def read_reference_config(rel):
    path = os.path.join(REF, PAPER, rel)
    spec = importlib.util.spec_from_file_location("ref_config_" + rel.replace("/", "_")[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.get_config()


def main():
    ConfigDict = _install_standins()
    sys.path.insert(0, REF)
    import lightning_data_modules.SyntheticDataset as ref_sd
    import lightning_data_modules.LineDataset as ref_line
    out = {}

    def put_config(p, cfg):
        flat = flatten(cfg, ConfigDict)
        out[f"{p}::cfg_keys"] = np.array(list(flat.keys()))
        out[f"{p}::cfg_vals"] = np.array(list(flat.values()))

    for p, rel in IMAGE_CONFIGS.items():
        cfg = read_reference_config(rel)
        put_config(p, cfg)
        cfg.data.data_samples = N_IMAGES
        d = cfg.data
        if d.dataset_type == "FixedSquaresManifold":
            ds = ref_sd.FixedSquaresManifold(cfg)
            table = ds.get_the_squares(cfg.seed, d.num_squares, d.square_range, d.image_size)
        else:
            ds = ref_sd.FixedGaussiansManifold(cfg)
            table = ds.get_the_gaussian_centers(cfg.seed, d.num_gaussians, d.std_range, d.image_size)
        assert ds.labels == [] and ds.data.dtype == torch.float32 and tuple(ds.data.shape) == (N_IMAGES, 1, d.image_size, d.image_size)
        out[f"{p}::table"] = np.array([[int(v) for v in row] for row in table], dtype=np.int64)
        out[f"{p}::images"] = ds.data[:, 0].numpy().copy()
        print(p, out[f"{p}::table"].shape, float(ds.data.min()), float(ds.data.max()))
    cfg = read_reference_config(LINE_CONFIG)
    put_config("line", cfg)
    torch.manual_seed(42)
    out["line::rows"] = ref_line.LineDataset(cfg).data[:N_ROWS].numpy().copy()
    print("line", out["line::rows"].shape)
    np.savez_compressed(os.path.join(HERE, "synthetic_manifolds.npz"), **out)


if __name__ == "__main__":
    main()
