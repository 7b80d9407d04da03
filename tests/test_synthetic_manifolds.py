"""Host side of the paper's synthetic manifolds (squares, Gaussian blobs, line): tables, random stream, configs, registry.

The fixture tests/golden/synthetic_manifolds.npz holds what the reference's own classes produced (make_synthetic_manifolds.py).
Nothing here needs a GPU; the rendering kernels are tested in test_hip_manifolds.py.
"""
import ast
import random

import numpy as np
import pytest
import torch

import id_diff_amd
from id_diff_amd.configs.config_dict import ConfigDict
from id_diff_amd.configs.utils import read_config
from id_diff_amd.lightning_data_modules import LineDataset, SyntheticDataset as sd
from id_diff_amd.lightning_data_modules.utils import create_lightning_datamodule, get_lightning_datamodule_by_name

from test_hip_manifolds import CONFIGS, blobs_bound, ref_blobs_f64, ref_squares_f32

PAPER = "configs/dimension_estimation/paper/"
LINE = PAPER + "euclidean_data/line/config.py"


@pytest.fixture(scope="module")
def z(golden):
    return golden("synthetic_manifolds.npz")


def _table(cfg):
    d = cfg.data
    if d.dataset_type == "FixedSquaresManifold":
        return sd.get_the_squares(cfg.seed, d.num_squares, d.square_range, d.image_size)
    return sd.get_the_gaussian_centers(cfg.seed, d.num_gaussians, d.std_range, d.image_size)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_tables_equal_the_reference(z, name):
    cfg = read_config(PAPER + CONFIGS[name])
    state = random.getstate()
    np.testing.assert_array_equal(np.asarray(_table(cfg)), z[f"{name}::table"])
    assert random.getstate() == state                      # the module's own generator: the global one is left alone


def test_square_rects_are_the_pixels_the_reference_paints(z):
    info = z["squares100::table"]
    rects = sd.square_rects(info)
    for (x, y, side), (r0, c0, s) in zip(info, rects):
        rows = [x - ((side + 1) // 2 - 1) + i for i in range(side)]          # SyntheticDataset.py:118-123 of the reference
        cols = [y - ((side + 1) // 2 - 1) + j for j in range(side)]
        assert (r0, c0, s) == (rows[0], cols[0], side) and rows[-1] == r0 + s - 1 and cols[-1] == c0 + s - 1
    assert rects.min() >= 0 and (rects[:, :2] + rects[:, 2:]).max() <= 32


@pytest.mark.parametrize("name", ["squares10", "blobs100"])
def test_transplanted_stream_equals_random_random_call_by_call(name):
    """After the table is drawn, numpy's RandomState with the transplanted Mersenne-Twister state returns, vectorised, the very
    doubles ``random.random()`` returns one call at a time -- and ``random.uniform`` is a + (b - a) * random()."""
    cfg = read_config(PAPER + CONFIGS[name])
    rng = random.Random()
    if name.startswith("squares"):
        sd.get_the_squares(cfg.seed, cfg.data.num_squares, cfg.data.square_range, 32, rng=rng)
    else:
        sd.get_the_gaussian_centers(cfg.seed, cfg.data.num_gaussians, cfg.data.std_range, 32, rng=rng)
    rs = sd.transplanted_stream(rng)
    first = rs.random_sample((7, 13))
    second = rs.random_sample((5, 13))                     # slabs continue the stream
    calls = np.array([rng.random() for _ in range(12 * 13)]).reshape(12, 13)
    np.testing.assert_array_equal(np.concatenate([first, second]), calls)
    rng2, rng3 = random.Random(5), random.Random(5)
    u = sd.transplanted_stream(rng2).random_sample(50)
    np.testing.assert_array_equal(1 + (5 - 1) * u, np.array([rng3.uniform(1, 5) for _ in range(50)]))


def _flat(cfg, prefix=""):
    out = {}
    for k, v in cfg.items():
        if isinstance(v, ConfigDict):
            out.update(_flat(v, f"{prefix}{k}."))
        else:
            out[f"{prefix}{k}"] = list(v) if isinstance(v, tuple) else v
    return out


# the groups this project's drivers read; of `training` the keys that describe the experiment (not the cluster it ran on)
_TRAINING = ("batch_size", "sde", "continuous", "likelihood_weighting", "reduce_mean", "lightning_module")


@pytest.mark.parametrize("name,path", sorted(CONFIGS.items()) + [("line", "euclidean_data/line/config.py")])
def test_config_scalars_equal_the_reference(z, name, path):
    ref = dict(zip((str(k) for k in z[f"{name}::cfg_keys"]), (ast.literal_eval(str(v)) for v in z[f"{name}::cfg_vals"])))
    ours = _flat(read_config(PAPER + path))
    want = [k for k in ref if k.split(".")[0] in ("data", "model") or k == "seed"
            or k in ("logging.log_path", "logging.log_name", "logging.top_k", "logging.every_n_epochs", "logging.svd_frequency",
                     "logging.save_svd", "logging.svd_points", "validation.batch_size", "eval.batch_size")
            or (k.startswith("training.") and k.split(".")[1] in _TRAINING)]
    assert len(want) >= 20
    for k in want:
        assert k in ours, f"{name}: {k} missing"
        assert ours[k] == ref[k], f"{name}: {k} = {ours[k]!r}, the reference has {ref[k]!r}"
    for k in ours:                                         # and no data / model setting of our own invention
        if k.split(".")[0] in ("data", "model"):
            assert k in ref, f"{name}: {k} is not a key of the reference's config"


def test_line_rows_within_one_ulp(z):
    cfg = read_config(LINE)
    torch.manual_seed(42)
    data = LineDataset.LineDataset(cfg).data
    assert tuple(data.shape) == (10000, 100) and data.dtype == torch.float32
    got, ref = data[:32].numpy(), z["line::rows"]
    assert np.all(np.abs(got - ref) <= np.spacing(np.abs(ref)))
    data_n = LineDataset.LineDataset(read_config(LINE)).data
    assert not torch.equal(data_n, data)                   # unseeded: another draw


def test_data_modules_registered_and_split(monkeypatch):
    assert get_lightning_datamodule_by_name("Synthetic") is sd.SyntheticDataModule
    assert get_lightning_datamodule_by_name("Line") is LineDataset.LineDataModule
    dm = create_lightning_datamodule(read_config(LINE))
    dm.setup()
    assert (len(dm.train_data), len(dm.valid_data), len(dm.test_data)) == (8000, 1000, 1000)
    # 'Synthetic': the split and the plumbing around the renderer (the renderer itself needs the GPU)
    cfg = read_config(PAPER + CONFIGS["squares10"])
    cfg.data.data_samples = 50
    seen = []

    def fake_slabs(config, device=None, slab=None):
        seen.append(config.data.dataset_type)
        yield 0, 20, torch.ones(20, 32, 32)
        yield 20, 50, torch.full((30, 32, 32), 2.0)
    monkeypatch.setattr(sd, "_slabs", fake_slabs)
    dm = create_lightning_datamodule(cfg)
    dm.setup()
    assert (len(dm.train_data), len(dm.valid_data), len(dm.test_data)) == (40, 5, 5) and seen == ["FixedSquaresManifold"]
    ds = dm.dataset
    assert isinstance(ds, sd.FixedSquaresManifold) and ds.labels == [] and tuple(ds.data.shape) == (50, 1, 32, 32)
    assert ds.data.device.type == "cpu" and float(ds.data[19].max()) == 1.0 and float(ds.data[20].min()) == 2.0
    batch = next(iter(dm.train_dataloader()))
    assert tuple(batch.shape) == (40, 1, 32, 32)


@pytest.mark.parametrize("kind", ["SquaresManifold", "GaussianBubbles", "Circles", None])
def test_other_dataset_types_are_refused_by_name(kind):
    cfg = read_config(PAPER + CONFIGS["squares10"])
    cfg.data.dataset_type = kind
    dm = create_lightning_datamodule(cfg)
    with pytest.raises(NotImplementedError, match=repr(kind)):
        dm.setup()


@pytest.mark.parametrize("K,rank", [(10, 10), (20, 20), (100, 99)])
def test_rank_of_the_mask_matrix(K, rank):
    from id_diff_amd.models import span_exact
    cfg = read_config(PAPER + CONFIGS[f"squares{K}"])
    M = span_exact.mask_matrix(sd.square_rects(_table(cfg)), 32)
    assert M.shape == (1024, K) and np.linalg.matrix_rank(M) == rank
    Q, r = span_exact.span_basis(M)
    assert r == rank and Q.shape == (1024, rank)
    np.testing.assert_allclose(Q.T @ Q, np.eye(rank), atol=1e-12)
    np.testing.assert_allclose(Q @ (Q.T @ M), M, atol=1e-12)           # span(Q) = span(M)


# ---- the numpy restatements the GPU tests compare against, checked here against the reference's own images
@pytest.mark.parametrize("K", [10, 20, 100])
def test_fp32_restatement_of_the_squares_is_the_reference_bit_for_bit(z, K):
    cfg = read_config(PAPER + CONFIGS[f"squares{K}"])
    rng = random.Random()
    rects = sd.square_rects(sd.get_the_squares(cfg.seed, K, cfg.data.square_range, 32, rng=rng))
    coef = sd.transplanted_stream(rng).random_sample((16, K)).astype(np.float32)
    np.testing.assert_array_equal(ref_squares_f32(coef, rects, 32), z[f"squares{K}::images"])


@pytest.mark.parametrize("K", [10, 20, 100])
def test_fp64_restatement_of_the_blobs_is_within_the_bar_of_the_reference(z, K):
    cfg = read_config(PAPER + CONFIGS[f"blobs{K}"])
    rng = random.Random()
    centres = np.asarray(sd.get_the_gaussian_centers(cfg.seed, K, cfg.data.std_range, 32, rng=rng))
    std = 1 + (5 - 1) * sd.transplanted_stream(rng).random_sample((16, K))
    img, vmin, vmax = ref_blobs_f64(std, centres, 32)
    err = np.abs(img - z[f"blobs{K}::images"].astype(np.float64)).reshape(16, -1).max(axis=1)
    bar = blobs_bound(K, vmin, vmax)
    print(f"K={K}: restatement vs reference max {err.max():.3e}, bar min {bar.min():.3e}")
    assert np.all(err <= bar)
