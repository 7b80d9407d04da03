"""GPU: the tangent basis on the two score models whose tangent spaces are known in closed form, and through the driver.

ksphere_exact: the data are x = Q y, |y| = 1, Q [100, 11] an isometry; the tangent space of the 10-sphere at x is Q y-perp.
span_exact: the data lie in the span of the squares' masks, which is its own tangent space everywhere.

For each point the device basis is compared with numpy's basis OF THE SAME SCORE MATRIX (the bar: sine of the largest principal
angle <= 1e-9) and must be no farther from the analytic space than numpy's is, plus 1e-9.  The angle to the analytic space
itself is a statistical property of the method, the noise level and the number of score vectors; it is printed, not asserted.
"""
import os
import pickle

import numpy as np
import pytest
import torch

import id_diff_amd
from id_diff_amd import _lib, dim_reduction
from id_diff_amd.configs.utils import read_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAPER = "configs/dimension_estimation/paper/"


def sine_of_largest_angle(T, Q):
    return float(np.linalg.norm(T - Q @ (Q.T @ T), 2))


def numpy_basis(S, d):
    """The d right singular vectors of the centred score matrix with the smallest singular values, fp64 on the host."""
    S64 = S.cpu().numpy().astype(np.float64)
    C = S64 - S64.mean(0)
    _, vec = np.linalg.eigh(C.T @ C)
    return vec[:, :d]


def check_point(S, x, analytic, known_dim, what):
    D = S.shape[1]
    sv = _lib.spectrum(S).cpu()
    d, k = dim_reduction.tangent_width(sv[:min(S.shape)].tolist(), D)
    assert d == known_dim and k == known_dim
    T, ritz, resid = _lib.tangent_basis(S, k)
    Th = T.cpu().numpy()
    ref = numpy_basis(S, k)
    to_numpy = sine_of_largest_angle(Th, ref)
    dev_far, np_far = sine_of_largest_angle(Th, analytic), sine_of_largest_angle(ref, analytic)
    print(f"\n[tangent {what}] d = {d}; sine(device, numpy) = {to_numpy:.3e}; sine to the analytic tangent space: device {dev_far:.6e}, "
          f"numpy {np_far:.6e}; resid = {float(resid):.3e}, ritz in [{float(ritz[0]):.3e}, {float(ritz[-1]):.3e}], "
          f"largest eigenvalue {float(sv[0]) ** 2:.3e}")
    assert float(np.abs(Th.T @ Th - np.eye(k)).max()) <= 1e-13 * k
    assert to_numpy <= 1e-9
    assert dev_far <= np_far + 1e-9


def ksphere_config(tmp_path):
    cfg = read_config(PAPER + 'euclidean_data/ksphere/10dim.py')
    cfg.model.name = 'ksphere_exact'
    cfg.data.data_samples = 2000
    cfg.device = DEV
    cfg.logging.log_path = str(tmp_path)
    cfg.dim_estimation.num_datapoints = 3
    return cfg


def test_ksphere_exact_tangent_is_q_y_perp(tmp_path):
    cfg = ksphere_config(tmp_path)
    torch.manual_seed(int(cfg.get('seed', 42)))
    DataModule, pl_module, score_fn, device = dim_reduction.setup_model(cfg)
    points = dim_reduction.collect_points(DataModule.train_dataloader(), 3)
    assert len(points) == 2 and points[0][0].shape == (100,)
    builder = dim_reduction.ScoreMatrixBuilder(score_fn, pl_module.sde, pl_module.sampling_eps, device)
    with torch.no_grad():
        S = dim_reduction.build_many(builder, [x.to(device) for x, _ in points], points[0][1], [1000003 * (p + 1) for p in range(2)])
    Q = pl_module.score_model.Q.detach().cpu().numpy().astype(np.float64)           # [100, 11]
    for p, (x, _) in enumerate(points):
        y = Q.T @ x.numpy().astype(np.float64)
        y /= np.linalg.norm(y)
        perp = np.linalg.svd(y[None, :])[2][1:].T                                   # [11, 10]: an orthonormal basis of y-perp
        check_point(S[p].contiguous(), x, Q @ perp, 10, f"ksphere_exact point {p}")


def test_span_exact_tangent_is_the_span_of_the_masks(tmp_path):
    cfg = read_config(PAPER + 'image_data/squares/10.py')
    cfg.model.name = 'span_exact'
    cfg.data.data_samples = 256
    cfg.device = DEV
    cfg.logging.log_path = str(tmp_path)
    torch.manual_seed(int(cfg.get('seed', 42)))
    DataModule, pl_module, score_fn, device = dim_reduction.setup_model(cfg)
    (x, batchsize), = dim_reduction.collect_points(DataModule.train_dataloader(), 2)
    builder = dim_reduction.ScoreMatrixBuilder(score_fn, pl_module.sde, pl_module.sampling_eps, device)
    with torch.no_grad():
        S = builder.build(x.to(device), batchsize, seed=1000003)
    assert S.shape[1] == 1024 and pl_module.score_model.rank == 10
    check_point(S, x, pl_module.score_model.Q.detach().cpu().numpy(), 10, "span_exact squares/10")


def test_driver_returns_bases_beside_unchanged_spectra(tmp_path):
    cfg = ksphere_config(tmp_path)
    plain_svd, plain_dims = dim_reduction.get_manifold_dimension(cfg, return_svd=True, return_dims=True)
    svd, dims, tangent = dim_reduction.get_manifold_dimension(cfg, return_svd=True, return_dims=True, return_tangent=True)
    assert svd == plain_svd and dims == plain_dims == [10, 10]            # bit-equal: the same floats, compared as Python values
    assert len(tangent) == 2
    for T in tangent:
        assert isinstance(T, np.ndarray) and T.dtype == np.float32 and T.shape == (100, 10)
        assert float(np.abs(T.astype(np.float64).T @ T - np.eye(10)).max()) <= 1e-6
    svd2, tangent2 = dim_reduction.get_manifold_dimension(cfg, return_svd=True, return_tangent=True)
    assert svd2 == plain_svd and all(np.array_equal(a, b) for a, b in zip(tangent, tangent2))
    # the CLI's form: the config key writes the bases beside the unchanged pickle
    cfg.dim_estimation.save_tangent = True
    assert dim_reduction.get_manifold_dimension(cfg, name='pts') is None
    folder = os.path.join(str(tmp_path), cfg.logging.log_name, 'svd')
    with open(os.path.join(folder, 'pts.pkl'), 'rb') as f:
        assert pickle.load(f) == plain_svd
    with open(os.path.join(folder, 'pts_tangent.pkl'), 'rb') as f:
        saved = pickle.load(f)
    assert sorted(saved) == ['dims', 'tangent'] and saved['dims'] == [10, 10]
    assert all(np.array_equal(a, b) for a, b in zip(tangent, saved['tangent']))
