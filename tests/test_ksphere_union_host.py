"""Host side of the union of k-spheres: the data set against the reference's output (tests/golden/ksphere_variants.npz, made by
tests/golden/make_ksphere_variants.py) and ``reference_score`` -- the fp64 restatement the GPU tests hold the kernel to -- against an
oracle that knows no Bessel function."""
import math

import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd.configs.config_dict import ConfigDict
from id_diff_amd.lightning_data_modules import KSphereDataset as ksd
from id_diff_amd.models import ksphere_union_exact as ku

UNIFORM = dict(n_spheres=2, ambient_dim=48, manifold_dim=[3, 10], radii=[1, 2], data_samples=64)
POLAR = dict(n_spheres=2, ambient_dim=16, radii=[1, 2], data_samples=64, embedding_type='first')


def _data(seed, **data):
    cfg = ConfigDict()
    cfg.data = ConfigDict(**data)
    torch.manual_seed(seed)
    return ksd.KSphereDataset(cfg).data


# ------------------------------------------------------------------------------------------ the data set
@pytest.mark.parametrize("noise", [0.0, 0.01])
@pytest.mark.parametrize("emb", ["separating", "along_axis", "first"])
def test_uniform_embeddings_bit_equal_to_the_reference(golden, emb, noise):
    z = golden("ksphere_variants.npz")
    got = _data(int(z["seed"]), noise_std=noise, embedding_type=emb, **UNIFORM)
    want = z[f"uniform::{emb}::noise{noise}"]
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (128, 48)
    assert np.array_equal(got.numpy(), want)


@pytest.mark.parametrize("noise", [0.0, 0.01])
@pytest.mark.parametrize("k", [1, 3, 10])
@pytest.mark.parametrize("std", [0.5, 1.0])
def test_polar_sampling_within_rounding_of_the_reference(golden, std, k, noise):
    """Same RNG consumption (one seed, same angles and same noise); the reference evaluates cos / sin row by row, a vectorised call
    may differ by an ulp in vector tails: k factors and one product each, |ours - ref| <= (2 k + 4) 2^-24 max(R, 1) per element."""
    z = golden("ksphere_variants.npz")
    got = _data(int(z["seed"]), noise_std=noise, angle_std=std, manifold_dim=k, **POLAR).numpy()
    want = z[f"polar::std{std}::k{k}::noise{noise}"]
    assert got.shape == want.shape == (128, 16)
    for i, R in enumerate(POLAR["radii"]):
        err = np.abs(got[64 * i:64 * (i + 1)].astype(np.float64) - want[64 * i:64 * (i + 1)]).max()
        print(f"polar std {std} k {k} noise {noise} sphere {i}: max |ours - ref| = {err:.3e}")
        assert err <= (2 * k + 4) * 2.0 ** -24 * max(R, 1)
    if noise == 0.0:
        np.testing.assert_allclose(np.linalg.norm(got[:64], axis=1), 1.0, atol=1e-5)
        assert np.abs(got[:, k + 1:]).max() == 0.0


def test_both_runtime_errors_of_the_reference():
    with pytest.raises(RuntimeError, match="Cant fit that many spheres. Enusre that"):
        _data(0, n_spheres=3, ambient_dim=12, manifold_dim=4, noise_std=0.0, embedding_type='separating', data_samples=4)
    with pytest.raises(RuntimeError, match="Cant fit that many spheres.$"):
        _data(0, n_spheres=3, ambient_dim=6, manifold_dim=4, noise_std=0.0, embedding_type='along_axis', data_samples=4)
    with pytest.raises(RuntimeError, match="Unknown embedding type"):
        _data(0, n_spheres=1, ambient_dim=6, manifold_dim=2, noise_std=0.0, embedding_type='nope', data_samples=4)


@pytest.mark.parametrize("emb", ["random_isometry", "first"])
def test_single_sphere_output_is_unchanged(emb):
    """The two placements the data set had before, restated as they were: same bits for one seed."""
    n, k, N = 100, 10, 32
    torch.manual_seed(42)
    pts = torch.randn((N, k + 1))
    pts = pts / torch.linalg.norm(pts, dim=1)[:, None]
    pts = pts * 1
    if emb == 'random_isometry':
        a = torch.randn(size=(n, k + 1), generator=torch.Generator().manual_seed(0))
        pts = (torch.from_numpy(np.linalg.qr(a.numpy())[0]) @ pts.T).T
    else:
        pts = torch.cat([pts, torch.zeros([N, n - pts.shape[1]])], dim=1)
    pts = pts + 0.01 * torch.randn_like(pts)
    got = _data(42, n_spheres=1, ambient_dim=n, manifold_dim=k, noise_std=0.01, embedding_type=emb, data_samples=N)
    assert torch.equal(got, pts)


def test_frames_place_the_spheres_where_the_data_is():
    for emb in ("random_isometry", "first", "separating", "along_axis"):
        cfg = ConfigDict()
        cfg.data = ConfigDict(noise_std=0.0, embedding_type=emb, **UNIFORM)
        torch.manual_seed(3)
        x = ksd.KSphereDataset(cfg).data.double().numpy()
        for i, (Q, R) in enumerate(ksd.frames(cfg)):
            assert Q.dtype == np.float64 and Q.shape == (48, UNIFORM["manifold_dim"][i] + 1)
            np.testing.assert_allclose(Q.T @ Q, np.eye(Q.shape[1]), atol=1e-6)
            xi = x[64 * i:64 * (i + 1)]
            np.testing.assert_allclose(xi @ Q @ Q.T, xi, atol=1e-6)          # inside span Q_i
            np.testing.assert_allclose(np.linalg.norm(xi, axis=1), R, rtol=1e-6)
    a = ksd.frames(cfg)[1][0]
    assert a[1, 0] == 1.0 and a[11, 10] == 1.0                                # along_axis: sphere 1 starts at coordinate 1


# ------------------------------------------------------------------------------------------ reference_score against quadrature
_THETA = 2.0 * np.pi * np.arange(4096) / 4096


def _log_density(x, sigma, frames):
    """log of the mixture of circles convolved with N(0, sigma^2 I), up to the constant all components share: the angle integral
    by 4096-point periodic quadrature (exact to rounding for these analytic periodic integrands), log-sum-exp throughout."""
    parts = []
    for Q, R in frames:
        y = R * (np.cos(_THETA)[:, None] * Q[:, 0] + np.sin(_THETA)[:, None] * Q[:, 1])
        e = -((x[:, None, :] - y[None]) ** 2).sum(-1) / (2.0 * sigma ** 2)
        m = e.max(axis=1)
        parts.append(m + np.log(np.exp(e - m[:, None]).mean(axis=1)) - math.log(len(frames)))
    parts = np.stack(parts, axis=1)
    m = parts.max(axis=1)
    return m + np.log(np.exp(parts - m[:, None]).sum(axis=1))


def _score_by_differences(x, sigma, frames, h=1e-5):
    g = np.zeros_like(x)
    for i in range(x.shape[1]):
        e = np.zeros(x.shape[1])
        e[i] = h
        g[:, i] = (_log_density(x + e, sigma, frames) - _log_density(x - e, sigma, frames)) / (2.0 * h)
    return g


def _circle_rows(Q, radii, sigma, rng, B=24):
    th = rng.uniform(0.0, 2.0 * np.pi, B)
    return (radii * np.cos(th))[:, None] * Q[:, 0] + (radii * np.sin(th))[:, None] * Q[:, 1] + sigma * rng.standard_normal((B, Q.shape[0]))


def test_reference_score_one_circle_against_quadrature():
    rng = np.random.default_rng(0)
    Q = np.linalg.qr(rng.standard_normal((3, 2)))[0]
    frames, sigma = [(Q, 1.0)], 0.05
    x = _circle_rows(Q, np.ones(24), sigma, rng)
    score, w, refused = ku.reference_score(x, sigma, frames)
    assert not refused.any() and np.array_equal(w, np.ones((24, 1)))
    err = (np.abs(_score_by_differences(x, sigma, frames) - score).max(axis=1) / np.abs(score).max(axis=1)).max()
    print(f"one circle: max relative difference to the quadrature oracle {err:.3e}")
    assert err <= 1e-6


def test_reference_score_two_mixing_circles_against_quadrature():
    """Radii 1 and 1.05 in one plane of R^4 at sigma = 0.02: between the circles both weights matter."""
    rng = np.random.default_rng(1)
    Q = np.linalg.qr(rng.standard_normal((4, 2)))[0]
    frames, sigma = [(Q, 1.0), (Q, 1.05)], 0.02
    x = _circle_rows(Q, np.linspace(0.97, 1.08, 24), sigma, rng)
    score, w, refused = ku.reference_score(x, sigma, frames)
    assert not refused.any()
    np.testing.assert_allclose(w.sum(axis=1), 1.0, rtol=1e-14)
    assert w[:, 0].min() < 0.01 and w[:, 0].max() > 0.99 and ((w[:, 0] > 0.1) & (w[:, 0] < 0.9)).any()
    err = (np.abs(_score_by_differences(x, sigma, frames) - score).max(axis=1) / np.abs(score).max(axis=1)).max()
    print(f"two circles: max relative difference to the quadrature oracle {err:.3e}")
    assert err <= 1e-6


def test_one_component_equals_the_single_sphere_closed_form():
    """J = 1 where kappa >= 5e3: models/ksphere_exact.py's four-term expansion of the Bessel ratio is exact to fp64 rounding there."""
    from id_diff_amd.models.ksphere_exact import isometry
    n, k, sigma = 100, 10, 0.01
    Q = isometry(n, k).numpy().astype(np.float64)
    rng = np.random.default_rng(2)
    y = rng.standard_normal((40, k + 1))
    x = (y / np.linalg.norm(y, axis=1, keepdims=True)) @ Q.T + sigma * rng.standard_normal((40, n))
    a = x @ Q
    r = np.linalg.norm(a, axis=1)
    kappa, p = r / sigma ** 2, k + 1
    assert kappa.min() >= 5e3
    ratio = 1 - (p - 1) / (2 * kappa) + (p - 1) * (p - 3) / (8 * kappa ** 2) + (p - 1) * (p - 3) / (8 * kappa ** 3)
    closed = (-x + (a @ Q.T) * (ratio / r)[:, None]) / sigma ** 2
    score, w, refused = ku.reference_score(x, sigma, [(Q, 1.0)])
    assert not refused.any()
    assert np.abs(score - closed).max() <= 1e-11 * np.abs(closed).max()


def test_refusal_rule():
    n = 12
    Qa, Qb = np.eye(n)[:, :3], np.eye(n)[:, 3:8]
    frames, sigma = [(Qa, 1.0), (Qb, 1.0)], 0.01
    on_a = np.zeros(n); on_a[0] = 1.0                 # on sphere a, at distance sqrt(2) from sphere b: b's kappa is 0
    origin = np.zeros(n)
    far_b = np.zeros(n); far_b[0] = 1.0; far_b[3] = 0.002         # b: kappa = 20 < 32, but its bound is 1e4 below E_a: weight 0
    inner = np.zeros(n); inner[0] = 0.05; inner[3] = 0.002        # a exact (kappa = 500) but far from its sphere: b's bound is close
    score, w, refused = ku.reference_score(np.stack([on_a, origin, far_b, inner]), sigma, frames)
    assert refused.tolist() == [False, True, False, True]
    for row in (0, 2):
        assert w[row, 0] == 1.0 and w[row, 1] == 0.0 and np.isfinite(score[row]).all()
    for row in (1, 3):
        assert np.isnan(score[row]).all() and np.isnan(w[row]).all()
    # the bound of the short component decides: U_b = log(1/2) + kappa_b - 1 / (2 sigma^2) against E_a - 800
    Ub = math.log(0.5) + 0.002 / sigma ** 2 - 1.0 / (2 * sigma ** 2)
    for r_a, want in ((1.0, False), (0.05, True)):
        ka = r_a / sigma ** 2
        Ea = math.log(0.5) + math.lgamma(1.5) - 1.0 / (2 * sigma ** 2) + 0.5 * math.log(2 / ka) + float(ku.log_bessel_i(0.5, ka))
        assert (not Ub < Ea - 800.0) == want
    # one component alone below its threshold: nothing exact, refused whatever the bound
    assert ku.reference_score(0.001 * np.ones((1, n)), 0.05, [(Qa, 1.0)])[2].all()


def test_series_against_scipy_ive():
    sp = pytest.importorskip("scipy.special")
    worst_a = worst_l = 0.0
    for p in range(2, 130):
        nu = 0.5 * p - 1.0
        kappa = np.geomspace(ku.kappa_min(p), 1e4 * ku.kappa_min(p), 33)
        i0, i1 = sp.ive(nu, kappa), sp.ive(nu + 1.0, kappa)
        worst_a = max(worst_a, np.abs(ku.bessel_ratio(nu, kappa) - i1 / i0).max())
        worst_l = max(worst_l, (np.abs(ku.log_bessel_i(nu, kappa) - (np.log(i0) + kappa)) / kappa).max())
    print(f"series against ive: worst |A - ratio| {worst_a:.3e}, worst |log I error| / kappa {worst_l:.3e}")
    assert worst_a <= 2e-14 and worst_l <= 4.0 * 2.0 ** -53


def test_model_is_registered_and_refuses_nonuniform_spheres():
    from id_diff_amd.configs.utils import read_config
    from id_diff_amd.models import utils as mutils
    cfg = read_config('configs/dimension_estimation/paper/euclidean_data/ksphere/union.py')
    assert cfg.model.name == 'ksphere_union_exact' and cfg.data.manifold_dim == [10, 30] and cfg.data.n_spheres == 2
    model = mutils.create_model(cfg)
    assert tuple(model.Qcat.shape) == (100, 42) and model.Qcat.dtype == torch.float64
    assert not any(p.requires_grad for p in model.parameters())          # nothing to restore from a checkpoint
    assert model.comp[:, :3].tolist() == [[0.0, 11.0, 1.0], [11.0, 31.0, 1.0]]
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(torch.zeros(2, 100), torch.zeros(2))
    cfg.data.angle_std = 0.5
    with pytest.raises(NotImplementedError, match="angle_std"):
        mutils.create_model(cfg)


def test_ok_limits_of_the_kernel():
    from id_diff_amd import _lib
    assert _lib.ksphere_union_ok(100, 2, 42) and _lib.ksphere_union_ok(100, 1, 11) and _lib.ksphere_union_ok(5, 1, 2)
    assert not _lib.ksphere_union_ok(100, 9, 18)           # more than 8 components
    assert not _lib.ksphere_union_ok(100, 0, 0)
    assert not _lib.ksphere_union_ok(300, 1, 129)          # a frame wider than 128
    assert not _lib.ksphere_union_ok(512, 8, 400)          # 512 x 402 doubles do not fit the LDS
