"""GPU tests of the empirical score: the fused kernel (csrc/empirical_score.hip) element-wise against the long-double
direct-difference oracle under the bound of tests/empirical_cases.py (validated on the CPU in test_empirical_host.py) plus the final
fp32 rounding, its ESS, the isolation of rows that are not finite, run-to-run and split-launch bit equality, and the intrinsic
dimension of the line and of a circle beside a 2-sphere through the whole driver and through ``empirical.local_dims``."""
import warnings

import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd import _lib, dim_reduction, empirical
from id_diff_amd.configs.utils import read_config
from id_diff_amd.models import empirical_exact as ee
from id_diff_amd.models import utils as mutils

import empirical_cases as ec

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINE = 'configs/dimension_estimation/paper/euclidean_data/line/empirical.py'
CAP = 192
REGIMES = [1e-3, 0.1, 1e3]          # times U(0.5, 2), row by row: one point holds all the weight / a neighbourhood / every point alike

CASES = [(1, 1, 1), (1, 3, 3), (17, 5, 4), (63, 65, 5), (65, 63, 23), (257, 1000, 100), (64, 4097, 128), (130, 257, CAP - 1), (33, 300, CAP)]
VARIANTS = ["plain", "offset1000", "far"]
_made = {}


def _case(B, N, D, variant):
    """(x, sigma, X, oracle out, oracle ess, r), made once: N points of a sphere of dimension min(2, D - 1) in R^D (D = 1: the two
    points +-1, many times over), rows at sigma = REGIMES[b % 3] U(0.5, 2) from a point of the cloud, or 100 units away from it."""
    key = (B, N, D, variant)
    if key not in _made:
        seed = 7 * B + 3 * N + D
        X = ec.sphere_cloud(N, min(2, D - 1), D, seed, offset=1000.0 if variant == "offset1000" else 0.0)
        x, sigma = ec.rows_near(X, B, REGIMES, seed + 1)
        if variant == "far":
            rng = np.random.default_rng(seed + 2)
            u = rng.standard_normal((B, D))
            x = (X[rng.integers(0, N, B)].astype(np.float64) + 100.0 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
        _made[key] = (x, sigma, X) + ec.oracle(x, sigma, X)
    return _made[key]


def _launch(x, sigma, X, mult=None):
    pack = _lib.empirical_pack(torch.from_numpy(X).to(DEV))
    out, ess = _lib.empirical_score(torch.from_numpy(x).to(DEV), pack, torch.from_numpy(sigma).to(DEV),
                                    None if mult is None else torch.from_numpy(mult).to(DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy(), ess.cpu().numpy()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,N,D", CASES, ids=[f"B{b}-N{n}-D{d}" for b, n, d in CASES])
def test_kernel_under_the_bound(B, N, D, variant):
    """|out - mult ref| <= |mult| bound + 2^-23 |mult ref| element by element, with and without mult; the ESS within
    (2^-22 + 4 L_b) of the oracle's."""
    x, sigma, X, ref, ref_ess, r = _case(B, N, D, variant)
    bd = ec.bound(x, sigma, X, r)
    L, _ = ec.logit_term(x, sigma, X)
    mult = (-1.0 / sigma.astype(np.float64) * np.random.default_rng(B + N).uniform(0.5, 2.0, B)).astype(np.float32)
    for m in (None, mult):
        out, ess = _launch(x, sigma, X, m)
        assert out.shape == x.shape and out.dtype == np.float32 and ess.shape == (B,) and ess.dtype == np.float32
        scale = np.ones((B, 1)) if m is None else m.astype(np.float64)[:, None]
        want = scale * ref
        allowed = np.abs(scale) * bd + 2.0 ** -23 * np.abs(want)
        err = np.abs(out.astype(np.float64) - want)
        ess_err = np.abs(ess.astype(np.float64) - ref_ess) / ((2.0 ** -22 + 4 * L) * ref_ess)
        ratio = np.divide(err, allowed, out=np.where(err > 0, np.inf, 0.0), where=allowed > 0)     # 0 / 0: an exact zero, allowed
        print(f"B={B} N={N} D={D} {variant} {'mult' if m is not None else 'nomult'}: worst |out - ref| / allowed = "
              f"{float(ratio.max()):.3f} (the arithmetic's share of allowed at most {float((np.abs(scale) * bd / np.maximum(allowed, 1e-300)).max()):.1e}), "
              f"worst ess error / allowed = {float(ess_err.max()):.3f}, ess {float(ref_ess.min()):.3g} .. {float(ref_ess.max()):.3g}")
        assert np.isfinite(out).all() and (err <= allowed).all()
        assert (ess_err <= 1.0).all()


def test_the_regimes_are_what_they_claim():
    """Of the rows of one case: the smallest sigmas leave one point with all the weight, the largest weigh all points alike."""
    x, sigma, X, ref, ref_ess, r = _case(257, 1000, 100, "plain")
    assert (ref_ess[0::3] < 1.001).all() and (ref_ess[2::3] > 990.0).all() and ((ref_ess[1::3] > 1.5) & (ref_ess[1::3] < 900.0)).any()


def test_rows_that_are_not_finite_are_nan_and_alone():
    x, sigma, X, _, _, _ = _case(65, 63, 23, "plain")
    clean, clean_ess = _launch(x, sigma, X)
    spoil = {3: ("x", np.nan), 17: ("x", np.inf), 20: ("sigma", 0.0), 21: ("sigma", -0.3), 37: ("sigma", np.nan), 64: ("x", -np.inf)}
    for rows in [[b] for b in spoil] + [list(spoil)]:
        xs, ss = x.copy(), sigma.copy()
        for b in rows:
            if spoil[b][0] == "x":
                xs[b, (5 * b) % 23] = spoil[b][1]
            else:
                ss[b] = spoil[b][1]
        out, ess = _launch(xs, ss, X)
        bad = np.zeros(65, dtype=bool)
        bad[rows] = True
        assert np.isnan(out[bad]).all() and np.isnan(ess[bad]).all()
        assert np.array_equal(out[~bad].view(np.uint32), clean[~bad].view(np.uint32))
        assert np.array_equal(ess[~bad].view(np.uint32), clean_ess[~bad].view(np.uint32))


def test_same_bits_every_run_and_however_the_rows_are_split():
    x, sigma, X, _, _, _ = _case(257, 1000, 100, "plain")
    mult = (-1.0 / sigma).astype(np.float32)
    a, a_ess = _launch(x, sigma, X, mult)
    b, b_ess = _launch(x, sigma, X, mult)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a_ess.view(np.uint32), b_ess.view(np.uint32))
    lo, lo_ess = _launch(x[:65], sigma[:65], X, mult[:65])
    hi, hi_ess = _launch(x[65:], sigma[65:], X, mult[65:])
    assert np.array_equal(np.concatenate([lo, hi]).view(np.uint32), a.view(np.uint32))
    assert np.array_equal(np.concatenate([lo_ess, hi_ess]).view(np.uint32), a_ess.view(np.uint32))


def test_wrapper_refuses_what_the_kernel_does_not_serve():
    pack = _lib.empirical_pack(torch.zeros(10, 8, device=DEV))
    x, sigma = torch.zeros(4, 8, device=DEV), torch.ones(4, device=DEV)
    with pytest.raises(RuntimeError, match="empirical_score: x"):
        _lib.empirical_score(torch.zeros(4, 9, device=DEV), pack, sigma)
    with pytest.raises(RuntimeError, match="mult holds 3 values for 4 rows"):
        _lib.empirical_score(x, pack, sigma, mult=torch.ones(3, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.empirical_score(x.cpu(), pack, sigma)
    wide = {"Y": torch.zeros(10, 196, device=DEV, dtype=torch.float64), "h": torch.zeros(10, device=DEV, dtype=torch.float64),
            "c": torch.zeros(193, device=DEV, dtype=torch.float64), "N": 10, "D": 193}
    with pytest.raises(RuntimeError, match="is not served"):
        _lib.empirical_score(torch.zeros(4, 193, device=DEV), wide, sigma)
    out, ess = _lib.empirical_score(torch.zeros(0, 8, device=DEV), pack, torch.ones(0, device=DEV))
    assert out.shape == (0, 8) and ess.shape == (0,)


# ------------------------------------------------------------------------------------------- end to end
def test_line_config_end_to_end(tmp_path):
    cfg = read_config(LINE)
    cfg.device = DEV
    cfg.logging.log_path = str(tmp_path)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*effective sample size.*")       # sigma_min = 0.2: no ESS warning
        svd, dims = dim_reduction.get_manifold_dimension(cfg, return_svd=True, return_dims=True)
    print(f"line, sigma_min 0.2: IDs {dims}")
    assert len(dims) == 4 and all(d == 1 for d in dims)


def test_ess_warning_fires_below_the_spacing_of_the_data_only():
    cfg = read_config(LINE)
    cloud = ee.train_split(cfg)
    x = (cloud[:1] + 0.01 * torch.randn(64, 100, generator=torch.Generator().manual_seed(3))).to(DEV)
    labels = torch.zeros(64, device=DEV)
    cfg.model.sigma_min = 0.01
    starved = ee.EmpiricalExact(cfg, data=cloud).to(DEV)
    with pytest.warns(UserWarning, match=r"median effective sample size of a call is 1\.\d\d at sigma = 0\.01"):
        starved(x, labels)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*effective sample size.*")
        starved(x, labels)                                           # once per model
        cfg.model.sigma_min = 0.2
        fed = ee.EmpiricalExact(cfg, data=cloud).to(DEV)
        out = fed(x, labels)
    assert bool(torch.isfinite(out).all()) and float(fed.last_ess.median()) >= 4.0


def _circle_and_sphere_config(tmp_path):
    cfg = read_config('configs/dimension_estimation/paper/euclidean_data/ksphere/union.py')
    cfg.data.ambient_dim, cfg.data.dim, cfg.data.shape = 16, 16, [16]
    cfg.data.manifold_dim, cfg.data.radii, cfg.data.data_samples = [1, 2], [1, 2], 3072
    cfg.model.name, cfg.model.state_size, cfg.model.sigma_min = 'empirical_exact', 16, 0.2
    cfg.logging.svd_points = 13
    cfg.logging.log_path = str(tmp_path)
    cfg.device = DEV
    cfg.seed = 42
    return cfg


def test_circle_beside_a_sphere_end_to_end_and_local_dims_agrees(tmp_path):
    cfg = _circle_and_sphere_config(tmp_path)
    # the points the driver will visit, in its order, and the cloud its model will hold
    torch.manual_seed(cfg.seed)
    from id_diff_amd.lightning_data_modules.utils import create_lightning_datamodule
    dm = create_lightning_datamodule(cfg)
    dm.setup()
    points = dim_reduction.collect_points(dm.train_dataloader(), dim_reduction._num_datapoints(cfg))
    cloud = ee.train_split(cfg).numpy()
    assert len(points) == 12 and cloud.shape == (int(0.8 * 6144), 16)
    xs = np.stack([x.numpy() for x, _ in points])
    want = np.where(np.linalg.norm(xs.astype(np.float64), axis=1) < 1.5, 1, 2)          # radius 1: the circle; radius 2: the sphere
    assert (want == 1).any() and (want == 2).any()
    for p in range(len(points)):                                     # on the CPU first: the rows have neighbours to average over
        got, ess = ec.oracle_id(xs[p], 0.2, cloud, 1501, p)
        assert ess >= 20.0 and got == want[p], f"oracle, point {p}: ID {got}, median ESS {ess:.1f}"
    svd, dims = dim_reduction.get_manifold_dimension(cfg, return_svd=True, return_dims=True)
    print(f"circle + 2-sphere in R^16: driver IDs {dims}, on manifolds of dimension {want.tolist()}")
    assert list(dims) == want.tolist()
    local, ess = empirical.local_dims(cloud, 0.2, points=xs, batchsize=500, seed=cfg.seed)
    assert local.tolist() == list(dims) and (ess >= 20.0).all()
    tangent = empirical.local_tangent(cloud, 0.2, points=xs[:3], batchsize=500, seed=cfg.seed)
    for p, T in enumerate(tangent):
        assert T.shape == (16, want[p]) and np.allclose(T.T @ T, np.eye(want[p]), atol=1e-5)


def test_sigma_from_knn_is_the_host_rule():
    X = ec.circle_and_sphere()
    Xd = X.astype(np.float64)
    sq = (Xd * Xd).sum(axis=1)
    d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * Xd @ Xd.T, 0.0)
    np.fill_diagonal(d2, np.inf)
    want = float(np.median(np.sqrt(np.partition(d2, 19, axis=1)[:, 19])))
    assert abs(empirical.sigma_from_knn(X, 20) - want) <= 1e-6 * want


def test_run_writes_the_pickle_and_prints_the_histogram(tmp_path, capsys):
    import pickle
    cfg = read_config(LINE)
    dims = empirical.run(cfg, sigma=0.2, points=np.arange(3), out_dir=str(tmp_path / "empirical"))
    assert dims.tolist() == [1, 1, 1]
    with open(tmp_path / "empirical" / "local_dims.pkl", "rb") as f:
        saved = pickle.load(f)
    assert saved["dims"].tolist() == [1, 1, 1] and saved["sigma"] == 0.2 and saved["batchsize"] == 500 and (saved["ess_median"] >= 4.0).all()
    assert "dim   1: 3" in capsys.readouterr().out
