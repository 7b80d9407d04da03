"""Host side of the empirical score (no GPU): ``reference_score`` against closed forms, the error bound the fused kernel is held to
(tests/empirical_cases.py) validated on the kernel's arithmetic restated in numpy, the intrinsic dimension through the oracle, and
what the C entry points and the model refuse before any device call."""
import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd import _lib, dim_reduction, empirical
from id_diff_amd.configs.utils import read_config
from id_diff_amd.lightning_data_modules.utils import create_lightning_datamodule
from id_diff_amd.models import empirical_exact as ee
from id_diff_amd.models import utils as mutils

import empirical_cases as ec

LINE = 'configs/dimension_estimation/paper/euclidean_data/line/empirical.py'
CAP = 192


@pytest.fixture(scope="module")
def line():
    return ec.line_cloud()


# ------------------------------------------------------------------------------------------- reference_score against closed forms
def test_one_point_gives_the_difference_and_ess_one():
    rng = np.random.default_rng(0)
    X, x = rng.standard_normal((1, 7)), rng.standard_normal((5, 7))
    out, ess, r = ee.reference_score(x, rng.uniform(0.01, 3.0, 5), X)
    np.testing.assert_allclose(out, X - x, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(ess, 1.0)
    np.testing.assert_allclose(r, np.linalg.norm(X - x, axis=1), rtol=1e-15)


def test_two_points_on_the_bisector_give_the_midpoint_and_ess_two():
    a, b = np.array([1.0, 0.0, 0.0]), np.array([-1.0, 0.0, 0.0])
    x = np.array([[0.0, 0.7, -0.3], [0.0, -2.0, 5.0]])
    out, ess, _ = ee.reference_score(x, [0.3, 2.0], np.stack([a, b]))
    np.testing.assert_allclose(out, 0.5 * (a + b) - x, rtol=0, atol=1e-15)
    np.testing.assert_allclose(ess, 2.0, rtol=1e-15)


def test_a_huge_sigma_gives_the_mean_and_ess_n():
    rng = np.random.default_rng(1)
    X, x = rng.standard_normal((300, 5)), rng.standard_normal((4, 5))
    out, ess, r = ee.reference_score(x, 1e6, X)
    np.testing.assert_allclose(out, X.mean(axis=0) - x, rtol=0, atol=1e-10)
    np.testing.assert_allclose(ess, 300.0, rtol=1e-10)
    np.testing.assert_allclose(r, np.linalg.norm(X[None] - x[:, None], axis=2).max(axis=1), rtol=1e-15)


def test_duplicating_every_point_doubles_the_ess_and_nothing_else():
    rng = np.random.default_rng(2)
    X, x = rng.standard_normal((200, 6)), rng.standard_normal((8, 6))
    sigma = rng.uniform(0.2, 2.0, 8)
    out, ess, r = ee.reference_score(x, sigma, X)
    out2, ess2, r2 = ee.reference_score(x, sigma, np.concatenate([X, X]))
    np.testing.assert_allclose(out2, out, rtol=0, atol=1e-14)
    np.testing.assert_allclose(ess2, 2.0 * ess, rtol=1e-13)
    assert (r2 <= r).all()                                           # every weight halves, so the 2^-60 floor can only cut sooner


# ------------------------------------------------------------------------------------------- the bound, on the kernel's arithmetic
@pytest.mark.parametrize("name", ["line", "sphere", "sphere+1000"])
def test_bound_holds_for_the_expanded_arithmetic(name, line):
    """48 rows a cloud, sigma in {0.01, 0.1, 1} U(0.5, 2) row by row: centre, expand, q @ Y.T - h in fp64 against direct differences
    in long double.  Prints how loose the bound is and how small it is against the row."""
    X = {"line": lambda: line, "sphere": lambda: ec.sphere_cloud(4096, 2, 16, 3),
         "sphere+1000": lambda: ec.sphere_cloud(4096, 2, 16, 3, offset=1000.0)}[name]()
    x, sigma = ec.rows_near(X, 48, [0.01, 0.1, 1.0], 5)
    got, ess = ec.expanded_score(x, sigma, X)
    ref, ref_ess, r = ec.oracle(x, sigma, X)
    bd = ec.bound(x, sigma, X, r)
    err = np.abs(got - ref)
    L, _ = ec.logit_term(x, sigma, X)
    print(f"{name}: worst error / bound {float((err / bd).max()):.2e}, worst bound / largest entry of the row "
          f"{float((bd[:, 0] / np.abs(ref).max(axis=1)).max()):.2e}, worst ess error / its bound "
          f"{float((np.abs(ess - ref_ess) / ((2.0 ** -22 + 4 * L) * ref_ess)).max()):.2e}")
    assert (err <= bd).all()
    assert (bd[:, 0] <= 1e-5 * np.abs(ref).max(axis=1)).all()        # a bound that a wrong tile or mask cannot hide under
    assert (np.abs(ess - ref_ess) <= (2.0 ** -22 + 4 * L) * ref_ess).all()


# ------------------------------------------------------------------------------------------- the ID through the oracle
def _driver_points(cfg):
    torch.manual_seed(int(cfg.get('seed', 42)))
    dm = create_lightning_datamodule(cfg)
    dm.setup()
    return dim_reduction.collect_points(dm.train_dataloader(), dim_reduction._num_datapoints(cfg))


def test_line_config_reports_one_at_the_drivers_points_and_starves_at_a_hundredth(line):
    cfg = read_config(LINE)
    assert cfg.model.name == 'empirical_exact' and cfg.model.sigma_min == 0.2
    points = _driver_points(cfg)
    assert len(points) == 4
    rows = dim_reduction.batching(tuple(points[0][0].shape), points[0][1])[2]
    assert rows == 1501
    for p, (x, _) in enumerate(points):
        got, ess = ec.oracle_id(x.numpy(), 0.2, line, rows, 100 + p)
        print(f"line point {p}: ID {got}, median ESS {ess:.1f}")
        assert got == 1 and ess >= 4.0
    # the restatement the IDs above went through, on rows of the same kind, against the direct-difference oracle
    xs = (points[0][0].numpy()[None, :] + 0.2 * np.random.default_rng(9).standard_normal((6, 100))).astype(np.float32)
    ref, ref_ess, r = ec.oracle(xs, 0.2, line)
    assert (np.abs(ec.expanded_score(xs, 0.2, line)[0] - ref) <= ec.bound(xs, 0.2, line, r)).all()
    # sigma below the spacing of the data: the condition of the model's warning
    _, starved = ec.oracle_id(points[0][0].numpy(), 0.01, line, rows, 100)
    print(f"line at sigma 0.01: median ESS {starved:.2f}")
    assert starved < 4.0


def _host_kth_distance(X, k):
    X = X.astype(np.float64)
    sq = (X * X).sum(axis=1)
    d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * X @ X.T, 0.0)
    np.fill_diagonal(d2, np.inf)
    return np.sqrt(np.partition(d2, k - 1, axis=1)[:, k - 1])


def test_circle_and_sphere_report_one_and_two():
    X = ec.circle_and_sphere()
    knn_sigma = empirical.sigma_rule(_host_kth_distance(X, 20))
    print(f"circle + 2-sphere: sigma from the 20th neighbour {knn_sigma:.3f}")
    assert 0.05 < knn_sigma < 0.4
    for sigma in (0.1, knn_sigma):
        for want, first in ((1, 0), (2, 1024)):
            for i in range(first, first + 6):
                got, ess = ec.oracle_id(X[i], sigma, X, 1501, i)
                assert got == want, f"sigma {sigma:.3f}, point {i}: ID {got} (median ESS {ess:.1f}), on a {want}-manifold"


# ------------------------------------------------------------------------------------------- the C ABI and the model's refusals
def test_ok_truth_table():
    assert _lib.empirical_score_ok(1, 1) and _lib.empirical_score_ok(8000, 100) and _lib.empirical_score_ok(40000, 128)
    assert _lib.empirical_score_ok(1, CAP)
    assert not _lib.empirical_score_ok(1, 0) and not _lib.empirical_score_ok(0, 1) and not _lib.empirical_score_ok(100, CAP + 1)
    assert not _lib.empirical_score_ok(-5, 10) and not _lib.empirical_score_ok(1 << 31, 10) and not _lib.empirical_score_ok(4000, 1024)


_A, _B, _C, _D, _E, _F, _G, _H = (0x10000 * i for i in range(1, 9))       # fabricated addresses: a call let through would fault
_CALL = lambda x=_A, Y=_B, h=_C, c=_D, sigma=_E, mult=_F, out=_G, ess=_H, B=4, N=100, D=3: [x, Y, h, c, sigma, mult, out, ess, B, N, D]
_REFUSED = {
    "null_x": _CALL(x=0), "null_Y": _CALL(Y=0), "null_h": _CALL(h=0), "null_c": _CALL(c=0), "null_sigma": _CALL(sigma=0),
    "null_out": _CALL(out=0), "negative_B": _CALL(B=-1), "N0": _CALL(N=0), "D0": _CALL(D=0), "D_above_cap": _CALL(D=CAP + 1),
    "N_above_limit": _CALL(N=1 << 31), "misaligned_Y": _CALL(Y=_B + 8), "misaligned_x": _CALL(x=_A + 2),
    "null_x_at_B0": _CALL(x=0, B=0),
}


@pytest.mark.parametrize("case", sorted(_REFUSED))
def test_entry_point_refuses_before_any_device_call(case):
    handle = _lib.lib()
    assert handle.idiff_empirical_score_f32(*_REFUSED[case], None) == 1001       # IDIFF_EINVAL
    assert handle.idiff_last_error().decode().startswith("empirical_score: ")


def test_model_refuses_a_dimension_over_the_cap():
    cfg = read_config(LINE)
    with pytest.raises(NotImplementedError, match=f"D <= {CAP}"):
        ee.EmpiricalExact(cfg, data=np.zeros((10, CAP + 1), dtype=np.float32))
    with pytest.raises(NotImplementedError, match=f"D <= {CAP}"):
        ee.EmpiricalExact(cfg, data=np.zeros((10, 1, 32, 32), dtype=np.float32))      # images flatten to D = 1024
    model = ee.EmpiricalExact(cfg, data=np.zeros((10, 2, 96), dtype=np.float64))
    assert tuple(model.cloud.shape) == (10, CAP) and model.cloud.dtype == torch.float32 and not model.cloud.requires_grad


def test_constructor_takes_the_drivers_split_and_leaves_the_rng_alone():
    cfg = read_config(LINE)
    torch.manual_seed(int(cfg.seed))
    dm = create_lightning_datamodule(cfg)
    dm.setup()
    want = dm.train_data.dataset.data[torch.as_tensor(dm.train_data.indices)]
    torch.manual_seed(777)
    before = torch.random.get_rng_state()
    model = mutils.create_model(cfg)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert isinstance(model, ee.EmpiricalExact) and model.ess_warn == 4.0
    assert tuple(model.cloud.shape) == (8000, 100) and torch.equal(model.cloud.data, want)
