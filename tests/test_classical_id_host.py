"""Host side of the classical ID estimators (mle.py, benchmark.py): the arithmetic given neighbour distances or
covariance eigenvalues, against the reference's results in tests/golden/classical_id.npz (make_classical_id.py)."""
import math

import numpy as np
import pytest

import id_diff_amd
from id_diff_amd import benchmark, mle

SETS = ("a", "b")


def full_dist(z, s):
    d = z[f"{s}::dist"]
    return np.concatenate([np.zeros((d.shape[0], 1)), d], axis=1)      # the reference's layout: self column first


@pytest.mark.parametrize("s", SETS)
def test_mle_with_given_dist_reproduces_the_reference(golden, s):
    z = golden("classical_id.npz")
    dist = full_dist(z, s)
    X = np.zeros((dist.shape[0], 1))                                     # only X.shape[0] is read when dist is given
    np.testing.assert_allclose(mle.intrinsic_dim_sample_wise(X, k=5, dist=dist), z[f"{s}::sw5"], rtol=1e-12)
    np.testing.assert_allclose(mle.intrinsic_dim_scale_interval(X, 10, 20, dist=dist), z[f"{s}::si"], rtol=1e-12)


@pytest.mark.parametrize("s", SETS)
def test_bootstrap_subsets_and_results_for_the_seed(golden, s, monkeypatch):
    z = golden("classical_id.npz")
    dist = full_dist(z, s)
    N = dist.shape[0]
    off, idx = z[f"{s}::boot_off"], z[f"{s}::boot_idx"]
    rng = np.random.RandomState(0)
    for i in range(len(off) - 1):
        np.testing.assert_array_equal(np.unique(rng.randint(0, N - 1, size=N)), idx[off[i]:off[i + 1]])
    assert N - 1 not in idx                                              # the reference never draws the last point
    monkeypatch.setattr(mle, "neighbour_distances", lambda X, k: dist[:, :k + 1])
    X = np.zeros((N, 1))
    res, Rs = mle.bootstrap_intrinsic_dim_scale_interval(X, nb_iter=10, random_state=0, average=False)
    assert res.shape == (10, 11)
    np.testing.assert_allclose(res, z[f"{s}::boot_F"], rtol=1e-12)
    np.testing.assert_allclose(Rs, z[f"{s}::Rs"], rtol=1e-12)
    mean, Rs2 = mle.bootstrap_intrinsic_dim_scale_interval(X, nb_iter=10, random_state=0, average=True)
    np.testing.assert_allclose(mean, z[f"{s}::boot_T"], rtol=1e-12)
    assert Rs2 == Rs


@pytest.mark.parametrize("s", SETS)
def test_ppca_rank_and_loglik_match_the_fixture(golden, s):
    z = golden("classical_id.npz")
    ev, N = z[f"{s}::ppca_ev"], z[f"{s}::dist"].shape[0]
    ll, ref = benchmark.ppca_loglik(ev, N), z[f"{s}::ppca_ll"]
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(np.isfinite(ll), fin)
    np.testing.assert_allclose(ll[fin], ref[fin], rtol=1e-10)
    assert benchmark.ppca_rank(ev, N) == int(z[f"{s}::ppca_n"])


@pytest.mark.parametrize("D,N,cut", [(12, 40, 3), (80, 300, 20), (200, 220, 0)])
def test_ppca_matches_sklearn_infer_dimension(D, N, cut):
    pca = pytest.importorskip("sklearn.decomposition._pca")
    rng = np.random.default_rng(D)
    X = rng.standard_normal((N, D))
    if cut:
        X[:, cut:] *= 0.03
    X -= X.mean(0)
    ev = np.linalg.svd(X, compute_uv=False) ** 2 / (N - 1)
    ev[-3:] = [1e-16, 5e-17, 0.0] if D > 100 else ev[-3:]                  # the 1e-15 rules: ranks sklearn does not score
    ll = benchmark.ppca_loglik(ev, N)
    ref = np.array([-np.inf] + [pca._assess_dimension(ev, r, N) for r in range(1, D)])
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(np.isfinite(ll), fin)
    np.testing.assert_allclose(ll[fin], ref[fin], rtol=1e-10)
    assert benchmark.ppca_rank(ev, N) == int(pca._infer_dimension(ev, N))


def test_ppca_refuses_fewer_samples_than_features():
    with pytest.raises(ValueError, match="only supported if n_samples >= n_features"):
        benchmark.ppca_dim(np.zeros((10, 20), dtype=np.float32))


def test_pca_fo_count():
    lam = np.array([10.0, 4.0, 0.6, 0.51, 0.5, 0.0])
    assert benchmark.pca_fo_count(lam) == 4                   # > 0.05 * 10, strictly
    assert benchmark.pca_fo_count(lam, alpha=0.3) == 2
    assert benchmark.pca_fo_count(lam[::-1].copy()) == 4      # the largest need not come first


def test_mle_aggregations_by_hand():
    # two points, k = 3: T = (1, 2, 4) and (1, 1, e)
    T = np.array([[1.0, 2.0, 4.0], [1.0, 1.0, math.e]])
    s = np.array([math.log(4.0) + math.log(2.0), 2.0])
    m = 2.0 / s
    assert benchmark.mle_aggregate(T, 3) == pytest.approx(1.0 / np.mean(1.0 / m), rel=1e-15)
    assert benchmark.mle_aggregate(T, 3, 'mean') == pytest.approx(np.mean(m), rel=1e-15)
    assert benchmark.mle_aggregate(T, 3, 'robust') == pytest.approx(np.median(m), rel=1e-15)
    assert benchmark.mle_aggregate(T, 3, unbiased=True) == pytest.approx(1.0 / np.mean(s), rel=1e-15)
    with pytest.raises(ValueError, match="aggregation"):
        benchmark.mle_aggregate(T, 3, 'mode')


def test_zero_distances_raise():
    dist = np.array([[0.0, 1.0, 2.0, 3.0], [0.0, 0.0, 2.0, 3.0], [0.0, 0.0, 0.0, 3.0]])
    with pytest.raises(ValueError, match="2 points have a zero distance"):
        mle.intrinsic_dim_sample_wise(np.zeros((3, 1)), k=3, dist=dist)
