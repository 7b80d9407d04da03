"""Host side of the empirical score's Jacobian (no GPU): the long-double oracle of C(x, sigma) against closed forms and against a
finite difference of ``reference_score``, the error bound the kernel is held to (tests/empirical_jacobian_cases.py) validated on the
kernel's arithmetic restated in numpy and shown to catch planted bugs, the rules that read dimensions off the spectra, the dimensions
of the line and of a circle beside a 2-sphere, and what the C entry points and the wrapper refuse before any device call."""
import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd import _lib, empirical
from id_diff_amd.models import empirical_exact as ee

import empirical_cases as ec
import empirical_jacobian_cases as jc

CAP = jc.CAP


# ------------------------------------------------------------------------------------------- the oracle against closed forms
def test_one_point_gives_zero_and_ess_one():
    rng = np.random.default_rng(0)
    X, x = rng.standard_normal((1, 7)).astype(np.float32), rng.standard_normal((5, 7)).astype(np.float32)
    C, mean, ess, r, R = jc.oracle(x, rng.uniform(0.01, 3.0, 5), X)
    np.testing.assert_array_equal(C, 0.0)
    np.testing.assert_allclose(mean, X.astype(np.float64) - x, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(ess, 1.0)
    np.testing.assert_allclose(r, R, rtol=0, atol=0)


def test_two_points_on_the_bisector_give_a_rank_one_c_and_ess_two():
    a = 0.75
    X = np.array([[a, 0.0, 0.0], [-a, 0.0, 0.0]], dtype=np.float32)
    x = np.array([[0.0, 0.5, -0.25], [0.0, -2.0, 5.0]], dtype=np.float32)
    sigma = np.array([0.5, 2.0])
    C, mean, ess, _, _ = jc.oracle(x, sigma, X)
    want = np.zeros((2, 3, 3))
    want[:, 0, 0] = a * a / (sigma * sigma)
    np.testing.assert_allclose(C, want, rtol=0, atol=1e-15)
    np.testing.assert_allclose(mean, -x, rtol=0, atol=1e-15)
    np.testing.assert_allclose(ess, 2.0, rtol=1e-15)


def test_a_huge_sigma_gives_the_population_covariance_and_ess_n():
    rng = np.random.default_rng(1)
    X, x = rng.standard_normal((300, 5)).astype(np.float32), rng.standard_normal((4, 5)).astype(np.float32)
    C, mean, ess, _, _ = jc.oracle(x, 1e6, X)
    np.testing.assert_allclose(C * 1e12, np.broadcast_to(np.cov(X.astype(np.float64).T, bias=True), (4, 5, 5)), rtol=0, atol=1e-9)
    np.testing.assert_allclose(ess, 300.0, rtol=1e-10)


def test_duplicating_every_point_doubles_the_ess_and_nothing_else():
    rng = np.random.default_rng(2)
    X, x = rng.standard_normal((200, 6)).astype(np.float32), rng.standard_normal((8, 6)).astype(np.float32)
    sigma = rng.uniform(0.2, 2.0, 8)
    C, mean, ess, _, _ = jc.oracle(x, sigma, X)
    C2, mean2, ess2, _, _ = jc.oracle(x, sigma, np.concatenate([X, X]))
    np.testing.assert_allclose(C2, C, rtol=0, atol=1e-13 * np.abs(C).max())
    np.testing.assert_allclose(mean2, mean, rtol=0, atol=1e-14)
    np.testing.assert_allclose(ess2, 2.0 * ess, rtol=1e-13)


# ------------------------------------------------------------------------------------------- the identity
def test_c_minus_identity_is_sigma_squared_times_the_jacobian_of_the_score():
    """A central difference of ``reference_score`` in long double, step 1e-6 sigma, column by column."""
    X = ec.sphere_cloud(300, 2, 6, 11)
    x, sigma = ec.rows_near(X, 5, [0.3], 12)
    C = jc.oracle(x, sigma, X)[0]
    Xl = X.astype(np.longdouble)
    for b in range(5):
        h = np.longdouble(1e-6) * np.longdouble(sigma[b])
        J = np.empty((6, 6))
        for j in range(6):
            e = np.zeros(6, dtype=np.longdouble)
            e[j] = h
            hi = ee.reference_score((x[b].astype(np.longdouble) + e)[None], np.longdouble(sigma[b]), Xl)[0][0]
            lo = ee.reference_score((x[b].astype(np.longdouble) - e)[None], np.longdouble(sigma[b]), Xl)[0][0]
            J[:, j] = ((hi - lo) / (2 * h)).astype(np.float64)
        err = np.abs(J - (C[b] - np.eye(6))).max()
        print(f"query {b}: sigma {sigma[b]:.3f}, |C| {np.abs(C[b]).max():.3f}, finite difference off by {err:.2e}")
        assert err <= 1e-5 * np.abs(C[b]).max()


# ------------------------------------------------------------------------------------------- the bound, on the kernel's arithmetic
HOST_SHAPES = [s for s in jc.SHAPES if s[1] <= 1000]


def _errors(got, x, sigma, X, ref):
    """(worst error / bound of C, of mean, of ess) of (C, mean, ess) ``got`` against the oracle tuple ``ref``."""
    C, mean, ess, r, R = ref
    bc, bm, be = jc.bound(sigma, X.shape[0], X.shape[1], r, R)
    return (jc.worst_ratio(np.abs(got[0] - C), bc), jc.worst_ratio(np.abs(got[1] - mean), bm),
            jc.worst_ratio(np.abs(got[2] - ess), be * ess))


@pytest.mark.parametrize("variant", jc.VARIANTS)
@pytest.mark.parametrize("B,N,D", HOST_SHAPES, ids=[f"B{b}-N{n}-D{d}" for b, n, d in HOST_SHAPES])
def test_restated_arithmetic_stays_under_a_tenth_of_the_bound(B, N, D, variant):
    x, sigma, X, *ref = jc.case(B, N, D, variant)
    worst = _errors(jc.restated(x, sigma, X), x, sigma, X, ref)
    print(f"B={B} N={N} D={D} {variant}: worst error / bound: C {worst[0]:.2e}, mean {worst[1]:.2e}, ess {worst[2]:.2e}")
    assert max(worst) <= 0.1


@pytest.mark.parametrize("mutate", ["drop", "no_mm", "pad"])
def test_a_planted_bug_exceeds_the_bound_a_thousand_times(mutate):
    worst = 0.0
    for B, N, D in [(17, 33, 5), (4, 1000, 100)]:
        x, sigma, X, *ref = jc.case(B, N, D, "plain")
        worst = max(worst, _errors(jc.restated(x, sigma, X, mutate=mutate), x, sigma, X, ref)[0])
    print(f"{mutate}: worst |C - ref| / bound {worst:.2e}")
    assert worst >= 1e3


# ------------------------------------------------------------------------------------------- the rules
def test_dims_from_jacobian_rules():
    eig = np.array([[[1.1, 0.9, 0.51, 0.5, 0.0], [0.4, 0.3, 0.0, 0.0, 0.0]],
                    [[1.0, 0.98, 0.2, 0.1, 0.0], [1.0, 1.0, 1.0, 1.0, 0.9]]])
    half = empirical.dims_from_jacobian(eig)
    assert half.dtype == np.int64 and half.tolist() == [[3, 0], [2, 5]]
    assert empirical.dims_from_jacobian(eig, rule='gap').tolist() == [[4, 2], [2, 4]]
    assert empirical.dims_from_jacobian(np.array([0.9, 0.1, 0.0])).tolist() == 1
    bad = eig.copy()
    bad[1, 0, 2] = np.nan
    with pytest.raises(ValueError, match="1 of 4 spectra are not finite"):
        empirical.dims_from_jacobian(bad)
    with pytest.raises(ValueError, match="unknown rule"):
        empirical.dims_from_jacobian(eig, rule='knee')


def test_stable_dims_takes_the_longest_qualifying_run():
    sg = np.array([0.1, 0.2, 0.4, 0.8, 1.6, 3.2])
    dims = np.array([[0, 1, 1, 1, 2, 2],           # the run of ones
                     [1, 1, 2, 2, 3, 3],           # three runs of two: the one at the smallest sigma
                     [1, 1, 1, 1, 2, 2],           # a gap in the qualifying bandwidths cuts the run of ones in two: the twos tie, smaller wins
                     [1, 1, 1, 1, 1, 1],           # nothing qualifies
                     [3, 2, 2, 2, 2, 1]])          # only the ends qualify: two runs of one, the smaller sigma
    ess = np.array([[20, 20, 20, 20, 20, 20],
                    [16, 16, 16, 16, 16, 16],
                    [30, 30, 5, 30, 30, 30],
                    [1, 2, 3, 15.9, np.nan, 4],
                    [99, 3, 3, 3, 3, 99]], dtype=np.float64)
    got, rng = empirical.stable_dims(dims, ess, sg, ess_min=16.0)
    assert got.dtype == np.int64 and got.tolist() == [1, 1, 1, -1, 3]
    np.testing.assert_array_equal(rng, [[0.2, 0.8], [0.1, 0.2], [0.1, 0.2], [np.nan, np.nan], [0.1, 0.1]])
    got, rng = empirical.stable_dims(dims, ess, sg, ess_min=25.0)
    assert got.tolist() == [-1, -1, 1, -1, 3]
    np.testing.assert_array_equal(rng[2], [0.1, 0.2])
    assert empirical.ESS_MIN == 32.0                                 # the default: only row 4 still has bandwidths that qualify
    assert empirical.stable_dims(dims, ess, sg)[0].tolist() == [-1, -1, -1, -1, 3]


def test_sigma_grid_is_eleven_half_octaves_around_the_knn_value(monkeypatch):
    monkeypatch.setattr(empirical, "sigma_from_knn", lambda X, k=20: 0.3 if k == 20 else 1.0)
    grid = empirical.sigma_grid(None)
    assert grid.shape == (11,)
    np.testing.assert_allclose(grid, 0.3 * 2.0 ** (np.arange(-4, 7) / 2.0), rtol=1e-15)
    np.testing.assert_allclose(empirical.sigma_grid(None, k=5, lo=-1.0, hi=1.0, per_octave=1), [0.5, 1.0, 2.0], rtol=1e-15)


# ------------------------------------------------------------------------------------------- the findings
def test_circle_and_sphere_read_one_and_two_at_three_bandwidths():
    X, x, refs, want = jc.circle_and_sphere_case()
    closest, least = np.inf, np.inf
    for sigma, ref in zip(jc.CS_SIGMAS, refs):
        for C, ess in ((ref[0], ref[2]), jc.restated(x, sigma, X)[::2]):
            eig = np.linalg.eigvalsh(C)[:, ::-1]
            assert empirical.dims_from_jacobian(eig).tolist() == want.tolist(), f"sigma {sigma}"
            closest, least = min(closest, float(np.abs(eig - 0.5).min())), min(least, float(ess.min()))
    print(f"circle + 2-sphere: 96 of 96 right, no eigenvalue closer to 0.5 than {closest:.3f}, smallest ESS {least:.1f}")
    assert closest >= 0.2


def test_line_reads_one_at_its_first_hundred_points():
    X = ec.line_cloud()
    for sigma in (0.4, 0.8):
        C, _, ess = jc.restated(X[:100], sigma, X)
        eig = np.linalg.eigvalsh(C)[:, ::-1]
        dims = empirical.dims_from_jacobian(eig)
        print(f"line, sigma {sigma}: {int((dims == 1).sum())} of 100 read 1, closest eigenvalue to 0.5 at {float(np.abs(eig - 0.5).min()):.3f}, "
              f"smallest ESS {float(ess.min()):.1f}")
        assert (dims == 1).all()


# ------------------------------------------------------------------------------------------- the C ABI and the wrapper's refusals
def test_ok_truth_table():
    assert _lib.empirical_jacobian_ok(1, 1) and _lib.empirical_jacobian_ok(8000, 100) and _lib.empirical_jacobian_ok(1, CAP)
    assert not _lib.empirical_jacobian_ok(100, CAP + 1) and not _lib.empirical_jacobian_ok(0, 1)
    assert not _lib.empirical_jacobian_ok(1 << 31, 10)
    assert _lib.empirical_jacobian_ok((1 << 31) - 33, 10) and not _lib.empirical_jacobian_ok((1 << 31) - 32, 10)
    assert _lib.JACOBIAN_D_MAX == CAP


_A, _B, _C, _D, _E, _F = (0x10000 * i for i in range(1, 7))              # fabricated addresses: a call let through would fault
_CALL = lambda x=_A, X=_B, sigma=_C, C=_D, mean=_E, ess=_F, B=4, N=100, D=3: [x, X, sigma, C, mean, ess, B, N, D]
_REFUSED = {
    "null_x": _CALL(x=0), "null_X": _CALL(X=0), "null_sigma": _CALL(sigma=0), "null_C": _CALL(C=0), "null_mean": _CALL(mean=0),
    "null_ess": _CALL(ess=0), "negative_B": _CALL(B=-1), "N0": _CALL(N=0), "D0": _CALL(D=0), "D_above_cap": _CALL(D=CAP + 1),
    "N_above_limit": _CALL(N=1 << 31), "misaligned_x": _CALL(x=_A + 2), "misaligned_X": _CALL(X=_B + 1), "misaligned_C": _CALL(C=_D + 4),
    "misaligned_mean": _CALL(mean=_E + 4), "misaligned_ess": _CALL(ess=_F + 2), "null_x_at_B0": _CALL(x=0, B=0),
}


@pytest.mark.parametrize("case", sorted(_REFUSED))
def test_entry_point_refuses_before_any_device_call(case):
    handle = _lib.lib()
    assert handle.idiff_empirical_jacobian_f64(*_REFUSED[case], None) == 1001    # IDIFF_EINVAL
    assert handle.idiff_last_error().decode().startswith("empirical_jacobian: ")


def test_b0_with_good_pointers_is_a_no_op():
    assert _lib.lib().idiff_empirical_jacobian_f64(*_CALL(B=0), None) == 0


def test_wrappers_have_no_cpu_path():
    x, X, sigma = torch.zeros(4, 8), torch.zeros(10, 8), torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.empirical_jacobian(x, X, sigma)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.sym_eigvals_batched(torch.zeros(2, 3, 3, dtype=torch.float64))
