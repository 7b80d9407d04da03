"""Host side of FLIPD on the empirical score (no GPU): the long-double oracle against closed forms and against the identity
sum_i w_i r_i^2 / sigma^2 = tr C + |m|^2 / sigma^2 with the oracle of the empirical Jacobian, the error bound the kernel is held to
(tests/empirical_flipd_cases.py) validated on the kernel's order of operations restated in numpy and shown to catch eight planted
bugs, the acceptance readings (circle 1, 2-sphere 2 at all 4096 points, D = 16 and D = 1024), the default split, ``flipd_dims``, and
what the C entry points refuse before any device call."""
import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd import _lib, empirical
from id_diff_amd.empirical import flipd_curve, flipd_dims  # noqa: F401  (every test here is about them and their kernel)

import empirical_cases as ec
import empirical_flipd_cases as fc
import empirical_jacobian_cases as jc


# ------------------------------------------------------------------------------------------- the oracle against closed forms
def test_one_point_reads_its_squared_distance_over_sigma_squared():
    rng = np.random.default_rng(0)
    X, x = rng.standard_normal((1, 7)).astype(np.float32), rng.standard_normal((5, 7)).astype(np.float32)
    sg = np.array([0.3, 2.0])
    flipd, ess, r, R = fc.oracle(x, sg, X)
    d2 = ((X.astype(np.float64) - x) ** 2).sum(axis=1)
    np.testing.assert_allclose(flipd, d2[:, None] / (sg * sg)[None, :], rtol=1e-15)
    np.testing.assert_array_equal(ess, 1.0)
    np.testing.assert_allclose(r, np.sqrt(d2)[:, None] * np.ones(2), rtol=1e-15)
    assert np.isnan(fc.oracle(x, sg, X, exclude=np.zeros(5, dtype=int))[0]).all()          # nothing admissible


def test_a_query_among_coincident_points_reads_zero_and_a_huge_sigma_reads_the_mean_square_distance():
    X = np.repeat(np.array([[1.0, 2.0, 3.0]], dtype=np.float32), 4, axis=0)
    flipd, ess, _, _ = fc.oracle(X[:1], [0.5], X)
    assert flipd[0, 0] == 0.0 and ess[0, 0] == 4.0
    rng = np.random.default_rng(1)
    X, x = rng.standard_normal((300, 5)).astype(np.float32), rng.standard_normal((3, 5)).astype(np.float32)
    flipd, ess, _, _ = fc.oracle(x, [1e6], X)
    want = ((X.astype(np.float64)[None] - x[:, None]) ** 2).sum(axis=2).mean(axis=1) / 1e12
    np.testing.assert_allclose(flipd[:, 0], want, rtol=1e-9)
    np.testing.assert_allclose(ess, 300.0, rtol=1e-10)


def test_flipd_is_the_trace_of_c_plus_the_squared_mean_over_sigma_squared():
    """The two closed forms of D + sigma^2 (tr grad s + |s|^2): tr C = D + sigma^2 tr grad s and m = sigma^2 s."""
    for B, N, D in [(17, 33, 5), (5, 65, 16), (4, 1000, 100)]:
        x, sigma, X, C, mean, ess, _, _ = jc.case(B, N, D, "plain")
        for b in range(B):
            flipd, fess, _, _ = fc.oracle(x[b:b + 1], [sigma[b]], X)
            s2 = float(sigma[b]) ** 2
            want = np.trace(C[b]) + (mean[b] ** 2).sum() / s2
            assert abs(flipd[0, 0] - want) <= 1e-11 * max(1.0, abs(want)), (B, N, D, b)
            assert abs(fess[0, 0] - ess[b]) <= 1e-12 * ess[b]


# ------------------------------------------------------------------------------------------- the bound, on the kernel's arithmetic
def _worst(got, x, sg, X, ref):
    flipd, ess, r, R = ref
    bf, be = fc.bound(x, sg, X, r, R)
    return fc.worst_ratio(np.abs(got[0] - flipd), bf), fc.worst_ratio(np.abs(got[1] - ess), be * ess)


@pytest.mark.parametrize("variant", fc.VARIANTS)
@pytest.mark.parametrize("P,N,D,S", fc.SHAPES, ids=[f"P{p}-N{n}-D{d}-S{s}" for p, n, d, s in fc.SHAPES])
def test_restated_arithmetic_stays_under_a_tenth_of_the_bound(P, N, D, S, variant):
    worst = (0.0, 0.0)
    for regime in fc.REGIMES:
        for mode in fc.EXCLUDES if N > 1 else ["none"]:
            x, X, sg, ex, *ref = fc.case(P, N, D, S, variant, regime, mode)
            assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
            for splits in fc.SPLITS:
                w = _worst(fc.restated(x, sg, X, ex, splits), x, sg, X, ref)
                worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    print(f"P={P} N={N} D={D} S={S} {variant}: worst error / bound: flipd {worst[0]:.2e}, ess {worst[1]:.2e}")
    assert max(worst) <= 0.1


# (shape, regime, exclusion, splits) on which each planted bug must show: N = 33 is no multiple of the tile, N = 2 < 7 leaves empty
# ranges, the bandwidths of regime 0.1 spread the weight over a neighbourhood
_WHERE = {"drop": [((17, 33, 5, 3), 0.1, "none", 2), ((4, 1000, 100, 11), 0.1, "none", 7)],
          "no_exclude": [((17, 33, 5, 3), 0.1, "first", 2), ((4, 1000, 100, 11), 0.1, "last", 7)],
          "pad": [((17, 33, 5, 3), 0.1, "none", 1), ((4, 1000, 100, 11), 0.1, "none", 7)],
          "lost_range": [((17, 33, 5, 3), 0.1, "none", 2), ((4, 1000, 100, 11), 0.1, "none", 7)],
          "empty_zero": [((3, 2, 3, 2), 0.1, "none", 7), ((3, 2, 3, 2), 0.1, "last", 2)],
          "no_rescale": [((4, 1000, 100, 11), 0.1, "none", 1), ((4, 1000, 100, 11), 0.1, "none", 7)],
          "no_sigma2": [((17, 33, 5, 3), 0.1, "none", 2), ((4, 1000, 100, 11), 0.1, "none", 7)],
          "ess_raw": [((17, 33, 5, 3), 0.1, "none", 2), ((4, 1000, 100, 11), 0.1, "none", 7)]}


@pytest.mark.parametrize("mutate", fc.MUTATIONS)
def test_a_planted_bug_exceeds_the_bound_a_thousand_times(mutate):
    worst = 0.0
    for shape, regime, mode, splits in _WHERE[mutate]:
        x, X, sg, ex, *ref = fc.case(*shape, "plain", regime, mode)
        clean = _worst(fc.restated(x, sg, X, ex, splits), x, sg, X, ref)
        assert max(clean) <= 0.1
        worst = max(worst, max(_worst(fc.restated(x, sg, X, ex, splits, mutate=mutate), x, sg, X, ref)))
    print(f"{mutate}: worst error / bound {worst:.2e}")
    assert worst >= 1e3


# ------------------------------------------------------------------------------------------- the acceptance readings
@pytest.mark.parametrize("D", [16, 1024])
def test_circle_reads_one_and_sphere_two_at_every_point(D):
    """Asserted OF THE ORACLE (the fp64 statement of the formula): all 4096 points round to their manifold's dimension at sigma = 0.4
    and 0.5, with and without the query's own point, inside the spreads recorded for the four cases."""
    X, want = fc.acceptance_cloud(D)
    spread = {0.4: ((0.949, 1.186), (1.553, 2.397), 100.0), 0.5: ((1.005, 1.240), (1.733, 2.303), 167.0)}
    for exclude_self in (True, False):
        flipd, ess = fc.acceptance(D, exclude_self)
        for s, sigma in enumerate(fc.ACCEPT_SIGMAS):
            (clo, chi), (slo, shi), least = spread[sigma]
            circle, sphere = flipd[:1024, s], flipd[1024:, s]
            print(f"D={D} sigma={sigma} exclude_self={exclude_self}: circle {circle.min():.3f} .. {circle.max():.3f}, sphere "
                  f"{sphere.min():.3f} .. {sphere.max():.3f}, smallest ESS {ess[:, s].min():.1f}")
            assert np.array_equal(np.rint(flipd[:, s]).astype(np.int64), want)
            h = 5e-4                                                     # the recorded spreads are rounded to three decimals
            assert clo - h <= circle.min() and circle.max() <= chi + h and slo - h <= sphere.min() and sphere.max() <= shi + h
            assert ess[:, s].min() >= least
    if D == 16:                                                          # the fp64 statement is the long-double oracle to 1e-11
        pts = jc.CS_POINTS
        sg = [np.float32(s) for s in fc.ACCEPT_SIGMAS]
        for exclude_self in (True, False):
            ref = fc.oracle(X[pts], sg, X, exclude=pts if exclude_self else None)
            np.testing.assert_allclose(fc.acceptance(D, exclude_self)[0][pts], ref[0], rtol=1e-11)
            np.testing.assert_allclose(fc.acceptance(D, exclude_self)[1][pts], ref[1], rtol=1e-11)


def test_line_readings_at_the_drivers_points_are_clear_of_a_half_integer():
    """The oracle on the line config's cloud at the config's own sigma_min = 0.2 (of its documented working range 0.05 .. 0.4), at the
    four points the driver visits, each left out of its own softmax: 1.602, 0.948, 1.028, 1.052, so [2, 1, 1, 1] -- what
    tests/test_hip_empirical_flipd.py expects of the driver.  (The first point's ESS is 8.5: the reading of a real number says so,
    where the count of eigenvalues at this bandwidth says 1.)"""
    _, xs, ex, flipd, ess = fc.line_driver_case()
    off = np.abs(flipd - np.floor(flipd) - 0.5)
    print(f"line, sigma {fc.LINE_SIGMA}: points {ex.tolist()}, FLIPD {np.round(flipd, 3).tolist()}, ESS {np.round(ess, 1).tolist()}")
    assert xs.shape == (4, 100) and off.min() >= 0.1
    assert np.rint(flipd).astype(int).tolist() == [2, 1, 1, 1]


# ------------------------------------------------------------------------------------------- the rule
def test_flipd_dims_takes_the_longest_qualifying_run_of_the_rounded_curve():
    curve = {'sigmas': np.array([0.1, 0.2, 0.4, 0.8]),
             'flipd': np.array([[0.2, 0.9, 1.1, 1.3], [2.2, 1.9, 3.4, 3.3], [1.0, 1.0, np.nan, 1.0], [5.0, 5.0, 5.0, 5.0]]),
             'ess': np.array([[50.0, 50, 50, 50], [50, 50, 50, 5], [50, 50, 50, 50], [1, 2, 3, 4]])}
    reading, dims, rng = empirical.flipd_dims(curve)
    assert dims.dtype == np.int64 and dims.tolist() == [1, 2, 1, -1]
    np.testing.assert_allclose(reading[:3], [1.1, 2.05, 1.0], rtol=1e-15)
    assert np.isnan(reading[3]) and np.isnan(rng[3]).all()
    np.testing.assert_array_equal(rng[:3], [[0.2, 0.8], [0.1, 0.2], [0.1, 0.2]])
    assert empirical.flipd_dims(curve, ess_min=60.0)[1].tolist() == [-1, -1, -1, -1]


# ------------------------------------------------------------------------------------------- the C ABI
def test_ok_truth_table_and_workspace():
    ok = _lib.empirical_flipd_ok
    assert ok(1, 1, 1) and ok(8000, 100, 11) and ok(4000, 1024, 32) and ok(10000, 3072) and ok(40, 12288, 1) and ok(1, 65536, 32)
    assert not ok(0, 1, 1) and not ok(1, 0, 1) and not ok(1, 1, 0) and not ok(100, 16, 33) and not ok(100, 65537, 1)
    assert ok((1 << 31) - 65, 10, 1) and not ok((1 << 31) - 64, 10, 1)
    assert _lib.FLIPD_S_MAX == 32
    ws = _lib.lib().idiff_empirical_flipd_workspace_doubles
    assert ws(100, 11, 7) == 4 * 100 * 11 * 7 and ws(0, 1, 1) == 0 and ws(1 << 31, 32, 1000) == 4 * (1 << 31) * 32 * 1000


def test_default_splits():
    """Two workgroups of 64 queries a CU (256) when the queries alone give fewer, never a range below one tile of 64 points; 1 when the
    queries fill the card; D plays no part."""
    sp = _lib.empirical_flipd_splits
    assert sp(8000, 8000, 100) == 5                                      # 125 workgroups of queries: ceil(512 / 125)
    assert sp(100, 8000, 100) == 125                                     # 2 workgroups: 256 wanted, the cloud has 125 tiles
    assert sp(100, 40000, 100) == 256
    assert sp(1, 10000, 3072) == 157 and sp(1, 10000, 16) == 157
    assert sp(16384, 8000, 100) == 1 and sp(16321, 8000, 100) == 1 and sp(16320, 8000, 100) == 3
    assert sp(1, 1, 1) == 1 and sp(7, 64, 5) == 1 and sp(7, 65, 5) == 2
    assert sp(0, 10, 3) == 1


_A, _B, _C, _D, _E, _F, _G, _H = (0x10000 * i for i in range(1, 9))         # fabricated addresses: a call let through would fault
_CALL = lambda x=_A, Y=_B, h=_C, c=_D, sigmas=_E, exclude=0, flipd=_F, ess=_G, ws=_H, wsn=4 * 4 * 3 * 2, P=4, N=100, D=3, S=3, splits=2: \
    [x, Y, h, c, sigmas, exclude, flipd, ess, ws, wsn, P, N, D, S, splits]
_REFUSED = {
    "null_x": _CALL(x=0), "null_Y": _CALL(Y=0), "null_h": _CALL(h=0), "null_c": _CALL(c=0), "null_sigmas": _CALL(sigmas=0),
    "null_flipd": _CALL(flipd=0), "null_ess": _CALL(ess=0), "null_workspace": _CALL(ws=0), "negative_P": _CALL(P=-1), "N0": _CALL(N=0),
    "D0": _CALL(D=0), "S0": _CALL(S=0), "S33": _CALL(S=33, wsn=1 << 20), "D_above_limit": _CALL(D=65537),
    "N_above_limit": _CALL(N=1 << 31), "splits0": _CALL(splits=0), "splits_above_grid": _CALL(splits=65536, wsn=1 << 30),
    "workspace_one_short": _CALL(wsn=4 * 4 * 3 * 2 - 1), "misaligned_x": _CALL(x=_A + 2), "misaligned_Y": _CALL(Y=_B + 8),
    "misaligned_h": _CALL(h=_C + 4), "misaligned_exclude": _CALL(exclude=_A + 1), "misaligned_flipd": _CALL(flipd=_F + 4),
    "misaligned_ess": _CALL(ess=_G + 2), "misaligned_workspace": _CALL(ws=_H + 4), "null_x_at_P0": _CALL(x=0, P=0),
}


@pytest.mark.parametrize("case", sorted(_REFUSED))
def test_entry_point_refuses_before_any_device_call(case):
    handle = _lib.lib()
    assert handle.idiff_empirical_flipd_f64(*_REFUSED[case], None) == 1001       # IDIFF_EINVAL
    assert handle.idiff_last_error().decode().startswith("empirical_flipd: ")


def test_a_too_small_workspace_names_what_is_needed():
    assert _lib.lib().idiff_empirical_flipd_f64(*_CALL(wsn=10), None) == 1001
    msg = _lib.lib().idiff_last_error().decode()
    assert "workspace of 10 doubles" in msg and "need 96" in msg


def test_p0_with_good_pointers_is_a_no_op():
    assert _lib.lib().idiff_empirical_flipd_f64(*_CALL(P=0, wsn=0), None) == 0


def test_wrapper_has_no_cpu_path():
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.empirical_flipd(torch.zeros(4, 8), {"Y": torch.zeros(10, 8), "h": torch.zeros(10), "c": torch.zeros(8), "N": 10, "D": 8},
                             torch.ones(3))
