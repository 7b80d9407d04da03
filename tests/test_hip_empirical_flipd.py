"""GPU tests of FLIPD on the empirical score: the kernel (csrc/empirical_flipd.hip) element by element against the long-double oracle
under the bound of tests/empirical_flipd_cases.py (validated on the CPU in test_empirical_flipd_host.py) at every shape, variant,
regime, split and exclusion, guard regions, bit equality at equal splits, the isolation of rows and columns that are not finite, the
refusals, the agreement with tr C + |m|^2 / sigma^2 of the Jacobian kernel, the acceptance clouds at all 4096 points in R^16 and
R^1024, and the driver on the line config."""
import pickle

import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd import _lib, dim_reduction, empirical
from id_diff_amd.empirical import flipd_curve, flipd_dims  # noqa: F401  (every test here is about them and their kernel)
from id_diff_amd.configs.utils import read_config

import empirical_flipd_cases as fc
import empirical_jacobian_cases as jc

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                                                               # elements of NaN in front of and behind each output
IDS = [f"P{p}-N{n}-D{d}-S{s}" for p, n, d, s in fc.SHAPES]
_packs = {}


def _pack(P, N, D, variant):
    """(x on the device, the pack of X), made once per input."""
    key = (P, N, D, variant)
    if key not in _packs:
        x, X = fc.inputs(P, N, D, variant)
        _packs[key] = (torch.from_numpy(x).to(DEV), _lib.empirical_pack(torch.from_numpy(X).to(DEV)))
    return _packs[key]


def _launch(xd, pack, sg, ex, splits):
    """(flipd, ess) as numpy, written into NaN-filled buffers between NaN guards that must come back intact."""
    P, S = xd.shape[0], len(sg)
    ff = torch.full((2 * GUARD + P * S,), float("nan"), device=DEV, dtype=torch.float64)
    ef = torch.full((2 * GUARD + P * S,), float("nan"), device=DEV, dtype=torch.float32)
    f, e = _lib.empirical_flipd(xd, pack, torch.from_numpy(np.asarray(sg, dtype=np.float32)).to(DEV), exclude=ex,
                                flipd=ff[GUARD:GUARD + P * S].view(P, S), ess=ef[GUARD:GUARD + P * S].view(P, S), splits=splits)
    torch.cuda.synchronize()
    for flat in (ff, ef):
        host = flat.cpu().numpy()
        assert np.isnan(host[:GUARD]).all() and np.isnan(host[GUARD + P * S:]).all()
    return f.cpu().numpy(), e.cpu().numpy()


@pytest.mark.parametrize("variant", fc.VARIANTS)
@pytest.mark.parametrize("P,N,D,S", fc.SHAPES, ids=IDS)
def test_kernel_under_the_bound(P, N, D, S, variant):
    """Every element of flipd and ess inside the bound, at every regime, exclusion and split: N = 2 < 7 leaves empty ranges, N = 31 at
    7 splits leaves row 30 alone in the last range, which the 'last' exclusion empties."""
    xd, pack = _pack(P, N, D, variant)
    worst = (0.0, 0.0)
    for regime in fc.REGIMES:
        for mode in fc.EXCLUDES if N > 1 else ["none"]:
            x, X, sg, ex, rf, re, r, R = fc.case(P, N, D, S, variant, regime, mode)
            bf, be = fc.bound(x, sg, X, r, R)
            for splits in fc.SPLITS:
                f, e = _launch(xd, pack, sg, ex, splits)
                assert f.shape == (P, S) and f.dtype == np.float64 and e.shape == (P, S) and e.dtype == np.float32
                w = (fc.worst_ratio(np.abs(f - rf), bf), fc.worst_ratio(np.abs(e.astype(np.float64) - re), be * re))
                assert max(w) <= 1.0, f"regime {regime}, exclude {mode}, splits {splits}: error / bound flipd {w[0]:.2e}, ess {w[1]:.2e}"
                worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    print(f"P={P} N={N} D={D} S={S} {variant}: worst error / bound: flipd {worst[0]:.2e}, ess {worst[1]:.2e}")


def test_a_point_alone_in_its_range_and_excluded():
    """N = 31 in 7 ranges of 5: row 30 is alone in the last one; N = 2 in 2 and in 7 ranges: each row alone, five ranges empty."""
    for (P, N, D, S), splits in (((9, 31, 17, 1), 7), ((3, 2, 3, 2), 2), ((3, 2, 3, 2), 7)):
        xd, pack = _pack(P, N, D, "plain")
        for regime in fc.REGIMES:
            x, X, sg, ex, rf, re, r, R = fc.case(P, N, D, S, "plain", regime, "last")
            assert (ex == N - 1).all() and -(-N // splits) * (splits - 1) >= N - 1
            bf, be = fc.bound(x, sg, X, r, R)
            f, e = _launch(xd, pack, sg, ex, splits)
            assert fc.worst_ratio(np.abs(f - rf), bf) <= 1.0 and fc.worst_ratio(np.abs(e.astype(np.float64) - re), be * re) <= 1.0


def test_same_bits_at_equal_splits():
    P, N, D, S = 4, 1000, 100, 11
    xd, pack = _pack(P, N, D, "plain")
    sg = fc.sigmas_of(S, 0.1, 5)
    ex = fc.exclude_of("first", P, N)
    runs = {}
    for splits in (1, 2, 7, None):
        a, b = _launch(xd, pack, sg, ex, splits), _launch(xd, pack, sg, ex, splits)
        assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        runs[splits] = a
    assert _lib.empirical_flipd_splits(P, N, D) == 16                    # the default: the cloud's 16 tiles
    np.testing.assert_allclose(runs[None][0], runs[1][0], rtol=1e-12)    # another split is another order of the same sums


def test_rows_and_columns_that_are_not_finite_are_nan_and_alone():
    P, N, D, S = 67, 63, 23, 6
    x, X = fc.inputs(P, N, D, "plain")
    sg = fc.sigmas_of(S, 0.1, 9)
    pack = _lib.empirical_pack(torch.from_numpy(X).to(DEV))
    clean = _launch(torch.from_numpy(x).to(DEV), pack, sg, None, 2)
    assert np.isfinite(clean[0]).all() and np.isfinite(clean[1]).all()
    bad_rows = {3: np.nan, 17: np.inf, 66: -np.inf}
    bad_cols = {1: 0.0, 2: -0.3, 4: np.nan, 5: np.inf}
    for rows, cols in [([r], []) for r in bad_rows] + [([], [c]) for c in bad_cols] + [(list(bad_rows), list(bad_cols))]:
        xs, ss = x.copy(), sg.copy()
        for r in rows:
            xs[r, (5 * r) % D] = bad_rows[r]
        for c in cols:
            ss[c] = bad_cols[c]
        got = _launch(torch.from_numpy(xs).to(DEV), pack, ss, None, 2)
        bad = np.zeros((P, S), dtype=bool)
        bad[rows, :] = True
        bad[:, cols] = True
        for g, c, bits in zip(got, clean, (np.uint64, np.uint32)):
            assert np.isnan(g[bad]).all()
            assert np.array_equal(g[~bad].view(bits), c[~bad].view(bits))


def test_no_admissible_point_is_nan():
    x, X = fc.inputs(1, 1, 1, "plain")
    pack = _lib.empirical_pack(torch.from_numpy(X).to(DEV))
    xd = torch.from_numpy(np.repeat(x, 3, axis=0)).to(DEV)
    for splits in (1, 7):
        f, e = _launch(xd, pack, [0.5, 2.0], np.array([0, -1, 0]), splits)
        assert np.isnan(f[[0, 2]]).all() and np.isnan(e[[0, 2]]).all()
        assert np.isfinite(f[1]).all() and (e[1] == 1.0).all()


def test_wrapper_refuses_without_a_launch():
    X = torch.zeros(10, 8, device=DEV)
    pack = _lib.empirical_pack(X)
    x, sg = torch.zeros(4, 8, device=DEV), torch.ones(3, device=DEV)
    with pytest.raises(RuntimeError, match="empirical_flipd: x"):
        _lib.empirical_flipd(torch.zeros(4, 9, device=DEV), pack, sg)
    with pytest.raises(RuntimeError, match="exclude out of range: values -1 .. 10"):
        _lib.empirical_flipd(x, pack, sg, exclude=[0, -1, 10, 3])
    with pytest.raises(RuntimeError, match="exclude out of range: values -2 .. 3"):
        _lib.empirical_flipd(x, pack, sg, exclude=np.array([0, -2, 1, 3]))
    with pytest.raises(RuntimeError, match="exclude holds 3 values for 4 queries"):
        _lib.empirical_flipd(x, pack, sg, exclude=[0, 1, 2])
    with pytest.raises(RuntimeError, match="checked on the host"):
        _lib.empirical_flipd(x, pack, sg, exclude=torch.zeros(4, device=DEV, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="S = 33 is not served"):
        _lib.empirical_flipd(x, pack, torch.ones(33, device=DEV))
    wide = {"Y": torch.zeros(2, 65540, device=DEV, dtype=torch.float64), "h": torch.zeros(2, device=DEV, dtype=torch.float64),
            "c": torch.zeros(65537, device=DEV, dtype=torch.float64), "N": 2, "D": 65537}
    with pytest.raises(RuntimeError, match="D = 65537, S = 3 is not served"):
        _lib.empirical_flipd(torch.zeros(1, 65537, device=DEV), wide, sg)
    with pytest.raises(RuntimeError, match="workspace of 95 doubles, P = 4, S = 3, splits = 2 need 96"):
        _lib.empirical_flipd(x, pack, sg, splits=2, workspace=torch.zeros(95, device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="splits = 0"):
        _lib.empirical_flipd(x, pack, sg, splits=0)
    with pytest.raises(RuntimeError, match="expected dtype"):
        _lib.empirical_flipd(x, pack, sg.double())
    with pytest.raises(RuntimeError, match="empirical_flipd: flipd"):
        _lib.empirical_flipd(x, pack, sg, flipd=torch.zeros(4, 2, device=DEV, dtype=torch.float64))
    f, e = _lib.empirical_flipd(torch.zeros(0, 8, device=DEV), pack, sg)
    assert f.shape == (0, 3) and e.shape == (0, 3)
    assert _lib.empirical_flipd_ok(4000, 1024, 11) and _lib.empirical_flipd_ok(10000, 3072) and _lib.empirical_flipd_ok(40, 12288)


def test_no_host_synchronisation():
    xd, pack = _pack(4, 1000, 100, "plain")
    sg = torch.from_numpy(fc.sigmas_of(11, 0.1, 5)).to(DEV)
    ex = fc.exclude_of("first", 4, 1000)
    first = _lib.empirical_flipd(xd, pack, sg, exclude=ex)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = _lib.empirical_flipd(xd, pack, sg, exclude=ex)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


# ------------------------------------------------------------------------------------------- beside the Jacobian kernel
def test_agrees_with_trace_c_plus_squared_mean_of_the_jacobian_kernel():
    """At D = 16 on CS_POINTS x CS_SIGMAS: |flipd - (tr C + |mean|^2 / sigma^2)| within this kernel's bound plus the Jacobian kernel's
    (D entries of C under its bound, and 2 |mean| D times the bound on an entry of mean, over sigma^2)."""
    X, x, refs, _ = jc.circle_and_sphere_case()
    Xd, xd = torch.from_numpy(X).to(DEV), torch.from_numpy(x).to(DEV)
    sg = np.asarray(jc.CS_SIGMAS, dtype=np.float32)
    f, e = _lib.empirical_flipd(xd, _lib.empirical_pack(Xd), torch.from_numpy(sg).to(DEV))
    f, e = f.cpu().numpy(), e.cpu().numpy()
    rf, re, r, R = fc.oracle(x, sg, X)
    bf, be = fc.bound(x, sg, X, r, R)
    assert fc.worst_ratio(np.abs(f - rf), bf) <= 1.0
    worst = 0.0
    for s, (sigma, (_, rmean, ress, rj, Rj)) in enumerate(zip(sg, refs)):
        C, mean, ess = _lib.empirical_jacobian(xd, Xd, torch.full((len(x),), float(sigma), device=DEV))
        C, mean, ess = C.cpu().numpy(), mean.cpu().numpy(), ess.cpu().numpy()
        s2 = float(sigma) ** 2
        other = np.trace(C, axis1=1, axis2=2) + (mean * mean).sum(axis=1) / s2
        bc, bm, bej = jc.bound(np.full(len(x), sigma), X.shape[0], 16, rj, Rj)
        allowed = bf[:, s] + 16 * bc[:, 0, 0] + 2 * np.abs(rmean).sum(axis=1) * bm[:, 0] / s2 + 16 * bm[:, 0] ** 2 / s2
        worst = max(worst, fc.worst_ratio(np.abs(f[:, s] - other), allowed))
        assert fc.worst_ratio(np.abs(e[:, s].astype(np.float64) - ess), (be[:, s] + bej) * ress) <= 1.0
    print(f"worst |flipd - (tr C + |m|^2 / sigma^2)| / allowed {worst:.2e}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------- the acceptance clouds
@pytest.mark.parametrize("D", [16, 1024])
def test_circle_reads_one_and_sphere_two_at_every_point(D):
    """All 4096 points through ``empirical.flipd_curve`` at sigma = 0.4 and 0.5, with and without the query's own point: every one
    rounds to its manifold's dimension and is the fp64 statement of the formula to 1e-9."""
    X, want = fc.acceptance_cloud(D)
    pts = np.arange(4096)
    for exclude_self in (True, False):
        curve = empirical.flipd_curve(X, sigmas=fc.ACCEPT_SIGMAS, points=pts, exclude_self=exclude_self)
        assert sorted(curve) == ['ess', 'flipd', 'sigmas'] and curve['flipd'].shape == (4096, 2) and curve['flipd'].dtype == np.float64
        rf, re = fc.acceptance(D, exclude_self)
        for s, sigma in enumerate(fc.ACCEPT_SIGMAS):
            col = curve['flipd'][:, s]
            print(f"D={D} sigma={sigma} exclude_self={exclude_self}: circle {col[:1024].min():.3f} .. {col[:1024].max():.3f}, sphere "
                  f"{col[1024:].min():.3f} .. {col[1024:].max():.3f}, smallest ESS {curve['ess'][:, s].min():.1f}")
            assert np.array_equal(np.rint(col).astype(np.int64), want)
        np.testing.assert_allclose(curve['flipd'], rf, rtol=1e-9)
        np.testing.assert_allclose(curve['ess'], re, rtol=1e-6)
    reading, dims, rng = empirical.flipd_dims(curve)
    assert np.array_equal(dims, want) and (np.abs(reading - want) < 0.5).all()
    by_coordinates = empirical.flipd_curve(X, sigmas=fc.ACCEPT_SIGMAS, points=X[:5])     # coordinates: nothing to exclude
    np.testing.assert_allclose(by_coordinates['flipd'], rf[:5], rtol=1e-9)


def test_existing_functions_still_refuse_what_flipd_serves():
    X, _ = fc.acceptance_cloud(1024)
    with pytest.raises(RuntimeError, match="is not served"):
        empirical.scale_curve(X[:64], sigmas=[0.4], points=np.arange(2))
    assert not _lib.empirical_score_ok(64, 1024) and not _lib.empirical_jacobian_ok(64, 1024) and _lib.empirical_flipd_ok(64, 1024)


# ------------------------------------------------------------------------------------------- the driver and the command line
def test_driver_on_the_line_config(tmp_path):
    """``method='flipd'`` on the line config returns the rounding the oracle gives at the config's sigma_min = 0.2 at the same four
    points (test_empirical_flipd_host.py: [2, 1, 1, 1], every reading at least 0.1 from a half-integer), and writes the pickle."""
    cloud, xs, ex, rf, re = fc.line_driver_case()
    cfg = read_config(fc.LINE)
    cfg.device = DEV
    cfg.logging.log_path = str(tmp_path)
    dims = dim_reduction.get_manifold_dimension(cfg, return_dims=True, method='flipd')
    assert dims == np.rint(rf).astype(int).tolist()
    cfg['dim_estimation.method'] = 'flipd'
    assert dim_reduction.get_manifold_dimension(cfg, name='line') is None
    with open(tmp_path / cfg.logging.log_name / 'svd' / 'line_flipd.pkl', 'rb') as f:
        saved = pickle.load(f)
    assert sorted(saved) == ['dims', 'flipd', 'sigma'] and saved['sigma'] == fc.LINE_SIGMA
    assert saved['flipd'].dtype == np.float64 and saved['dims'].tolist() == dims
    np.testing.assert_allclose(saved['flipd'], rf, rtol=1e-9)
    with pytest.raises(NotImplementedError, match="no spectrum"):
        dim_reduction.get_manifold_dimension(cfg, return_svd=True)
    del cfg['dim_estimation']
    svd, sampled = dim_reduction.get_manifold_dimension(cfg, return_svd=True, return_dims=True)      # the default has not moved
    assert list(sampled) == [1, 1, 1, 1]


def test_run_flipd_writes_the_pickle_and_prints_the_histogram(tmp_path, capsys):
    cfg = read_config(fc.LINE)
    curve = empirical.run(cfg, flipd=True, sigmas=[0.2, 0.4], points=np.arange(20), out_dir=str(tmp_path / "f"))
    with open(tmp_path / "f" / "flipd.pkl", "rb") as f:
        saved = pickle.load(f)
    assert sorted(saved) == ['dims', 'ess', 'flipd', 'range', 'reading', 'sigmas'] and saved['sigmas'].tolist() == [0.2, 0.4]
    assert saved['flipd'].shape == (20, 2) and saved['ess'].shape == (20, 2) and saved['dims'].shape == (20,)
    assert np.array_equal(saved['flipd'], curve['flipd'])
    assert sorted(p.name for p in (tmp_path / "f").iterdir()) == ['flipd.pkl']
    out = capsys.readouterr().out
    assert "sigma = 0.2: median ESS" in out and "median FLIPD" in out and "dim   1:" in out
    empirical.main(["--config", fc.LINE, "--flipd", "--sigmas", "0.3", "--out_dir", str(tmp_path / "cli")])
    with open(tmp_path / "cli" / "flipd.pkl", "rb") as f:
        assert pickle.load(f)['flipd'].shape == (100, 1)
