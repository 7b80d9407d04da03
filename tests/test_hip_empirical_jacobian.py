"""GPU tests of the empirical score's Jacobian: the kernel (csrc/empirical_jacobian.hip) element-wise against the long-double oracle
under the bound of tests/empirical_jacobian_cases.py (validated on the CPU in test_empirical_jacobian_host.py), the bit symmetry of
C, its agreement with the score kernel, the isolation of queries that are not finite, run-to-run and split-launch bit equality, the
batched eigenvalues, and the dimensions, the stable range and the tangent spaces of a circle beside a 2-sphere and of the line."""
import pickle

import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd import _lib, empirical, lpca
from id_diff_amd.configs.utils import read_config

import empirical_cases as ec
import empirical_jacobian_cases as jc

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINE = 'configs/dimension_estimation/paper/euclidean_data/line/empirical.py'
IDS = [f"B{b}-N{n}-D{d}" for b, n, d in jc.SHAPES]


def _launch(x, sigma, X):
    C, mean, ess = _lib.empirical_jacobian(torch.from_numpy(x).to(DEV), torch.from_numpy(X).to(DEV), torch.from_numpy(sigma).to(DEV))
    torch.cuda.synchronize()
    return C.cpu().numpy(), mean.cpu().numpy(), ess.cpu().numpy()


@pytest.mark.parametrize("variant", jc.VARIANTS)
@pytest.mark.parametrize("B,N,D", jc.SHAPES, ids=IDS)
def test_kernel_under_the_bound(B, N, D, variant):
    """C, mean and ess element by element under the bound against the oracle; C equal to its transpose bit for bit."""
    x, sigma, X, rC, rmean, ress, r, R = jc.case(B, N, D, variant)
    bc, bm, be = jc.bound(sigma, N, D, r, R)
    C, mean, ess = _launch(x, sigma, X)
    assert C.shape == (B, D, D) and C.dtype == np.float64 and mean.shape == (B, D) and mean.dtype == np.float64
    assert ess.shape == (B,) and ess.dtype == np.float32
    worst = (jc.worst_ratio(np.abs(C - rC), bc), jc.worst_ratio(np.abs(mean - rmean), bm),
             jc.worst_ratio(np.abs(ess.astype(np.float64) - ress), be * ress))
    print(f"B={B} N={N} D={D} {variant}: worst error / bound: C {worst[0]:.2e}, mean {worst[1]:.2e}, ess {worst[2]:.2e}; "
          f"ess {float(ress.min()):.3g} .. {float(ress.max()):.3g}")
    assert np.isfinite(C).all() and np.isfinite(mean).all() and np.isfinite(ess).all()
    assert np.array_equal(C.view(np.uint64), np.ascontiguousarray(C.transpose(0, 2, 1)).view(np.uint64))
    assert max(worst) <= 1.0


@pytest.mark.parametrize("variant", jc.VARIANTS)
@pytest.mark.parametrize("B,N,D", jc.SHAPES, ids=IDS)
def test_mean_and_ess_agree_with_the_score_kernel(B, N, D, variant):
    """``mean`` is the score kernel's output (fp32, its own bound) and ``ess`` its ESS."""
    x, sigma, X, _, rmean, ress, r, R = jc.case(B, N, D, variant)
    _, bm, be = jc.bound(sigma, N, D, r, R)
    _, mean, ess = _launch(x, sigma, X)
    out, sess = _lib.empirical_score(torch.from_numpy(x).to(DEV), _lib.empirical_pack(torch.from_numpy(X).to(DEV)),
                                     torch.from_numpy(sigma).to(DEV))
    out, sess = out.cpu().numpy().astype(np.float64), sess.cpu().numpy().astype(np.float64)
    L, _ = ec.logit_term(x, sigma, X)
    allowed = ec.bound(x, sigma, X, r) + 2.0 ** -23 * np.abs(out) + bm
    worst = jc.worst_ratio(np.abs(mean - out), allowed)
    worst_ess = jc.worst_ratio(np.abs(ess.astype(np.float64) - sess), (be + 2.0 ** -22 + 4 * L) * ress)
    print(f"B={B} N={N} D={D} {variant}: worst |mean - score| / allowed {worst:.2e}, ess {worst_ess:.2e}")
    assert worst <= 1.0 and worst_ess <= 1.0


def test_queries_that_are_not_finite_are_nan_and_alone():
    x, sigma, X = jc.inputs(65, 63, 23, "plain")
    clean = _launch(x, sigma, X)
    spoil = {3: ("x", np.nan), 17: ("x", np.inf), 20: ("sigma", 0.0), 21: ("sigma", -0.3), 37: ("sigma", np.nan), 64: ("x", -np.inf)}
    for rows in [[b] for b in spoil] + [list(spoil)]:
        xs, ss = x.copy(), sigma.copy()
        for b in rows:
            if spoil[b][0] == "x":
                xs[b, (5 * b) % 23] = spoil[b][1]
            else:
                ss[b] = spoil[b][1]
        got = _launch(xs, ss, X)
        bad = np.zeros(65, dtype=bool)
        bad[rows] = True
        for g, c, bits in zip(got, clean, (np.uint64, np.uint64, np.uint32)):
            assert np.isnan(g[bad]).all()
            assert np.array_equal(g[~bad].view(bits), c[~bad].view(bits))


def test_same_bits_every_run_and_however_the_queries_are_split():
    x, sigma, X = jc.inputs(33, 1000, 100, "plain")
    a, b = _launch(x, sigma, X), _launch(x, sigma, X)
    lo, hi = _launch(x[:7], sigma[:7], X), _launch(x[7:], sigma[7:], X)
    for u, v, l, h, bits in zip(a, b, lo, hi, (np.uint64, np.uint64, np.uint32)):
        assert np.isfinite(u).all()
        assert np.array_equal(u.view(bits), v.view(bits))
        assert np.array_equal(np.concatenate([l, h]).view(bits), u.view(bits))


def test_wrapper_refuses_what_the_kernel_does_not_serve():
    x, X, sigma = torch.zeros(4, 8, device=DEV), torch.zeros(10, 8, device=DEV), torch.ones(4, device=DEV)
    with pytest.raises(RuntimeError, match="empirical_jacobian: x"):
        _lib.empirical_jacobian(torch.zeros(4, 9, device=DEV), X, sigma)
    with pytest.raises(RuntimeError, match="empirical_jacobian: x"):
        _lib.empirical_jacobian(x, X, sigma[:3])
    with pytest.raises(RuntimeError, match="is not served"):
        _lib.empirical_jacobian(torch.zeros(4, jc.CAP + 1, device=DEV), torch.zeros(10, jc.CAP + 1, device=DEV), sigma)
    with pytest.raises(RuntimeError, match="expected dtype"):
        _lib.empirical_jacobian(x, X.double(), sigma)
    with pytest.raises(RuntimeError, match="empirical_jacobian: C"):
        _lib.empirical_jacobian(x, X, sigma, C=torch.zeros(4, 8, 7, device=DEV, dtype=torch.float64))
    C, mean, ess = _lib.empirical_jacobian(torch.zeros(0, 8, device=DEV), X, torch.ones(0, device=DEV))
    assert C.shape == (0, 8, 8) and mean.shape == (0, 8) and ess.shape == (0,)


# ------------------------------------------------------------------------------------------- eigenvalues, many matrices a call
@pytest.mark.parametrize("D", [3, 100, 128, 130])
def test_sym_eigvals_batched(D):
    """Within 5e-14 max|lambda| of numpy, the tolerance tests/test_hip_spectrum.py holds ``sym_eigvals`` to; up to D = 128 the same
    bits as one ``sym_eigvals`` call per matrix (the same kernels, one workgroup a matrix)."""
    rng = np.random.default_rng(D)
    A = rng.standard_normal((5, D, D))
    G = A + A.transpose(0, 2, 1)
    G[1] *= 1e-3
    G[2] = (A[2, :, :2] @ A[2, :, :2].T)                             # rank two: D - 2 eigenvalues at zero
    want = np.linalg.eigvalsh(G)
    got = _lib.sym_eigvals_batched(torch.from_numpy(G).to(DEV)).cpu().numpy()
    assert got.shape == (5, D) and (np.diff(got, axis=1) >= 0).all()
    err = np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)
    print(f"D={D}: worst |eig - numpy| / max|eig| {float(err.max()):.2e}")
    assert (err <= 5e-14).all()
    if D <= 128:
        one = np.stack([_lib.sym_eigvals(torch.from_numpy(G[p].copy()).to(DEV)).cpu().numpy() for p in range(5)])
        assert np.array_equal(one.view(np.uint64), got.view(np.uint64))
    assert _lib.sym_eigvals_batched(torch.zeros(0, 4, 4, device=DEV, dtype=torch.float64)).shape == (0, 4)


# ------------------------------------------------------------------------------------------- a circle beside a 2-sphere, and the line
def test_jacobian_spectra_and_scale_curve_on_circle_and_sphere():
    """The eigenvalues within D bound + 5e-14 lambda_1 of those of the oracle's C (Weyl); 1 / 2 at all 96 (point, sigma) pairs; the
    stable dimension 1 / 2 at all 32 points."""
    X, x, refs, want = jc.circle_and_sphere_case()
    eig, ess = empirical.jacobian_spectra(X, jc.CS_SIGMAS, points=jc.CS_POINTS)
    assert eig.shape == (32, 3, 16) and eig.dtype == np.float64 and ess.shape == (32, 3)
    for s, (sigma, (rC, _, ress, r, R)) in enumerate(zip(jc.CS_SIGMAS, refs)):
        ref = np.linalg.eigvalsh(rC)[:, ::-1]
        allowed = 16 * jc.bound(np.full(32, sigma), X.shape[0], 16, r, R)[0][:, 0] + 5e-14 * ref[:, :1]
        worst = jc.worst_ratio(np.abs(eig[:, s] - ref), allowed)
        print(f"sigma {sigma}: worst |eig - ref| / allowed {worst:.2e}, smallest ESS {float(ess[:, s].min()):.1f}")
        assert worst <= 1.0
        np.testing.assert_allclose(ess[:, s], ress, rtol=1e-6)
    dims = empirical.dims_from_jacobian(eig)
    assert dims.shape == (32, 3) and (dims == want[:, None]).all()
    curve = empirical.scale_curve(X, sigmas=jc.CS_SIGMAS, points=x)                    # the same points, by their coordinates
    assert sorted(curve) == ['dims', 'eigenvalues', 'ess', 'sigmas', 'stable_dims', 'stable_range']
    assert np.array_equal(curve['eigenvalues'].view(np.uint64), eig.view(np.uint64)) and np.array_equal(curve['dims'], dims)
    assert curve['stable_dims'].tolist() == want.tolist()
    lowest = np.where(ess[:, 0] >= empirical.ESS_MIN, 0.2, 0.3)                        # sigma = 0.2 qualifies at some points only
    np.testing.assert_array_equal(curve['stable_range'], np.stack([lowest, np.full(32, 0.5)], axis=1))


def test_jacobian_tangent_on_circle_and_sphere():
    """At sigma = 0.3 against ``eigh`` of the oracle's C: the sine of the largest principal angle at most
    1e-9 + 2 D bound / (lambda_d - lambda_(d+1)) (Davis-Kahan) for the basis as computed (fp64).  The float32 basis that is returned by
    default is that basis rounded; the rounding alone turns an exact basis by 2.3e-8 .. 3.0e-8 here, where the bound allows
    1.5e-8 .. 2.0e-8, so it is the fp64 basis that is held to the bound and the float32 one to being its rounding."""
    X, x, refs, want = jc.circle_and_sphere_case()
    rC, _, _, r, R = refs[1]
    bc = jc.bound(np.full(32, 0.3), X.shape[0], 16, r, R)[0][:, 0, 0]
    T64 = empirical.jacobian_tangent(X, 0.3, points=jc.CS_POINTS, dtype=np.float64)
    T32 = empirical.jacobian_tangent(X, 0.3, points=jc.CS_POINTS)
    assert len(T64) == len(T32) == 32
    worst = 0.0
    for p in range(32):
        d = int(want[p])
        assert T32[p] is not None and T32[p].shape == (16, d) and T32[p].dtype == np.float32
        assert T64[p].shape == (16, d) and T64[p].dtype == np.float64 and np.array_equal(T64[p].astype(np.float32), T32[p])
        lam, V = np.linalg.eigh(rC[p])
        sine = lpca.subspace_sine(T64[p], V[:, ::-1][:, :d])
        allowed = 1e-9 + 2 * 16 * bc[p] / (lam[::-1][d - 1] - lam[::-1][d])
        worst = max(worst, sine / allowed)
        assert sine <= allowed, f"point {p}: sine {sine:.2e}, allowed {allowed:.2e}"
    print(f"worst sine / allowed {worst:.2e}")


def test_line_config_sweep_end_to_end(tmp_path, capsys):
    cfg = read_config(LINE)
    curve = empirical.run(cfg, sweep=True, sigmas=[0.4, 0.8], out_dir=str(tmp_path / "sweep"))
    with open(tmp_path / "sweep" / "scale_curve.pkl", "rb") as f:
        saved = pickle.load(f)
    assert sorted(saved) == ['dims', 'eigenvalues', 'ess', 'rule', 'sigmas', 'stable_dims', 'stable_range']
    assert saved['rule'] == 'half' and saved['sigmas'].tolist() == [0.4, 0.8]
    assert saved['dims'].shape == (100, 2) and saved['ess'].shape == (100, 2) and saved['eigenvalues'].shape == (100, 2, 100)
    assert saved['stable_dims'].shape == (100,) and saved['stable_range'].shape == (100, 2)
    assert (saved['dims'] == 1).all() and np.array_equal(curve['dims'], saved['dims'])
    assert (saved['ess'][:, 1] >= empirical.ESS_MIN).all() and (saved['stable_dims'] == 1).all()      # sigma = 0.8: 39.8 at the least
    assert sorted(p.name for p in (tmp_path / "sweep").iterdir()) == ['scale_curve.pkl']
    out = capsys.readouterr().out
    assert "sigma = 0.4: median ESS" in out and "dim   1: 100" in out
    dims = empirical.run(cfg, sigma=0.2, points=np.arange(3), out_dir=str(tmp_path / "plain"))
    assert dims.tolist() == [1, 1, 1]
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ['local_dims.pkl']
