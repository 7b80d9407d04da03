"""GPU: the tangent-space basis beside the spectrum (idiff_sym_lowvecs_f64, _lib.sym_lowvecs, _lib.tangent_basis).

Oracle: fp64 numpy on the host -- ``numpy.linalg.eigh`` of the fp64 centred Gram matrix of the same fp32 score matrix.

Inputs are built from known factors: S = (U diag(s)) V^T + c with U [M, D], V [D, D] orthonormal, M = 2 D + 5, cast to fp32;
the D - k normal singular values log-spaced in [1, 10], the k tangent ones in [1e-3, 1e-2], so the relative eigen-gap
(lambda_k+1 - lambda_k) / lambda_max is about 1e-2 and the first-order perturbation bound D 2^-53 lambda_max / gap on the sine
of the angle is at most 6e-12: the bar of 1e-9 leaves two orders of margin.  (On the host, for exactly these inputs, eigh and svd
agree to 2e-14 and three steps of an fp64 Cholesky inverse iteration agree with eigh to 4e-12 .. 9e-12.)
"""
import functools

import numpy as np
import pytest
import torch

import id_diff_amd
from id_diff_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(40, 1),       # below one panel, a single vector
          (96, 3),
          (130, 33),     # just past 128: ragged last panel, k past one block of 32
          (257, 32),
          (512, 128)]    # the cap


def make_scores(D, k, zero_tangent=False, seed=0):
    rng = np.random.default_rng(1000 * D + k + seed)
    M = 2 * D + 5
    U, _ = np.linalg.qr(rng.standard_normal((M, D)))
    V, _ = np.linalg.qr(rng.standard_normal((D, D)))
    normal = np.logspace(0.0, 1.0, D - k)[::-1]
    tangent = np.zeros(k) if zero_tangent else np.logspace(-3.0, -2.0, k)[::-1]
    s = np.concatenate([normal, tangent])
    c = rng.standard_normal(D)
    return ((U * s) @ V.T + c).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(D, k, zero_tangent=False):
    """(S fp32, eigenvalues ascending, eigenvectors) -- the oracle, computed once per shape and shared."""
    S = make_scores(D, k, zero_tangent)
    S64 = S.astype(np.float64)
    C = S64 - S64.mean(0)
    lam, vec = np.linalg.eigh(C.T @ C)
    for a in (S, lam, vec):
        a.setflags(write=False)
    return S, lam, vec


def sine_of_largest_angle(T, Q):
    """sin of the largest principal angle between span(T) and span(Q) (both with orthonormal columns)."""
    return float(np.linalg.norm(T - Q @ (Q.T @ T), 2))


def device_gram(S):
    """The fp64 centred Gram matrix exactly as tangent_basis hands it to the solver (the stages are deterministic)."""
    M = S.shape[0]
    return _lib.centered_gram(S, _lib.column_sums(S) / float(M))


@pytest.mark.parametrize("D,k", SHAPES, ids=[f"D{D}-k{k}" for D, k in SHAPES])
def test_basis_ritz_and_residual_against_eigh(D, k):
    S_host, lam, vec = case(D, k)
    S = torch.from_numpy(S_host.copy()).to(DEV)
    T, ritz, resid = _lib.tangent_basis(S, k)
    assert T.shape == (D, k) and T.dtype == torch.float64 and ritz.shape == (k,) and resid.ndim == 0
    Th, rh, res = T.cpu().numpy(), ritz.cpu().numpy(), float(resid)
    lmax = float(lam[-1])
    orth = float(np.abs(Th.T @ Th - np.eye(k)).max())
    sine = sine_of_largest_angle(Th, vec[:, :k])
    dritz = float(np.abs(rh - lam[:k]).max())
    _, eig = _lib.spectrum(S, return_eig=True)
    dspec = float(np.abs(rh - eig.cpu().numpy()[:k]).max())
    G = device_gram(S).cpu().numpy()
    res_host = float(np.linalg.norm(G @ Th - Th * rh))
    print(f"\n[tangent D={D} k={k}] |T^T T - I|_max = {orth:.3e} (bar {1e-13 * k:.1e}); sine = {sine:.3e} (bar 1e-9); "
          f"|ritz - eigh| = {dritz:.3e}, |ritz - spectrum| = {dspec:.3e} (bar {1e-12 * lmax:.1e}); "
          f"resid device {res:.3e}, host {res_host:.3e}")
    assert np.isfinite(Th).all() and np.isfinite(rh).all() and np.isfinite(res)
    assert orth <= 1e-13 * k
    assert sine <= 1e-9
    assert (np.diff(rh) >= 0).all()
    assert dritz <= 1e-12 * lmax
    assert dspec <= 1e-12 * lmax
    assert 0.5 * res_host <= res <= 2.0 * res_host


def test_same_basis_on_every_call():
    S = torch.from_numpy(case(96, 3)[0].copy()).to(DEV)
    a, b = _lib.tangent_basis(S, 3), _lib.tangent_basis(S, 3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_gram_is_left_untouched():
    S = torch.from_numpy(case(96, 3)[0].copy()).to(DEV)
    G = device_gram(S)
    before = G.clone()
    _lib.sym_lowvecs(G, 3)
    assert torch.equal(G, before)


def test_exactly_rank_deficient_gram_is_factored():
    """Zero tangent singular values before the fp32 cast: the lowest eigenvalues are rounding noise around zero (some below it), so
    the factorisation stands on the diagonal shift alone."""
    D, k = 96, 5
    S_host, lam, vec = case(D, k, True)
    T, ritz, resid = _lib.tangent_basis(torch.from_numpy(S_host.copy()).to(DEV), k)
    Th = T.cpu().numpy()
    assert np.isfinite(Th).all() and bool(torch.isfinite(ritz).all()) and bool(torch.isfinite(resid))
    sine = sine_of_largest_angle(Th, vec[:, :k])
    print(f"\n[tangent rank-deficient] lowest eigenvalues {lam[:k]}, sine = {sine:.3e}")
    assert sine <= 1e-9
    assert float(np.abs(Th.T @ Th - np.eye(k)).max()) <= 1e-13 * k


@pytest.mark.parametrize("D,k", [(130, 0), (130, 129), (40, 40), (40, -1)])
def test_bad_k_is_refused(D, k):
    G = torch.eye(D, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="sym_lowvecs"):
        _lib.sym_lowvecs(G, k)


def test_cpu_tensor_is_refused():
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.sym_lowvecs(torch.eye(8, dtype=torch.float64), 2)


@pytest.mark.parametrize("where", ["diagonal", "below", "above"])
def test_nan_in_gram_poisons_every_output(where):
    S = torch.from_numpy(case(96, 3)[0].copy()).to(DEV)
    G = device_gram(S)
    i, j = {"diagonal": (50, 50), "below": (70, 20), "above": (20, 70)}[where]
    G[i, j] = float("nan")
    T, ritz, resid = _lib.sym_lowvecs(G, 3)
    torch.cuda.synchronize()                   # returns: nothing waits on a value that never comes
    assert bool(torch.isnan(T).all()) and bool(torch.isnan(ritz).all()) and bool(torch.isnan(resid))


def test_indefinite_matrix_poisons_every_output():
    G = torch.eye(64, dtype=torch.float64, device=DEV)
    G[10, 10] = -1.0
    T, ritz, resid = _lib.sym_lowvecs(G, 4)
    assert bool(torch.isnan(T).all()) and bool(torch.isnan(ritz).all()) and bool(torch.isnan(resid))
