"""GPU: the largest eigenpairs of a symmetric indefinite fp64 matrix (csrc/topvecs.hip, _lib.sym_topvecs).

Oracles: the prescribed spectrum of K = Q diag(lambda) Q^T built in numpy fp64, and numpy.linalg.eigvalsh for the centred geodesic
kernels of the three fixture point sets (tests/golden/isomap.npz).

Bounds (fixed by the contract of the routine, not by what it returns): resid <= 1e-9 |lambda_1| sqrt(k), the bound Isomap.fit
enforces; |V^T V - I|_max <= 1e-12; Ritz values within 1e-10 |lambda_1| of the true top k.  The subspace is measured by
|(I - U U^T) V|_F, U the eigenvectors of every eigenvalue >= lambda_k (a degenerate partner of lambda_k included), against the
Davis-Kahan bound resid_bound / gap, gap = lambda_k minus the largest eigenvalue outside U: sqrt(1 - cos^2) would bottom out at
1e-8.
"""
import numpy as np
import pytest
import torch

import id_diff_amd
from id_diff_amd import _lib, isomap

pytestmark = pytest.mark.gpu
DEV = "cuda"


def spectrum(N, case, k):
    """Descending eigenvalues: a quadratic decay from 1 to -0.1, then (a) lambda_min = -2 lambda_1, (b) lambda_1 = 1e6 lambda_2,
    (c) an exactly double eigenvalue inside the top k (for k = 1 the pair lambda_1 = lambda_2, the only one that touches it),
    (d) lambda_k = lambda_(k+1)."""
    lam = np.sort(np.linspace(1.0, 0.0, N) ** 2 * 0.9 - 0.1)[::-1].copy()
    lam[0] = 1.0
    if case == "a":
        lam[-1] = -2.0
    elif case == "b":
        lam[0] = 1e6 * lam[1]
    elif case == "c":
        j = max(k // 2, 1)
        lam[j] = lam[j - 1]
    elif case == "d":
        lam[k] = lam[k - 1]
    return np.sort(lam)[::-1].copy()


@pytest.fixture(scope="module")
def bases():
    rng = np.random.default_rng(5)
    return {N: np.linalg.qr(rng.standard_normal((N, N)))[0] for N in (130, 257)}


def check(K, lam, k, V, ritz, resid, U=None, gap=None, what=""):
    N = K.shape[0]
    V, ritz, resid = V.cpu().numpy(), ritz.cpu().numpy(), float(resid)
    top = abs(lam[0])
    orth = np.abs(V.T @ V - np.eye(k)).max()
    own = np.linalg.norm(K @ V - V * ritz)
    dr = np.abs(ritz - lam[:k]).max()
    print(f"{what}: resid / (|lambda_1| sqrt(k)) = {resid / (top * np.sqrt(k)):.3g} (recomputed {own / (top * np.sqrt(k)):.3g}), "
          f"|V^T V - I| = {orth:.3g}, |ritz - lambda| / |lambda_1| = {dr / top:.3g}")
    assert V.shape == (N, k) and ritz.shape == (k,)
    assert resid <= 1e-9 * top * np.sqrt(k)
    assert own <= 1e-9 * top * np.sqrt(k)                      # the reported residual is the residual
    assert orth <= 1e-12
    assert dr <= 1e-10 * top
    assert np.all(np.diff(ritz) <= 0)
    if U is not None:
        out = np.linalg.norm(V - U @ (U.T @ V))
        print(f"{what}: |(I - U U^T) V|_F = {out:.3g}, bound {1e-9 * top * np.sqrt(k) / gap:.3g}")
        assert out <= 1e-9 * top * np.sqrt(k) / gap


@pytest.mark.parametrize("k", [1, 2, 16, 64])
@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
@pytest.mark.parametrize("N", [130, 257])
def test_synthetic_spectra(bases, N, case, k):
    Q, lam = bases[N], spectrum(N, case, k)
    K = (Q * lam) @ Q.T
    K = 0.5 * (K + K.T)
    V, ritz, resid = _lib.sym_topvecs(torch.from_numpy(K).to(DEV), k, lam)
    inside = int(np.count_nonzero(lam >= lam[k - 1]))          # k, or k + 1 where lambda_k has a partner below it
    check(K, lam, k, V, ritz, resid, U=Q[:, :inside], gap=lam[k - 1] - lam[inside], what=f"N = {N}, case {case}, k = {k}")


@pytest.fixture(scope="module")
def kernels(golden):
    """name -> (K as numpy, eigenvalues descending by LAPACK, K on the device): the centred geodesic kernel of each fixture set."""
    gold, out = golden("isomap.npz"), {}
    for name in ("roll257", "roll1000", "sphere193"):
        K, _ = _lib.double_center(isomap.geodesics(gold[f"{name}_X"], int(gold[f"{name}_nn"])))
        Kh = K.cpu().numpy()
        out[name] = (Kh, np.linalg.eigvalsh(Kh)[::-1].copy(), K)
    return out


@pytest.mark.parametrize("name,k", [("roll257", 2), ("roll257", 3), ("roll257", 10), ("roll1000", 2), ("roll1000", 3),
                                    ("sphere193", 5), ("sphere193", 10)])
def test_fixture_kernels(kernels, name, k):
    Kh, lam, K = kernels[name]
    assert lam[-1] < -0.004 * lam[0]                            # indefinite: a negative eigenvalue of some weight
    V, ritz, resid = _lib.sym_topvecs(K, k, lam)
    check(Kh, lam, k, V, ritz, resid, what=f"{name}, k = {k}")
    assert np.array_equal(K.cpu().numpy(), Kh)                  # K is only read


def test_nan_poisons_all_three_and_k_is_only_read(bases):
    Q, lam = bases[130], spectrum(130, "a", 3)
    K = (Q * lam) @ Q.T
    K = 0.5 * (K + K.T)
    Kd = torch.from_numpy(K).to(DEV)
    V, ritz, resid = _lib.sym_topvecs(Kd, 3, lam)
    assert np.array_equal(Kd.cpu().numpy(), K)                  # bit-unchanged
    assert bool(torch.isfinite(V).all()) and bool(torch.isfinite(ritz).all()) and bool(torch.isfinite(resid))
    bad = K.copy()
    bad[77, 5] = bad[5, 77] = np.nan
    V, ritz, resid = _lib.sym_topvecs(torch.from_numpy(bad).to(DEV), 3, lam)
    assert bool(torch.isnan(V).all()) and bool(torch.isnan(ritz).all()) and bool(torch.isnan(resid))
