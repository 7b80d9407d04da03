"""GPU: isomap.Isomap end to end (fit, embedding_, transform, reconstruction_error) against scikit-learn's stored results
(tests/golden/isomap_embed.npz, written by tests/golden/make_isomap_embed.py).

Bounds.  fit() accepts a basis with |K V - V diag(lambda)|_F <= 1e-9 lambda_1 sqrt(k); an eigenvector is then within residual / gap
of the true one to first order, gap = g_min lambda_1 the smallest distance between the eigenvalues the columns depend on (stored
per case by the generator), so  |embedding_ - scikit-learn|_max <= 10 (1e-9 / g_min) max|Z|  with the factor 10 for the second-order
term.  Column signs are compared as returned: the svd_flip convention is part of the contract.  sphere193 at 10 components has
eigenvalues 0.003 lambda_1 apart inside the block, so there Z Z^T is compared (it depends on the subspace alone, whose gap to
lambda_11 is 0.011 lambda_1) within 10 (1e-9 / 0.011) lambda_1.  transform() of new points gets 100 (1e-9 / g_min) max|Z|: the kernel
row of a new point is not in the range of K and the first-order bound is only indicative.
"""
import numpy as np
import pytest
import torch

import id_diff_amd
from id_diff_amd import isomap

pytestmark = pytest.mark.gpu
CASES = [("roll257", 3), ("roll1000", 2), ("sphere193", 5)]
SUBSPACE_GAP = 0.011                 # (lambda_10 - lambda_11) / lambda_1 of sphere193


@pytest.fixture(scope="module")
def gold(golden):
    return golden("isomap.npz"), golden("isomap_embed.npz")


@pytest.fixture(scope="module")
def fits(gold):
    """(set, k) -> the fitted Isomap, each fitted once."""
    pts, _ = gold
    return {(name, k): isomap.Isomap(int(pts[f"{name}_nn"]), k).fit(pts[f"{name}_X"]) for name, k in CASES + [("sphere193", 10)]}


@pytest.mark.parametrize("name,k", CASES)
def test_embedding_and_transform_against_sklearn(gold, fits, name, k):
    pts, emb = gold
    iso = fits[(name, k)]
    want, want_tr, gmin = emb[f"{name}_k{k}_emb"], emb[f"{name}_k{k}_tr"], float(emb[f"{name}_k{k}_gmin"])
    Z = iso.embedding_.cpu().numpy()
    scale = np.abs(want).max()
    assert Z.shape == want.shape and iso.embedding_.dtype == torch.float64
    d_emb = np.abs(Z - want).max()
    d_tr = np.abs(iso.transform(emb[f"{name}_Xq"]).cpu().numpy() - want_tr).max()
    print(f"{name}, k = {k}: g_min = {gmin:.3g}; |embedding_ - scikit-learn| / max|Z| = {d_emb / scale:.3g} (bound {10 * 1e-9 / gmin:.3g}); "
          f"|transform - scikit-learn| / max|Z| = {d_tr / scale:.3g} (bound {100 * 1e-9 / gmin:.3g}); residual / lambda_1 = "
          f"{iso.residual_ / iso.eigenvalues_[0]:.3g}, plan {iso.plan_}")
    assert d_emb <= 10 * (1e-9 / gmin) * scale
    assert d_tr <= 100 * (1e-9 / gmin) * scale
    top = np.abs(Z).argmax(axis=0)
    assert (Z[top, np.arange(k)] > 0).all()                     # svd_flip: the entry of largest magnitude is positive
    np.testing.assert_allclose(iso.eigenvalues_, emb[f"{name}_eig64"][:k], rtol=0, atol=1e-10 * emb[f"{name}_eig64"][0])
    assert iso.dist_matrix_.shape == (want.shape[0],) * 2


def test_near_degenerate_columns_are_compared_as_a_subspace(gold, fits):
    _, emb = gold
    iso = fits[("sphere193", 10)]
    want, want_tr, lam1 = emb["sphere193_k10_emb"], emb["sphere193_k10_tr"], emb["sphere193_eig64"][0]
    Z = iso.embedding_.cpu().numpy()
    T = iso.transform(emb["sphere193_Xq"]).cpu().numpy()
    d_emb = np.abs(Z @ Z.T - want @ want.T).max()
    d_tr = np.abs(T @ Z.T - want_tr @ want.T).max()
    print(f"sphere193, k = 10: |Z Z^T - scikit-learn's| / lambda_1 = {d_emb / lam1:.3g} (bound {10 * 1e-9 / SUBSPACE_GAP:.3g}), "
          f"|T Z^T - scikit-learn's| / lambda_1 = {d_tr / lam1:.3g} (bound {100 * 1e-9 / SUBSPACE_GAP:.3g})")
    assert d_emb <= 10 * (1e-9 / SUBSPACE_GAP) * lam1
    assert d_tr <= 100 * (1e-9 / SUBSPACE_GAP) * lam1


@pytest.mark.parametrize("name,k", CASES)
def test_consistency_with_the_curve_and_with_the_fit(gold, fits, name, k):
    pts, emb = gold
    X, nn, iso = pts[f"{name}_X"], int(pts[f"{name}_nn"]), fits[(name, k)]
    assert iso.reconstruction_error() == isomap.reconstruction_errors(X, [k], n_neighbors=nn)[0]      # bit for bit
    Z = iso.embedding_.cpu().numpy()
    again = iso.transform(X[:16]).cpu().numpy()                 # a fitted point is its own nearest neighbour at distance 0
    tol = 10 * (1e-9 / float(emb[f"{name}_k{k}_gmin"])) * np.abs(Z).max()
    print(f"{name}, k = {k}: |transform(X[:16]) - embedding_[:16]| / max|Z| = {np.abs(again - Z[:16]).max() / np.abs(Z).max():.3g}")
    assert np.abs(again - Z[:16]).max() <= tol
    assert torch.equal(iso.fit_transform(X), iso.embedding_)


def test_a_disconnected_set_raises_the_existing_error():
    rng = np.random.default_rng(12)
    X = np.concatenate([rng.standard_normal((40, 3)), rng.standard_normal((45, 3)) + 100.0]).astype(np.float32)
    with pytest.raises(ValueError, match="2 connected components"):
        isomap.Isomap(4, 2).fit(X)
