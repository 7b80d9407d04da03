"""GPU: the out-of-sample side of Isomap (csrc/isomap_project.hip): the neighbours of new points among the fitted ones and the fused
projection onto the fitted embedding.

Oracles: numpy fp64 brute force for the neighbours; isomap.transform_from_geodesics (numpy fp64) fed with scikit-learn's own
eigenvectors, neighbour indices and geodesic matrix from the fixtures for the projection.

Bounds.  Neighbour distances: the differences of fp32 coordinates are exact in fp64, so either side's sum of D squares carries at
most D roundings and the square root one more: 4 D 2^-53 relative covers both.  Projection, per component c of query i: every
term of Z_ic = sum_j (g'_ij - colmean_j - r_i + grand) A_jc is summed over N entries in some order on either side, so with
r_i = mean_j g'_ij the difference is within
8 N 2^-53 (sum_j |g'_ij| |A_jc| + sum_j |colmean_j| |A_jc| + (|r_i| + |grand|) sum_j |A_jc|), computed here from the fixture inputs.
"""
import numpy as np
import pytest
import torch

import id_diff_amd
from id_diff_amd import _lib, isomap

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -53


def np_knn_cross(Xq, X, k):
    d = Xq.astype(np.float64)[:, None, :] - X.astype(np.float64)[None, :, :]
    d2 = (d * d).sum(axis=2)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]          # equal distances: the lower index first
    return np.sqrt(np.take_along_axis(d2, idx, axis=1)), idx


@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("M,N,D", [(1, 7, 3), (40, 193, 16), (65, 257, 12)])
def test_knn_cross_against_numpy(M, N, D, k):
    rng = np.random.default_rng(1000 * M + N)
    X = rng.standard_normal((N, D)).astype(np.float32)
    Xq = rng.standard_normal((M, D)).astype(np.float32)
    if N > 200:                                                  # an exact tie in front of a query that is a fitted point
        X[200] = X[3]
        Xq[0] = X[3]
    dist, idx = _lib.knn_cross(torch.from_numpy(Xq).to(DEV), torch.from_numpy(X).to(DEV), k)
    want_d, want_i = np_knn_cross(Xq, X, k)
    got_d, got_i = dist.cpu().numpy(), idx.cpu().numpy()
    assert got_d.shape == (M, k) and got_i.shape == (M, k) and got_i.dtype == np.int64
    assert np.array_equal(got_i, want_i)
    rel = np.abs(got_d - want_d) / np.maximum(want_d, np.finfo(float).tiny)
    print(f"M, N, D, k = {M}, {N}, {D}, {k}: largest relative difference / (4 D 2^-53) = {rel.max() / (4 * D * U):.3g}")
    assert rel.max() <= 4 * D * U
    assert np.all(np.diff(got_d, axis=1) >= 0)
    if N > 200:
        assert got_d[0, 0] == 0.0 and got_i[0, 0] == 3 and (k == 1 or (got_d[0, 1] == 0.0 and got_i[0, 1] == 200))


@pytest.fixture(scope="module")
def fitted(golden):
    """scikit-learn's fit of sphere193 at 10 components: geodesics, eigenvectors, eigenvalues, the queries' neighbours."""
    gold, emb = golden("isomap.npz"), golden("isomap_embed.npz")
    D, V, lam = gold["sphere193_dist"], emb["sphere193_k10_vec"], emb["sphere193_eig64"][:10]
    S = -0.5 * D ** 2
    return {"D": D, "V": V, "lam": lam, "A": V / np.sqrt(lam), "colmean": S.mean(axis=0), "grand": S.mean(),
            "qd": emb["sphere193_k10_qdist"], "qi": emb["sphere193_k10_qidx"], "tr": emb["sphere193_k10_tr"]}


def device_project(f, qd, qi):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return _lib.isomap_project(t(qd), t(qi.astype(np.int64)), t(f["D"]), t(f["A"]), t(f["colmean"]),
                               torch.tensor(f["grand"], dtype=torch.float64, device=DEV)).cpu().numpy()


def projection_bound(f, qd, qi):
    N = f["D"].shape[0]
    G = -0.5 * (qd[:, :, None] + f["D"][qi]).min(axis=1) ** 2
    r = G.mean(axis=1)
    absA = np.abs(f["A"])
    return 8 * N * U * (np.abs(G) @ absA + (np.abs(f["colmean"]) @ absA)[None, :]
                        + (np.abs(r) + abs(f["grand"]))[:, None] * absA.sum(axis=0)[None, :])


@pytest.mark.parametrize("M", [1, 40])
def test_isomap_project_against_the_host_oracle(fitted, M):
    qd, qi = fitted["qd"][:M], fitted["qi"][:M]
    want = isomap.transform_from_geodesics(fitted["D"], fitted["V"], fitted["lam"], qd, qi)
    got = device_project(fitted, qd, qi)
    bound = projection_bound(fitted, qd, qi)
    print(f"M = {M}: largest |got - oracle| / bound = {(np.abs(got - want) / bound).max():.3g}; "
          f"|oracle - scikit-learn| = {np.abs(want - fitted['tr'][:M]).max():.3g}")
    assert got.shape == (M, 10)
    assert np.all(np.abs(got - want) <= bound)
    assert np.abs(want - fitted["tr"][:M]).max() <= 1e-9 * np.abs(fitted["tr"]).max()      # the oracle is scikit-learn's transform
    assert np.array_equal(got, device_project(fitted, qd, qi))                              # the same bits on every launch


def test_isomap_project_ignores_an_index_outside_the_fit(fitted):
    """An extra neighbour column with indices N + 5 and -1 at distance 0 (it would win every minimum if it were used)."""
    qd, qi = fitted["qd"], fitted["qi"]
    N = fitted["D"].shape[0]
    extra = np.where(np.arange(len(qi)) % 2 == 0, N + 5, -1)[:, None]
    got = device_project(fitted, np.concatenate([np.zeros((len(qd), 1)), qd], axis=1), np.concatenate([extra, qi], axis=1))
    assert np.array_equal(got, device_project(fitted, qd, qi))
