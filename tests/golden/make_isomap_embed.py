"""Generator of tests/golden/isomap_embed.npz: scikit-learn's Isomap embedding and out-of-sample transform (CPU only).

    python tests/golden/make_isomap_embed.py

Needs scikit-learn, scipy and numpy.  The point sets are those of make_isomap.py (same generators, same seeds), the hold-out
queries 40 points of the same generator with seed 9 (its own isometry: they lie off the fitted manifold); eigen_solver="dense" on fp64 copies of the fp32 points, as there.  Per set
`s` and n_components `k` of CASES the file holds

    s_Xq            the queries [40, D] float32 (once per set)
    s_k{k}_emb      Isomap(nn, k).fit(X).embedding_                      [N, k]
    s_k{k}_tr       .transform(Xq)                                       [40, k]
    s_k{k}_gmin     min_{i <= k} (lambda_i - lambda_{i+1}) / lambda_1    the smallest relative gap the columns depend on
    s_eig64         the top 64 eigenvalues of the centred kernel (LAPACK, descending)
    s_eigmin        its smallest (most negative) eigenvalue
    sphere193_k10_vec, _qidx, _qdist   scikit-learn's eigenvectors_ [N, 10], kneighbors(Xq) indices [40, nn] and the distances
                    recomputed in numpy fp64 by direct differences (sum_d (q_d - x_d)^2, then sqrt)

The generator asserts that the nn-th and (nn+1)-th neighbour distances of every query differ by more than 1e-9 relative: the
neighbour sets do not hang on a rounding.
"""
import os
import warnings

import numpy as np
from sklearn.manifold import Isomap
from sklearn.preprocessing import KernelCenterer

from make_isomap import sphere, swiss_roll

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"roll257": (3,), "roll1000": (2,), "sphere193": (5, 10)}


def direct_distances(Xq, X):
    d = Xq.astype(np.float64)[:, None, :] - X.astype(np.float64)[None, :, :]
    return np.sqrt((d * d).sum(axis=2))


def record(out, name, X, Xq, nn, dist_check=None):
    X64, Xq64 = X.astype(np.float64), Xq.astype(np.float64)
    full = np.sort(direct_distances(Xq, X), axis=1)
    gap = (full[:, nn] - full[:, nn - 1]) / full[:, nn]
    assert gap.min() > 1e-9, (name, gap.min())
    out[f"{name}_Xq"] = Xq
    for k in CASES[name]:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            iso = Isomap(n_neighbors=nn, n_components=k, eigen_solver="dense").fit(X64)
            tr = iso.transform(Xq64)
        if dist_check is not None:
            assert np.array_equal(iso.dist_matrix_, dist_check)
        lam = np.linalg.eigvalsh(KernelCenterer().fit_transform(-0.5 * iso.dist_matrix_ ** 2))[::-1]
        gmin = float(np.min((lam[:k] - lam[1:k + 1]) / lam[0]))
        out[f"{name}_k{k}_emb"] = iso.embedding_
        out[f"{name}_k{k}_tr"] = tr
        out[f"{name}_k{k}_gmin"] = np.float64(gmin)
        out[f"{name}_eig64"] = lam[:64].copy()
        out[f"{name}_eigmin"] = np.float64(lam[-1])
        print(f"{name}: k = {k}: g_min = {gmin:.4g}, max |Z| = {np.abs(iso.embedding_).max():.4g}, lambda_min / lambda_1 = {lam[-1] / lam[0]:.3g}")
        if name == "sphere193" and k == 10:
            _, qidx = iso.nbrs_.kneighbors(Xq64, return_distance=True)
            out[f"{name}_k10_vec"] = iso.kernel_pca_.eigenvectors_
            out[f"{name}_k10_qidx"] = qidx.astype(np.int64)
            out[f"{name}_k10_qdist"] = np.take_along_axis(direct_distances(Xq, X), qidx, axis=1)


def main():
    out = {}
    gold = np.load(os.path.join(HERE, "isomap.npz"))
    sets = {"roll257": (swiss_roll(257, 1), swiss_roll(40, 9), 8), "roll1000": (swiss_roll(1000, 2), swiss_roll(40, 9), 8),
            "sphere193": (sphere(193, 3), sphere(40, 9), 6)}
    for name, (X, Xq, nn) in sets.items():
        assert np.array_equal(X, gold[f"{name}_X"]) and nn == int(gold[f"{name}_nn"])
        record(out, name, X, Xq, nn, dist_check=gold["sphere193_dist"] if name == "sphere193" else None)
    path = os.path.join(HERE, "isomap_embed.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes (isomap.npz:", os.path.getsize(os.path.join(HERE, "isomap.npz")), "bytes)")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "isomap.npz"))


if __name__ == "__main__":
    main()
