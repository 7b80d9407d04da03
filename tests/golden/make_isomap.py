"""Generator of tests/golden/isomap.npz: scikit-learn's Isomap on three small seeded point sets (CPU only).

    python tests/golden/make_isomap.py

Needs scikit-learn, scipy and numpy.  eigen_solver="dense" (LAPACK): "auto" would take ARPACK with a random start vector for
k < 10 at N > 200 and the file would differ from run to run in the 12th digit.  The points are float32 (what the device path
takes); scikit-learn gets the same values as float64, as the reference's isomap.py:28 does.  Per set `s` the file holds

    s_X           the points [N, D] float32
    s_nn          n_neighbors
    s_ks, s_err   Isomap(n_neighbors, n_components=k).fit(X).reconstruction_error() for k in {1, 2, 3, 5, 10} and every k of the
                  reference's list up to 101 that scikit-learn accepts
    s_rows        16 fixed row indices,  s_dist_rows = dist_matrix_[rows]
    s_eig         the top 32 eigenvalues of the centred kernel (LAPACK, descending)
    s_dist        the full dist_matrix_ (sphere193 only: 300 KB)
"""
import os
import warnings

import numpy as np
from sklearn.datasets import make_swiss_roll
from sklearn.manifold import Isomap
from sklearn.preprocessing import KernelCenterer

HERE = os.path.dirname(os.path.abspath(__file__))
KS = sorted(set([1, 2, 3, 5, 10] + list(range(1, 11)) + list(range(11, 102, 10))))


def isometry(rng, d_out, d_in):
    q, _ = np.linalg.qr(rng.standard_normal((d_out, d_in)))
    return q                                                # [d_out, d_in], orthonormal columns


def swiss_roll(n, seed):
    rng = np.random.default_rng(seed)
    roll, _ = make_swiss_roll(n, random_state=seed)
    return (roll @ isometry(rng, 12, 3).T).astype(np.float32)


def sphere(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((n, 5))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    return (p @ isometry(rng, 16, 5).T).astype(np.float32)


def record(out, name, X, nn):
    X64 = X.astype(np.float64)
    ks, errs, dist = [], [], None
    for k in KS:
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("error")              # a disconnected graph (sklearn repairs it with a warning) is no fixture
                iso = Isomap(n_neighbors=nn, n_components=k, eigen_solver="dense").fit(X64)
            err = float(iso.reconstruction_error())
        except Exception as e:                              # scikit-learn refuses this k
            print(f"{name}: k = {k} refused by scikit-learn: {type(e).__name__}: {e}")
            continue
        if not np.isfinite(err):
            print(f"{name}: k = {k}: scikit-learn returns {err}")
            continue
        ks.append(k)
        errs.append(err)
        if dist is None:
            dist = np.array(iso.dist_matrix_, dtype=np.float64)
        else:
            assert np.array_equal(dist, iso.dist_matrix_)
    assert {1, 2, 3, 5, 10} <= set(ks), ks
    assert np.isfinite(dist).all()
    N = X.shape[0]
    rows = np.sort(np.random.default_rng(N).choice(N, size=16, replace=False))
    K = KernelCenterer().fit_transform(-0.5 * dist ** 2)
    eig = np.linalg.eigvalsh(K)[::-1][:32]
    out[f"{name}_X"] = X
    out[f"{name}_nn"] = np.int64(nn)
    out[f"{name}_ks"] = np.array(ks, dtype=np.int64)
    out[f"{name}_err"] = np.array(errs, dtype=np.float64)
    out[f"{name}_rows"] = rows.astype(np.int64)
    out[f"{name}_dist_rows"] = dist[rows]
    out[f"{name}_eig"] = eig
    print(f"{name}: N = {N}, ks = {ks}, err[0] = {errs[0]:.6g}, eig[0] = {eig[0]:.6g}")
    return dist


def main():
    out = {}
    record(out, "roll257", swiss_roll(257, 1), 8)
    record(out, "roll1000", swiss_roll(1000, 2), 8)
    out["sphere193_dist"] = record(out, "sphere193", sphere(193, 3), 6)
    path = os.path.join(HERE, "isomap.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
