"""Isomap reconstruction error against the embedding dimension (the curve of the reference's isomap.py, figures/isomap.png).

The reference fits ``sklearn.manifold.Isomap(n_components=k)`` once per k (isomap.py:54-60): 29 neighbour graphs, 29
all-pairs shortest paths and 29 eigen-decompositions of the same matrix.  Every error follows from ONE geodesic matrix D and
ONE eigenvalue list:

    K = -1/2 J (D o D) J,   J = I - 1 1^T / N           (KernelCenterer on -1/2 D^2)
    error(k) = sqrt(||K||_F^2 - sum_{i < k} lambda_i^2) / N,   lambda_1 >= lambda_2 >= ... the eigenvalues of K

which is what ``Isomap(n_neighbors, n_components=k).fit(X).reconstruction_error()`` returns.  The device path is
``_lib.knn`` (exact fp64 neighbour distances) -> ``_lib.knn_graph`` -> ``_lib.geodesic_distances`` (blocked Floyd-Warshall,
csrc/geodesic.hip) -> ``_lib.double_center`` -> ``_lib.sym_eigvals``; the O(len(ks)) arithmetic after it is host fp64.

Not here: the embedding itself (eigenvectors), ``transform`` of new points, the random-forest score the reference computes
on the embedding (isomap.py:62-67), more than one GPU.
"""
import os
import pickle
import warnings

import numpy as np
import torch

from . import _lib
from .mle import _points

N_MAX = 12288                  # the largest matrix the eigensolver is exercised at in this project
_SMALL_POS_RATIO = 1e-12       # an eigenvalue counts as positive above this fraction of the largest (sklearn's fp64 ratio)
DEFAULT_KS = list(range(1, 11)) + list(range(11, 200, 10))        # isomap.py:51


# ------------------------------------------------------------------------------------------- host arithmetic
def count_components(finite):
    """Number of connected components from the finite pattern [N, N] (bool) of a shortest-path matrix: two vertices share a
    component exactly when their distance is finite, so a vertex's component is named by the first vertex it reaches."""
    finite = np.asarray(finite, dtype=bool)
    if finite.ndim != 2 or finite.shape[0] != finite.shape[1]:
        raise ValueError(f"finite pattern must be [N, N], got {finite.shape}")
    return int(np.unique(finite.argmax(axis=1)).size)


def n_positive(lam):
    """How many of the eigenvalues ``lam`` (descending) are positive: above 1e-12 of the largest."""
    lam = np.asarray(lam, dtype=np.float64)
    if lam.size == 0 or lam[0] <= 0:
        return 0
    return int(np.count_nonzero(lam > _SMALL_POS_RATIO * lam[0]))


def errors_from_eigenvalues(fro2, lam, N, ks):
    """error(k) for every k of ``ks`` from ||K||_F^2 and the eigenvalues of K in descending order (fp64 numpy)."""
    lam = np.asarray(lam, dtype=np.float64)
    ks = [int(k) for k in ks]
    pos = n_positive(lam)
    bad = [k for k in ks if k < 1 or k > pos]
    if bad:
        raise ValueError(f"n_components {bad} outside 1..{pos}: the centred geodesic kernel has {pos} positive eigenvalues")
    head = np.concatenate([[0.0], np.cumsum(lam[:max(ks, default=0)] ** 2)])
    return [float(np.sqrt(max(float(fro2) - head[k], 0.0)) / N) for k in ks]


def _center(D):
    S = np.asarray(D, dtype=np.float64) ** 2
    K = -0.5 * (S - S.mean(axis=1, keepdims=True) - S.mean(axis=0, keepdims=True) + S.mean())
    return K


def errors_from_geodesics(D, ks, return_eigenvalues=False):
    """The same arithmetic from a given geodesic matrix D [N, N], in numpy fp64 on the host (LAPACK eigenvalues)."""
    D = np.asarray(D, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError(f"D must be [N, N], got {D.shape}")
    if not np.isfinite(D).all():
        raise ValueError(f"the neighbourhood graph has {count_components(np.isfinite(D))} connected components")
    K = _center(D)
    lam = np.linalg.eigvalsh(K)[::-1]
    err = errors_from_eigenvalues(float((K * K).sum()), lam, D.shape[0], ks)
    return (err, lam) if return_eigenvalues else err


# ------------------------------------------------------------------------------------------- device path
def _n_rows(X):
    return int(X.shape[0]) if hasattr(X, "shape") else len(X)


def geodesics(X, n_neighbors=5):
    """Geodesic distances [N, N] (fp64 device tensor) of the points X over their ``n_neighbors``-nearest-neighbour graph.

    Raises ``ValueError`` naming the number of connected components when some pair is unreachable.  scikit-learn instead
    joins the components with extra edges (the closest pair of points between each two) and warns; we do not: a curve from
    such a repaired graph measures the repair."""
    Xd = _points(X)
    dist, idx, _ = _lib.knn(Xd, int(n_neighbors))
    D = _lib.geodesic_distances(_lib.knn_graph(dist, idx))
    finite = torch.isfinite(D)
    if not bool(finite.all()):
        raise ValueError(f"the {n_neighbors}-nearest-neighbour graph of the {Xd.shape[0]} points has "
                         f"{count_components(finite.cpu().numpy())} connected components: geodesic distances between them "
                         "are infinite (raise n_neighbors)")
    return D


def _kernel_spectrum(X, n_neighbors):
    """(||K||_F^2, eigenvalues of K descending [numpy fp64], N): one geodesic matrix, one centring, one eigensolve."""
    N = _n_rows(X)
    if N > N_MAX:
        raise ValueError(f"N = {N} points: the eigensolver of this project is exercised up to N = {N_MAX}")
    D = geodesics(X, n_neighbors)
    K, fro2 = _lib.double_center(D)
    eig = _lib.sym_eigvals(K)                               # K is overwritten
    if bool(torch.isnan(eig).any()):
        eig = _lib.solve_with_fallbacks(lambda: _lib.sym_eigvals(_lib.double_center(D)[0]))
    return float(fro2), eig.cpu().numpy()[::-1].copy(), N


def reconstruction_errors(X, ks, n_neighbors=5, return_eigenvalues=False):
    """``[Isomap(n_neighbors=n_neighbors, n_components=k).fit(X).reconstruction_error() for k in ks]`` as a list of floats.
    ``return_eigenvalues=True`` adds the eigenvalues of the centred kernel (descending, all N, fp64 numpy).  A k above the
    number of positive eigenvalues (those above 1e-12 of the largest) raises ``ValueError``.  scikit-learn raises where the top
    k include a significantly negative eigenvalue and sets tiny ones to zero without raising: in the narrow band of a k that
    reaches only eigenvalues within 1e-12 of zero it returns a value where this function raises.  N is limited to 12288."""
    fro2, lam, N = _kernel_spectrum(X, n_neighbors)
    err = errors_from_eigenvalues(fro2, lam, N, ks)
    return (err, lam) if return_eigenvalues else err


# ------------------------------------------------------------------------------------------- the reference script's job
def run(config, N=1000, ks=None, out_dir='isomap', n_neighbors=5):
    """isomap.py:37-75 of the reference: the first N points of the train loader, the error for every k of ``ks`` (default the
    reference's list) into ``out_dir/reconstruction_error.pkl`` (a plain list of floats) and, when matplotlib imports,
    ``reconstruction_error.png``.  Values of k beyond the positive eigenvalues are cut off with one warning.  -> (ks, errors)"""
    from .lightning_data_modules.utils import create_lightning_datamodule
    ks = list(DEFAULT_KS if ks is None else ks)
    DataModule = create_lightning_datamodule(config)
    DataModule.setup()
    rows, have = [], 0
    for item in DataModule.train_dataloader():
        x = item[0] if isinstance(item, (list, tuple)) else item
        rows.append(x.reshape(x.shape[0], -1))
        have += x.shape[0]
        if have >= N:
            break
    X = torch.cat(rows, dim=0)[:N]
    fro2, lam, n = _kernel_spectrum(X, n_neighbors)
    pos = n_positive(lam)
    kept = [k for k in ks if k <= pos]
    if len(kept) < len(ks):
        warnings.warn(f"isomap: the centred geodesic kernel of the {n} points has {pos} positive eigenvalues; "
                      f"n_components {[k for k in ks if k > pos]} are left out of the curve")
    values = errors_from_eigenvalues(fro2, lam, n, kept)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'reconstruction_error.pkl'), 'wb') as f:
        pickle.dump(values, f)
    try:
        from matplotlib.figure import Figure            # no pyplot: the process's backend is left alone
    except ImportError:
        Figure = None
    if Figure is not None:
        fig = Figure(figsize=(10, 10))
        fig.subplots().plot(kept, values)
        fig.savefig(os.path.join(out_dir, 'reconstruction_error.png'), dpi=300, facecolor='white')
    return kept, values


def main(argv=None):
    import argparse
    from .configs.utils import read_config
    ap = argparse.ArgumentParser(description="Isomap reconstruction-error curve of a data set's first N training points")
    ap.add_argument('--config', required=True)
    ap.add_argument('--N', type=int, default=1000)
    ap.add_argument('--n_neighbors', type=int, default=5)
    ap.add_argument('--out_dir', default='isomap')
    args = ap.parse_args(argv)
    ks, values = run(read_config(args.config), N=args.N, out_dir=args.out_dir, n_neighbors=args.n_neighbors)
    for k, v in zip(ks, values):
        print(f'k = {k}  reconstruction error: {v}')


if __name__ == '__main__':
    main()
