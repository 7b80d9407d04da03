"""Local PCA: the intrinsic dimension and the tangent space of every point from the spectrum of its neighbourhood's covariance.

Fukunaga-Olsen's estimator in its original form (R ``intrinsicDimension::pcaLocalDimEst``, which the reference reaches through
rpy2 and applies to the WHOLE data set, benchmark.py:64): for every point take its k nearest neighbours and read the dimension
off the eigenvalues of the covariance of those k + 1 points; the leading eigenvectors are the classical estimate of the tangent
space, to set beside ``get_manifold_dimension(..., return_tangent=True)``.

On the MI355X this is ``_lib.knn`` (exact, csrc/knn.hip) followed by ``_lib.local_pca`` (csrc/lpca.hip): one launch, one
workgroup per point, the (k + 1) x (k + 1) Gram matrix of the neighbourhood on the fp64 matrix cores and a cyclic Jacobi solve in
LDS.  What remains on the host is the threshold rule on [N, k] eigenvalues.  ``local_spectra_host`` restates the kernel's
arithmetic in fp64 numpy (the oracle of tests/test_hip_lpca.py).  Not checked against R or scikit-dimension: neither is available
to this project's tests.
"""
import os
import pickle

import numpy as np
import torch

from . import _lib
from .mle import _points

FO_ALPHA = 0.05                   # Fukunaga-Olsen: eigenvalues above this fraction of the largest count
RATIO_ALPHA = 0.95                # 'ratio': the leading eigenvalues that hold this fraction of the total variance
BASIS_BYTES = 256 << 20           # most bytes of the fp64 [Q, n_vectors, D] basis one launch of local_tangent may ask for
RULES = ('FO', 'ratio')


# ------------------------------------------------------------------------------------------- the spectra
def local_spectra(X, k=20, n_vectors=0, rows=None):
    """``(eig, basis, idx)`` for every row of X [N, D] -- or for the rows listed in ``rows`` (the neighbour search still runs over
    all of X): eig [Q, min(k, D)] fp64 descending, the covariance eigenvalues of the point and its k nearest neighbours; basis
    [Q, n_vectors, D] fp64 (None for n_vectors = 0), row v the unit eigenvector of eig[:, v]; idx [Q, k] int64 the neighbours.
    All on the GPU."""
    Xd = _points(X)
    _, idx, _ = _lib.knn(Xd, k)
    if rows is None:
        centre = torch.arange(Xd.shape[0], dtype=torch.int64, device=Xd.device)
    else:
        centre = torch.as_tensor(rows, dtype=torch.int64).reshape(-1).cpu()      # checked on the host: it indexes idx below
        if centre.numel() and (int(centre.min()) < 0 or int(centre.max()) >= Xd.shape[0]):
            raise IndexError(f"rows outside [0, {Xd.shape[0]})")
        centre = centre.to(Xd.device)
        idx = idx[centre].contiguous()
    eig, basis = _lib.local_pca(Xd, centre, idx, n_vectors)
    return eig, basis, idx


def local_spectra_host(X, idx, centre=None, n_vectors=0):
    """The arithmetic of csrc/lpca.hip in fp64 numpy: X [N, D], idx [Q, k] neighbour rows, centre [Q] (default 0 .. Q - 1) ->
    ``(eig [Q, min(k, D)], basis [Q, n_vectors, D] or None)``.  y_j = x_j - x_centre, G = Y Y^T over the m = k + 1 rows,
    B = J G J / (m - 1), eigh; vectors Y^T J u / sqrt((m - 1) lambda), NaN where lambda <= m 2^-52 lambda_1, largest component
    positive."""
    X = np.asarray(X.detach().cpu() if isinstance(X, torch.Tensor) else X, dtype=np.float64)
    idx = np.asarray(idx.detach().cpu() if isinstance(idx, torch.Tensor) else idx, dtype=np.int64)
    Q, k = idx.shape
    centre = np.arange(Q) if centre is None else np.asarray(
        centre.detach().cpu() if isinstance(centre, torch.Tensor) else centre, dtype=np.int64).reshape(-1)
    X = X.reshape(X.shape[0], -1)
    D, m = X.shape[1], k + 1
    r = min(k, D)
    eig = np.zeros((Q, r))
    basis = np.full((Q, n_vectors, D), np.nan) if n_vectors > 0 else None
    for q in range(Q):
        Y = X[np.concatenate([[centre[q]], idx[q]])] - X[centre[q]]
        G = Y @ Y.T
        rm = G.sum(axis=1) / m
        B = (G - (rm[:, None] + rm[None, :]) + rm.sum() / m) / (m - 1)
        lam, U = np.linalg.eigh(B)
        lam, U = lam[::-1], U[:, ::-1]
        eig[q] = np.maximum(lam[:r], 0.0)
        for v in range(n_vectors):
            if lam[0] > 0.0 and lam[v] > m * 2.0 ** -52 * lam[0]:
                u = U[:, v] - U[:, v].mean()
                t = (Y.T @ u) / np.sqrt((m - 1) * lam[v])
                basis[q, v] = -t if t[np.argmax(np.abs(t))] < 0.0 else t
    return eig, basis


# ------------------------------------------------------------------------------------------- dimensions from spectra
def dims_from_spectra(eig, rule='FO', alpha=None):
    """int64 [Q] from eig [Q, r] (descending): 'FO' the number of eigenvalues above alpha (0.05) times the largest
    (``benchmark.pca_fo_count``); 'ratio' the smallest d whose d leading eigenvalues hold at least alpha (0.95) of their sum.
    A zero spectrum gives 0; a spectrum that is not finite raises ``ValueError`` (no dimension is read off a NaN).  (No max-gap rule: on noiseless data in a (d + 1)-dimensional subspace its trailing ratios are
    rounding noise, and it answers k - 1.)"""
    from .benchmark import pca_fo_count
    eig = np.asarray(eig.detach().cpu() if isinstance(eig, torch.Tensor) else eig, dtype=np.float64)
    if eig.ndim != 2:
        raise ValueError(f"eig must be [Q, r], got {eig.shape}")
    if rule not in RULES:
        raise ValueError(f"unknown rule {rule!r} {RULES}")
    alpha = (FO_ALPHA if rule == 'FO' else RATIO_ALPHA) if alpha is None else float(alpha)
    if not np.isfinite(eig).all():
        raise ValueError(f"{int((~np.isfinite(eig)).any(axis=1).sum())} of {eig.shape[0]} spectra are not finite")
    dims = np.zeros(eig.shape[0], dtype=np.int64)
    for q, lam in enumerate(eig):
        if not lam.size or not lam.max() > 0.0:
            continue
        if rule == 'FO':
            dims[q] = pca_fo_count(lam, alpha)
        else:
            dims[q] = 1 + int(np.argmax(np.cumsum(lam) >= alpha * lam.sum()))
    return dims


def local_dims(X, k=20, rule='FO', alpha=None):
    """The local-PCA intrinsic dimension of every point of X: int64 numpy [N]."""
    eig, _, _ = local_spectra(X, k)
    return dims_from_spectra(eig, rule, alpha)


def local_tangent(X, k=20, dims=None, rule='FO', cap=_lib.TANGENT_MAX):
    """One float32 numpy array [D, d] per point, its orthonormal columns the d leading eigenvectors of the neighbourhood's
    covariance (d = dims[i], by default ``local_dims(X, k, rule)``) -- the layout of ``get_manifold_dimension(return_tangent=
    True)``, so the two compare column space to column space (``subspace_sine``) -- or None where d < 1 or d > min(cap, k).
    The queries go through the kernel in chunks whose fp64 basis stays under BASIS_BYTES."""
    Xd = _points(X)
    N, D = Xd.shape
    _, idx, _ = _lib.knn(Xd, k)
    if dims is None:
        eig, _ = _lib.local_pca(Xd, torch.arange(N, dtype=torch.int64, device=Xd.device), idx, 0)
        dims = dims_from_spectra(eig, rule)
    dims = np.asarray(dims, dtype=np.int64).reshape(-1)
    if dims.shape[0] != N:
        raise ValueError(f"dims has {dims.shape[0]} entries, X {N} rows")
    served = (dims >= 1) & (dims <= min(cap, k, D))
    out = [None] * N
    todo = np.flatnonzero(served)
    if todo.size == 0:
        return out
    # widest first, so that a chunk asks for no more vectors than its points need
    todo = todo[np.argsort(-dims[todo], kind='stable')]
    at = 0
    while at < todo.size:
        nv = int(dims[todo[at]])
        rows = todo[at:at + max(1, BASIS_BYTES // (8 * nv * D))]
        centre = torch.from_numpy(rows).to(Xd.device)
        _, basis = _lib.local_pca(Xd, centre, idx[centre].contiguous(), nv)
        basis = basis.to(torch.float32).cpu().numpy()
        for i, b in zip(rows, basis):
            out[i] = np.ascontiguousarray(b[:dims[i]].T)
        at += rows.size
    return out


def subspace_sine(A, B):
    """Sine of the largest principal angle between the column spaces of A and B ([D, d] each, orthonormal columns):
    || (I - A A^T) B ||_2, in fp64."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if A.ndim != 2 or A.shape != B.shape:
        raise ValueError(f"two [D, d] bases of one shape expected, got {A.shape} and {B.shape}")
    return float(np.linalg.norm(B - A @ (A.T @ B), 2))


# ------------------------------------------------------------------------------------------- a data set from a config
def run(config, k=20, rule='FO', out_dir='lpca'):
    """The train split of the config's data set, taken exactly as ``benchmark.Benchmark.create_dataset`` takes it -> the
    local-PCA dimension of every point into ``out_dir/local_dims.pkl`` = {'dims', 'eigenvalues', 'k', 'rule'}; prints the
    histogram of the dimensions.  -> dims."""
    from .lightning_data_modules.utils import create_lightning_datamodule
    DataModule = create_lightning_datamodule(config)
    DataModule.setup()
    X = _points(torch.cat([x.reshape(x.shape[0], -1) for x in DataModule.train_dataloader()], dim=0))
    eig, _, _ = local_spectra(X, k)
    eig = eig.cpu().numpy()
    dims = dims_from_spectra(eig, rule)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'local_dims.pkl'), 'wb') as f:
        pickle.dump({'dims': dims, 'eigenvalues': eig, 'k': k, 'rule': rule}, f)
    values, counts = np.unique(dims, return_counts=True)
    print(f'local PCA ({rule}, k = {k}) on {len(dims)} points: mean {dims.mean():.3f}')
    for v, c in zip(values, counts):
        print(f'  dim {int(v):3d}: {int(c)}')
    return dims


def main(argv=None):
    import argparse
    from .configs.utils import read_config
    ap = argparse.ArgumentParser(description="Local-PCA intrinsic dimension of every training point of a data set")
    ap.add_argument('--config', required=True)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--rule', choices=RULES, default='FO')
    ap.add_argument('--out_dir', default='lpca')
    args = ap.parse_args(argv)
    run(read_config(args.config), k=args.k, rule=args.rule, out_dir=args.out_dir)


if __name__ == '__main__':
    main()
