"""Isomap: the reconstruction error against the embedding dimension (the curve of the reference's isomap.py, figures/isomap.png),
the embedding itself, and the coordinates of points that were not in the fit.

The reference fits ``sklearn.manifold.Isomap(n_components=k)`` once per k (isomap.py:54-60): 29 neighbour graphs, 29
all-pairs shortest paths and 29 eigen-decompositions of the same matrix.  Every error follows from ONE geodesic matrix D and
ONE eigenvalue list:

    K = -1/2 J (D o D) J,   J = I - 1 1^T / N           (KernelCenterer on -1/2 D^2)
    error(k) = sqrt(||K||_F^2 - sum_{i < k} lambda_i^2) / N,   lambda_1 >= lambda_2 >= ... the eigenvalues of K

which is what ``Isomap(n_neighbors, n_components=k).fit(X).reconstruction_error()`` returns.  The device path is
``_lib.knn`` (exact fp64 neighbour distances) -> ``_lib.knn_graph`` -> ``_lib.geodesic_distances`` (blocked Floyd-Warshall,
csrc/geodesic.hip) -> ``_lib.double_center`` -> ``_lib.sym_eigvals``; the O(len(ks)) arithmetic after it is host fp64.

The embedding (class ``Isomap``) adds the k largest eigenpairs of K: ``_lib.double_center`` once more (the eigenvalue solver
overwrites K) -> ``_lib.sym_topvecs`` (Chebyshev-filtered subspace iteration, csrc/topvecs.hip, scheduled from the eigenvalues
already at hand), embedding = V sqrt(lambda) with scikit-learn's column signs.  ``transform`` places new points with
``_lib.knn_cross`` -> ``_lib.isomap_project`` (csrc/isomap_project.hip).  ``run(embed=True)`` writes the embeddings and, given
labels and scikit-learn, the random-forest scores the reference computes on them (isomap.py:56-67), fitted on the host.

A neighbourhood graph that is not connected raises by default (``connect="raise"``).  ``connect="closest"`` does what scikit-learn
does without being asked (``sklearn.utils.graph._fix_connected_components``, mode "distance"): it joins every two components by
the closest pair of points between them, warns once, and carries on.  The components are read off the first shortest-path matrix
(``_lib.component_labels``), the closest pairs are an fp64 brute force over the pairs of points of different components
(``_lib.component_bridges``, csrc/graph_connect.hip), and the matrix is updated through the few endpoints of the new edges instead
of being solved again (``_lib.repair_geodesics``).  ``component_labels``, ``bridges_from_points`` and ``repair_geodesics`` below
restate the three steps in numpy.  At most 1024 components.

Not here: more than one GPU, n_components > 64, radius neighbourhoods.
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
C_MAX = 1024                   # most connected components connect="closest" joins (523,776 pairs of them)
CONNECT = ("raise", "closest")


# ------------------------------------------------------------------------------------------- host arithmetic
def count_components(finite):
    """Number of connected components from the finite pattern [N, N] (bool) of a shortest-path matrix: two vertices share a
    component exactly when their distance is finite, so a vertex's component is named by the first vertex it reaches."""
    finite = np.asarray(finite, dtype=bool)
    if finite.ndim != 2 or finite.shape[0] != finite.shape[1]:
        raise ValueError(f"finite pattern must be [N, N], got {finite.shape}")
    return int(np.unique(finite.argmax(axis=1)).size)


def _check_connect(connect):
    if connect not in CONNECT:
        raise ValueError(f"connect = {connect!r}, expected one of {CONNECT}")
    return connect


def _check_count(C):
    if C > C_MAX:
        raise ValueError(f"the neighbourhood graph has {C} connected components: connect='closest' joins at most {C_MAX}")
    return C


def component_labels(finite):
    """Component labels [N] (int64) from the finite pattern [N, N] (bool) of a shortest-path matrix: 0 .. C - 1 in the order of each
    component's smallest vertex, as ``scipy.sparse.csgraph.connected_components`` numbers them."""
    finite = np.asarray(finite, dtype=bool)
    if finite.ndim != 2 or finite.shape[0] != finite.shape[1]:
        raise ValueError(f"finite pattern must be [N, N], got {finite.shape}")
    first = finite.argmax(axis=1)
    return np.searchsorted(np.unique(first), first).astype(np.int64)


def bridges_from_points(X, labels):
    """The edges scikit-learn joins the components with (``_fix_connected_components``, mode "distance"), in numpy fp64 from the fp32
    values of X [N, D]: ``(i, j, w)``, int64 [B], int64 [B], fp64 [B], B = C (C - 1) / 2.  For every component a = 0 .. C - 1 and every
    b < a, the pair (i in a, j in b) of smallest Euclidean distance w (the square root of the sum of squared differences); on an
    exact tie the first in row-major order over (rank of i in a, rank of j in b), ranks by ascending index: ``D.argmin()`` on
    ``X[idx_a]`` x ``X[idx_b]``.  More than 1024 components raise ``ValueError``."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    labels = np.asarray(labels).astype(np.int64)
    if X.ndim != 2 or labels.shape != (X.shape[0],):
        raise ValueError(f"X must be [N, D] and labels [N], got {X.shape} and {labels.shape}")
    C = _check_count(int(labels.max()) + 1 if labels.size else 0)
    members = [np.flatnonzero(labels == c) for c in range(C)]
    bi, bj, bw = [], [], []
    for a in range(C):
        for b in range(a):
            diff = X[members[a]][:, None, :] - X[members[b]][None, :, :]
            d = np.sqrt((diff * diff).sum(axis=2))
            ii, jj = np.unravel_index(d.argmin(), d.shape)
            bi.append(members[a][ii]); bj.append(members[b][jj]); bw.append(d[ii, jj])
    return np.array(bi, dtype=np.int64), np.array(bj, dtype=np.int64), np.array(bw, dtype=np.float64)


def repair_geodesics(D0, bridges):
    """All-pairs shortest paths of the graph behind D0 [N, N] (its shortest paths, +inf between components) plus the undirected edges
    ``bridges`` = (i, j, w), in numpy fp64: the edges are min-ed in, then one Floyd-Warshall step per distinct endpoint (a path
    that uses a new edge passes only endpoints between its two legs inside a component, and those legs are entries of D0)."""
    D = np.array(D0, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError(f"D0 must be [N, N], got {D.shape}")
    bi, bj, bw = (np.asarray(v) for v in bridges)
    D[bi, bj] = np.minimum(D[bi, bj], bw)
    D[bj, bi] = np.minimum(D[bj, bi], bw)
    for k in np.unique(np.concatenate([bi, bj])).astype(np.int64):
        np.minimum(D, D[:, k:k + 1] + D[k:k + 1, :], out=D)
    return D


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


def svd_flip_columns(V):
    """V with each column's sign chosen so that its entry of largest magnitude is positive (scikit-learn's ``svd_flip`` on the
    eigenvectors, as KernelPCA applies it); numpy array or torch tensor."""
    if isinstance(V, torch.Tensor):
        top = V.gather(0, V.abs().argmax(dim=0, keepdim=True))
        return V * torch.where(top < 0, -torch.ones_like(top), torch.ones_like(top))
    V = np.asarray(V)
    top = V[np.abs(V).argmax(axis=0), np.arange(V.shape[1])]
    return V * np.where(top < 0, -1.0, 1.0)


def errors_from_geodesics(D, ks, return_eigenvalues=False, return_embedding=False):
    """The same arithmetic from a given geodesic matrix D [N, N], in numpy fp64 on the host (LAPACK).  ``return_embedding=True``
    adds ``(V, lam_k)`` for k = max(ks): the eigenvectors [N, k] of the k largest eigenvalues with scikit-learn's signs and those
    eigenvalues; the embedding is ``V * sqrt(lam_k)``."""
    D = np.asarray(D, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError(f"D must be [N, N], got {D.shape}")
    if not np.isfinite(D).all():
        raise ValueError(f"the neighbourhood graph has {count_components(np.isfinite(D))} connected components")
    K = _center(D)
    if return_embedding:
        w, W = np.linalg.eigh(K)
        lam = w[::-1]
    else:
        lam = np.linalg.eigvalsh(K)[::-1]
    err = errors_from_eigenvalues(float((K * K).sum()), lam, D.shape[0], ks)
    out = (err, lam) if return_eigenvalues else (err,)
    if return_embedding:
        k = max(int(k) for k in ks)
        out += ((svd_flip_columns(W[:, ::-1][:, :k]), lam[:k].copy()),)
    return out if len(out) > 1 else err


def transform_from_geodesics(D, V, lam, dist, idx):
    """scikit-learn's ``Isomap.transform`` in numpy fp64 on the host: D [N, N] the fitted geodesic matrix, V [N, k] and lam [k] the
    eigenvectors and eigenvalues of the embedding, dist / idx [M, n] the distances to and the indices of each new point's nearest
    fitted points.  -> Z [M, k]"""
    D, V, lam = np.asarray(D, dtype=np.float64), np.asarray(V, dtype=np.float64), np.asarray(lam, dtype=np.float64)
    dist, idx = np.asarray(dist, dtype=np.float64), np.asarray(idx)
    G = (dist[:, :, None] + D[idx]).min(axis=1)                    # [M, N]
    G = -0.5 * G ** 2
    S = -0.5 * D ** 2
    colmean = S.mean(axis=0)
    G = G - colmean[None, :] - G.mean(axis=1, keepdims=True) + colmean.mean()
    return G @ (V / np.sqrt(lam))


# ------------------------------------------------------------------------------------------- device path
def _n_rows(X):
    return int(X.shape[0]) if hasattr(X, "shape") else len(X)


_NO_BRIDGES = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float64))


def _geodesics(X, n_neighbors, connect):
    """(D, number of components of the neighbourhood graph, the bridges (i, j, w) as numpy): what ``geodesics`` documents."""
    _check_connect(connect)
    Xd = _points(X)
    dist, idx, _ = _lib.knn(Xd, int(n_neighbors))
    D = _lib.geodesic_distances(_lib.knn_graph(dist, idx))
    if connect == "raise":
        finite = torch.isfinite(D)
        if not bool(finite.all()):
            raise ValueError(f"the {n_neighbors}-nearest-neighbour graph of the {Xd.shape[0]} points has "
                             f"{count_components(finite.cpu().numpy())} connected components: geodesic distances between them "
                             "are infinite (raise n_neighbors)")
        return D, 1, _NO_BRIDGES
    labels, count = _lib.component_labels(D)
    C = int(count)                                               # the one host read the default path spends on isfinite().all()
    if C == 1:
        return D, 1, _NO_BRIDGES
    _check_count(C)
    warnings.warn(f"isomap: the {n_neighbors}-nearest-neighbour graph of the {Xd.shape[0]} points has {C} connected components; "
                  "connect='closest' joins every two of them by their closest pair of points, as scikit-learn does", UserWarning,
                  stacklevel=3)
    bi, bj, bw = _lib.component_bridges(Xd, labels, C)
    D = _lib.repair_geodesics(D, bi, bj, bw, knn=(dist, idx))
    return D, C, (bi.cpu().numpy(), bj.cpu().numpy(), bw.cpu().numpy())


def geodesics(X, n_neighbors=5, connect="raise"):
    """Geodesic distances [N, N] (fp64 device tensor) of the points X over their ``n_neighbors``-nearest-neighbour graph.

    ``connect="raise"``: raises ``ValueError`` naming the number of connected components when some pair is unreachable: a curve
    from a repaired graph measures the repair.  ``connect="closest"``: what scikit-learn does instead.  It joins the components
    with extra edges (the closest pair of points between each two), warns once with their number, and returns the shortest paths
    of the joined graph; on a connected graph it changes nothing and does not warn."""
    return _geodesics(X, n_neighbors, connect)[0]


def _kernel_spectrum(X, n_neighbors, return_geodesics=False, connect="raise"):
    """(||K||_F^2, eigenvalues of K descending [numpy fp64], N): one geodesic matrix, one centring, one eigensolve.
    ``return_geodesics=True`` adds (D, number of components, bridges)."""
    _check_connect(connect)
    N = _n_rows(X)
    if N > N_MAX:
        raise ValueError(f"N = {N} points: the eigensolver of this project is exercised up to N = {N_MAX}")
    D, C, bridges = _geodesics(X, n_neighbors, connect)
    K, fro2 = _lib.double_center(D)
    eig = _lib.sym_eigvals(K)                               # K is overwritten
    if bool(torch.isnan(eig).any()):
        eig = _lib.solve_with_fallbacks(lambda: _lib.sym_eigvals(_lib.double_center(D)[0]))
    out = float(fro2), eig.cpu().numpy()[::-1].copy(), N
    return out + (D, C, bridges) if return_geodesics else out


def reconstruction_errors(X, ks, n_neighbors=5, return_eigenvalues=False, connect="raise"):
    """``[Isomap(n_neighbors=n_neighbors, n_components=k).fit(X).reconstruction_error() for k in ks]`` as a list of floats.
    ``return_eigenvalues=True`` adds the eigenvalues of the centred kernel (descending, all N, fp64 numpy).  A k above the
    number of positive eigenvalues (those above 1e-12 of the largest) raises ``ValueError``.  scikit-learn raises where the top
    k include a significantly negative eigenvalue and sets tiny ones to zero without raising: in the narrow band of a k that
    reaches only eigenvalues within 1e-12 of zero it returns a value where this function raises.  N is limited to 12288.
    ``connect``: as in ``geodesics``."""
    fro2, lam, N = _kernel_spectrum(X, n_neighbors, connect=connect)
    err = errors_from_eigenvalues(fro2, lam, N, ks)
    return (err, lam) if return_eigenvalues else err


RESID_TOL = 1e-9                # fit() accepts |K V - V diag(lambda)|_F up to this times lambda_1 sqrt(k)


class Isomap:
    """``sklearn.manifold.Isomap(n_neighbors, n_components)`` on the device path of this module: ``fit`` / ``fit_transform`` /
    ``transform`` / ``reconstruction_error``.  After ``fit``: ``embedding_`` [N, k] fp64 device tensor (= V sqrt(lambda), each
    column's entry of largest magnitude positive, as scikit-learn's ``svd_flip`` leaves it), ``dist_matrix_`` [N, N] fp64 device
    tensor (the geodesic distances), ``eigenvalues_`` [k] fp64 numpy, descending, ``n_connected_components_`` (int) of the
    neighbourhood graph and ``bridges_`` = (i, j, w), numpy int64 [B], int64 [B], fp64 [B], the edges ``connect="closest"`` joined
    them with (B = C (C - 1) / 2; empty for one component).  A disconnected neighbourhood graph (unless ``connect="closest"``, see
    ``geodesics``), N > 12288 and an n_components above the number of positive eigenvalues raise ``ValueError`` as
    ``reconstruction_errors`` does; a basis whose residual exceeds 1e-9 lambda_1 sqrt(k) raises ``RuntimeError``.  n_components <= 64."""

    def __init__(self, n_neighbors=5, n_components=2, connect="raise"):
        self.n_neighbors, self.n_components, self.connect = int(n_neighbors), int(n_components), _check_connect(connect)
        if not 1 <= self.n_components <= _lib.TOPVECS_MAX:
            raise ValueError(f"n_components = {n_components} outside 1..{_lib.TOPVECS_MAX}")

    def fit(self, X):
        k = self.n_components
        fro2, lam, N, D, C, bridges = _kernel_spectrum(X, self.n_neighbors, return_geodesics=True, connect=self.connect)   # refuses N > 12288 before any device call
        self.n_connected_components_, self.bridges_ = int(C), bridges
        self._error = errors_from_eigenvalues(fro2, lam, N, [k])[0]           # raises for k beyond the positive eigenvalues
        self.plan_ = _lib.topvecs_plan(lam, k)
        K, _, (colmean, grand) = _lib.double_center(D, return_means=True)     # again: the eigenvalue solver has overwritten K
        V, ritz, resid = _lib.sym_topvecs(K, k, lam, plan=self.plan_)
        Xd = _points(X).to(D.device)
        resid, top = float(resid), float(lam[0])
        if not resid <= RESID_TOL * top * np.sqrt(k):
            raise RuntimeError(f"isomap: the eigenvector residual |K V - V diag(lambda)|_F = {resid!r} exceeds "
                               f"{RESID_TOL} * lambda_1 * sqrt(k) = {RESID_TOL * top * np.sqrt(k)!r} (n_components = {k})")
        V = svd_flip_columns(V)
        root = torch.sqrt(ritz)
        self.embedding_ = V * root
        self.eigenvalues_ = ritz.cpu().numpy()
        self.dist_matrix_, self.residual_ = D, resid
        self._fit_X, self._A, self._colmean, self._grand = Xd, (V / root).contiguous(), colmean.contiguous(), grand.reshape(1).contiguous()
        return self

    def fit_transform(self, X):
        return self.fit(X).embedding_

    def transform(self, X):
        """Coordinates [M, k] (fp64 device tensor) of new points: their ``n_neighbors`` nearest fitted points, the shortest way into
        the fitted graph through one of them, and the projection onto the fitted eigenvectors."""
        Xq = _points(X).to(self._fit_X.device)
        if Xq.shape[1] != self._fit_X.shape[1]:
            raise ValueError(f"transform: points of dimension {Xq.shape[1]}, fitted on dimension {self._fit_X.shape[1]}")
        dist, idx = _lib.knn_cross(Xq, self._fit_X, self.n_neighbors)
        return _lib.isomap_project(dist, idx, self.dist_matrix_, self._A, self._colmean, self._grand)

    def reconstruction_error(self):
        return self._error


# ------------------------------------------------------------------------------------------- the reference script's job
def classifier_scores(train, y_train, test, y_test):
    """Accuracy of ``RandomForestClassifier(random_state=0)`` fitted to ``train`` / ``y_train`` and scored on ``test`` / ``y_test``
    (isomap.py:62-67 of the reference), on the host.  Needs scikit-learn."""
    from sklearn.ensemble import RandomForestClassifier
    clf = RandomForestClassifier(random_state=0).fit(np.asarray(train), np.asarray(y_train))
    return float(clf.score(np.asarray(test), np.asarray(y_test)))


def _first_rows(loader, N):
    """(X [<= N, D], labels [<= N] or None) from the first batches of a loader."""
    rows, labels, have = [], [], 0
    for item in loader:
        pair = isinstance(item, (list, tuple))
        x = item[0] if pair else item
        rows.append(x.reshape(x.shape[0], -1))
        if pair and len(item) > 1 and labels is not None and torch.is_tensor(item[1]) and item[1].shape[:1] == x.shape[:1]:
            labels.append(item[1].reshape(x.shape[0], -1)[:, 0])
        else:
            labels = None
        have += x.shape[0]
        if have >= N:
            break
    return torch.cat(rows, dim=0)[:N], (torch.cat(labels)[:N].cpu().numpy() if labels else None)


def _embed(DataModule, X, y, N, ks, out_dir, n_neighbors, pos, connect="raise"):
    """The ``embed=True`` part of ``run``: embedding.pkl ({k: [N, k] array} for k in (2, 3)) and, with labels and scikit-learn,
    clf_scores.pkl ({k: accuracy} for every k <= 64 of ``ks``).  ONE fit, at the largest k asked for: column i of the embedding
    and of ``transform`` belongs to eigenvalue i whatever n_components is, so the embedding of k components is the first k
    columns.  A largest k whose eigenvectors ``_lib.topvecs_plan`` refuses (eigenvalues too close to separate) is given up for
    the next smaller one, with one warning that names the values of k left out."""
    wanted = sorted({k for k in list(ks) + [2, 3] if 1 <= k <= min(pos, _lib.TOPVECS_MAX, X.shape[0] - 1)})
    iso, refused = None, []
    while wanted and iso is None:
        try:
            iso = Isomap(n_neighbors, wanted[-1], connect=connect).fit(X)
        except ValueError as e:
            if "topvecs_plan" not in str(e):
                raise
            refused.insert(0, wanted.pop())
            why = str(e)
    if refused:
        warnings.warn(f"isomap: no embedding for n_components {refused}: {why}")
    Z = iso.embedding_.cpu().numpy() if iso is not None else None
    emb = {k: Z[:, :k].copy() for k in (2, 3) if k in wanted}
    with open(os.path.join(out_dir, 'embedding.pkl'), 'wb') as f:
        pickle.dump(emb, f)
    try:
        import sklearn  # noqa: F401
        have_sklearn = True
    except ImportError:
        have_sklearn = False
    Xt, yt = _first_rows(DataModule.test_dataloader(), N) if y is not None and have_sklearn and iso is not None else (None, None)
    if yt is None:
        warnings.warn("isomap: no classifier scores (" + ("scikit-learn is not installed" if not have_sklearn else
                                                           "the loaders yield no labels") + ")")
        return emb, None
    T = iso.transform(Xt).cpu().numpy()
    scores = {k: classifier_scores(Z[:, :k], y, T[:, :k], yt) for k in wanted if k in ks}
    with open(os.path.join(out_dir, 'clf_scores.pkl'), 'wb') as f:
        pickle.dump(scores, f)
    return emb, scores


def run(config, N=1000, ks=None, out_dir='isomap', n_neighbors=5, embed=False, connect="raise"):
    """isomap.py:37-75 of the reference: the first N points of the train loader, the error for every k of ``ks`` (default the
    reference's list) into ``out_dir/reconstruction_error.pkl`` (a plain list of floats) and, when matplotlib imports,
    ``reconstruction_error.png``.  Values of k beyond the positive eigenvalues are cut off with one warning.  -> (ks, errors)
    ``embed=True`` also writes ``embedding.pkl`` (n_components 2 and 3) and, when the loaders yield labels and scikit-learn
    imports, ``clf_scores.pkl``: the random-forest accuracy on the transformed test points for every k <= 64 of ``ks``.
    ``connect``: as in ``geodesics``; checked before the data are loaded."""
    from .lightning_data_modules.utils import create_lightning_datamodule
    _check_connect(connect)
    ks = list(DEFAULT_KS if ks is None else ks)
    DataModule = create_lightning_datamodule(config)
    DataModule.setup()
    X, y = _first_rows(DataModule.train_dataloader(), N)
    fro2, lam, n = _kernel_spectrum(X, n_neighbors, connect=connect)
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
    if embed:
        _embed(DataModule, X, y, N, kept, out_dir, n_neighbors, pos, connect)
    return kept, values


def main(argv=None):
    import argparse
    from .configs.utils import read_config
    ap = argparse.ArgumentParser(description="Isomap reconstruction-error curve of a data set's first N training points")
    ap.add_argument('--config', required=True)
    ap.add_argument('--N', type=int, default=1000)
    ap.add_argument('--n_neighbors', type=int, default=5)
    ap.add_argument('--out_dir', default='isomap')
    ap.add_argument('--embed', action='store_true', help='also write embedding.pkl and, with labels and scikit-learn, clf_scores.pkl')
    ap.add_argument('--connect', choices=CONNECT, default='raise',
                    help="a disconnected neighbourhood graph: 'raise' (default) or 'closest', scikit-learn's repair (join every two "
                         "components by their closest pair of points, with a warning)")
    args = ap.parse_args(argv)
    ks, values = run(read_config(args.config), N=args.N, out_dir=args.out_dir, n_neighbors=args.n_neighbors, embed=args.embed,
                     connect=args.connect)
    for k, v in zip(ks, values):
        print(f'k = {k}  reconstruction error: {v}')


if __name__ == '__main__':
    main()
