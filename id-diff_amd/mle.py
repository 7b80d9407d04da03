"""Levina-Bickel maximum-likelihood intrinsic dimension (drop-in for /root/reference/mle.py).

Same three functions, signatures and return shapes.  The neighbour distances come from one exact kNN on the MI355X
(``_lib.knn``, csrc/knn.hip) instead of sklearn's ball tree (``NearestNeighbors(...).kneighbors``, mle.py:19-20 /
:47-48 / :80-81); a zero self column is put in front of them so that the reference's column arithmetic (self first,
then the neighbours) applies unchanged.  ``dist``, when given, has the reference's layout: [N, >= k + 1], self first.
The per-point arithmetic stays on the host in fp64 (mle.py:21-28).
"""
import numpy as np
import torch

from . import _lib


def _points(X):
    """X (numpy array, pandas DataFrame or torch tensor) as a [N, D] fp32 contiguous tensor on the GPU."""
    if isinstance(X, torch.Tensor):
        t = X
    else:
        if hasattr(X, "to_numpy"):                    # pandas DataFrame
            X = X.to_numpy()
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(X)))
    dev = t.device if t.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    return t.reshape(t.shape[0], -1).to(device=dev, dtype=torch.float32).contiguous()


def neighbour_distances(X, k):
    """[N, k + 1] fp64 numpy: a zero self column, then the distances to the k nearest other points (ascending)."""
    dist, _, _ = _lib.knn(_points(X), k)
    d = dist.cpu().numpy()
    return np.concatenate([np.zeros((d.shape[0], 1)), d], axis=1)


def _sample_wise(dist, k):
    dist = np.asarray(dist, dtype=np.float64)[:, 1:(k + 1)]
    if dist.shape[1] != k:
        raise ValueError(f"dist has {dist.shape[1] + 1} columns, k = {k} needs {k + 1} (self first)")
    zero = int(np.count_nonzero(~np.all(dist > 0, axis=1)))
    if zero:
        # the reference asserts np.all(dist > 0) (mle.py:23): duplicate points have zero distances and log(0)
        raise ValueError(f"{zero} points have a zero distance among their {k} nearest neighbours (duplicate points); "
                         "the Levina-Bickel estimate is undefined for them")
    d = np.log(dist[:, k - 1: k] / dist[:, 0:k - 1])
    d = d.sum(axis=1) / (k - 2)                       # the unbiased k - 2 divisor (mle.py:25)
    return 1. / d


def _scale_interval(dist, k1, k2):
    return [_sample_wise(dist, k).mean() for k in range(k1, k2 + 1)]


def intrinsic_dim_sample_wise(X, k=5, dist=None):
    """Levina-Bickel estimate of every point for k neighbours (mle.py:6-28): array of shape (N,)."""
    if dist is None:
        dist = neighbour_distances(X, k)
    if np.asarray(dist).shape[0] != X.shape[0]:
        raise ValueError(f"dist has {np.asarray(dist).shape[0]} rows, X {X.shape[0]}")
    return _sample_wise(dist, k)


def intrinsic_dim_scale_interval(X, k1=10, k2=20, dist=None):
    """Mean Levina-Bickel estimate for k = k1 .. k2 (mle.py:31-51): a list of k2 - k1 + 1 floats."""
    if dist is None:
        dist = neighbour_distances(X, k2)
    if np.asarray(dist).shape[0] != X.shape[0]:
        raise ValueError(f"dist has {np.asarray(dist).shape[0]} rows, X {X.shape[0]}")
    return _scale_interval(dist, k1, k2)


def bootstrap_intrinsic_dim_scale_interval(X, nb_iter=100, random_state=None, k1=10, k2=20, average=False):
    """The scale-interval estimate over nb_iter bootstrap subsets (mle.py:54-91): (results, Rs) with results of shape
    (nb_iter, k2 - k1 + 1), or its mean over the subsets when ``average``; Rs[i] = max(dist[:, :k1 + i])."""
    if random_state is None:
        rng = np.random
    else:
        rng = np.random.RandomState(random_state)
    nb_examples = X.shape[0]
    results = []
    dist = neighbour_distances(X, k2)
    Rs = []
    for i in range(k1, k2 + 1):
        Rs.append(np.max(dist[:, :i]))                # mle.py:83-85: max over the first i columns, self column included
    for i in range(nb_iter):
        # mle.py:88: randint's upper bound is exclusive, so the last point is never drawn; kept for equal subsets per seed
        idx = np.unique(rng.randint(0, nb_examples - 1, size=nb_examples))
        # mle.py:89: the subset reuses the full set's neighbour distances (its neighbours are not searched again)
        results.append(_scale_interval(dist[idx, :], k1, k2))
    results = np.array(results)
    if average:
        return results.mean(axis=0), Rs
    else:
        return results, Rs
