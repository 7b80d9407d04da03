"""Classical intrinsic-dimension baselines (drop-in ``Benchmark`` for /root/reference/benchmark.py, without rpy2).

The reference fills a CSV (index ``method``: mle_5, mle_20, lpca, ppca; one column per dataset) from R's
``intrinsicDimension`` package through rpy2 (mle_*, lpca) and sklearn's ``PCA(n_components='mle')`` (ppca)
(benchmark.py:57-68).  Here the estimators are module functions on the MI355X: the neighbour search of the ML
estimators is one exact kNN (``_lib.knn``), the PCA estimators read the covariance eigenvalues of the fp64 spectrum
kernels (``_lib.spectrum(X, return_eig=True)``); what remains is O(N k) or O(D^2) host arithmetic in fp64.
An opt-in fifth kind of name, ``lpca_knn_<k>``, is the per-point form of lpca (``lpca.py``), and a sixth, ``ess_knn_<k>``, the
per-point simplex skewness (``simplex.py``).
"""
import math
import os

import numpy as np
import pandas as pd
import torch

from . import _lib
from .lightning_data_modules.utils import create_lightning_datamodule
from .mle import _points

_SKLEARN_EPS = 1e-15


# ------------------------------------------------------------------------------------------- ML estimator
def mle_global_dim(X, k, aggregation='maximum.likelihood', unbiased=False):
    """Global maximum-likelihood dimension, as R ``intrinsicDimension::maxLikGlobalDimEst(data, k)`` with its defaults
    reads to us (neighbourhood-based, Levina-Bickel per point).  Definition used here, T_j the distance of point i to its
    j-th nearest other point:

        m_i = (k - 1 - unbiased) / sum_{j < k} log(T_k / T_j)
        'maximum.likelihood':  1 / mean_i(1 / m_i)      'mean':  mean_i(m_i)      'robust':  median_i(m_i)

    Not checked against R (R is not available to this project's tests)."""
    dist, _, _ = _lib.knn(_points(X), k)
    T = dist.cpu().numpy()
    zero = int(np.count_nonzero(~np.all(T > 0, axis=1)))
    if zero:
        raise ValueError(f"{zero} points have a zero distance among their {k} nearest neighbours (duplicate points)")
    return mle_aggregate(T, k, aggregation, unbiased)


def mle_aggregate(T, k, aggregation='maximum.likelihood', unbiased=False):
    """The aggregation of ``mle_global_dim`` for given neighbour distances T [N, >= k] (self excluded)."""
    T = np.asarray(T, dtype=np.float64)[:, :k]
    s = np.log(T[:, k - 1:k] / T[:, :k - 1]).sum(axis=1)
    m = (k - 1 - int(bool(unbiased))) / s
    if aggregation == 'maximum.likelihood':
        return float(1.0 / np.mean(1.0 / m))
    if aggregation == 'mean':
        return float(np.mean(m))
    if aggregation == 'robust':
        return float(np.median(m))
    raise ValueError(f"unknown aggregation {aggregation!r} (maximum.likelihood, mean, robust)")


# ------------------------------------------------------------------------------------------- PCA estimators
def covariance_eigenvalues(X):
    """Eigenvalues of the sample covariance of X [N, D], descending, min(N, D) of them (fp64 numpy)."""
    Xd = _points(X)
    _, eig = _lib.spectrum(Xd, return_eig=True)
    lam = eig.cpu().numpy()[::-1] / (Xd.shape[0] - 1)
    return np.maximum(lam, 0.0)


def ppca_loglik(spectrum, n_samples):
    """Minka's log-likelihood of every rank 0 .. D - 1 (ll[0] = -inf), equal to sklearn's ``_assess_dimension`` per rank
    (sklearn.decomposition._pca), including its 1e-15 rules.

    sklearn's pair sum pa(r) = sum_{i < r} sum_{j > i} [log((l_i - l_j)(1/s_j - 1/l_i)) + log n], s_j = l_j for j < r and
    v_r (the mean of the tail) otherwise, costs O(D^2) per rank.  Split as
        pairs inside the head  sum_{i < j < r} log((l_i - l_j)(1/l_j - 1/l_i))          (grows by one column per rank)
        head x tail            sum_{i < r, j >= r} log(l_i - l_j)  +  (D - r) sum_{i < r} log(1/v_r - 1/l_i)
    all ranks together cost O(D^2), in row blocks so that no D x D array is formed."""
    lam = np.asarray(spectrum, dtype=np.float64)
    D = lam.shape[0]
    n = float(n_samples)
    eps = _SKLEARN_EPS
    ll = np.full(D, -np.inf)
    if D < 2:
        return ll
    # ranks sklearn evaluates: spectrum[rank - 1] >= eps (a descending spectrum: a prefix of 1 .. D - 1)
    r_max = 0
    while r_max + 1 < D and lam[r_max] >= eps:
        r_max += 1
    if r_max == 0:
        return ll
    ranks = np.arange(1, r_max + 1)
    tail = np.cumsum(lam[::-1])[::-1]                      # tail[r] = sum_{j >= r} lam_j
    v = np.maximum(eps, tail[ranks] / (D - ranks))
    # pu: -r log 2 + sum_{i=1..r} lgamma((D - i + 1) / 2) - log(pi) (D - i + 1) / 2
    gi = np.array([math.lgamma((D - i + 1) / 2.0) - math.log(math.pi) * (D - i + 1) / 2.0 for i in range(1, r_max + 1)])
    pu = -ranks * math.log(2.0) + np.cumsum(gi)
    with np.errstate(divide='ignore'):
        pl = -np.cumsum(np.log(lam[:r_max])) * n / 2.0
    pv = -np.log(v) * n * (D - ranks) / 2.0
    m = D * ranks - ranks * (ranks + 1.0) / 2.0
    pp = math.log(2.0 * math.pi) * (m + ranks) / 2.0
    # pair sums, in blocks of rows i
    head = np.zeros(r_max + 1)        # head[r] = sum_{i < j < r} P(i, j), P = log((l_i - l_j)(1/l_j - 1/l_i))
    colP = np.zeros(D)                # colP[j] = sum_{i < min(j, r_max)} P(i, j)
    rowL = np.zeros(r_max)            # rowL[i] = sum_{j > i} log(l_i - l_j)
    colL = np.zeros(D)                # colL[j] = sum_{i < min(j, r_max)} log(l_i - l_j)
    B = max(1, (1 << 20) // D)
    with np.errstate(divide='raise', invalid='raise'):
        try:
            for i0 in range(0, r_max, B):
                i1 = min(r_max, i0 + B)
                li = lam[i0:i1, None]
                upper = np.arange(D)[None, :] > np.arange(i0, i1)[:, None]
                diff = np.where(upper, li - lam[None, :], 1.0)
                L = np.where(upper, np.log(diff), 0.0)
                rowL[i0:i1] = L.sum(axis=1)
                colL += L.sum(axis=0)
                # P only where both ends are head eigenvalues (j < r_max: l_j >= 1e-15)
                up = upper[:, :r_max]
                lj = np.where(up, lam[None, :r_max], 1.0)
                P = np.where(up, np.log(np.where(up, diff[:, :r_max] * (1.0 / lj - 1.0 / li), 1.0)), 0.0)
                colP[:r_max] += P.sum(axis=0)
        except FloatingPointError:
            # sklearn takes math.log of the same products and stops there (equal or non-positive eigenvalues)
            raise ValueError("math domain error: equal eigenvalues in Minka's pair sum (as sklearn's _assess_dimension)")
    # the column sums above run over all i < r_max; the head of rank r needs i < j < r only: colP[j] restricted to i < j
    # is the same (i < j <= r - 1 < r_max), so head[r] = sum_{j < r} colP[j]
    head[1:] = np.cumsum(colP[:r_max])
    # head x tail: Q[r] = sum_{i < r, j >= r} L(i, j) = sum_{i < r} rowL[i] - sum_{j < r} colL[j]
    Q = np.cumsum(rowL) - np.cumsum(colL[:r_max])
    # (D - r) sum_{i < r} log(1/v_r - 1/l_i), in blocks of ranks
    cross = np.empty(r_max)
    inv_l = 1.0 / lam[:r_max]
    Rb = max(1, (1 << 20) // r_max)
    with np.errstate(divide='raise', invalid='raise'):
        try:
            for r0 in range(0, r_max, Rb):
                rr = ranks[r0:r0 + Rb]
                vv = v[r0:r0 + Rb]
                mask = np.arange(r_max)[None, :] < rr[:, None]
                arg = np.where(mask, 1.0 / vv[:, None] - inv_l[None, :], 1.0)
                cross[r0:r0 + Rb] = np.where(mask, np.log(arg), 0.0).sum(axis=1)
        except FloatingPointError:
            raise ValueError("math domain error: equal eigenvalues in Minka's pair sum (as sklearn's _assess_dimension)")
    npairs = ranks * (D - 1) - ranks * (ranks - 1) / 2.0
    pa = head[1:] + Q + (D - ranks) * cross + npairs * math.log(n)
    ll[1:r_max + 1] = pu + pl + pv + pp - pa / 2.0 - ranks * math.log(n) / 2.0
    return ll


def ppca_rank(spectrum, n_samples):
    """argmax of ``ppca_loglik``: sklearn's ``_infer_dimension``."""
    return int(np.argmax(ppca_loglik(spectrum, n_samples)))


def ppca_dim(X):
    """Minka's PCA dimension, ``sklearn.decomposition.PCA(n_components='mle').fit(X).n_components_``."""
    N, D = X.shape[0], int(np.prod(X.shape[1:]))
    if N < D:
        raise ValueError("n_components='mle' is only supported if n_samples >= n_features")
    return ppca_rank(covariance_eigenvalues(X), N)


def pca_fo_dim(X, alpha=0.05):
    """Fukunaga-Olsen rule of R ``intrinsicDimension::pcaLocalDimEst(data, 'FO')`` applied to the whole set, as the
    reference's benchmark.py:64 does: the number of covariance eigenvalues greater than alpha times the largest.
    Not checked against R (R is not available to this project's tests)."""
    return pca_fo_count(covariance_eigenvalues(X), alpha)


def pca_fo_count(eigenvalues, alpha=0.05):
    lam = np.asarray(eigenvalues, dtype=np.float64)
    return int(np.count_nonzero(lam > alpha * lam.max()))


def lpca_knn_k(name):
    """k of an estimator name ``lpca_knn_<k>`` (local PCA over the k nearest neighbours of every point, Fukunaga-Olsen per
    point, the mean over the points: ``lpca.local_dims``), or None for any other name.  Not in the default list: a user opts
    in with ``benchmark.estimators.append('lpca_knn_20')``."""
    head, _, tail = str(name).rpartition('_')
    return int(tail) if head == 'lpca_knn' and tail.isdigit() and tail.isascii() else None


def ess_knn_k(name):
    """k of an estimator name ``ess_knn_<k>`` (Expected Simplex Skewness over the k nearest neighbours of every point, the mean
    over the points: ``simplex.local_dims``), or None for any other name.  Opt-in, exactly as ``lpca_knn_<k>`` is."""
    head, _, tail = str(name).rpartition('_')
    return int(tail) if head == 'ess_knn' and tail.isdigit() and tail.isascii() else None


def _opt_in(name):
    return lpca_knn_k(name) is not None or ess_knn_k(name) is not None


# ------------------------------------------------------------------------------------------- the benchmark
class Benchmark():
    """benchmark.py:21-91 of the reference: same constructor, CSV layout, skip-if-filled and error-tolerant loop."""

    def __init__(self, file_name, configs_dict) -> None:
        self.file_name = file_name
        self.estimators = ['mle_5', 'mle_20', 'lpca', 'ppca']
        self.configs_dict = configs_dict
        # create a df for results
        self.results = pd.DataFrame(columns=list(configs_dict.keys()), index=self.estimators, dtype=object)
        self.results.index.name = 'method'
        # load what is already saved
        if os.path.exists(self.file_name):
            exisiting_results = pd.read_csv(self.file_name, index_col='method')
            # opt-in rows a run before this one saved: update() fills only labels the frame has, and to_csv writes only the frame
            self._add_rows(name for name in exisiting_results.index if _opt_in(name))
            self.results.update(exisiting_results)

    def _add_rows(self, names):
        for name in names:
            if name not in self.results.index:
                self.results.loc[name] = np.nan

    def _add_opt_in_rows(self):
        """The rows of the ``lpca_knn_<k>`` and ``ess_knn_<k>`` names in ``self.estimators`` (appended after the constructor built the frame of the four
        defaults), so that the filled-already tests below see them."""
        self._add_rows(name for name in self.estimators if _opt_in(name))

    def run(self):
        print('--------- STARTING BENCHMARK -----------')
        for dataset_name, config in self.configs_dict.items():
            print(f'------ Benchmarking on dataset {dataset_name} --------')
            data = None
            try:
                data = self.create_dataset(dataset_name, config)
            except Exception as e:
                print(f'!!!!------ ERROR: Couldnt create dataset {dataset_name}------!!!!')
                print(e)
            for estimator_type in self.estimators:
                try:
                    self.evaluate_estimator(data, estimator_type=estimator_type, dataset_name=dataset_name)
                except Exception as e:
                    print(f'!!!!------ ERROR: Couldnt evaluate {estimator_type} on dataset {dataset_name}------!!!!')
                    print(e)
            print(f'------ Benchmarking on dataset {dataset_name} completed --------')

    def evaluate_estimator(self, data, estimator_type, dataset_name):
        knn_k, ess_k = lpca_knn_k(estimator_type), ess_knn_k(estimator_type)
        if knn_k is not None or ess_k is not None:
            self._add_rows([estimator_type])                    # an opt-in name: its row is not in the frame of the defaults
        if pd.isna(self.results[dataset_name].loc[estimator_type]):
            print(f'{estimator_type} on {dataset_name} START')
            if estimator_type == 'mle_5':
                estimated_dim = mle_global_dim(data, k=5)
            elif estimator_type == 'mle_20':
                estimated_dim = mle_global_dim(data, k=20)
            elif estimator_type == 'lpca':
                estimated_dim = pca_fo_dim(data)
            elif estimator_type == 'ppca':
                estimated_dim = ppca_dim(data)
            elif knn_k is not None:
                from . import lpca
                estimated_dim = float(lpca.local_dims(data, knn_k).mean())
            elif ess_k is not None:
                from . import simplex
                estimated_dim = float(simplex.local_dims(data, ess_k).mean())
            else:
                raise ValueError(f"unknown estimator {estimator_type!r}")
            self.results.loc[estimator_type, dataset_name] = estimated_dim
            self.results.to_csv(self.file_name)
            print(f'{estimator_type} on {dataset_name} DONE')
        else:
            print(f'{estimator_type} on {dataset_name} was already benchmarked')

    def create_dataset(self, dataset_name, config):
        """The train split of the dataset as one [N, D] fp32 tensor on the GPU (moved once per dataset)."""
        self._add_opt_in_rows()
        if pd.isna(self.results[dataset_name]).any():
            print(f'------ Creating dataset: {dataset_name} --------')
            DataModule = create_lightning_datamodule(config)
            DataModule.setup()
            X = [x.reshape(x.shape[0], -1) for x in DataModule.train_dataloader()]
            data = _points(torch.cat(X, dim=0))
            print(f'------ Dataset {dataset_name} created --------')
            return data
        else:
            print(f'------ Dataset {dataset_name} was already benchmarked ------')
