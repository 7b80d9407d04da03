"""Expected Simplex Skewness: a real-valued intrinsic dimension of every point, at one neighbourhood size or across a list of them.

Johnsson, Soneson and Fontes (2015), R ``intrinsicDimension::essLocalDimEst`` with d = 1 -- the package the reference reaches through
rpy2 for ``mle_*`` and ``lpca`` (benchmark.py), and the classical local baseline of the FLIPD paper (Kamkari et al. 2024).  Take a
point and its k nearest neighbours, centre the k + 1 rows on their mean, and over ALL pairs of centred rows form the weighted mean
of |sin| (variant 'a') or |cos| (variant 'b') of the angle between them, weighted by the product of their lengths.  For directions
uniform on the sphere S^(n-1) that mean has a closed form, ``reference(n, ver)``; the dimension is the real n at which the piecewise
linear interpolation of the closed form meets the measured value.

The module is called ``simplex`` because ``empirical.py`` already says "ESS" for the effective sample size of a softmax.

Differences from R, all on purpose: every pair is taken (R draws 5000 simplices at random), so a reading is a function of the data
alone; the table of reference values is not walked linearly (that walk does not end usefully near ess_a -> 1, where
ref_a(n) = 1 - 1 / (2 n) + ...) but searched by doubling and bisection on the closed forms; d = 1 only.  The rows are centred on
the neighbourhood's MEAN, as R's package does to our reading of it; centring on the query point instead reads a 4-sphere as 4 at
16 of 1024 points where this reads 1024.  Not checked against R or scikit-dimension: neither is available to this project's tests.

On the MI355X this is ``_lib.knn`` (exact, csrc/knn.hip) at the largest neighbourhood size followed by ONE launch of
``_lib.simplex_skewness`` (csrc/simplex.hip): the neighbours come back in ascending distance, so the Gram matrix of the largest
neighbourhood holds every smaller one as a leading block, and one launch serves a whole list of sizes (``scale_curve``: how a
classical reading depends on k, the parameter users get wrong -- the counterpart of ``empirical.scale_curve`` over sigma).
``skewness_host`` restates the kernel's arithmetic in fp64 numpy (tests/simplex_cases.py holds the long-double oracle and the bound).
"""
import math
import os
import pickle

import numpy as np
import torch

from . import _lib
from .mle import _points

VERSIONS = ('a', 'b')
DIM_MAX = float(1 << 20)          # a reading above this is inf: ess_a is within 2^-21 of 1, nothing is left to interpolate
SCALES = (8, 12, 16, 24, 32, 48, 64)
_SERIES_FROM = 64                 # n from which log q(n) is taken from its asymptotic series, below it from lgamma


def _numpy(a, dtype):
    return np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=dtype)


def _scales(ks):
    ks = [int(k) for k in (ks if np.ndim(ks) else [ks])]
    if not ks or any(b <= a for a, b in zip(ks, ks[1:])) or ks[0] < 2:
        raise ValueError(f"neighbourhood sizes must be at least 2 and strictly ascending, got {ks}")
    return ks


def _check_d(d):
    if d != 1:
        raise NotImplementedError(f"simplex skewness with d = {d}: only d = 1 (pairs of centred rows) is implemented")


# ------------------------------------------------------------------------------------------- the skewness
def skewness(X, ks=(20,), rows=None, d=1):
    """``(ess, idx)`` for every row of X [N, D] -- or for the rows listed in ``rows`` (the neighbour search still runs over all of
    X): ess [Q, S, 3] fp64 = (ess_a, ess_b, weight sum) at each neighbourhood size of ``ks`` (strictly ascending, 2 .. 64); idx
    [Q, max(ks)] int64 the neighbours.  One ``_lib.knn`` at max(ks) and one launch; all on the GPU."""
    _check_d(d)
    ks = _scales(ks)
    Xd = _points(X)
    _, idx, _ = _lib.knn(Xd, ks[-1])
    if rows is None:
        centre = torch.arange(Xd.shape[0], dtype=torch.int64, device=Xd.device)
    else:
        centre = torch.as_tensor(rows, dtype=torch.int64).reshape(-1).cpu()      # checked on the host: it indexes idx below
        if centre.numel() and (int(centre.min()) < 0 or int(centre.max()) >= Xd.shape[0]):
            raise IndexError(f"rows outside [0, {Xd.shape[0]})")
        centre = centre.to(Xd.device)
        idx = idx[centre].contiguous()
    return _lib.simplex_skewness(Xd, centre, idx, ks), idx


def skewness_host(X, idx, ks, centre=None):
    """The arithmetic of csrc/simplex.hip in fp64 numpy: X [N, D], idx [Q, k] neighbour rows in ascending distance, ks the
    neighbourhood sizes (<= k), centre [Q] (default 0 .. Q - 1) -> ess [Q, S, 3].  y_j = x_j - x_centre, G = Y Y^T; per size k',
    on the leading m' x m' block (m' = k' + 1): B = G - (r_i + r_j) + g, then over i < j the sums of sqrt(max(0, B_ii B_jj -
    B_ij^2)), |B_ij| and sqrt(B_ii) sqrt(B_jj), the first two divided by the third; NaN, NaN, 0 where the third is 0."""
    X = _numpy(X, np.float64)
    idx = _numpy(idx, np.int64)
    ks = _scales(ks)
    Q, k = idx.shape
    if ks[-1] > k:
        raise ValueError(f"neighbourhood size {ks[-1]} above the {k} neighbours of idx")
    centre = np.arange(Q) if centre is None else _numpy(centre, np.int64).reshape(-1)
    X = X.reshape(X.shape[0], -1)
    out = np.empty((Q, len(ks), 3))
    step = max(1, (32 << 20) // (8 * (k + 1) * max(X.shape[1], k + 1)))          # queries per batch: about 32 MiB of rows
    for q0 in range(0, Q, step):
        c = centre[q0:q0 + step]
        Y = X[np.concatenate([c[:, None], idx[q0:q0 + step]], axis=1)] - X[c][:, None, :]
        G = Y @ Y.transpose(0, 2, 1)
        for s, kk in enumerate(ks):
            m = kk + 1
            Gs = G[:, :m, :m]
            r = Gs.sum(axis=2) / m
            g = r.sum(axis=1) / m
            B = Gs - (r[:, :, None] + r[:, None, :]) + g[:, None, None]
            diag = np.maximum(np.einsum('qii->qi', B), 0.0)
            nrm = np.sqrt(diag)
            i, j = np.triu_indices(m, 1)
            area = np.sqrt(np.maximum(diag[:, i] * diag[:, j] - B[:, i, j] ** 2, 0.0)).sum(axis=1)
            dot = np.abs(B[:, i, j]).sum(axis=1)
            w = (nrm[:, i] * nrm[:, j]).sum(axis=1)
            with np.errstate(divide='ignore', invalid='ignore'):
                out[q0:q0 + step, s, 0] = np.where(w == 0.0, np.nan, area / w)
                out[q0:q0 + step, s, 1] = np.where(w == 0.0, np.nan, dot / w)
            out[q0:q0 + step, s, 2] = w
    return out


# ------------------------------------------------------------------------------------------- the reference curves
# both are ratios of q(n) = Gamma(n / 2) / Gamma((n + 1) / 2):   ref_a(n) = q(n) / q(n - 1),   ref_b(n) = q(n) / sqrt(pi)
_LOG_Q_SMALL = np.array([np.nan] + [math.lgamma(n / 2.0) - math.lgamma((n + 1) / 2.0) for n in range(1, _SERIES_FROM)])
# log Gamma(z + 1/2) - log Gamma(z) = log(z) / 2 + sum over even j of (2^(1 - j) - 2) B_j / (j (j - 1) z^(j - 1)), B_j Bernoulli
_BERNOULLI = ((2, 1.0 / 6), (4, -1.0 / 30), (6, 1.0 / 42), (8, -1.0 / 30), (10, 5.0 / 66), (12, -691.0 / 2730), (14, 7.0 / 6))
_SERIES = tuple((j - 1, (2.0 ** (1 - j) - 2.0) * b / (j * (j - 1))) for j, b in _BERNOULLI)


def _series_tail(z):
    """log Gamma(z + 1/2) - log Gamma(z) - log(z) / 2 for z >= 31: the first omitted term is below 1e-23."""
    return sum(c / z ** p for p, c in _SERIES)


def _log_q(n):
    n = np.asarray(n, dtype=np.float64)
    small = n < _SERIES_FROM
    z = np.where(small, _SERIES_FROM, n) / 2.0
    return np.where(small, _LOG_Q_SMALL[np.where(small, n, 0).astype(np.int64)], -(0.5 * np.log(z) + _series_tail(z)))


def reference(n, ver='a'):
    """The expected skewness of directions uniform on S^(n-1), for integer n >= 1 (array or scalar) -> fp64:
    'a'  E|sin| = Gamma(n/2)^2 / (Gamma((n+1)/2) Gamma((n-1)/2)), 0 at n = 1, increasing to 1;
    'b'  E|cos| = Gamma(n/2) / (sqrt(pi) Gamma((n+1)/2)), 1 at n = 1, decreasing to 0.
    Through lgamma below n = 64; from there through the asymptotic series of log Gamma(z + 1/2) - log Gamma(z), in which
    log ref_a(n) = log q(n) - log q(n - 1) is formed term by term: lgamma itself is good to 1e-16 of values near n log n, which at
    n = 10^6 would leave nothing of the step ref_a(n + 1) - ref_a(n) = 1 / (2 n^2)."""
    if ver not in VERSIONS:
        raise ValueError(f"unknown version {ver!r} {VERSIONS}")
    n = np.asarray(n)
    nf = n.astype(np.float64)
    if nf.size and (np.any(nf < 1) or np.any(nf != np.floor(nf))):
        raise ValueError("reference(n): n must be integers >= 1")
    if ver == 'b':
        out = np.exp(_log_q(nf)) / math.sqrt(math.pi)
        return np.where(nf == 1, 1.0, out)
    small = nf <= _SERIES_FROM                           # n - 1 is still in the table
    with np.errstate(invalid='ignore'):
        low = _log_q(np.where(small & (nf > 1), nf, 2)) - _log_q(np.where(small & (nf > 1), nf - 1, 1))
    z = np.where(small, _SERIES_FROM + 1, nf) / 2.0
    # log q(n) - log q(n - 1) with z = n / 2:  -(log(z) - log(z - 1/2)) / 2 - (tail(z) - tail(z - 1/2))
    high = 0.5 * np.log1p(-0.5 / z) - (_series_tail(z) - _series_tail(z - 0.5))
    return np.where(nf == 1, 0.0, np.exp(np.where(small, low, high)))


def dims_from_skewness(ess, ver='a'):
    """The real-valued dimension of each skewness value (any shape) -> fp64 of that shape: with n the integer whose reference
    values enclose the value, n + (ess - ref(n)) / (ref(n + 1) - ref(n)), at least 1.  n is found by doubling and bisection on the
    closed forms.  inf where the reading would exceed 2^20 and where ess_a >= 1 or ess_b <= 0 (no finite sphere gives that); NaN
    stays NaN."""
    if ver not in VERSIONS:
        raise ValueError(f"unknown version {ver!r} {VERSIONS}")
    e = _numpy(ess, np.float64)
    shape = e.shape
    e = e.reshape(-1)
    out = np.full(e.shape, np.nan)
    nan = np.isnan(e)
    beyond = ~nan & ((e >= 1.0) if ver == 'a' else (e <= 0.0))
    out[beyond] = np.inf
    todo = np.flatnonzero(~nan & ~beyond)
    v = e[todo]
    # ref(n) is on the low side of the value: 'a' climbs with n, 'b' falls
    below = (lambda n: reference(n, 'a') <= v) if ver == 'a' else (lambda n: reference(n, 'b') >= v)
    lo, hi = np.ones(v.shape, dtype=np.int64), np.full(v.shape, 2, dtype=np.int64)
    for _ in range(21):                                  # doubling: ref(lo) on the low side, hi = 2 lo, up to lo = 2^21
        grow = below(hi)
        lo, hi = np.where(grow, hi, lo), np.where(grow, 2 * hi, hi)
    for _ in range(22):                                  # bisection down to hi = lo + 1
        mid = (lo + hi) // 2
        up = (mid > lo) & below(mid)
        lo, hi = np.where(up, mid, lo), np.where(up | (mid == lo), hi, mid)
    r0, r1 = reference(lo, ver), reference(lo + 1, ver)
    dim = np.maximum(lo + (v - r0) / (r1 - r0), 1.0)     # a value on the far side of ref(1) (ess_b > 1 by rounding) reads 1
    dim[dim > DIM_MAX] = np.inf
    out[todo] = dim
    return out.reshape(shape)


# ------------------------------------------------------------------------------------------- dimensions of a data set
def _column(ver):
    if ver not in VERSIONS:
        raise ValueError(f"unknown version {ver!r} {VERSIONS}")
    return VERSIONS.index(ver)


def local_dims(X, k=20, ver='a', d=1):
    """The simplex-skewness dimension of every point of X over its k nearest neighbours: fp64 numpy [N]."""
    col = _column(ver)
    ess, _ = skewness(X, (int(k),), d=d)
    return dims_from_skewness(ess[:, 0, col].cpu().numpy(), ver)


def scale_curve(X, ks=SCALES, ver='a', d=1):
    """The dimension of every point of X at every neighbourhood size of ``ks``: fp64 numpy [N, S], from one neighbour search and one
    launch.  ``stable_dims`` reads a single dimension per point off the curve."""
    col = _column(ver)
    ess, _ = skewness(X, ks, d=d)
    return dims_from_skewness(ess[:, :, col].cpu().numpy(), ver)


def stable_dims(curve, ks):
    """int64 [N] from a curve [N, S] over the sizes ks [S] (host only): per point, the rounded dimension of the longest run of
    consecutive sizes whose rounded readings agree; of two runs of one length, the one at the larger sizes.  -1 where no reading
    is finite.  A heuristic, as ``empirical.stable_dims`` is: it says where the reading does not move with k, not that it is
    right there."""
    curve, ks = np.asarray(curve, dtype=np.float64), np.asarray(ks).ravel()
    if curve.ndim != 2 or curve.shape[1] != ks.size:
        raise ValueError(f"curve {curve.shape}, ks {ks.shape}")
    finite = np.isfinite(curve)
    rounded = np.where(finite, np.rint(np.where(finite, curve, 0.0)), -1).astype(np.int64)
    out = np.full(curve.shape[0], -1, dtype=np.int64)
    for p in range(curve.shape[0]):
        best, s = 0, 0
        while s < ks.size:
            if not finite[p, s]:
                s += 1
                continue
            e = s
            while e + 1 < ks.size and finite[p, e + 1] and rounded[p, e + 1] == rounded[p, s]:
                e += 1
            if e - s + 1 >= best:                        # >=: the later run, at the larger sizes, wins a tie
                best, out[p] = e - s + 1, rounded[p, s]
            s = e + 1
    return out


# ------------------------------------------------------------------------------------------- a data set from a config
def run(config, k=20, ver='a', sweep=False, out_dir='simplex', ks=SCALES):
    """The train split of the config's data set, taken exactly as ``benchmark.Benchmark.create_dataset`` takes it -> the
    simplex-skewness dimension of every point into ``out_dir/local_dims.pkl`` = {'dims', 'skewness', 'k' | 'ks', 'ver'}: dims [N]
    at the size k, or with ``sweep`` dims [N, S] at the sizes ks; skewness the [N, S, 3] the readings come from.  Prints the
    histogram of the rounded readings (per size with ``sweep``, then that of ``stable_dims``).  -> dims."""
    from .lightning_data_modules.utils import create_lightning_datamodule
    col = _column(ver)
    DataModule = create_lightning_datamodule(config)
    DataModule.setup()
    X = _points(torch.cat([x.reshape(x.shape[0], -1) for x in DataModule.train_dataloader()], dim=0))
    sizes = _scales(ks) if sweep else [int(k)]
    ess, _ = skewness(X, sizes)
    ess = ess.cpu().numpy()
    curve = dims_from_skewness(ess[:, :, col], ver)
    dims = curve if sweep else curve[:, 0]
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'local_dims.pkl'), 'wb') as f:
        pickle.dump({'dims': dims, 'skewness': ess, ('ks' if sweep else 'k'): (sizes if sweep else int(k)), 'ver': ver}, f)

    def histogram(title, rounded):
        print(title)
        values, counts = np.unique(rounded, return_counts=True)
        for v, c in zip(values, counts):
            print(f'  dim {int(v):3d}: {int(c)}')

    for s, size in enumerate(sizes):
        column = curve[:, s]
        ok = np.isfinite(column)
        histogram(f'simplex skewness ({ver}, k = {size}) on {len(column)} points: mean {column[ok].mean():.3f}'
                  + (f', {int((~ok).sum())} not finite' if not ok.all() else ''), np.rint(column[ok]))
    if sweep:
        histogram(f'stable over k = {sizes}:', stable_dims(curve, sizes))
    return dims


def main(argv=None):
    import argparse
    from .configs.utils import read_config
    ap = argparse.ArgumentParser(description="Simplex-skewness intrinsic dimension of every training point of a data set")
    ap.add_argument('--config', required=True)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--ver', choices=VERSIONS, default='a')
    ap.add_argument('--sweep', action='store_true', help="every size of --ks from one launch, and the stable reading")
    ap.add_argument('--ks', type=lambda s: tuple(int(t) for t in s.split(',')), default=SCALES)
    ap.add_argument('--out_dir', default='simplex')
    args = ap.parse_args(argv)
    run(read_config(args.config), k=args.k, ver=args.ver, sweep=args.sweep, out_dir=args.out_dir, ks=args.ks)


if __name__ == '__main__':
    main()
