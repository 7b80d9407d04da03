"""Training-free diffusion ID of an array: the intrinsic dimension and the tangent space of points of a cloud X [N, D] from the
spectrum of the score matrix of the cloud's OWN empirical distribution (models/empirical_exact.py) -- the diffusion-side counterpart
of ``lpca.py`` for data with no closed-form score and no checkpoint.

Everything is the driver's: ``dim_reduction.ScoreMatrixBuilder`` draws the reference's number of perturbed rows around a point for
the given loader batch size (1501 for D = 100, batch size 500) with the driver's position-keyed noise, the rows go through the fused
kernel (csrc/empirical_score.hip) many points a launch, ``_lib.spectrum`` gives the singular values and ``plot_utils.estimate_dim``
reads the dimension off the largest gap.  ``sigma`` is the kernel bandwidth (``model.sigma_min`` of a config): the estimate means
something only where the effective sample size of the rows is well above 1, so the median ESS of every point is returned beside its
dimension.  A sample-based score needs N to grow exponentially in the intrinsic dimension; see the model's docstring.
"""
import os
import pickle

import numpy as np
import torch

from . import _lib, dim_reduction, sde_lib
from .configs.config_dict import ConfigDict
from .mle import _points
from .models import utils as mutils
from .models.empirical_exact import EmpiricalExact, train_split
from .plot_utils import estimate_dim

SIGMA_MAX, NUM_SCALES = 4.0, 1000          # of the paper's Euclidean configs: with them sigma(t = sampling_eps) is a config's
ROWS_PER_LAUNCH = 131072                   # the driver's default launch group


def _config(sigma):
    cfg = ConfigDict()
    cfg.data = ConfigDict(noise_std=0.0, use_data_mean=False)
    cfg.training = ConfigDict(sde='vesde')
    cfg.model = ConfigDict(sigma_min=float(sigma), sigma_max=max(SIGMA_MAX, float(sigma)), num_scales=NUM_SCALES)
    return cfg


def _setup(X, sigma, points):
    """(model, builder, xs [P, D] on the device) for the cloud X at bandwidth sigma; ``points``: None (the first 100 rows), integer
    row indices, or [P, D] coordinates of one's own."""
    if not float(sigma) > 0.0:
        raise ValueError(f"sigma must be positive, got {sigma}")
    Xd = _points(X)
    cfg = _config(sigma)
    model = EmpiricalExact(cfg, data=Xd).to(Xd.device).eval()
    model.ess_warn = 0.0                                             # the ESS is returned instead
    sde, eps = sde_lib.configure_sde(cfg)
    score_fn = mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=True)
    builder = dim_reduction.ScoreMatrixBuilder(score_fn, sde, eps, Xd.device)
    if points is None:
        xs = Xd[:100]
    else:
        pts = np.asarray(points.detach().cpu() if isinstance(points, torch.Tensor) else points)
        if pts.ndim == 1 and np.issubdtype(pts.dtype, np.integer):
            if pts.size and (pts.min() < 0 or pts.max() >= Xd.shape[0]):
                raise IndexError(f"points outside [0, {Xd.shape[0]})")
            xs = Xd[torch.from_numpy(pts.astype(np.int64)).to(Xd.device)]
        else:
            xs = _points(pts.reshape(-1, Xd.shape[1]) if pts.ndim >= 1 else pts)
            if xs.shape[1] != Xd.shape[1]:
                raise ValueError(f"points {tuple(pts.shape)} for a cloud in R^{Xd.shape[1]}")
    return model, builder, xs.contiguous()


def _groups(model, builder, xs, batchsize, seed):
    """Yields (first point, S [P', M, D], ess_median [P']) launch group by launch group; point i draws the noise the driver draws for
    its point i under ``config.seed = seed``."""
    D = xs.shape[1]
    rows = dim_reduction.batching((D,), batchsize)[2]
    group = max(1, ROWS_PER_LAUNCH // rows)
    with torch.no_grad():
        for lo in range(0, xs.shape[0], group):
            part = xs[lo:lo + group]
            S = dim_reduction.build_many(builder, list(part), batchsize, [seed + 1000003 * (lo + i + 1) for i in range(len(part))])
            yield lo, S, model.last_ess.view(len(part), rows).median(dim=1).values


def local_dims(X, sigma, points=None, batchsize=500, seed=0):
    """``(dims [P] int64, ess_median [P] float64)`` numpy: the diffusion ID of every listed point of the cloud X [N, D] at kernel
    bandwidth ``sigma``, and the median effective sample size of the point's score rows (a dimension read where it is near 1 says
    nothing).  -1 where the spectrum has fewer than three values."""
    model, builder, xs = _setup(X, sigma, points)
    D = xs.shape[1]
    keep = dim_reduction._sv_count((D,), batchsize)
    dims, ess = [], []
    for _, S, e in _groups(model, builder, xs, batchsize, seed):
        for sv in dim_reduction.checked_spectra(_lib.spectrum(S)):
            dims.append(estimate_dim(sv[:keep].tolist()) if keep >= 3 else -1)
        ess.append(e.double().cpu().numpy())
    return np.asarray(dims, dtype=np.int64), (np.concatenate(ess) if ess else np.zeros(0))


def local_tangent(X, sigma, points=None, batchsize=500, seed=0):
    """One float32 numpy array [D, d] per listed point, its orthonormal columns spanning the estimated tangent space (the right
    singular vectors of the d smallest singular values of the point's score matrix, d its ID: ``_lib.tangent_basis``, the layout of
    ``get_manifold_dimension(return_tangent=True)``), or None where no basis is served (``dim_reduction.tangent_width``)."""
    model, builder, xs = _setup(X, sigma, points)
    D = xs.shape[1]
    keep = dim_reduction._sv_count((D,), batchsize)
    out = []
    for _, S, _ in _groups(model, builder, xs, batchsize, seed):
        for S_p, sv in zip(S, dim_reduction.checked_spectra(_lib.spectrum(S))):
            _, k = dim_reduction.tangent_width(sv[:keep].tolist(), D)
            out.append(None if k is None else _lib.tangent_basis(S_p.contiguous(), k)[0].to(torch.float32).cpu().numpy())
    return out


def sigma_rule(kth_distance):
    """The bandwidth ``sigma_from_knn`` proposes from every point's distance to its k-th neighbour: their median."""
    return float(np.median(np.asarray(kth_distance, dtype=np.float64)))


def sigma_from_knn(X, k=20):
    """A HEURISTIC starting value for ``sigma``, not a rule: the median distance from a point to its k-th nearest neighbour
    (``_lib.knn``), so that the ball of radius sigma around a typical point holds about k others.  Check the returned ESS, and try a
    few values around it: the dimension should be stable over a range."""
    dist, _, _ = _lib.knn(_points(X), k)
    return sigma_rule(dist[:, k - 1].cpu().numpy())


# ------------------------------------------------------------------------------------------- a data set from a config
def run(config, sigma=None, points=None, out_dir='empirical'):
    """The train split of the config's data set (as the driver splits it) -> the diffusion ID of its first 100 points (or
    ``points``) at bandwidth ``sigma`` (default: ``sigma_from_knn``) into ``out_dir/local_dims.pkl`` = {'dims', 'ess_median',
    'sigma', 'batchsize'}; prints the histogram of the dimensions.  -> dims."""
    X = _points(train_split(config))
    sigma = sigma_from_knn(X) if sigma is None else float(sigma)
    batchsize = int(config.training.batch_size)
    dims, ess = local_dims(X, sigma, points=points, batchsize=batchsize, seed=int(config.get('seed', 42)))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'local_dims.pkl'), 'wb') as f:
        pickle.dump({'dims': dims, 'ess_median': ess, 'sigma': sigma, 'batchsize': batchsize}, f)
    values, counts = np.unique(dims, return_counts=True)
    print(f'empirical score (sigma = {sigma:.4g}) on {len(dims)} of {X.shape[0]} points: mean {dims.mean():.3f}, '
          f'median ESS {np.median(ess):.1f}')
    for v, c in zip(values, counts):
        print(f'  dim {int(v):3d}: {int(c)}')
    return dims


def main(argv=None):
    import argparse
    from .configs.utils import read_config
    ap = argparse.ArgumentParser(description="Training-free diffusion ID of the first training points of a data set")
    ap.add_argument('--config', required=True)
    ap.add_argument('--sigma', type=float, default=None)
    ap.add_argument('--out_dir', default='empirical')
    args = ap.parse_args(argv)
    run(read_config(args.config), sigma=args.sigma, out_dir=args.out_dir)


if __name__ == '__main__':
    main()
