"""Training-free diffusion ID of an array: the intrinsic dimension and the tangent space of points of a cloud X [N, D] from the
spectrum of the score matrix of the cloud's OWN empirical distribution (models/empirical_exact.py) -- the diffusion-side counterpart
of ``lpca.py`` for data with no closed-form score and no checkpoint.

Everything is the driver's: ``dim_reduction.ScoreMatrixBuilder`` draws the reference's number of perturbed rows around a point for
the given loader batch size (1501 for D = 100, batch size 500) with the driver's position-keyed noise, the rows go through the fused
kernel (csrc/empirical_score.hip) many points a launch, ``_lib.spectrum`` gives the singular values and ``plot_utils.estimate_dim``
reads the dimension off the largest gap.  ``sigma`` is the kernel bandwidth (``model.sigma_min`` of a config): the estimate means
something only where the effective sample size of the rows is well above 1, so the median ESS of every point is returned beside its
dimension.  A sample-based score needs N to grow exponentially in the intrinsic dimension; see the model's docstring.

The second half of the module needs no sampling: the Jacobian of the empirical score has a closed form, I + sigma^2 grad s(x) = C(x,
sigma), the softmax-weighted covariance of the cloud seen from x in units of sigma^2 (csrc/empirical_jacobian.hip).  The driver's
centred score matrix estimates |1 - eig(C)| with Monte-Carlo noise; ``jacobian_spectra`` gives eig(C) itself for many points at many
bandwidths a launch, ``dims_from_jacobian`` reads the dimension off it (tangent eigenvalues are near 1, normal ones near 0), and
``scale_curve`` / ``stable_dims`` find the range of bandwidths over which that dimension holds -- the range ``sigma_from_knn`` only
asks the user to look for.

The third part needs no matrix either: FLIPD, D + sigma^2 (tr grad s + |s|^2) of the same score, is for a cloud the softmax-weighted
mean of squared distances sum_i w_i |x_i - x|^2 / sigma^2 -- one real number per (point, bandwidth), every bandwidth from one pass over
the distances, and nothing of width D kept per point, so it serves any D (csrc/empirical_flipd.hip): ``flipd_curve``, ``flipd_dims``.
The D <= 192 of everything above does not apply to it; the need for N to grow exponentially in the intrinsic dimension does.
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
    return model, builder, _select(Xd, points)


def _select(Xd, points):
    """xs [P, D] on the device: the first 100 rows of the cloud (None), its rows ``points`` (integers) or ``points`` themselves."""
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
    return xs.contiguous()


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


# ------------------------------------------------------------------------------------------- the Jacobian in closed form
ESS_MIN = 32.0                 # a HEURISTIC: the largest ESS of a wrong fp64 reading on the test clouds is 19.8
JACOBIAN_RULES = ('half', 'gap')
C_BYTES_PER_LAUNCH = 256 << 20


def _sigmas(sigmas):
    sg = np.atleast_1d(np.asarray(sigmas, dtype=np.float64)).ravel()
    if not sg.size or not (np.isfinite(sg).all() and (sg > 0.0).all()):
        raise ValueError(f"sigmas must be positive and finite, got {sg.tolist()}")
    return sg


def _jacobians(Xd, xs, sg):
    """Yields (first query, C [Q', D, D], mean [Q', D], ess [Q']) launch by launch; query p S + s is point p at bandwidth sg[s], and a
    launch's C stays under C_BYTES_PER_LAUNCH."""
    P, D, S = xs.shape[0], xs.shape[1], len(sg)
    xq = xs.repeat_interleave(S, dim=0)
    sq = torch.from_numpy(sg.astype(np.float32)).to(xs.device).repeat(P)
    step = max(1, C_BYTES_PER_LAUNCH // (8 * D * D))
    for lo in range(0, P * S, step):
        yield (lo,) + _lib.empirical_jacobian(xq[lo:lo + step].contiguous(), Xd, sq[lo:lo + step].contiguous())


def jacobian_spectra(X, sigmas, points=None):
    """``(eig [P, S, D] fp64, ess [P, S] fp64)`` numpy: the eigenvalues, DESCENDING, of C(x, sigma) = I + sigma^2 grad s(x) of the
    cloud X [N, D] at every listed point (``points`` as in ``local_dims``) and every bandwidth of ``sigmas`` [S], and the effective
    sample size of each.  No sampling: ``_lib.empirical_jacobian`` forms C in fp64 from the raw cloud, many (point, sigma) queries a
    launch, and ``_lib.sym_eigvals_batched`` takes its eigenvalues.  The cloud goes to the device once."""
    sg = _sigmas(sigmas)
    Xd = _points(X)
    xs = _select(Xd, points)
    P, D, S = xs.shape[0], xs.shape[1], len(sg)
    eig = torch.empty(P * S, D, dtype=torch.float64, device=Xd.device)
    ess = torch.empty(P * S, dtype=torch.float32, device=Xd.device)
    for lo, C, _, e in _jacobians(Xd, xs, sg):
        eig[lo:lo + C.shape[0]] = _lib.sym_eigvals_batched(C)
        ess[lo:lo + C.shape[0]] = e
    return eig.flip(1).cpu().numpy().reshape(P, S, D), ess.double().cpu().numpy().reshape(P, S)


def dims_from_jacobian(eig, rule='half'):
    """int64 [...] from eig [..., D] (descending eigenvalues of C): 'half' the number of eigenvalues above 0.5, the midpoint between
    a tangent direction (1) and a normal one (0); 'gap' 1 + argmax(lambda_j - lambda_(j+1)).  (``plot_utils.estimate_dim`` divides
    by the second gap, which is exactly zero for a cloud that does not span R^D.)  A spectrum that is not finite raises
    ``ValueError``."""
    eig = np.asarray(eig, dtype=np.float64)
    if eig.ndim < 1 or eig.shape[-1] < 1:
        raise ValueError(f"eig must be [..., D >= 1], got {eig.shape}")
    if rule not in JACOBIAN_RULES:
        raise ValueError(f"unknown rule {rule!r} {JACOBIAN_RULES}")
    if not np.isfinite(eig).all():
        raise ValueError(f"{int((~np.isfinite(eig)).any(axis=-1).sum())} of {eig[..., 0].size} spectra are not finite")
    if rule == 'half':
        return (eig > 0.5).sum(axis=-1).astype(np.int64)
    if eig.shape[-1] < 2:
        return np.ones(eig.shape[:-1], dtype=np.int64)
    return (1 + np.argmax(eig[..., :-1] - eig[..., 1:], axis=-1)).astype(np.int64)


def sigma_grid(X, k=20, lo=-2.0, hi=3.0, per_octave=2):
    """``sigma_from_knn(X, k) 2^(j / per_octave)`` for the integers j with lo <= j / per_octave <= hi, ascending: 11 bandwidths from
    a quarter of the heuristic value to eight times it by default."""
    j = np.arange(int(np.ceil(lo * per_octave - 1e-9)), int(np.floor(hi * per_octave + 1e-9)) + 1)
    return sigma_from_knn(X, k) * 2.0 ** (j / float(per_octave))


def stable_dims(dims, ess, sigmas, ess_min=ESS_MIN):
    """``(dim [P] int64, range [P, 2])`` from dims [P, S], ess [P, S] and the grid sigmas [S] (host only): of the bandwidths with
    ess >= ess_min, the longest run of consecutive grid positions with one and the same dimension -- a tie goes to the run at the
    smaller sigma -- gives the point's dimension and the run's (first, last) sigma.  -1 and (nan, nan) where no bandwidth qualifies."""
    dims, ess, sg = np.asarray(dims), np.asarray(ess, dtype=np.float64), np.asarray(sigmas, dtype=np.float64).ravel()
    if dims.ndim != 2 or dims.shape != ess.shape or dims.shape[1] != sg.size:
        raise ValueError(f"dims {dims.shape}, ess {ess.shape}, sigmas {sg.shape}")
    out = np.full(dims.shape[0], -1, dtype=np.int64)
    rng = np.full((dims.shape[0], 2), np.nan)
    for p in range(dims.shape[0]):
        best, s = None, 0                                                 # (length, first, last)
        while s < sg.size:
            if not ess[p, s] >= ess_min:
                s += 1
                continue
            e = s
            while e + 1 < sg.size and ess[p, e + 1] >= ess_min and dims[p, e + 1] == dims[p, s]:
                e += 1
            if best is None or e - s + 1 > best[0] or (e - s + 1 == best[0] and sg[s] < sg[best[1]]):
                best = (e - s + 1, s, e)
            s = e + 1
        if best is not None:
            out[p], rng[p] = dims[p, best[1]], (sg[best[1]], sg[best[2]])
    return out, rng


def scale_curve(X, sigmas=None, points=None, rule='half'):
    """The dimension of every listed point at every bandwidth (default: ``sigma_grid(X)``) and where it is stable:
    {'sigmas' [S], 'dims' [P, S], 'ess' [P, S], 'eigenvalues' [P, S, D], 'stable_dims' [P], 'stable_range' [P, 2]}."""
    Xd = _points(X)
    sg = sigma_grid(Xd) if sigmas is None else _sigmas(sigmas)
    eig, ess = jacobian_spectra(Xd, sg, points=points)
    dims = dims_from_jacobian(eig, rule)
    stable, rng = stable_dims(dims, ess, sg)
    return {'sigmas': sg, 'dims': dims, 'ess': ess, 'eigenvalues': eig, 'stable_dims': stable, 'stable_range': rng}


def jacobian_tangent(X, sigma, points=None, rule='half', dtype=np.float32):
    """One float32 numpy array [D, d] per listed point, in the layout of ``local_tangent``: the d leading eigenvectors of C(x, sigma),
    d the point's dimension by ``rule``; None where d < 1, d > ``_lib.TANGENT_MAX`` or d >= D.  (``dtype=np.float64`` keeps the vectors
    as computed: rounding an exact basis to float32 alone turns it by about 3e-8.)  C comes from the kernel; the vectors
    from ``numpy.linalg.eigh`` on the host, a matter of milliseconds for a hundred matrices of D <= 192.  The device eigenvector
    kernels do not fit: ``_lib.sym_lowvecs`` wants the eigenvalues it returns at the BOTTOM of a positive definite matrix (here they
    are at the top, and I - C is not definite), and ``_lib.sym_topvecs`` is planned for kernel matrices of thousands of rows."""
    sg = _sigmas(sigma)
    if sg.size != 1:
        raise ValueError(f"one bandwidth expected, got {sg.tolist()}")
    Xd = _points(X)
    xs = _select(Xd, points)
    D = xs.shape[1]
    out = []
    for _, C, _, _ in _jacobians(Xd, xs, sg):
        lam, vec = np.linalg.eigh(C.cpu().numpy())                        # ascending
        for d, V in zip(dims_from_jacobian(lam[:, ::-1], rule), vec):
            out.append(None if d < 1 or d > _lib.TANGENT_MAX or d >= D else np.ascontiguousarray(V[:, ::-1][:, :d], dtype=dtype))
    return out


# ------------------------------------------------------------------------------------------- FLIPD: one scalar per (point, bandwidth)
def flipd_curve(X, sigmas=None, points=None, exclude_self=True):
    """FLIPD (Kamkari et al. 2024; LIDL of Tempczyk et al. 2022 through the Fokker-Planck equation) of the cloud's empirical
    distribution, D + sigma^2 (tr grad s + |s|^2) = sum_i w_i |x_i - x|^2 / sigma^2, at every listed point and every bandwidth
    (default: ``sigma_grid(X)``): {'sigmas' [S], 'flipd' [P, S] fp64, 'ess' [P, S] fp64}.  A REAL-valued local dimension, not a count,
    from one pass over the distances for the whole grid (``_lib.empirical_flipd``); nothing of width D is kept per point, so any D the
    kernel admits is served, the image manifolds included.  ``points`` as in ``local_dims``; where they are rows of the cloud (None or
    integers) and ``exclude_self``, each point is left out of its own softmax.  The reading means something only where the ESS is well
    above 1 (``flipd_dims``): a sample-based score needs N to grow exponentially in the intrinsic dimension."""
    Xd = _points(X)
    sg = sigma_grid(Xd) if sigmas is None else _sigmas(sigmas)
    xs = _select(Xd, points)
    exclude = None
    if exclude_self:
        if points is None:
            exclude = np.arange(xs.shape[0])
        else:
            pts = np.asarray(points.detach().cpu() if isinstance(points, torch.Tensor) else points)
            if pts.ndim == 1 and np.issubdtype(pts.dtype, np.integer):
                exclude = pts.astype(np.int64)
    pack = _lib.empirical_pack(Xd)
    sd = torch.from_numpy(sg.astype(np.float32)).to(Xd.device)
    flipd = torch.empty(xs.shape[0], len(sg), dtype=torch.float64, device=Xd.device)
    ess = torch.empty(xs.shape[0], len(sg), dtype=torch.float32, device=Xd.device)
    for lo in range(0, len(sg), _lib.FLIPD_S_MAX):
        f, e = _lib.empirical_flipd(xs, pack, sd[lo:lo + _lib.FLIPD_S_MAX].contiguous(), exclude=exclude)
        flipd[:, lo:lo + f.shape[1]], ess[:, lo:lo + f.shape[1]] = f, e
    return {'sigmas': sg, 'flipd': flipd.cpu().numpy(), 'ess': ess.double().cpu().numpy()}


def flipd_dims(curve, ess_min=ESS_MIN):
    """``(reading [P] float64, dims [P] int64, range [P, 2])`` from a ``flipd_curve`` (host only): ``stable_dims`` on the ROUNDED
    curve -- of the bandwidths with ess >= ess_min, the longest run on which rint(flipd) stays the same -- gives the integer and the
    run's (first, last) sigma; the real-valued reading is the mean of flipd over that run.  The same HEURISTIC as ``stable_dims``, no
    more: -1, nan and (nan, nan) where no bandwidth qualifies or the curve is not finite there."""
    sg, f, ess = np.asarray(curve['sigmas'], dtype=np.float64).ravel(), np.asarray(curve['flipd'], dtype=np.float64), \
        np.asarray(curve['ess'], dtype=np.float64)
    ok = np.isfinite(f)
    rounded = np.where(ok, np.rint(np.where(ok, f, 0.0)), -1).astype(np.int64)
    dims, rng = stable_dims(rounded, np.where(ok, ess, np.nan), sg, ess_min=ess_min)
    reading = np.full(f.shape[0], np.nan)
    for p in np.flatnonzero(dims >= 0):
        run = (sg >= rng[p, 0]) & (sg <= rng[p, 1])
        reading[p] = f[p, run].mean()
    return reading, dims, rng


def run_flipd(X, sigmas=None, points=None, out_dir='empirical'):
    """``flipd_curve`` of the cloud into ``out_dir/flipd.pkl`` (the curve's dict plus 'reading', 'dims', 'range' of ``flipd_dims``);
    prints the histogram of the rounded readings beside the median ESS at every bandwidth, then that of the stable ones.  -> the dict."""
    curve = flipd_curve(X, sigmas=sigmas, points=points)
    curve['reading'], curve['dims'], curve['range'] = flipd_dims(curve)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'flipd.pkl'), 'wb') as f:
        pickle.dump(curve, f)
    print(f"FLIPD of the empirical score on {curve['flipd'].shape[0]} of {X.shape[0]} points, {len(curve['sigmas'])} bandwidths")
    for s, sigma in enumerate(curve['sigmas']):
        col = curve['flipd'][:, s]
        print(f" sigma = {sigma:.4g}: median ESS {np.median(curve['ess'][:, s]):.1f}, median FLIPD {np.median(col):.3f}")
        _histogram(np.rint(col[np.isfinite(col)]))
    print(f" stable over the bandwidths with ESS >= {ESS_MIN:g} (-1: none qualifies):")
    _histogram(curve['dims'])
    return curve


# ------------------------------------------------------------------------------------------- a data set from a config
def _histogram(dims):
    for v, c in zip(*np.unique(dims, return_counts=True)):
        print(f'  dim {int(v):3d}: {int(c)}')


def run_sweep(X, sigmas=None, points=None, out_dir='empirical', rule='half'):
    """``scale_curve`` of the cloud into ``out_dir/scale_curve.pkl`` (the curve's dict plus 'rule'); prints the histogram of the
    dimensions and the median ESS at every bandwidth, then the histogram of the stable dimensions.  -> the dict."""
    curve = scale_curve(X, sigmas=sigmas, points=points, rule=rule)
    curve['rule'] = rule
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'scale_curve.pkl'), 'wb') as f:
        pickle.dump(curve, f)
    print(f"empirical score Jacobian (rule {rule!r}) on {curve['dims'].shape[0]} of {X.shape[0]} points, {len(curve['sigmas'])} bandwidths")
    for s, sigma in enumerate(curve['sigmas']):
        print(f" sigma = {sigma:.4g}: median ESS {np.median(curve['ess'][:, s]):.1f}")
        _histogram(curve['dims'][:, s])
    print(f" stable over the bandwidths with ESS >= {ESS_MIN:g} (-1: none qualifies):")
    _histogram(curve['stable_dims'])
    return curve


def run(config, sigma=None, points=None, out_dir='empirical', sweep=False, sigmas=None, flipd=False):
    """The train split of the config's data set (as the driver splits it) -> the diffusion ID of its first 100 points (or
    ``points``) at bandwidth ``sigma`` (default: ``sigma_from_knn``) into ``out_dir/local_dims.pkl`` = {'dims', 'ess_median',
    'sigma', 'batchsize'}; prints the histogram of the dimensions.  -> dims.  ``sweep=True`` takes the sampling-free path instead
    (``run_sweep`` over ``sigmas``, default ``sigma_grid``): ``out_dir/scale_curve.pkl``, -> its dict.  ``flipd=True`` takes
    ``run_flipd`` over ``sigmas``: ``out_dir/flipd.pkl``, -> its dict; it serves any D the kernel admits."""
    X = _points(train_split(config))
    if flipd:
        return run_flipd(X, sigmas=sigmas, points=points, out_dir=out_dir)
    if sweep:
        return run_sweep(X, sigmas=sigmas, points=points, out_dir=out_dir)
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
    ap.add_argument('--sweep', action='store_true', help="the sampling-free scale curve (scale_curve.pkl) instead of one bandwidth")
    ap.add_argument('--flipd', action='store_true', help="FLIPD at every bandwidth (flipd.pkl): a real-valued reading, any D")
    ap.add_argument('--sigmas', default=None, help="comma-separated bandwidths of --sweep / --flipd (default: sigma_grid)")
    args = ap.parse_args(argv)
    sigmas = None if args.sigmas is None else [float(v) for v in args.sigmas.split(',')]
    run(read_config(args.config), sigma=args.sigma, out_dir=args.out_dir, sweep=args.sweep, sigmas=sigmas, flipd=args.flipd)


if __name__ == '__main__':
    main()
