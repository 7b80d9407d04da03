"""FLIPD from the rows the sampled path has already evaluated: Stein's identity instead of a JVP of the network.

The sampled ID estimator evaluates s_i = score_fn(y_i, t) at y_i = mean(t) x + sigma z_i, z_i ~ N(0, I), sigma = std(t), M rows a point.
Stein's identity,

    E[z . s(y + sigma z)] = sigma tr grad s~(y),      s~ = s convolved with N(0, sigma^2 I),

(the Monte-Carlo divergence of Ramani, Blu and Unser 2008 with the probe scale equal to the noise level) is exact -- no small
difference, no cancellation --, so the same rows hold FLIPD (Kamkari et al. 2024), D + sigma^2 (tr grad s + |s|^2), for EVERY model
``get_score_fn`` accepts, at zero extra network evaluations.  With s^ = mean_i s_i, a_i = sigma z_i . (s_i - s^) and q_i = |z_i|^2:

    plain = D + mean(a) + sigma^2 |s^|^2                                    standard error sqrt(2 (D - d) / M)
    flipd = plain - beta (mean(q) - D),   beta = cov(a, q) / var(q)          standard error sqrt(2 d (D - d) / (D M))

The second line is a control variate: near a d-dimensional manifold a_i ~ -|P_N z_i|^2 is strongly correlated with q_i, whose mean D is
known.  ``stderr = std(a - beta q) / sqrt(M)`` is read from the sample itself.

WHAT IT READS: the divergence of the score SMOOTHED over the sampling ball, i.e. FLIPD of the field averaged at the scale the method
samples at.  It agrees with FLIPD at the centre up to curvature x sigma (unit circle in R^16 at sigma = 0.05: 1.01-1.04 where the
centre reads 0.99-1.13; unit 2-sphere at sigma = 0.1: 2.09-2.17 against 1.90-1.96).  That is a property of the estimator.

FINITE M: the two sample means above are biased upwards by (D - d) / M each -- s^ contains s_i / M, so mean(a) estimates
(1 - 1 / M) sigma tr, and E|s^|^2 = |E s|^2 + tr Cov(s) / M.  That is 0.12 for D = 100 at M = 1501 but 0.43 for D = 1024 at M = 4696 and
1.37 for D = 3072 at M = 4480: the sampled path takes M ~ 4 D rows, so for images the bias is half a dimension and more.  Both terms
have exact corrections: mean(a) M / (M - 1), and |s^|^2 - T / (M (M - 1)) with T = sum_i |s_i - s^|^2, the trace of the centred Gram -- which
is the sum of the squared singular values the spectrum path returns for the same S.  ``centred_trace`` switches them on
(``reading_from_sums``, ``reading_host(debias=True)``); the driver and ``sampled_flipd`` always pass it.

The device work is ``_lib.stein_rows`` (csrc/stein.hip): per row a'_i = z_i . (s_i - s^) and q_i in fp64, per point five sums; the
[P, 5] sums are the only read-back, and ``reading_from_sums`` turns them into the reading on the host.  ``reading_host`` is the whole
estimator in numpy (any float type, ``np.longdouble`` for the tests)."""
import numpy as np

SUMS = ('a', 'aa', 'q', 'qq', 'aq')          # the columns of ``sums``: sum a', sum a'^2, sum q, sum q^2, sum a' q
KEYS = ('flipd', 'stderr', 'plain', 'beta')
U = 2.0 ** -53


def reading_from_sums(sums, M, D, sigma, mean_norm2, centred_trace=None):
    """``{'flipd', 'stderr', 'plain', 'beta'}`` (float64 [P]) from the [P, 5] sums of ``_lib.stein_rows`` over M rows of width D, the
    noise level ``sigma`` = std(t) and ``mean_norm2`` [P] = |s^|^2: the scalars ``jacobian.flipd`` combines, D + sigma^2 (tr + |s|^2) with
    sigma tr read as mean_i z_i . (s_i - s^), so VE, VP and subVP differ only in the sigma they pass.

    beta = 0 when M < 3 or var(q) = 0 -- the latter decided at the rounding level of the sums: a centred second moment below
    4 (M + 2) 2^-53 of its raw sum is the cancellation error of a constant q --; ``stderr`` (ddof 1) is NaN when M < 2.

    ``centred_trace`` [P] = sum_i |s_i - s^|^2 (the sum of the squared singular values of the centred score matrix) removes the
    finite-M bias of 'plain' and 'flipd' (module docstring): mean(a) M / (M - 1) and |s^|^2 - centred_trace / (M (M - 1)).  Ignored
    when M < 2."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 5)
    M, D = int(M), int(D)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), s.shape[:1])
    mean_norm2 = np.broadcast_to(np.asarray(mean_norm2, dtype=np.float64), s.shape[:1])
    sa, saa, sq, sqq, saq = s.T
    with np.errstate(invalid='ignore', divide='ignore'):
        caa = saa - sa * sa / M                                     # centred second moments of a' and q
        cqq = sqq - sq * sq / M
        caq = saq - sa * sq / M
        if centred_trace is not None and M >= 2:
            trace = np.broadcast_to(np.asarray(centred_trace, dtype=np.float64), s.shape[:1])
            plain = D + sigma * sa / (M - 1) + sigma * sigma * (mean_norm2 - trace / (M * (M - 1.0)))
        else:
            plain = D + sigma * sa / M + sigma * sigma * mean_norm2
        usable = (M >= 3) & (cqq > 4.0 * (M + 2) * U * sqq)
        beta = np.where(usable, sigma * caq / np.where(usable, cqq, 1.0), 0.0)
        beta = np.where(np.isnan(cqq + caq), np.nan, beta)          # a poisoned point stays poisoned
        flipd = plain - beta * (sq / M - D)
        resid = np.maximum(sigma * sigma * caa - 2.0 * beta * sigma * caq + beta * beta * cqq, 0.0)
        resid = np.where(np.isnan(caa + beta), np.nan, resid)
        stderr = np.sqrt(resid / (M - 1) / M) if M >= 2 else np.full(s.shape[:1], np.nan)
    return {'flipd': flipd, 'stderr': stderr, 'plain': plain, 'beta': beta}


def reading_host(S, Z, sigma, dtype=np.float64, debias=False, centred_trace=None):
    """The whole estimator for ONE point in numpy, every step in ``dtype`` (``np.longdouble``: the oracle of the tests): S, Z [M, D].
    -> the four readings as scalars of ``dtype`` and what the kernel is held to: 'rows' [M, 2] = (a', q), 'sums' [5], 'mean' [D],
    'mean_norm2', 'centred_trace'.  Moments are formed from centred values, not from raw sums.  ``debias``: the finite-M corrections of
    ``reading_from_sums(centred_trace=...)``, with the trace computed here unless ``centred_trace`` hands one in (a caller that checks
    a reading made with the spectrum's sum of squared singular values passes that very number)."""
    S, Z = np.asarray(S, dtype=dtype), np.asarray(Z, dtype=dtype)
    if S.ndim != 2 or S.shape != Z.shape:
        raise ValueError(f"reading_host: S {S.shape} and Z {Z.shape} must be the same [M, D]")
    M, D = S.shape
    sigma = dtype(sigma)
    mean = S.sum(axis=0) / dtype(M)
    a1 = (Z * (S - mean)).sum(axis=1)
    q = (Z * Z).sum(axis=1)
    a = sigma * a1
    norm2 = (mean * mean).sum()
    trace = ((S - mean) * (S - mean)).sum()
    if debias and M >= 2:
        used = trace if centred_trace is None else dtype(centred_trace)
        plain = dtype(D) + a.sum() / dtype(M - 1) + sigma * sigma * (norm2 - used / (dtype(M) * dtype(M - 1)))
    else:
        plain = dtype(D) + a.sum() / dtype(M) + sigma * sigma * norm2
    ac, qc = a - a.sum() / dtype(M), q - q.sum() / dtype(M)
    vq = (qc * qc).sum()
    beta = (ac * qc).sum() / vq if M >= 3 and vq > 0 else dtype(0)
    flipd = plain - beta * (q.sum() / dtype(M) - dtype(D))
    r = ac - beta * qc
    stderr = np.sqrt((r * r).sum() / dtype(M - 1) / dtype(M)) if M >= 2 else dtype(np.nan)
    return {'flipd': flipd, 'stderr': stderr, 'plain': plain, 'beta': beta, 'rows': np.stack([a1, q], axis=1),
            'sums': np.array([a1.sum(), (a1 * a1).sum(), q.sum(), (q * q).sum(), (a1 * q).sum()], dtype=dtype), 'mean': mean,
            'mean_norm2': norm2, 'centred_trace': trace}


def level_sigma(sde, t):
    """std(t) of the SDE's perturbation kernel, evaluated in fp64 on the host (as ``jacobian.flipd`` evaluates it)."""
    import torch
    return float(sde.marginal_prob(torch.ones((), dtype=torch.float64), torch.full((1,), float(t), dtype=torch.float64))[1].reshape(-1)[0])


def trace_of(singular_values):
    """sum of the squared singular values (float64, over the last axis): the trace of the centred Gram, sum_i |s_i - s^|^2."""
    sv = np.asarray(singular_values, dtype=np.float64)
    return (sv * sv).sum(axis=-1)


def sums_of(S, seeds=None, Z=None):
    """The device half for the score matrices S [P, M, D] (contiguous) of P points: (sums [P, 5], |s^|^2 [P]) fp64 on the device.  Noise as
    ``_lib.stein_rows`` takes it: the points' seeds (D % 4 == 0) or their noise matrices Z."""
    from . import _lib
    mean = _lib.column_means(S)
    _, sums = _lib.stein_rows(S, mean, seeds=seeds, Z=Z)
    return sums, (mean * mean).sum(dim=1)


def sampled_flipd(score_fn, sde, x, t, batchsize, seed, inflight_rows=None):
    """The reading of one point ``x`` (on the device) at time ``t`` for callers with a model object and no config: the score matrix of
    the sampled path through ``ScoreMatrixBuilder`` (M rows as the reference batches them for a loader batch of ``batchsize``), the
    noise keyed by ``seed``, then the Stein sums and the spectrum (``_lib.spectrum``: its squared singular values sum to the centred
    trace of the finite-M correction).  -> the dict of ``reading_from_sums`` as Python floats, with 'sigma', 't' and 'M'."""
    import torch
    from . import _lib, dim_reduction
    builder = dim_reduction.ScoreMatrixBuilder(score_fn, sde, t, x.device, inflight_rows)
    with torch.no_grad():
        S = builder.build(x, batchsize, t=t, seed=seed)
        M, D = S.shape
        Z = builder._seeded_noise(M, D, seed)[None] if D % 4 else None
        sums, norm2 = sums_of(S[None], seeds=None if D % 4 else [seed], Z=Z)
        sv = _lib.spectrum(S, full=True)
        if bool(torch.isnan(sv).any()):
            sv = _lib.resolve_failed_spectrum(S, full=True)
    sigma = level_sigma(sde, t)
    out = reading_from_sums(sums.cpu().numpy(), M, D, sigma, norm2.cpu().numpy(), centred_trace=trace_of(sv.cpu().numpy()))
    return {**{k: float(v[0]) for k, v in out.items()}, 'sigma': sigma, 't': float(t), 'M': M}
