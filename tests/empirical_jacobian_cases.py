"""What tests/test_empirical_jacobian_host.py and tests/test_hip_empirical_jacobian.py share: the long-double oracle of
C(x, sigma) = sum_i w_i (d_i - m)(d_i - m)^T / sigma^2 (= I + sigma^2 times the Jacobian of the empirical score), the numpy restatement
of the arithmetic of csrc/empirical_jacobian.hip, the shapes and clouds of the GPU tests, and the error bound the kernel is held to.

The bound, per query b and on every entry of C, with u = 2^-53, r_b the distance to the farthest point whose weight is at least 2^-60
(``ee.reference_score``'s r), R_b the distance to the farthest point of the cloud and delta_b = (D + 4) u r_b^2 / sigma_b^2:

    |C - ref| <= [4 delta_b + 2 (N + D + 8) u] 4 r_b^2 / sigma_b^2  +  N 2^-60 4 R_b^2 / sigma_b^2

A length-D fp64 sum of squares errs by (D + 2) u relatively, so a logit -- and the difference of two -- by delta_b; a weight therefore
by 2 delta_b relatively, numerator and normaliser together 4 delta_b; every term w (d - m)(d - m)^T, and each of the two terms M / sum w
and m m^T the kernel subtracts, is at most (2 r_b)^2 / sigma^2; the streamed sums add N u, the products and the final subtraction and
division the rest of (N + D + 8); the points below 2^-60, which r_b does not see, are the last term.  ``mean`` has the same bound with
2 r_b (and 2 R_b) in place of 4 r_b^2 / sigma_b^2, the ESS (2^-22 + 4 delta_b) relatively (it is rounded to fp32).
"""
import numpy as np

from id_diff_amd.models import empirical_exact as ee

import empirical_cases as ec

U = 2.0 ** -53
TN = 32                                                                  # points per tile of the kernel
CAP = 192
REGIMES = [1e-3, 0.1, 1e3]          # times U(0.5, 2), query by query: one point holds all the weight / a neighbourhood / all alike
SHAPES = [(1, 1, 1), (3, 2, 3), (17, 33, 5), (5, 65, 16), (9, 31, 17), (6, 64, 33), (4, 1000, 100), (3, 4097, 128),
          (2, 257, CAP - 1), (2, 300, CAP)]
VARIANTS = ["plain", "offset1000", "far"]
CS_POINTS = np.concatenate([np.arange(0, 1024, 64), np.arange(1024, 4096, 192)])     # 16 of the circle, 16 of the sphere
CS_SIGMAS = [0.2, 0.3, 0.5]
_made = {}


def oracle(x, sigma, X):
    """C [B, D, D], mean [B, D], ess [B], r [B], R [B] as float64, computed in np.longdouble from direct differences and the
    definition, one query at a time, on the fp32 inputs as they are."""
    x, X = np.asarray(x, dtype=np.longdouble), np.asarray(X, dtype=np.longdouble)
    B, D = x.shape
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.longdouble), (B,))
    C, mean = np.empty((B, D, D)), np.empty((B, D))
    ess, r, R = np.empty(B), np.empty(B), np.empty(B)
    for b in range(B):
        d = X - x[b]
        d2 = (d * d).sum(axis=1)
        lg = -d2 / (2 * sigma[b] * sigma[b])
        w = np.exp(lg - lg.max())
        w = w / w.sum()
        m = (w[:, None] * d).sum(axis=0)
        e = d - m
        C[b] = ((w[:, None] * e).T @ e) / (sigma[b] * sigma[b])
        mean[b], ess[b] = m, 1 / (w * w).sum()
        r[b], R[b] = np.sqrt(d2[w >= ee.W_FLOOR].max()), np.sqrt(d2.max())
    return C, mean, ess, r, R


def restated(x, sigma, X, mutate=None):
    """The kernel's order of operations in fp64 numpy -> (C, mean, ess): pass 1 the largest logit over tiles of 32 points, pass 2
    w = exp(l - max) with the logits recomputed, sum w, sum w^2, sum w d and M = sum w d d^T tile after tile (a tile whose weights
    are all exactly 0 skipped), C = (M / sum w - m m^T) / sigma^2.  ``mutate`` plants one of the bugs the bound must catch: 'drop'
    loses the second-heaviest point, 'no_mm' forgets - m m^T, 'pad' lets the rows past N of the last tile act as points at the
    query."""
    x, X = np.asarray(x, dtype=np.float32), np.asarray(X, dtype=np.float32)
    B, D = x.shape
    N = X.shape[0]
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float32), (B,)).astype(np.float64)
    tiles = -(-N // TN)
    valid = (np.arange(tiles * TN) < N).reshape(tiles, TN)
    C, mean, ess = np.empty((B, D, D)), np.empty((B, D)), np.empty(B)
    for b in range(B):
        d = np.zeros((tiles * TN, D))
        d[:N] = X.astype(np.float64) - x[b].astype(np.float64)
        d = d.reshape(tiles, TN, D)
        inv2 = 0.5 / (sigma[b] * sigma[b])
        lg = np.where(valid | (mutate == 'pad'), -((d * d).sum(axis=2) * inv2), -np.inf)
        lmax = lg[valid].max()                                            # pass 1
        with np.errstate(over='ignore'):
            w = np.where(lg == -np.inf, 0.0, np.exp(lg - lmax))           # pass 2
        if mutate == 'drop' and N > 1:
            w.reshape(-1)[np.argsort(w.reshape(-1))[-2]] = 0.0
        live = (w != 0.0).any(axis=1)
        tot, tot2 = 0.0, 0.0
        md, M = np.zeros(D), np.zeros((D, D))
        for t in np.flatnonzero(live):
            tot, tot2 = tot + w[t].sum(), tot2 + (w[t] * w[t]).sum()
            md = md + w[t] @ d[t]
            M = M + (d[t] * w[t][:, None]).T @ d[t]
        m = md / tot
        C[b] = (M / tot - (0.0 if mutate == 'no_mm' else np.outer(m, m))) / (sigma[b] * sigma[b])
        mean[b], ess[b] = m, tot * tot / tot2
    return C, mean, ess


def bound(sigma, N, D, r, R):
    """(on C [B, 1, 1], on mean [B, 1], on ess relatively [B]): the bounds of the module docstring."""
    sigma, r, R = (np.asarray(v, dtype=np.float64) for v in (sigma, r, R))
    delta = (D + 4) * U * r * r / (sigma * sigma)
    rel = 4 * delta + 2 * (N + D + 8) * U
    tail = N * 2.0 ** -60
    bc = rel * 4 * r * r / (sigma * sigma) + tail * 4 * R * R / (sigma * sigma)
    bm = rel * 2 * r + tail * 2 * R
    return bc[:, None, None], bm[:, None], 2.0 ** -22 + 4 * delta


def inputs(B, N, D, variant):
    """(x, sigma, X), made once: N points of a sphere of dimension min(2, D - 1) in R^D, queries at sigma = REGIMES[b % 3] U(0.5, 2)
    from a point of the cloud, or 100 units away from it -- as tests/test_hip_empirical.py makes them."""
    key = (B, N, D, variant)
    if key not in _made:
        seed = 7 * B + 3 * N + D
        X = ec.sphere_cloud(N, min(2, D - 1), D, seed, offset=1000.0 if variant == "offset1000" else 0.0)
        x, sigma = ec.rows_near(X, B, REGIMES, seed + 1)
        if variant == "far":
            rng = np.random.default_rng(seed + 2)
            u = rng.standard_normal((B, D))
            x = (X[rng.integers(0, N, B)].astype(np.float64) + 100.0 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
        _made[key] = (x, sigma, X)
    return _made[key]


def case(B, N, D, variant):
    """``inputs`` and their oracle, made once: (x, sigma, X, C, mean, ess, r, R)."""
    key = (B, N, D, variant, "oracle")
    if key not in _made:
        _made[key] = inputs(B, N, D, variant) + oracle(*inputs(B, N, D, variant))
    return _made[key]


def worst_ratio(err, allowed):
    """max err / allowed, an error that is not finite counting as infinite and 0 / 0 as 0."""
    err = np.where(np.isfinite(err), err, np.inf)
    allowed = np.broadcast_to(allowed, err.shape)
    return float(np.divide(err, allowed, out=np.where(err > 0, np.inf, 0.0), where=allowed > 0).max())


def circle_and_sphere_case():
    """(X, x [32, 16], oracle per sigma of CS_SIGMAS: (C, mean, ess, r, R), want [32]) on ``ec.circle_and_sphere()``, made once.  The
    oracle takes each bandwidth as the fp32 number the kernel is given."""
    if "cs" not in _made:
        X = ec.circle_and_sphere()
        x = X[CS_POINTS]
        _made["cs"] = (X, x, [oracle(x, np.float32(s), X) for s in CS_SIGMAS], np.where(CS_POINTS < 1024, 1, 2))
    return _made["cs"]
