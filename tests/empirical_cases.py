"""What tests/test_empirical_host.py and tests/test_hip_empirical.py share: the clouds, the numpy restatement of the arithmetic of
csrc/empirical_score.hip, the long-double oracle and the error bound the fused kernel is held to.

The bound, with u = 2^-53, q_b = x_b - c and Ymax = max_i |y_i| (y_i = x_i - c, c the column mean):

    |out - ref|_bd <= u [ 4 (D + 8) (|q_b| Ymax + Ymax^2) / sigma_b^2  r_b  +  4 (N + D) Ymax ]

First order: a length-D fp64 dot product errs by at most D u |q| |y|, so a logit by delta = L_b of that size over sigma^2; a logit error
delta changes each weight by at most 2 delta w, hence the result by at most 2 delta sum_i w_i |x_i - x| <= 2 delta r_b (r_b the distance
to the farthest point that carries weight); the streamed sum of N terms adds at most N u Ymax.  It is loose against the arithmetic
(test_empirical_host.py measures 1e-3 of it) and far tighter than any wrong tile, mask or rescale: a dropped or doubled point, a
padded row acting as a point at the centre or a missed rescale moves the result by a fraction of the spacing of the data, 10^6 bounds.
"""
import numpy as np

from id_diff_amd.models import empirical_exact as ee

U = 2.0 ** -53


def line_cloud():
    """The train split of the committed line config, [8000, 100] fp32 numpy (the cloud of its ``empirical_exact`` model)."""
    from id_diff_amd.configs.utils import read_config
    cfg = read_config('configs/dimension_estimation/paper/euclidean_data/line/empirical.py')
    return ee.train_split(cfg).numpy()


def sphere_cloud(n, k, D, seed, radius=1.0, offset=0.0):
    """n uniform points of a radius-R k-sphere in a random (k + 1)-dimensional subspace of R^D, fp32."""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((D, k + 1)))[0]
    z = rng.standard_normal((n, k + 1))
    return (radius * (z / np.linalg.norm(z, axis=1, keepdims=True)) @ Q.T + offset).astype(np.float32)


def circle_and_sphere():
    """A unit circle (1024 points) and a radius-2 2-sphere (3072 points) in R^16; rows 0 .. 1023 are the circle."""
    return np.concatenate([sphere_cloud(1024, 1, 16, 21), sphere_cloud(3072, 2, 16, 22, radius=2.0)])


def expanded_score(x, sigma, X):
    """The kernel's arithmetic in fp64 numpy: centre, expand, ``q @ Y.T - h``, one softmax, ``w @ Y``.
    -> (sum_i w_i x_i - x [B, D], ess [B])."""
    x, X = np.asarray(x, dtype=np.float64), np.asarray(X, dtype=np.float64)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (x.shape[0],))
    c = X.mean(axis=0)
    Y = X - c
    h = 0.5 * (Y * Y).sum(axis=1)
    q = x - c
    lg = (q @ Y.T - h) / (sigma * sigma)[:, None]
    w = np.exp(lg - lg.max(axis=1, keepdims=True))
    return (w @ Y) / w.sum(axis=1, keepdims=True) - q, w.sum(axis=1) ** 2 / (w * w).sum(axis=1)


def oracle(x, sigma, X):
    """``reference_score`` (direct differences) in np.longdouble on the fp32 inputs as they are -> (out, ess, r) as float64."""
    out, ess, r = ee.reference_score(np.asarray(x, dtype=np.longdouble), np.asarray(sigma, dtype=np.longdouble),
                                     np.asarray(X, dtype=np.longdouble))
    return out.astype(np.float64), ess.astype(np.float64), r.astype(np.float64)


def logit_term(x, sigma, X):
    """L_b [B] = u 4 (D + 8) (|q_b| Ymax + Ymax^2) / sigma_b^2."""
    x, X = np.asarray(x, dtype=np.float64), np.asarray(X, dtype=np.float64)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (x.shape[0],))
    c = X.mean(axis=0)
    ymax = np.sqrt(((X - c) ** 2).sum(axis=1).max())
    qn = np.sqrt(((x - c) ** 2).sum(axis=1))
    return U * 4 * (X.shape[1] + 8) * (qn * ymax + ymax * ymax) / (sigma * sigma), ymax


def bound(x, sigma, X, r):
    """[B, 1]: the bound of the module docstring on every entry of row b."""
    L, ymax = logit_term(x, sigma, X)
    return (L * r + U * 4 * (X.shape[0] + X.shape[1]) * ymax)[:, None]


def rows_near(X, B, scales, seed):
    """B fp32 query rows: a point of the cloud plus sigma_b times standard normal noise, sigma_b = scales[b % len] U(0.5, 2) (fp32)."""
    rng = np.random.default_rng(seed)
    sigma = (np.asarray(scales, dtype=np.float64)[np.arange(B) % len(scales)] * rng.uniform(0.5, 2.0, B)).astype(np.float32)
    x = X[rng.integers(0, X.shape[0], B)].astype(np.float64) + sigma[:, None].astype(np.float64) * rng.standard_normal((B, X.shape[1]))
    return x.astype(np.float32), sigma


def oracle_id(point, sigma, X, rows, seed, score=expanded_score):
    """The driver's recipe on the host: ``rows`` draws x + sigma z around ``point``, their scores, numpy SVD of the column-centred
    score matrix, ``estimate_dim`` -> (ID, median ESS)."""
    from id_diff_amd.plot_utils import estimate_dim
    rng = np.random.default_rng(seed)
    xs = (np.asarray(point, dtype=np.float64)[None, :] + sigma * rng.standard_normal((rows, X.shape[1]))).astype(np.float32)
    out, ess = score(xs, sigma, X)[:2]
    S = out / (sigma * sigma)
    sv = np.linalg.svd(S - S.mean(axis=0), compute_uv=False)
    return estimate_dim(sv.tolist()), float(np.median(ess))
