"""Shapes, long-double oracle and error bound of the simplex-skewness tests (tests/test_simplex_host.py, tests/test_hip_simplex.py).

Oracle: direct from the fp32 rows in long double (x87: 64-bit mantissa), no Gram matrix of point-centred rows and no subtraction
of near-equal products.  Per neighbourhood: v_j = x_j - mean over its m' rows; per pair the weight |v_i| |v_j|, the product
|v_i . v_j| and the area as |v_big| |v_small - (v_small . v_big / |v_big|^2) v_big|, a length times a length.

Bound, from the arithmetic of csrc/simplex.hip alone, never from its output.  u = 2^-53, R^2 = max_j |y_j|^2 over the
neighbourhood's rows, y_j = x_j - x_centre.
  entry of B:   y rounded once (2 u R^2 in a product), the dot product over D (D u R^2), a row mean (m' u R^2 on top), the grand
                mean (2 m' u R^2 on top), three additions (9 u R^2):  (4 D + 4 m' + 17) u R^2  <=  eps = C (D + 4 m') u R^2, C = 8
                (C = 8 leaves a factor of at least 2 at every D >= 1, m' >= 3; the constant of the local-PCA tests).
  |B_ij|:       eps.
  |v_i|:        e_i = min(sqrt(eps), eps / |v_i|) + 2 u |v_i|           [|sqrt(a + d) - sqrt(a)| <= min(sqrt|d|, |d| / sqrt(a))]
  w_ij:         e_i |v_j| + e_j |v_i| + e_i e_j + u w_ij                 (linear in eps wherever eps < |v|^2)
  area:         its square B_ii B_jj - B_ij^2 is off by d = eps (|v_i|^2 + |v_j|^2 + 2 |B_ij|) + 2 eps^2 + 3 u w_ij^2; the same
                inequality gives min(sqrt(d), d / area) + u area -- the sqrt(d) branch is what admits about 1e-8 w on vectors
                that are exactly collinear (a clamped negative square is inside it: 0 <= true square <= d there)
  sums:         the pair terms above, and (m' + 32) u of each sum for adding it up (at most ceil(m'^2 / 256) + 8 additions deep in
                the kernel, 16 + log2(pairs / 128) in numpy)
  quotient:     |A~ / W~ - A / W| <= (dA + (A / W) dW) / (W - dW) + u A / W, infinite (nothing is claimed) where W <= dW.
"""
import functools
import hashlib

import numpy as np
import torch

C = 8.0
U = 2.0 ** -53
LD = np.longdouble
K64_SCALES = (2, 14, 15, 16, 17, 31, 32, 47, 48, 63, 64)


def cases(chunk):
    """(N, D, k, scales): the shapes of tests/test_hip_lpca.py (chunk = the columns one gather step takes), the scales on the
    edges of the 16 x 16 tiles (m' = k' + 1 = 16, 17, 32, 33, 48, 49, 64, 65), the smallest (k' = 2) and the largest (k' = k)."""
    return [(4, 1, 2, (2,)), (40, 3, 15, (2, 7, 15)), (40, 3, 16, (2, 15, 16)), (100, 17, 16, (3, 15, 16)),
            (300, 100, 20, (2, 14, 15, 16, 20)), (200, 100, 64, K64_SCALES), (150, chunk + 1, 31, (2, 15, 16, 30, 31)),
            (150, 2 * chunk - 3, 31, (15, 16, 31)), (120, 3072, 20, (2, 15, 16, 20))]


def data(N, D, k):
    g = torch.Generator().manual_seed(N + D + k)
    X = torch.randn(N, D, generator=g)
    X[:, 20:] *= 0.05                  # a low-dimensional structure, as the ID data have (test_hip_lpca.py)
    return X


def brute_knn(X, k):
    """idx [N, k] int64: the k nearest OTHER rows in fp64, ascending, equal distances by lower index (what _lib.knn returns)."""
    X = np.asarray(X, dtype=np.float64)
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2) if X.shape[0] * X.shape[0] * X.shape[1] <= 1 << 24 else \
        (X * X).sum(1)[:, None] - 2.0 * X @ X.T + (X * X).sum(1)[None, :]
    np.fill_diagonal(d2, np.inf)
    return np.argsort(d2, axis=1, kind='stable')[:, :k].astype(np.int64)


def two_spheres():
    """The acceptance data: a unit 2-sphere (rows 0 .. 1023) and a unit 4-sphere moved by 5 along axis 8 (rows 1024 .. 2047) in
    R^16, fp32."""
    rng = np.random.default_rng(0)
    a = rng.standard_normal((1024, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = rng.standard_normal((1024, 5))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    X = np.zeros((2048, 16))
    X[:1024, :3] = a
    X[1024:, :5] = b
    X[1024:, 8] += 5
    return X.astype(np.float32)


def line_points():
    """Ten points exactly on a line in R^5 (small integers, exact in fp32), row 0 the query: X [10, 5] fp32."""
    direction = np.array([1.0, -2.0, 0.0, 3.0, 1.0])
    t = np.array([0.0, 1.0, -1.0, 2.0, 4.0, -3.0, 5.0, 7.0, -6.0, 8.0])
    return (t[:, None] * direction[None, :] + np.array([1.0, 2.0, 3.0, 4.0, 5.0])).astype(np.float32)


def _as_numpy(a, dtype):
    return np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=dtype)


def oracle(X, idx, ks, centre=None):
    """``(ess, bound)``, both [Q, S, 3] fp64: the long-double values of (ess_a, ess_b, weight sum) of every neighbourhood
    {centre[q]} + idx[q, :ks[s]] of the fp32 rows X, and the bound on what csrc/simplex.hip (and its numpy restatement) may
    differ from them by.  NaN, NaN, 0 where the weight sum is 0; the bound is inf where the weight sum is not above its own."""
    X = _as_numpy(X, np.float32)
    X = X.reshape(X.shape[0], -1)
    idx = _as_numpy(idx, np.int64)
    Q, k = idx.shape
    D = X.shape[1]
    centre = np.arange(Q) if centre is None else _as_numpy(centre, np.int64).reshape(-1)
    ids = np.concatenate([centre[:, None], idx], axis=1)
    ess, bound = np.empty((Q, len(ks), 3)), np.empty((Q, len(ks), 3))
    step = max(1, (1 << 20) // ((k + 1) * D))
    with np.errstate(divide='ignore', invalid='ignore'):
        for q0 in range(0, Q, step):
            rows = X[ids[q0:q0 + step]].astype(LD)                               # [q, m, D]
            for s, kk in enumerate(ks):
                m = kk + 1
                e, b = _oracle_block(rows[:, :m], D)
                ess[q0:q0 + step, s], bound[q0:q0 + step, s] = e, b
    return ess, bound


def _oracle_block(rows, D):
    q, m, _ = rows.shape
    V = rows - rows.sum(axis=1, keepdims=True) / LD(m)
    Y = rows - rows[:, :1]
    R2 = np.einsum('qjd,qjd->qj', Y, Y).max(axis=1)
    eps = LD(C * (D + 4 * m) * U) * R2                                           # [q]
    n = np.sqrt(np.einsum('qjd,qjd->qj', V, V))
    order = np.argsort(-n.astype(np.float64), axis=1, kind='stable')             # the longer vector of a pair comes first
    V = np.take_along_axis(V, order[:, :, None], axis=1)
    n = np.take_along_axis(n, order, axis=1)
    e = np.minimum(np.sqrt(eps)[:, None], np.where(n > 0, eps[:, None] / np.where(n > 0, n, 1), np.inf)) + 2 * U * n
    A, B, W, dA, dB, dW = (np.zeros(q, dtype=LD) for _ in range(6))
    for i in range(m - 1):
        vi, ni, rest, nj = V[:, i], n[:, i:i + 1], V[:, i + 1:], n[:, i + 1:]
        dots = np.einsum('qrd,qd->qr', rest, vi)
        coef = np.where(ni > 0, dots / np.where(ni > 0, ni * ni, 1), 0)
        resid = rest - coef[:, :, None] * vi[:, None, :]
        area = ni * np.sqrt(np.einsum('qrd,qrd->qr', resid, resid))
        w = ni * nj
        ei, ej = e[:, i:i + 1], e[:, i + 1:]
        d = eps[:, None] * (ni * ni + nj * nj + 2 * np.abs(dots)) + 2 * eps[:, None] ** 2 + 3 * U * w * w
        d_area = np.minimum(np.sqrt(d), np.where(area > 0, d / np.where(area > 0, area, 1), np.inf)) + U * area
        A += area.sum(axis=1); B += np.abs(dots).sum(axis=1); W += w.sum(axis=1)
        dA += d_area.sum(axis=1); dB += eps * dots.shape[1]; dW += (ei * nj + ej * ni + ei * ej + U * w).sum(axis=1)
    tail = LD((m + 32) * U)
    dA, dB, dW = dA + tail * A, dB + tail * B, dW + tail * W
    ok, sure = W > 0, W > dW
    Wd = np.where(ok, W, 1)
    a, b = np.where(ok, A / Wd, np.nan), np.where(ok, B / Wd, np.nan)
    room = np.where(sure, W - dW, 1)
    ba = np.where(sure, (dA + a * dW) / room + U * a, np.inf)
    bb = np.where(sure, (dB + b * dW) / room + U * b, np.inf)
    ess = np.stack([a, b, W], axis=1).astype(np.float64)
    bound = np.stack([np.where(ok, ba, np.nan), np.where(ok, bb, np.nan), dW], axis=1).astype(np.float64)
    return ess, bound


_CACHE = {}


def oracle_cached(X, idx, ks, centre=None):
    """``oracle`` once per (rows, neighbours, scales): the host test and the GPU test of one run share it when the GPU's
    neighbours are the brute-force ones.  The arrays returned are shared: never modified."""
    h = hashlib.sha1()
    for a in (_as_numpy(X, np.float32), _as_numpy(idx, np.int64), np.asarray(ks, dtype=np.int64),
              np.zeros(0) if centre is None else _as_numpy(centre, np.int64)):
        h.update(np.ascontiguousarray(a).tobytes())
        h.update(str(a.shape).encode())
    key = h.hexdigest()
    if key not in _CACHE:
        _CACHE[key] = oracle(X, idx, ks, centre)
    return _CACHE[key]


@functools.lru_cache(maxsize=None)
def host_case(N, D, k, ks):
    """(X fp32 torch, brute-force idx) of a shape, shared."""
    X = data(N, D, k)
    return X, brute_knn(X.numpy(), k)


def worst_ratio(got, ref, bound):
    """max over the entries of |got - ref| / bound, the NaN pattern of got and ref having to agree (inf if it does not); an entry
    whose bound is inf claims nothing."""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return np.inf
    live = ~np.isnan(ref) & np.isfinite(bound)
    if not live.any():
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(got[live] == ref[live], 0.0, np.abs(got[live] - ref[live]) / bound[live])
    return float(np.max(ratio))
