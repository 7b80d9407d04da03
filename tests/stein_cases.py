"""Cases, oracle and error bounds for the Stein-divergence pass (csrc/stein.hip, id_diff_amd/stein.py).

ORACLE: ``stein.reading_host`` in ``np.longdouble`` on the fp32 inputs (64-bit mantissa on x86: 2^11 finer than the kernel's fp64).

BOUND, from the arithmetic of the kernel and not from what it returns.  With u = 2^-53, a row's a' = sum_c z_c (s_c - m_c) is D terms:
the mean handed to the kernel is the oracle's rounded to fp64 (1 u on |m_c|), the difference s_c - m_c is rounded once (1 u on
|s_c| + |m_c|), the product is fused into the accumulation, and D - 1 additions in any order (lane chains, then a butterfly) cost at most
(D - 1) u of sum |terms| to first order -- (D + 1) u sum_c |z_c| (|s_c| + |m_c|) in all; the issue's (D + 4) leaves room for the second-order
terms.  q = sum z_c^2 has no difference: D u q, held to (D + 2) u q.  A sum over M rows adds M - 1 additions and, for the second moments,
one fused product whose operands carry the row errors: the same with M + 2 more terms, on the sum of the absolute values:

    |a' - ref|         <= (D + 4) u A_i,                         A_i = sum_c |z_c| (|s_c| + |m_c|)
    |q - ref|          <= (D + 2) u q_i
    |sum a' - ref|     <= (D + M + 6) u sum_i A_i
    |sum a'^2 - ref|   <= 2 (D + M + 6) u sum_i A_i^2            (|a'| <= A_i; two factors)
    |sum q - ref|      <= (D + M + 4) u sum_i q_i
    |sum q^2 - ref|    <= 2 (D + M + 4) u sum_i q_i^2
    |sum a' q - ref|   <= (2 D + M + 8) u sum_i A_i q_i

``restated`` replays the kernel's order of operations in numpy fp64 (64 lanes over 4-column groups, butterfly, 256 threads over rows,
tree), without the fused multiply-add numpy lacks (one more rounding a term, inside the bound's allowance); ``MUTATIONS`` are ten
planted bugs of that replay, each of which must leave the bound."""
import numpy as np

from id_diff_amd import stein

LD = np.longdouble
U = 2.0 ** -53

# (P, M, D, given Z): one row, rows that are no multiple of the 4 waves of a workgroup, D no multiple of 4 (given Z only), more than
# one pass of the 64 lanes over a row (D > 256), more than one pass of the 256 threads of the sums over the rows (M > 256)
SHAPES = [(1, 1, 4, False), (2, 3, 8, False), (3, 65, 100, False), (1, 257, 12, False), (2, 17, 5, True), (1, 130, 193, True),
          (1, 40, 1024, False)]


def shape_id(shape):
    P, M, D, given = shape
    return f"P{P}-M{M}-D{D}" + ("-givenZ" if given else "")


def inputs(P, M, D, seed=0, sigma=0.05, Z=None):
    """(S [P, M, D] fp32, Z [P, M, D] fp32): a score field with a normal part, s = -P_N z / sigma + offset + noise, so that a' is a
    sum of like-signed terms of size |z|^2 / sigma, the column mean is not small and no row is special.  ``Z``: the noise to build
    the field on (the device's Philox draws) instead of numpy's."""
    rng = np.random.default_rng(1000 * seed + 7 * P + 3 * M + D)
    drawn = rng.standard_normal((P, M, D)).astype(np.float32)
    Z = drawn if Z is None else np.asarray(Z, dtype=np.float32).reshape(P, M, D)
    keep = (rng.random((P, 1, D)) < 0.8)                                  # the "normal" columns of each point
    S = -(Z.astype(np.float64) * keep) / sigma + rng.standard_normal((P, 1, D)) * 3.0 + 0.1 * rng.standard_normal((P, M, D))
    return S.astype(np.float32), Z


def oracle(S, Z):
    """Per point the long-double reference: rows [P, M, 2], sums [P, 5], mean [P, D] (long double) and the bound's weights A [P, M]."""
    P = S.shape[0]
    refs = [stein.reading_host(S[p], Z[p], 1.0, LD) for p in range(P)]
    rows, sums, mean = (np.stack([r[k] for r in refs]) for k in ('rows', 'sums', 'mean'))
    A = (np.abs(Z.astype(LD)) * (np.abs(S.astype(LD)) + np.abs(mean)[:, None, :])).sum(axis=2)
    return rows, sums, mean, A


def bounds(M, D, rows_ref, A, extra=0):
    """(bound on rows [P, M, 2], bound on sums [P, 5]) as derived above, float64.  ``extra``: further roundings on the mean the kernel
    was handed (M + 34 for the device's two-stage column mean, ``_lib.column_means``: M additions in 32 partial sums and a division),
    each worth u |z_c| |m_c| <= u A_i a row."""
    q = np.abs(rows_ref[..., 1]).astype(np.float64)
    A = A.astype(np.float64)
    Da = D + extra
    rows = np.stack([(Da + 4) * U * A, (D + 2) * U * q], axis=2)
    sums = np.stack([(Da + M + 6) * U * A.sum(1), 2 * (Da + M + 6) * U * (A * A).sum(1), (D + M + 4) * U * q.sum(1),
                     2 * (D + M + 4) * U * (q * q).sum(1), (Da + D + M + 8) * U * (A * q).sum(1)], axis=1)
    return rows, sums


def reading_tolerance(sums_ref, b_sums, M, D, sigma, norm2, trace=None, extra=0):
    """What the bound on the five sums allows the four readings to move: ``stein.reading_from_sums`` at the 32 corners sums_ref +- b_sums
    against its value at sums_ref, the largest move per key, doubled (the readings are smooth but not linear in the sums), plus what
    the device's |mean|^2 may differ by, sigma^2 (2 extra + D + 2) u |mean|^2.  One point: sums_ref, b_sums [5]."""
    s0 = np.asarray(sums_ref, dtype=np.float64)
    centre = stein.reading_from_sums(s0[None], M, D, sigma, norm2, centred_trace=trace)
    tol = {k: 0.0 for k in stein.KEYS}
    for corner in range(32):
        signs = np.array([1.0 if corner >> i & 1 else -1.0 for i in range(5)])
        moved = stein.reading_from_sums((s0 + signs * b_sums)[None], M, D, sigma, norm2, centred_trace=trace)
        for k in stein.KEYS:
            tol[k] = max(tol[k], abs(float(moved[k][0]) - float(centre[k][0])))
    slack = sigma * sigma * (2 * extra + D + 2) * U * abs(float(norm2))
    return {k: 2.0 * v + (slack if k in ('flipd', 'plain') else 0.0) for k, v in tol.items()}


def worst_ratio(err, bound):
    """max err / bound, a zero bound demanding a zero error."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


MUTATIONS = ("no_centre", "fp32_product", "fp32_accumulate", "mean_fp32", "drop_tail", "lost_lanes", "next_row_noise", "q_is_zs",
             "sums_drop_last_pass", "aq_is_qq")


def restated(S, Z, mean, mutate=None):
    """The kernel's order of operations for ONE point in numpy fp64: S, Z [M, D] fp32, mean [D] fp64 -> (rows [M, 2], sums [5])."""
    M, D = S.shape
    s, z, m = S.astype(np.float64), Z.astype(np.float64), np.asarray(mean, dtype=np.float64)
    if mutate == "mean_fp32":
        m = m.astype(np.float32).astype(np.float64)
    if mutate == "no_centre":
        m = np.zeros_like(m)
    if mutate == "next_row_noise":
        z = np.roll(z, -1, axis=0)
    if mutate == "drop_tail":
        s, z, m, D = s[:, :D // 4 * 4], z[:, :D // 4 * 4], m[:D // 4 * 4], D // 4 * 4
    G = (D + 3) // 4
    K = (G + 63) // 64
    pad = K * 256 - D

    def lanes(v):                                                          # [M, D] -> [M, K, 64, 4]: pass k, lane l, column j
        return np.pad(v, ((0, 0), (0, pad))).reshape(M, K, 64, 4)
    sl, zl, ml = lanes(s), lanes(z), lanes(np.broadcast_to(m, (M, D)))
    a, q = np.zeros((M, 64)), np.zeros((M, 64))
    for k in range(K):
        for j in range(4):
            zz, diff = zl[:, k, :, j], sl[:, k, :, j] - ml[:, k, :, j]
            if mutate == "fp32_product":
                term = (zz.astype(np.float32) * diff.astype(np.float32)).astype(np.float64)
            else:
                term = zz * diff
            a = (a.astype(np.float32) + term.astype(np.float32)).astype(np.float64) if mutate == "fp32_accumulate" else a + term
            q = q + (zz * sl[:, k, :, j] if mutate == "q_is_zs" else zz * zz)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        if mutate == "lost_lanes" and off == 32:
            continue
        a, q = a + a[:, lane ^ off], q + q[:, lane ^ off]
    rows = np.stack([a[:, 0], q[:, 0]], axis=1)
    passes = (M + 255) // 256
    part = np.zeros((5, 256))
    for k in range(passes):
        if mutate == "sums_drop_last_pass" and (k + 1) * 256 > M:
            break
        blk = np.zeros((256, 2))
        n = min(256, M - 256 * k)
        blk[:n] = rows[256 * k:256 * k + n]
        av, qv = blk[:, 0], blk[:, 1]
        part += np.stack([av, av * av, qv, qv * qv, qv * qv if mutate == "aq_is_qq" else av * qv])
    half = 128
    while half >= 1:
        part[:, :half] += part[:, half:2 * half]
        half //= 2
    return rows, part[:, 0].copy()


def linear_field(seed=0, D=64, d=5, M=1501, sigma=0.05):
    """(S, Z) fp32 of the synthetic linear field s = -P_N z / sigma around a point of a flat d-dimensional manifold in R^D, P_N the
    projector onto a random (D - d)-dimensional normal space: the rows the sampled path would evaluate for the exact score."""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((D, D)))[0]
    PN = Q[:, d:] @ Q[:, d:].T
    Z = rng.standard_normal((M, D)).astype(np.float32)
    return (-(Z.astype(np.float64) @ PN) / sigma).astype(np.float32), Z
