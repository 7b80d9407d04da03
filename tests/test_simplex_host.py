"""Host side of the simplex skewness (id_diff_amd/simplex.py): the reference curves against quadrature, their inversion, the inf
and NaN rules, ``stable_dims``, the fp64 numpy restatement of csrc/simplex.hip against the long-double oracle under the bound of
tests/simplex_cases.py, planted mutations of that restatement against the same bound, the ``ess_knn_<k>`` name of
``benchmark.Benchmark`` and what idiff_simplex_skewness_f64 refuses before any device call.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd import _lib, benchmark, simplex

import simplex_cases as sc

CHUNK = 64                             # _lib.LOCAL_PCA_CHUNK, which needs the library; test_hip_simplex.py asserts they agree


# ------------------------------------------------------------------------------------------- the reference curves
def _quadrature(n, f):
    """int f(theta) sin^(n-2) theta dtheta / int sin^(n-2) theta dtheta over [0, pi], Gauss-Legendre on the halves (|cos| has a
    kink at pi / 2); the weight is formed as exp((n - 2) log sin) so that it neither overflows nor underflows to garbage."""
    x, w = _NODES
    num = den = 0.0
    for lo, hi in ((0.0, math.pi / 2), (math.pi / 2, math.pi)):
        th = 0.5 * (hi - lo) * x + 0.5 * (hi + lo)
        wt = w * np.exp((n - 2) * np.log(np.sin(th)))
        num, den = num + np.sum(wt * f(th)), den + np.sum(wt)
    return num / den


_NODES = np.polynomial.legendre.leggauss(400)


def test_reference_against_quadrature():
    worst = 0.0
    for n in range(2, 201):
        a, b = float(simplex.reference(n, 'a')), float(simplex.reference(n, 'b'))
        worst = max(worst, abs(a - _quadrature(n, lambda t: np.abs(np.sin(t)))), abs(b - _quadrature(n, lambda t: np.abs(np.cos(t)))))
    print(f"reference(n) against Gauss-Legendre, n = 2 .. 200: worst difference {worst:.2e}")
    assert worst <= 1e-12
    assert abs(float(simplex.reference(2, 'a')) - 2 / math.pi) <= 1e-15 and abs(float(simplex.reference(2, 'b')) - 2 / math.pi) <= 1e-15
    assert abs(float(simplex.reference(3, 'a')) - math.pi / 4) <= 1e-15 and abs(float(simplex.reference(3, 'b')) - 0.5) <= 1e-15
    assert float(simplex.reference(1, 'a')) == 0.0 and float(simplex.reference(1, 'b')) == 1.0
    with pytest.raises(ValueError):
        simplex.reference(0, 'a')
    with pytest.raises(ValueError):
        simplex.reference(2, 'c')


def test_reference_is_strictly_monotone_where_the_two_formulas_meet():
    n = np.arange(1, 4097)
    assert np.all(np.diff(simplex.reference(n, 'a')) > 0) and np.all(np.diff(simplex.reference(n, 'b')) < 0)
    big = np.arange((1 << 20) - 2000, (1 << 20) + 3)
    assert np.all(np.diff(simplex.reference(big, 'a')) > 0) and np.all(np.diff(simplex.reference(big, 'b')) < 0)


@pytest.mark.parametrize("ver", ['a', 'b'])
def test_dims_invert_the_reference(ver):
    rng = np.random.default_rng(1)
    n = np.unique(np.concatenate([np.arange(1, 200), 2 ** np.arange(1, 20), 2 ** np.arange(1, 20) + 1, 2 ** np.arange(2, 20) - 1,
                                  rng.integers(200, 10 ** 6, 2000), [10 ** 6]]))
    assert np.array_equal(simplex.dims_from_skewness(simplex.reference(n, ver), ver), n.astype(np.float64))
    # in between: linear in the value, so the midpoint of two neighbouring reference values reads n + 1/2, and monotone
    n = n[n < 10 ** 5]
    mid = 0.5 * (simplex.reference(n, ver) + simplex.reference(n + 1, ver))
    np.testing.assert_allclose(simplex.dims_from_skewness(mid, ver), n + 0.5, rtol=0, atol=1e-3)
    grid = np.linspace(0.001, 0.999, 4001)
    dims = simplex.dims_from_skewness(grid, ver)
    assert np.all(np.isfinite(dims)) and np.all(dims >= 1.0)
    assert np.all(np.diff(dims) > 0) if ver == 'a' else np.all(np.diff(dims) < 0)


def test_inf_and_nan_rules():
    a = simplex.dims_from_skewness(np.array([[0.0, 1.0, 1.5, np.nan], [1 - 2.0 ** -22, 1 - 2.0 ** -19, 2 / math.pi, np.inf]]), 'a')
    assert a.shape == (2, 4)
    assert a[0, 0] == 1.0 and np.isinf(a[0, 1]) and np.isinf(a[0, 2]) and np.isnan(a[0, 3])
    assert np.isinf(a[1, 0]) and 2 ** 17 < a[1, 1] < 2 ** 20 and abs(a[1, 2] - 2.0) <= 1e-14 and np.isinf(a[1, 3])
    b = simplex.dims_from_skewness(np.array([1.0, 1.0 + 1e-12, 0.0, -0.1, np.nan, 1e-4, 1e-2]), 'b')
    assert b[0] == 1.0 and b[1] == 1.0 and np.isinf(b[2]) and np.isinf(b[3]) and np.isnan(b[4]) and np.isinf(b[5])
    assert 6000 < b[6] < 6800                              # ref_b(n) ~ sqrt(2 / (pi n))
    assert simplex.dims_from_skewness(torch.tensor([math.pi / 4], dtype=torch.float64))[0] == pytest.approx(3.0, abs=1e-12)
    with pytest.raises(ValueError):
        simplex.dims_from_skewness(np.zeros(3), 'c')


def test_only_pairs_are_implemented():
    for call in (lambda: simplex.skewness(np.zeros((4, 2), np.float32), (2,), d=2), lambda: simplex.local_dims(None, 5, d=3),
                 lambda: simplex.scale_curve(None, (2, 3), d=0)):
        with pytest.raises(NotImplementedError, match="d = "):
            call()


def test_stable_dims():
    ks = (8, 12, 16, 24, 32)
    curve = np.array([[2.1, 2.2, 2.6, 3.4, 3.3],           # 2 2 3 3 3 -> 3
                      [2.1, 2.2, 3.3, 3.4, 4.1],           # 2 2 3 3 4: a tie -> the run at the larger sizes
                      [np.nan, 4.2, 4.3, np.inf, 5.0],     # a non-finite reading ends a run
                      [np.nan, np.nan, np.inf, np.nan, np.nan],
                      [1.0, 2.0, 3.0, 4.0, 5.0]])
    assert simplex.stable_dims(curve, ks).tolist() == [3, 3, 4, -1, 5]
    assert simplex.stable_dims(curve, ks).dtype == np.int64
    with pytest.raises(ValueError):
        simplex.stable_dims(curve, ks[:3])


# ------------------------------------------------------------------------------------------- the restatement and its bound
@pytest.mark.parametrize("case", range(9))
def test_host_restatement_inside_the_bound(case):
    N, D, k, ks = sc.cases(CHUNK)[case]
    X, idx = sc.host_case(N, D, k, ks)
    ref, bound = sc.oracle_cached(X, idx, ks)
    got = simplex.skewness_host(X, idx, ks)
    assert got.shape == (N, len(ks), 3) and np.isfinite(got).all() and np.isfinite(bound).all()
    ratio = sc.worst_ratio(got, ref, bound)
    print(f"N={N} D={D} k={k} scales {ks}: skewness_host max |err| / bound {ratio:.3e}; bound on ess_a {bound[..., 0].min():.1e} .. "
          f"{bound[..., 0].max():.1e}")
    assert ratio <= 1.0


def test_host_restatement_on_the_edge_cases():
    g = torch.Generator().manual_seed(11)
    X = (1000.0 + 0.01 * torch.randn(200, 8, generator=g, dtype=torch.float64)).float()
    idx = sc.brute_knn(X.numpy(), 12)
    ref, bound = sc.oracle_cached(X, idx, (2, 6, 12))
    assert sc.worst_ratio(simplex.skewness_host(X, idx, (2, 6, 12)), ref, bound) <= 1.0
    # points exactly on a line: no area, all cosines 1
    L, lidx = sc.line_points(), np.arange(1, 10)[None, :]
    ref, bound = sc.oracle(L, lidx, (4, 9))
    got = simplex.skewness_host(L, lidx, (4, 9))
    assert np.all(ref[..., 0] <= 1e-18) and np.all(np.abs(ref[..., 1] - 1.0) <= 1e-18)      # the long-double mean is rounded too
    assert np.all(got[..., 0] <= bound[..., 0]) and np.all(np.abs(got[..., 1] - 1.0) <= bound[..., 1])
    assert np.all(np.abs(simplex.dims_from_skewness(got[..., 0], 'a') - 1.0) <= 1e-6)
    print(f"line: ess_a {got[0, :, 0]} under the bound {bound[0, :, 0]}")
    # identical points: NaN, NaN, 0 -- and the other scales of a query are served
    same = np.tile(np.array([[1.5, -2.0, 0.25]], dtype=np.float32), (6, 1))
    same = np.concatenate([same, np.array([[3.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)])
    got = simplex.skewness_host(same, np.array([[1, 2, 3, 4, 5, 6, 7]]), (3, 5, 7))
    assert np.isnan(got[0, :2, :2]).all() and np.all(got[0, :2, 2] == 0.0) and np.isfinite(got[0, 2]).all()
    ref, _ = sc.oracle(same, np.array([[1, 2, 3, 4, 5, 6, 7]]), (3, 5, 7))
    assert np.array_equal(np.isnan(ref), np.isnan(got))
    # a subset of the queries
    X, idx = sc.host_case(40, 3, 15, (2, 7, 15))
    full = simplex.skewness_host(X, idx, (2, 7, 15))
    assert np.array_equal(simplex.skewness_host(X, idx[[4, 17]], (2, 7, 15), centre=[4, 17]), full[[4, 17]])
    assert np.array_equal(simplex.skewness_host(X, idx, (7,)), full[:, 1:2])
    with pytest.raises(ValueError):
        simplex.skewness_host(X, idx, (7, 7))
    with pytest.raises(ValueError):
        simplex.skewness_host(X, idx, (16,))


# ------------------------------------------------------------------------------------------- planted mutations
def _mutant(X, idx, ks, kind):
    """``simplex.skewness_host`` with one planted mistake (query by query, plainly)."""
    X = np.asarray(X, dtype=np.float64)
    Q, k = idx.shape
    out = np.empty((Q, len(ks), 3))
    for q in range(Q):
        rows = X[np.concatenate([[q], idx[q]])]
        if kind == 'reversed_neighbours':
            rows = np.concatenate([rows[:1], rows[:0:-1]])
        Y = rows - rows[0]
        if kind == 'gram_of_raw_rows':
            Y = rows
        G = (Y.astype(np.float32) @ Y.astype(np.float32).T).astype(np.float64) if kind == 'fp32_gram' else Y @ Y.T
        for s, kk in enumerate(ks):
            m = kk + 1
            if kind == 'centre_left_out':
                Gs = G[1:m, 1:m]
                m = m - 1
            else:
                Gs = G[:m, :m]
            div = k + 1 if kind == 'mean_over_m' else m
            r = (G[:m, :].sum(axis=1) if kind == 'row_mean_over_full_block' else Gs.sum(axis=1)) / div
            g = 0.0 if kind == 'no_grand_mean' else r.sum() / div
            B = Gs.copy() if kind == 'point_centred' else Gs - (r[:, None] + r[None, :]) + g
            if kind == 'padding_rows':
                mp = 16 * ((m + 15) // 16)
                P = np.zeros((mp, mp))
                P[:m, :m] = Gs
                rp = np.concatenate([r, np.zeros(mp - m)])
                B, m = P - (rp[:, None] + rp[None, :]) + g, mp
            diag = np.maximum(np.diag(B), 0.0)
            nrm = np.sqrt(np.maximum(np.diag(Gs), 0.0)) if kind == 'weights_from_G' else np.sqrt(diag)
            i, j = np.triu_indices(m, 0 if kind == 'diagonal_pairs' else 1)
            sq = diag[i] * diag[j] - B[i, j] ** 2
            with np.errstate(invalid='ignore'):
                area = np.sqrt(sq if kind == 'no_clamp' else np.maximum(sq, 0.0)).sum()
            dot = B[i, j].sum() if kind == 'signed_cosine' else np.abs(B[i, j]).sum()
            w = (0.5 * (diag[i] + diag[j])).sum() if kind == 'arithmetic_weights' else (nrm[i] * nrm[j]).sum()
            with np.errstate(divide='ignore', invalid='ignore'):
                out[q, s] = (area / w, dot / w, w)
    return out


MUTATIONS = ('mean_over_m', 'point_centred', 'no_clamp', 'diagonal_pairs', 'padding_rows', 'row_mean_over_full_block', 'weights_from_G',
             'no_grand_mean', 'reversed_neighbours', 'fp32_gram', 'gram_of_raw_rows', 'signed_cosine', 'arithmetic_weights',
             'centre_left_out')


def test_planted_mutations_leave_the_bound():
    """Each mistake, on the data that can show it: (100, 17, 16) at scales below and at k; the line for the clamp (a negative
    square needs collinear rows); the translated cloud for the Gram matrix of raw rows.  The unmutated restatement passes on all
    three (the tests above)."""
    N, D, k, ks = 100, 17, 16, (3, 15, 16)
    X, idx = sc.host_case(N, D, k, ks)
    generic = (X.numpy(), idx, ks) + sc.oracle_cached(X, idx, ks)
    L, lidx = sc.line_points(), np.arange(1, 10)[None, :]
    line = (L, lidx, (4, 9)) + sc.oracle(L, lidx, (4, 9))
    g = torch.Generator().manual_seed(11)
    T = (1000.0 + 0.01 * torch.randn(200, 8, generator=g, dtype=torch.float64)).float().numpy()
    tidx = sc.brute_knn(T, 12)
    far = (T[:], tidx[:40], (2, 6, 12)) + tuple(a[:40] for a in sc.oracle_cached(T, tidx, (2, 6, 12)))
    assert len(MUTATIONS) >= 10
    factors = {}
    for kind in MUTATIONS:
        Xm, im, km, ref, bound = line if kind == 'no_clamp' else far if kind == 'gram_of_raw_rows' else generic
        factors[kind] = sc.worst_ratio(_mutant(Xm, im, km, kind), ref, bound)
    for kind, f in sorted(factors.items(), key=lambda t: t[1]):
        print(f"  {kind:26s} leaves the bound by a factor of {f:.3e}")
    mildest = min(factors, key=factors.get)
    print(f"mildest mutation: {mildest}, {factors[mildest]:.3e} times the bound")
    assert all(f > 1.0 for f in factors.values()), {k_: f for k_, f in factors.items() if not f > 1.0}


# ------------------------------------------------------------------------------------------- the arithmetic on two spheres
def test_two_spheres_on_the_host():
    """The acceptance data with brute-force neighbours: the floors tests/test_hip_simplex.py holds the GPU to, here on the
    restatement."""
    X = sc.two_spheres()
    assert X.shape == (2048, 16) and X.dtype == np.float32
    idx = sc.brute_knn(X, 64)
    ess = simplex.skewness_host(X, idx, simplex.SCALES)
    curve = simplex.dims_from_skewness(ess[..., 0], 'a')
    two = {k: int((np.rint(curve[:1024, s]) == 2).sum()) for s, k in enumerate(simplex.SCALES)}
    four = {k: int((np.rint(curve[1024:, s]) == 4).sum()) for s, k in enumerate(simplex.SCALES)}
    stable = simplex.stable_dims(curve, simplex.SCALES)
    s2, s4 = int((stable[:1024] == 2).sum()), int((stable[1024:] == 4).sum())
    print(f"2-sphere reads 2: {two}; 4-sphere reads 4: {four}; stable_dims: {s2} and {s4} of 1024")
    print("mean reading: " + ", ".join(f"k={k}: {curve[:1024, s].mean():.2f} / {curve[1024:, s].mean():.2f}"
                                       for s, k in enumerate(simplex.SCALES)))
    assert all(two[k] >= 1016 for k in (12, 16, 24, 32, 48, 64))
    assert four[48] >= 1016 and four[64] >= 1016 and four[32] >= 940 and four[16] >= 780
    assert s2 >= 1000 and s4 >= 1000


# ------------------------------------------------------------------------------------------- Benchmark's estimator name
def test_benchmark_understands_ess_knn_names(tmp_path, monkeypatch):
    assert benchmark.ess_knn_k('ess_knn_20') == 20
    assert [benchmark.ess_knn_k(n) for n in ('ess', 'ess_knn_', 'ess_knn_x', 'ess_knn_-3', 'lpca_knn_4', 'xess_knn_4')] == [None] * 6
    seen = {}

    def fake_local_dims(X, k=20, ver='a', d=1):
        seen['k'], seen['X'] = k, X
        return np.array([2.0, 2.5, 3.0, 4.5])

    monkeypatch.setattr(simplex, 'local_dims', fake_local_dims)
    bm = benchmark.Benchmark(str(tmp_path / 'out.csv'), {'u': None})
    assert bm.estimators == ['mle_5', 'mle_20', 'lpca', 'ppca']              # the default list is unchanged
    assert list(bm.results.index) == bm.estimators
    data = object()
    bm.evaluate_estimator(data, 'ess_knn_20', 'u')
    assert seen['k'] == 20 and seen['X'] is data
    assert bm.results.loc['ess_knn_20', 'u'] == 3.0
    import pandas as pd
    saved = pd.read_csv(bm.file_name, index_col='method')
    assert list(saved.index) == ['mle_5', 'mle_20', 'lpca', 'ppca', 'ess_knn_20'] and saved.loc['ess_knn_20', 'u'] == 3.0
    seen.clear()
    bm.evaluate_estimator(data, 'ess_knn_20', 'u')                            # filled: not evaluated again
    assert not seen
    again = benchmark.Benchmark(bm.file_name, {'u': None, 'v': None})         # a saved row is kept by a later run
    assert again.estimators == ['mle_5', 'mle_20', 'lpca', 'ppca'] and again.results.loc['ess_knn_20', 'u'] == 3.0
    with pytest.raises(KeyError):
        again.evaluate_estimator(None, 'ess_knn', 'u')


# ------------------------------------------------------------------------------------------- refusals before any device call
def _raw(k=4, S=2, scales=(2, 4), N=10, D=3, Q=1, null=None):
    """idiff_simplex_skewness_f64 with pointers that are never dereferenced on the device: every call here is refused on the host."""
    buf = (ctypes.c_int * max(len(scales), 1))(*scales)
    ptr = {name: 64 for name in ('X', 'centre', 'idx', 'ess', 'status')}
    ptr['scales'] = ctypes.cast(buf, ctypes.c_void_p).value
    if null:
        ptr[null] = 0
    rc = _lib.lib().idiff_simplex_skewness_f64(ptr['X'], N, D, ptr['centre'], ptr['idx'], Q, k, ptr['scales'], S, ptr['ess'],
                                               ptr['status'], 0)
    return rc, _lib.lib().idiff_last_error().decode()


REFUSALS = [(dict(k=1, scales=(1,), S=1), "k = 1 outside 2..64"), (dict(k=65, scales=(2,), S=1), "k = 65 outside 2..64"),
            (dict(S=0, scales=()), "S = 0 scales outside 1..16"), (dict(k=64, S=17, scales=tuple(range(2, 19))), "S = 17 scales"),
            (dict(scales=(2, 5)), "scales[1] = 5 outside 2..k = 4"), (dict(scales=(1, 4)), "scales[0] = 1 outside"),
            (dict(scales=(3, 2)), "ascend strictly"), (dict(scales=(3, 3)), "ascend strictly"), (dict(N=0), "N = 0"),
            (dict(D=0), "D = 0"), (dict(Q=-1), "Q = -1")] + [(dict(null=n), "null pointer") for n in
                                                             ('X', 'centre', 'idx', 'scales', 'ess', 'status')]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_raw_call_refuses_before_any_device_call(case):
    kwargs, message = REFUSALS[case]
    rc, text = _raw(**kwargs)
    assert rc == 1001 and text.startswith("simplex_skewness: ") and message in text, (rc, text)


def test_ok_query():
    ok = _lib.lib().idiff_simplex_skewness_ok
    assert ok(10, 3, 2, 1) == 1 and ok(10, 3, 64, 16) == 1
    assert ok(10, 3, 1, 1) == 0 and ok(10, 3, 65, 1) == 0 and ok(10, 3, 4, 0) == 0 and ok(10, 3, 4, 17) == 0
    assert ok(0, 3, 4, 1) == 0 and ok(10, 0, 4, 1) == 0 and ok(1 << 30, 1 << 11, 4, 1) == 0
    rc, _ = _raw(Q=0)                                       # Q = 0 is a no-op
    assert rc == 0
