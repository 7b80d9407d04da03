"""Host side of local PCA (id_diff_amd/lpca.py): the dimension rules, the fp64 numpy restatement of csrc/lpca.hip against the
direct covariance route, the acceptance of the arithmetic on a union of a 2-sphere and a 4-sphere, the ``lpca_knn_<k>`` name of
``benchmark.Benchmark`` and what idiff_local_pca_f64 refuses before any device call.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import id_diff_amd
from id_diff_amd import _lib, benchmark, lpca
from id_diff_amd.configs.config_dict import ConfigDict
from id_diff_amd.lightning_data_modules import KSphereDataset as ksd


# ------------------------------------------------------------------------------------------- dims_from_spectra
def test_fo_threshold_on_either_side():
    eig = np.array([[1.0, 0.5, 0.0501, 0.0499, 0.0],
                    [2.0, 0.2, 0.1, 0.0999, 0.0],          # alpha lambda_1 = 0.1 itself does not count (strictly greater)
                    [4.0, 0.0, 0.0, 0.0, 0.0]])
    assert lpca.dims_from_spectra(eig).tolist() == [3, 2, 1]
    assert lpca.dims_from_spectra(eig, 'FO', alpha=0.5).tolist() == [1, 1, 1]
    assert lpca.dims_from_spectra(eig[:1], 'FO', alpha=0.0498).tolist() == [4]
    assert lpca.dims_from_spectra(eig).dtype == np.int64
    assert lpca.dims_from_spectra(torch.from_numpy(eig)).tolist() == [3, 2, 1]


def test_ratio_rule_at_the_exact_boundary():
    eig = np.array([[3.0, 1.0, 0.0, 0.0],                  # 3 / 4 = 0.75 exactly
                    [2.0, 1.0, 1.0, 0.0],
                    [1.0, 1.0, 1.0, 1.0]])
    assert lpca.dims_from_spectra(eig, 'ratio', alpha=0.75).tolist() == [1, 2, 3]
    assert lpca.dims_from_spectra(eig, 'ratio', alpha=0.75 + 2.0 ** -40).tolist() == [2, 3, 4]
    assert lpca.dims_from_spectra(eig, 'ratio', alpha=1.0).tolist() == [2, 3, 4]
    assert lpca.dims_from_spectra(np.array([[90.0, 5.0, 4.0, 1.0]]), 'ratio').tolist() == [2]      # default 0.95: 95 of 100


def test_zero_spectrum_gives_zero_and_bad_arguments_raise():
    z = np.zeros((2, 5))
    assert lpca.dims_from_spectra(z).tolist() == [0, 0]
    assert lpca.dims_from_spectra(z, 'ratio').tolist() == [0, 0]
    with pytest.raises(ValueError, match="unknown rule"):
        lpca.dims_from_spectra(z, 'maxgap')
    with pytest.raises(ValueError):
        lpca.dims_from_spectra(np.zeros(5))


# ------------------------------------------------------------------------------------------- the numpy restatement
def _brute_knn(X, k):
    X = np.asarray(X, dtype=np.float64)
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    return np.argsort(d2, axis=1, kind='stable')[:, :k]


@pytest.mark.parametrize("N,D,k", [(60, 3, 12), (40, 200, 9)], ids=["D<<m", "D>>m"])
def test_host_restatement_against_the_covariance(N, D, k):
    rng = np.random.default_rng(N + D)
    X = rng.standard_normal((N, D)) * np.linspace(1.0, 0.2, D) + 5.0
    idx = _brute_knn(X, k)
    r, nv = min(k, D), min(3, k, D)
    eig, basis = lpca.local_spectra_host(X, idx, n_vectors=nv)
    assert eig.shape == (N, r) and basis.shape == (N, nv, D)
    for q in range(N):
        nb = X[np.concatenate([[q], idx[q]])]
        lam, V = np.linalg.eigh(np.atleast_2d(np.cov(nb.T)))
        lam, V = lam[::-1], V[:, ::-1]
        np.testing.assert_allclose(eig[q], lam[:r], rtol=1e-10, atol=0)
        B = basis[q]
        np.testing.assert_allclose(B @ B.T, np.eye(nv), atol=1e-12)
        assert all(b[np.argmax(np.abs(b))] > 0 for b in B)
        for d in range(1, min(nv, D - 1) + 1):          # d = D is the whole space
            gap = lam[d - 1] - lam[d]
            assert lpca.subspace_sine(B[:d].T, V[:, :d]) <= 1e-12 * lam[0] / gap


def test_host_restatement_rows_centres_and_degenerate_neighbourhoods():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((30, 6))
    idx = _brute_knn(X, 7)
    full, _ = lpca.local_spectra_host(X, idx)
    some, _ = lpca.local_spectra_host(X, idx[[4, 17]], centre=[4, 17])
    assert np.array_equal(some, full[[4, 17]])
    same = np.tile(X[:1], (9, 1))
    eig, basis = lpca.local_spectra_host(same, np.arange(1, 9)[None, :], n_vectors=2)
    assert not eig.any() and np.isnan(basis).all()
    assert lpca.subspace_sine(np.eye(4)[:, :2], np.eye(4)[:, :2]) == 0.0
    assert lpca.subspace_sine(np.eye(4)[:, :2], np.eye(4)[:, 1:3]) == pytest.approx(1.0)


def _union_2_4():
    """The union of a 2-sphere and a 4-sphere in R^16: rows 0 .. 1023 on the 2-sphere, 1024 .. 2047 on the 4-sphere."""
    cfg = ConfigDict()
    cfg.data = ConfigDict(n_spheres=2, manifold_dim=[2, 4], ambient_dim=16, data_samples=1024, noise_std=0.0,
                          embedding_type='random_isometry')
    torch.manual_seed(0)
    return ksd.KSphereDataset(cfg).data


def test_local_pca_separates_a_2_sphere_from_a_4_sphere():
    """The arithmetic itself, on the CPU: fp64 brute-force neighbours, k = 16, Fukunaga-Olsen on ``local_spectra_host``.
    Seen with this generator and seed: 1024 / 1024 rows of the 2-sphere report 2 and 1023 / 1024 rows of the 4-sphere report 4;
    on the 2-sphere lambda_3 / lambda_1 <= 0.0102 and lambda_2 / lambda_1 >= 0.1345."""
    X = _union_2_4().numpy()
    assert X.shape == (2048, 16)
    eig, _ = lpca.local_spectra_host(X, _brute_knn(X, 16))
    dims = lpca.dims_from_spectra(eig, 'FO')
    two, four = int((dims[:1024] == 2).sum()), int((dims[1024:] == 4).sum())
    print(f"2-sphere rows reporting 2: {two} / 1024; 4-sphere rows reporting 4: {four} / 1024; "
          f"max l3/l1 {np.max(eig[:1024, 2] / eig[:1024, 0]):.4f}, min l2/l1 {np.min(eig[:1024, 1] / eig[:1024, 0]):.4f}")
    assert two >= 0.99 * 1024
    assert four >= 0.95 * 1024


# ------------------------------------------------------------------------------------------- Benchmark's estimator names
def test_benchmark_understands_lpca_knn_names(tmp_path, monkeypatch):
    assert benchmark.lpca_knn_k('lpca_knn_12') == 12
    assert [benchmark.lpca_knn_k(n) for n in ('lpca', 'lpca_knn_', 'lpca_knn_x', 'lpca_knn_-3', 'mle_5', 'xlpca_knn_4')] == [None] * 6
    seen = {}

    def fake_local_dims(X, k=20, rule='FO', alpha=None):
        seen['k'], seen['X'] = k, X
        return np.array([2, 2, 3, 5], dtype=np.int64)

    monkeypatch.setattr(lpca, 'local_dims', fake_local_dims)
    bm = benchmark.Benchmark(str(tmp_path / 'out.csv'), {'u': None})
    assert bm.estimators == ['mle_5', 'mle_20', 'lpca', 'ppca']              # the default list is unchanged
    assert list(bm.results.index) == bm.estimators
    data = object()
    bm.evaluate_estimator(data, 'lpca_knn_12', 'u')
    assert seen['k'] == 12 and seen['X'] is data
    assert bm.results.loc['lpca_knn_12', 'u'] == 3.0
    import pandas as pd
    saved = pd.read_csv(bm.file_name, index_col='method')
    assert list(saved.index) == ['mle_5', 'mle_20', 'lpca', 'ppca', 'lpca_knn_12'] and saved.loc['lpca_knn_12', 'u'] == 3.0
    seen.clear()
    bm.evaluate_estimator(data, 'lpca_knn_12', 'u')                           # filled: not evaluated again
    assert not seen


def test_benchmark_unknown_name_still_raises(tmp_path):
    bm = benchmark.Benchmark(str(tmp_path / 'out.csv'), {'u': None})
    with pytest.raises(KeyError):                                             # a name outside the frame, as before
        bm.evaluate_estimator(None, 'lpca_knn', 'u')
    bm.results.loc['lpca_knn'] = np.nan
    with pytest.raises(ValueError, match="unknown estimator"):
        bm.evaluate_estimator(None, 'lpca_knn', 'u')


def _stub_estimators(monkeypatch, calls):
    """The real ``Benchmark`` with the GPU taken out: stub estimators, and a data module whose train loader yields two batches."""
    def fake_local_dims(X, k=20, rule='FO', alpha=None):
        calls.append(('lpca_knn', k, tuple(X.shape)))
        return np.array([2, 3], dtype=np.int64)

    class FakeModule:
        def __init__(self, config):
            calls.append(('dataset', config))

        def setup(self):
            pass

        def train_dataloader(self):
            return [torch.zeros(3, 2, 2), torch.zeros(1, 2, 2)]

    monkeypatch.setattr(lpca, 'local_dims', fake_local_dims)
    for name, value in (('mle_global_dim', 1.5), ('pca_fo_dim', 4), ('ppca_dim', 5)):
        monkeypatch.setattr(benchmark, name, lambda data, *a, _v=value, **kw: _v)
    monkeypatch.setattr(benchmark, 'create_lightning_datamodule', FakeModule)
    monkeypatch.setattr(benchmark, '_points', lambda t: t)


def test_benchmark_opt_in_row_survives_a_reload(tmp_path, monkeypatch):
    """A saved ``lpca_knn_<k>`` value is loaded again, is not computed again, and is not overwritten when a data set is added."""
    import pandas as pd
    calls, path = [], str(tmp_path / 'out.csv')
    _stub_estimators(monkeypatch, calls)
    bm = benchmark.Benchmark(path, {'a': 'A'})
    bm.estimators.append('lpca_knn_16')
    bm.run()
    assert pd.read_csv(path, index_col='method').loc['lpca_knn_16', 'a'] == 2.5
    assert calls == [('dataset', 'A'), ('lpca_knn', 16, (4, 4))]
    calls.clear()
    bm = benchmark.Benchmark(path, {'a': 'A', 'b': 'B'})
    assert bm.results.loc['lpca_knn_16', 'a'] == 2.5                       # kept by the load, before any name is appended
    bm.estimators.append('lpca_knn_16')
    bm.run()
    saved = pd.read_csv(path, index_col='method')
    assert saved.loc['lpca_knn_16', 'a'] == 2.5 and saved.loc['lpca_knn_16', 'b'] == 2.5
    assert calls == [('dataset', 'B'), ('lpca_knn', 16, (4, 4))]      # 'a' was complete: neither built nor evaluated
    # a later run that does not list the name still writes the row back
    bm = benchmark.Benchmark(path, {'a': 'A', 'b': 'B', 'c': 'C'})
    bm.run()
    saved = pd.read_csv(path, index_col='method')
    assert saved.loc['lpca_knn_16', ['a', 'b']].tolist() == [2.5, 2.5] and pd.isna(saved.loc['lpca_knn_16', 'c'])


def test_benchmark_name_appended_to_a_complete_csv_is_computed(tmp_path, monkeypatch):
    import pandas as pd
    calls, path = [], str(tmp_path / 'out.csv')
    _stub_estimators(monkeypatch, calls)
    benchmark.Benchmark(path, {'a': 'A'}).run()                            # the four defaults, complete
    assert list(pd.read_csv(path, index_col='method').index) == ['mle_5', 'mle_20', 'lpca', 'ppca']
    calls.clear()
    bm = benchmark.Benchmark(path, {'a': 'A'})
    bm.estimators.append('lpca_knn_12')
    bm.run()
    assert calls == [('dataset', 'A'), ('lpca_knn', 12, (4, 4))]
    saved = pd.read_csv(path, index_col='method')
    assert saved.loc['lpca_knn_12', 'a'] == 2.5 and saved.loc['ppca', 'a'] == 5


# ------------------------------------------------------------------------------------------- C ABI: refusals
_X, _CEN, _IDX, _EIG, _BAS, _ST = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000      # fabricated addresses


def _refusal_cases():
    cases = []

    def call(tag, X=_X, N=100, D=8, centre=_CEN, idx=_IDX, Q=4, k=5, n_vec=0, eig=_EIG, basis=0, status=_ST):
        cases.append((tag, [X, N, D, centre, idx, Q, k, n_vec, eig, basis, status]))
    call("k_1", k=1); call("k_65", k=65)
    call("n_vec_above_k", k=5, n_vec=6, basis=_BAS); call("n_vec_above_D", D=3, k=5, n_vec=4, basis=_BAS)
    call("n_vec_negative", n_vec=-1)
    call("D_0", D=0); call("N_0", N=0); call("Q_negative", Q=-1)
    call("null_X", X=0); call("null_centre", centre=0); call("null_idx", idx=0); call("null_eig", eig=0)
    call("null_status", status=0); call("null_basis", n_vec=2, basis=0)
    call("no_queries", Q=0)
    return cases


_REFUSALS = {
    'k_1': (1001, 'local_pca: k = 1 outside 2..64'),
    'k_65': (1001, 'local_pca: k = 65 outside 2..64'),
    'n_vec_above_k': (1001, 'local_pca: n_vec = 6 outside 0..min(k, D) = 5'),
    'n_vec_above_D': (1001, 'local_pca: n_vec = 4 outside 0..min(k, D) = 3'),
    'n_vec_negative': (1001, 'local_pca: n_vec = -1 outside 0..min(k, D) = 5'),
    'D_0': (1001, 'local_pca: D = 0, need at least 1 dimension'),
    'N_0': (1001, 'local_pca: N = 0, need at least 1 row'),
    'Q_negative': (1001, 'local_pca: Q = -1, need at least 0 queries'),
    'null_X': (1001, 'local_pca: null pointer'),
    'null_centre': (1001, 'local_pca: null pointer'),
    'null_idx': (1001, 'local_pca: null pointer'),
    'null_eig': (1001, 'local_pca: null pointer'),
    'null_status': (1001, 'local_pca: null pointer'),
    'null_basis': (1001, 'local_pca: null pointer'),
    'no_queries': (0, ''),
}


@pytest.mark.parametrize("case", _refusal_cases(), ids=lambda c: c[0])
def test_local_pca_refuses_before_any_device_call(case):
    """No GPU needed: host code turns every call away in front of the first HIP call (the addresses are fabricated: a launcher that
    let one through would fault, not pass)."""
    ident, args = case
    handle = _lib.lib()
    rc = handle.idiff_local_pca_f64(*args, None)
    text = handle.idiff_last_error().decode() if rc else ""
    assert (rc, text) == _REFUSALS[ident]


def test_local_pca_refusal_table_is_complete_and_queries_agree():
    assert sorted(_REFUSALS) == sorted(c[0] for c in _refusal_cases())
    ok = _lib.lib().idiff_local_pca_ok
    assert ok(100, 8, 5, 0) == 1 and ok(100, 8, 64, 8) == 1 and ok(1, 1, 2, 1) == 1
    assert ok(100, 8, 1, 0) == 0 and ok(100, 8, 65, 0) == 0 and ok(100, 8, 5, 6) == 0 and ok(100, 0, 5, 0) == 0
    assert ok(100, 3, 5, 4) == 0 and ok(0, 8, 5, 0) == 0
    chunk = _lib.lib().idiff_local_pca_chunk()
    assert chunk == _lib.LOCAL_PCA_CHUNK and chunk >= 16 and chunk % 16 == 0
