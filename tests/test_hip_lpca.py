"""GPU: local PCA (csrc/lpca.hip through _lib.local_pca and id_diff_amd/lpca.py) against ``lpca.local_spectra_host``, the fp64
numpy restatement of the kernel's arithmetic, fed the neighbour indices the GPU returned (``_lib.knn`` has its own tests).

Bound per query, from the arithmetic and not from the kernel's output:
    |lambda - lambda_ref| <= 8 (D + 4 m) 2^-53 trace(B_ref),    m = k + 1.
"""
import functools

import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd import _lib, benchmark, lpca
from id_diff_amd.configs.utils import read_config
from id_diff_amd.lightning_data_modules import KSphereDataset as ksd

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _data(N, D, k):
    g = torch.Generator().manual_seed(N + D + k)
    X = torch.randn(N, D, generator=g)
    X[:, 20:] *= 0.05                  # a low-dimensional structure, as the ID data have (test_hip_knn.py)
    return X


def _tol(eig_ref, D, k):
    """The bound on an eigenvalue, per query [Q]: trace(B_ref) is the sum of the min(k, D) eigenvalues (the others are zero)."""
    return 8.0 * (D + 4 * (k + 1)) * 2.0 ** -53 * eig_ref.sum(axis=1)


@functools.lru_cache(maxsize=None)
def _run(N, D, k, n_vec=0):
    """One launch and its reference, shared by the tests that read it (never modified)."""
    X = _data(N, D, k)
    eig, basis, idx = lpca.local_spectra(X.to(DEV), k, n_vectors=n_vec)
    ref_eig, ref_basis = lpca.local_spectra_host(X, idx, n_vectors=n_vec)
    return X, eig.cpu().numpy(), None if basis is None else basis.cpu().numpy(), idx.cpu().numpy(), ref_eig, ref_basis


def _shapes():
    c = _lib.LOCAL_PCA_CHUNK
    return [(4, 1, 2), (40, 3, 15), (40, 3, 16), (100, 17, 16), (300, 100, 20), (200, 100, 64), (150, c + 1, 31),
            (150, 2 * c - 3, 31), (120, 3072, 20)]


@pytest.mark.parametrize("case", range(9))
def test_spectra_against_fp64(case):
    N, D, k = _shapes()[case]
    X, eig, _, idx, ref, _ = _run(N, D, k)
    assert eig.shape == (N, min(k, D)) and eig.dtype == np.float64 and idx.shape == (N, k)
    tol = _tol(ref, D, k)
    err = np.abs(eig - ref).max(axis=1)
    print(f"N={N} D={D} k={k}: max |err| / bound {np.max(err / tol):.3e}")
    assert np.all(eig >= 0.0) and np.all(np.diff(eig, axis=1) <= 0.0)
    assert np.all(err <= tol), f"{int((err > tol).sum())} queries beyond the bound, worst ratio {np.max(err / tol):.3e}"


def test_translation_does_not_reach_the_spectrum():
    """Rows far from the origin against their own spread: a Gram matrix of uncentred rows is off by (1000 / 0.01)^2 2^-53."""
    N, D, k = 200, 8, 12
    g = torch.Generator().manual_seed(11)
    X = (1000.0 + 0.01 * torch.randn(N, D, generator=g, dtype=torch.float64)).float()
    eig, _, idx = lpca.local_spectra(X.to(DEV), k)
    ref, _ = lpca.local_spectra_host(X, idx)
    tol = _tol(ref, D, k)
    err = np.abs(eig.cpu().numpy() - ref).max(axis=1)
    print(f"translation: max |err| / bound {np.max(err / tol):.3e}, trace(B) about {ref.sum(axis=1).mean():.3e}")
    assert np.all(ref.sum(axis=1) > 0.0) and np.all(err <= tol)


@pytest.mark.parametrize("Q", [1, 7])
def test_rows_restrict_the_queries_bit_for_bit(Q):
    N, D, k = 300, 100, 20
    X, eig, basis, idx, _, _ = _run(N, D, k, 10)
    rows = list(range(N // 2, N // 2 + Q))
    e, b, i = lpca.local_spectra(X.to(DEV), k, n_vectors=10, rows=rows)
    assert e.shape == (Q, k) and b.shape == (Q, 10, D) and i.shape == (Q, k)
    assert np.array_equal(i.cpu().numpy(), idx[rows])
    assert np.array_equal(e.cpu().numpy(), eig[rows])
    assert np.array_equal(b.cpu().numpy(), basis[rows])


def test_identical_points_give_zeros_and_nan_vectors():
    X = torch.randn(1, 7, generator=torch.Generator().manual_seed(3)).repeat(12, 1).contiguous().to(DEV)
    centre = torch.tensor([0, 5], dtype=torch.int64, device=DEV)
    idx = torch.tensor([[1, 2, 3, 4, 6, 7], [0, 1, 2, 3, 4, 11]], dtype=torch.int64, device=DEV)
    eig, basis = _lib.local_pca(X, centre, idx, n_vectors=3)              # raises unless every status is 0
    assert eig.shape == (2, 6) and not eig.cpu().numpy().any()
    assert basis.shape == (2, 3, 7) and bool(torch.isnan(basis).all())


def test_points_on_a_line():
    """Points on a line in R^5, exactly so in fp32 (small integers): lambda_2 .. lambda_r are zero to the absolute bound and their
    vectors NaN, vector 1 is the line."""
    D, k = 5, 9
    direction = np.array([1.0, -2.0, 0.0, 3.0, 1.0])
    t = np.array([0.0, 1.0, -1.0, 2.0, 4.0, -3.0, 5.0, 7.0, -6.0, 8.0])
    X = torch.from_numpy(t[:, None] * direction[None, :] + np.array([1.0, 2.0, 3.0, 4.0, 5.0])).float()
    centre = torch.zeros(1, dtype=torch.int64, device=DEV)
    idx = torch.arange(1, k + 1, dtype=torch.int64, device=DEV)[None, :]
    eig, basis = _lib.local_pca(X.to(DEV), centre, idx, n_vectors=3)
    eig, basis = eig.cpu().numpy()[0], basis.cpu().numpy()[0]
    ref, _ = lpca.local_spectra_host(X, idx, centre=centre)
    tol = _tol(ref, D, k)[0]
    assert abs(eig[0] - np.var(t, ddof=1) * direction @ direction) <= tol
    assert np.all(eig[1:] <= tol)
    assert np.isnan(basis[1:]).all()
    np.testing.assert_allclose(basis[0], direction / np.linalg.norm(direction) * np.sign(direction[3]), atol=1e-14)


def test_out_of_range_index_is_refused_on_the_device():
    X = _data(50, 6, 4).to(DEV)
    centre = torch.arange(3, dtype=torch.int64, device=DEV)
    idx = torch.tensor([[1, 2, 3, 4], [0, 2, 50, 4], [0, 1, -1, 4]], dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match=r"2 hold an index outside \[0, 50\)"):
        _lib.local_pca(X, centre, idx, n_vectors=1)


def test_non_finite_rows_are_reported_not_solved():
    """A NaN or an Inf in a neighbourhood is status 3: ``_lib.local_pca`` raises and names the count; the other queries are unharmed."""
    X = _data(60, 6, 4)
    X[7, 2], X[31, 0] = float('nan'), float('inf')
    centre = torch.tensor([0, 7, 31, 40], dtype=torch.int64, device=DEV)
    idx = torch.tensor([[1, 2, 3, 4], [8, 9, 10, 11], [30, 32, 33, 34], [41, 7, 42, 43]], dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match=r"3 have a neighbourhood that is not finite"):
        _lib.local_pca(X.to(DEV), centre, idx, n_vectors=1)
    eig, _ = _lib.local_pca(X.to(DEV), centre[:1], idx[:1])
    ref, _ = lpca.local_spectra_host(X, idx[:1], centre=centre[:1])
    assert np.all(np.abs(eig.cpu().numpy() - ref) <= _tol(ref, 6, 4)[:, None])
    with pytest.raises(ValueError, match="not finite"):
        lpca.dims_from_spectra(np.array([[1.0, float('nan')]]))


@pytest.mark.parametrize("N,D,k,n_vec", [(300, 100, 20, 10), (120, 3072, 20, 5)])
def test_vectors_against_fp64(N, D, k, n_vec):
    _, eig, basis, _, ref, ref_basis = _run(N, D, k, n_vec)
    assert basis.shape == (N, n_vec, D) and np.isfinite(basis).all()
    tol = _tol(ref, D, k)
    assert np.all(np.abs(eig - ref).max(axis=1) <= tol)
    gram = basis @ basis.transpose(0, 2, 1)
    ortho = np.abs(gram - np.eye(n_vec)).max()
    lead = np.take_along_axis(basis, np.abs(basis).argmax(axis=2)[:, :, None], axis=2)
    skipped, worst = 0, 0.0
    for q in range(N):
        for d in range(1, n_vec + 1):
            gap = ref[q, d - 1] - ref[q, d]
            if gap / ref[q, 0] < 1e-3:
                skipped += 1
                continue
            sine = lpca.subspace_sine(basis[q, :d].T, ref_basis[q, :d].T)
            worst = max(worst, sine / (2.0 * tol[q] / gap))
    print(f"N={N} D={D} k={k} n_vec={n_vec}: orthonormal to {ortho:.2e}, worst sine / Davis-Kahan bound {worst:.3e}, "
          f"{skipped} of {N * n_vec} pairs skipped")
    assert ortho <= 1e-12
    assert np.all(lead > 0.0)                                       # the component of largest magnitude is positive
    assert skipped <= 0.01 * N * n_vec
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------- end to end on the [2, 4] union
def _union_config():
    cfg = read_config('configs/dimension_estimation/paper/euclidean_data/ksphere/union.py')
    cfg.data.ambient_dim, cfg.data.dim, cfg.data.shape = 16, 16, [16]
    cfg.data.manifold_dim, cfg.data.data_samples = [2, 4], 1024
    cfg.model.state_size = 16
    return cfg


@functools.lru_cache(maxsize=None)
def _union():
    torch.manual_seed(0)
    X = ksd.KSphereDataset(_union_config()).data
    _, _, idx = lpca.local_spectra(X.to(DEV), 16)
    ref, ref_basis = lpca.local_spectra_host(X, idx, n_vectors=2)
    return X, ref, ref_basis


def test_local_dims_on_the_union():
    X, ref, _ = _union()
    dims = lpca.local_dims(X.to(DEV), 16)
    assert dims.shape == (2048,) and dims.dtype == np.int64
    safe = (np.abs(ref - lpca.FO_ALPHA * ref[:, :1]) > 1e-9 * ref[:, :1]).all(axis=1)
    assert (~safe).sum() <= 0.01 * 2048
    want = lpca.dims_from_spectra(ref)
    assert np.array_equal(dims[safe], want[safe])
    print(f"2-sphere rows reporting 2: {(dims[:1024] == 2).sum()}, 4-sphere rows reporting 4: {(dims[1024:] == 4).sum()}")
    assert (dims[:1024] == 2).sum() >= 0.99 * 1024 and (dims[1024:] == 4).sum() >= 0.95 * 1024


def test_local_tangent_on_the_union():
    X, ref, ref_basis = _union()
    dims = lpca.dims_from_spectra(ref)
    tangent = lpca.local_tangent(X.to(DEV), 16, dims=dims)
    assert len(tangent) == 2048
    worst = 0.0
    for i in np.flatnonzero(dims[:1024] == 2):
        T = tangent[i]
        assert T.shape == (16, 2) and T.dtype == np.float32
        worst = max(worst, lpca.subspace_sine(np.linalg.qr(T.astype(np.float64))[0], ref_basis[i].T))
    print(f"worst sine between local_tangent and the host vectors on the 2-sphere: {worst:.3e}")
    assert worst <= 1e-6
    assert all(t is not None and t.shape == (16, d) for t, d in zip(tangent[1024:], dims[1024:]))
    none = lpca.local_tangent(X[:64].to(DEV), 16, dims=np.array([0] * 32 + [17] * 32))
    assert none == [None] * 64


def test_benchmark_opt_in_name(tmp_path):
    cfg = _union_config()
    bm = benchmark.Benchmark(str(tmp_path / 'a.csv'), {'u': cfg})
    bm.estimators = ['lpca_knn_16']
    torch.manual_seed(5)
    bm.run()
    import pandas as pd
    saved = pd.read_csv(bm.file_name, index_col='method', float_precision='round_trip')
    torch.manual_seed(5)
    data = benchmark.Benchmark(str(tmp_path / 'b.csv'), {'u': cfg}).create_dataset('u', cfg)
    assert data.shape == (1638, 16)
    assert saved.loc['lpca_knn_16', 'u'] == lpca.local_dims(data, 16).mean()
    assert saved.loc[['mle_5', 'mle_20', 'lpca', 'ppca'], 'u'].isna().all()


def test_run_writes_the_pickle(tmp_path, capsys):
    import pickle
    cfg = _union_config()
    torch.manual_seed(5)
    dims = lpca.run(cfg, k=16, rule='FO', out_dir=str(tmp_path / 'lpca'))
    with open(tmp_path / 'lpca' / 'local_dims.pkl', 'rb') as f:
        saved = pickle.load(f)
    assert sorted(saved) == ['dims', 'eigenvalues', 'k', 'rule'] and saved['k'] == 16 and saved['rule'] == 'FO'
    assert saved['dims'].shape == (1638,) and saved['eigenvalues'].shape == (1638, 16) and np.array_equal(saved['dims'], dims)
    assert np.array_equal(saved['dims'], lpca.dims_from_spectra(saved['eigenvalues']))
    torch.manual_seed(5)                                # the train split, exactly as Benchmark.create_dataset takes it
    data = benchmark.Benchmark(str(tmp_path / 'b.csv'), {'u': cfg}).create_dataset('u', cfg)
    assert np.array_equal(lpca.local_dims(data, 16), dims)
    out = capsys.readouterr().out
    assert 'dim   2:' in out and 'dim   4:' in out
