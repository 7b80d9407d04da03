"""GPU: the simplex skewness (csrc/simplex.hip through _lib.simplex_skewness and id_diff_amd/simplex.py) against the long-double
oracle of tests/simplex_cases.py, fed the neighbour indices the GPU returned (``_lib.knn`` has its own tests), under the bound that
module derives from the kernel's arithmetic -- never from the kernel's output.

Seen on one MI355X: the largest |err| / bound over the nine shapes is 3.1e-2 (the three collinear rows of (4, 1, 2), where the
bound is the square-root branch) and 4.0e-3 elsewhere; 1.8e-2 on the translated cloud; on the exact line ess_a = 8.6e-9 under a
bound of 9.3e-7."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd import _lib, simplex

import simplex_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _run(case):
    """One launch of a shape and its oracle, shared by the tests that read it (never modified)."""
    N, D, k, ks = sc.cases(_lib.LOCAL_PCA_CHUNK)[case]
    X = sc.data(N, D, k)
    ess, idx = simplex.skewness(X.to(DEV), ks)
    idx = idx.cpu().numpy()
    ref, bound = sc.oracle_cached(X, idx, ks)
    return X, ess.cpu().numpy(), idx, ref, bound


@pytest.mark.parametrize("case", range(9))
def test_skewness_against_the_oracle(case):
    assert _lib.LOCAL_PCA_CHUNK == 64                  # the gather step of both kernels; tests/test_simplex_host.py assumes it
    N, D, k, ks = sc.cases(_lib.LOCAL_PCA_CHUNK)[case]
    X, ess, idx, ref, bound = _run(case)
    assert ess.shape == (N, len(ks), 3) and ess.dtype == np.float64 and idx.shape == (N, k)
    assert np.isfinite(ess).all() and np.isfinite(bound).all()
    ratio = sc.worst_ratio(ess, ref, bound)
    print(f"N={N} D={D} k={k} scales {ks}: max |err| / bound {ratio:.3e}")
    assert np.all(ess[..., :2] >= 0.0) and np.all(ess[..., :2] <= 1.0 + bound[..., :2])
    assert ratio <= 1.0, f"{int((np.abs(ess - ref) > bound).sum())} values beyond the bound, worst ratio {ratio:.3e}"


def test_a_scale_does_not_depend_on_the_launch_it_is_in():
    """k' = 20 out of a k = 64 launch with eleven scales is, bit for bit, the launch with that scale alone (whose k is 20 too)."""
    X, _, idx, _, _ = _run(5)
    Xd = X.to(DEV)
    centre = torch.arange(X.shape[0], dtype=torch.int64, device=DEV)
    idx_d = torch.from_numpy(idx).to(DEV)
    among = _lib.simplex_skewness(Xd, centre, idx_d, (2, 17, 20, 33, 64)).cpu().numpy()[:, 2]
    alone, idx20 = simplex.skewness(Xd, (20,))
    assert np.array_equal(idx20.cpu().numpy(), idx[:, :20])
    assert np.array_equal(alone.cpu().numpy()[:, 0], among)
    wide = _lib.simplex_skewness(Xd, centre, idx_d, (20,)).cpu().numpy()[:, 0]       # k = 64, one scale
    assert np.array_equal(wide, among)


@pytest.mark.parametrize("Q", [1, 7])
def test_rows_restrict_the_queries_bit_for_bit(Q):
    X, ess, idx, _, _ = _run(4)
    N, _, _, ks = sc.cases(_lib.LOCAL_PCA_CHUNK)[4]
    rows = list(range(N // 2, N // 2 + Q))
    e, i = simplex.skewness(X.to(DEV), ks, rows=rows)
    assert e.shape == (Q, len(ks), 3) and i.shape == (Q, 20)
    assert np.array_equal(i.cpu().numpy(), idx[rows])
    assert np.array_equal(e.cpu().numpy(), ess[rows])
    with pytest.raises(IndexError):
        simplex.skewness(X.to(DEV), ks, rows=[N])


def test_translation_does_not_reach_the_skewness():
    """Rows far from the origin against their own spread: a Gram matrix of uncentred rows is off by (1000 / 0.01)^2 2^-53."""
    g = torch.Generator().manual_seed(11)
    X = (1000.0 + 0.01 * torch.randn(200, 8, generator=g, dtype=torch.float64)).float()
    ess, idx = simplex.skewness(X.to(DEV), (2, 6, 12))
    ref, bound = sc.oracle_cached(X, idx.cpu().numpy(), (2, 6, 12))
    ratio = sc.worst_ratio(ess.cpu().numpy(), ref, bound)
    print(f"translation: max |err| / bound {ratio:.3e}, bound on ess_a up to {bound[..., 0].max():.1e}")
    assert np.isfinite(bound).all() and ratio <= 1.0


def test_points_on_a_line():
    """Points on a line in R^5, exactly so in fp32 (small integers): no area, every cosine 1, dimension 1."""
    X = sc.line_points()
    centre = torch.zeros(1, dtype=torch.int64, device=DEV)
    idx = torch.arange(1, 10, dtype=torch.int64, device=DEV)[None, :]
    ess = _lib.simplex_skewness(torch.from_numpy(X).to(DEV), centre, idx, (4, 9)).cpu().numpy()
    ref, bound = sc.oracle(X, idx.cpu().numpy(), (4, 9))
    print(f"line: ess_a {ess[0, :, 0]} under the bound {bound[0, :, 0]}; |ess_b - 1| {np.abs(ess[0, :, 1] - 1.0)}")
    assert np.all(ess[..., 0] >= 0.0) and np.all(ess[..., 0] <= bound[..., 0])
    assert np.all(np.abs(ess[..., 1] - 1.0) <= bound[..., 1])
    assert np.all(np.abs(ess[..., 2] - ref[..., 2]) <= bound[..., 2])
    assert np.all(np.abs(simplex.dims_from_skewness(ess[..., 0], 'a') - 1.0) <= 1e-6)


def test_identical_points_are_status_4_not_an_error():
    same = torch.tensor([[1.5, -2.0, 0.25]]).repeat(6, 1)
    X = torch.cat([same, torch.tensor([[3.0, 1.0, 0.0], [0.0, 0.0, 1.0]])]).contiguous().to(DEV)
    centre = torch.tensor([0, 6], dtype=torch.int64, device=DEV)
    idx = torch.tensor([[1, 2, 3, 4, 5, 6, 7], [7, 0, 1, 2, 3, 4, 5]], dtype=torch.int64, device=DEV)
    ess = _lib.simplex_skewness(X, centre, idx, (3, 5, 7)).cpu().numpy()              # does not raise
    assert np.isnan(ess[0, :2, :2]).all() and np.all(ess[0, :2, 2] == 0.0)
    want = simplex.skewness_host(X.cpu(), idx.cpu(), (3, 5, 7), centre=centre.cpu())
    assert np.array_equal(np.isnan(ess), np.isnan(want))
    np.testing.assert_allclose(ess[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-13)
    status = torch.empty(2, dtype=torch.int32, device=DEV)
    out = torch.empty(2, 3, 3, dtype=torch.float64, device=DEV)
    scales = (ctypes.c_int * 3)(3, 5, 7)
    rc = _lib.lib().idiff_simplex_skewness_f64(X.data_ptr(), 8, 3, centre.data_ptr(), idx.data_ptr(), 2, 7,
                                               ctypes.cast(scales, ctypes.c_void_p), 3, out.data_ptr(), status.data_ptr(), 0)
    torch.cuda.synchronize()
    assert rc == 0 and status.cpu().tolist() == [4, 0]
    dims = simplex.dims_from_skewness(ess[..., 0])
    assert np.isnan(dims[0, :2]).all() and np.isfinite(dims[0, 2]) and np.isfinite(dims[1]).all()


def test_out_of_range_index_is_refused_on_the_device():
    X = sc.data(50, 6, 4).to(DEV)
    centre = torch.arange(3, dtype=torch.int64, device=DEV)
    idx = torch.tensor([[1, 2, 3, 4], [0, 2, 50, 4], [0, 1, -1, 4]], dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match=r"2 of 3 queries hold an index outside \[0, 50\)"):
        _lib.simplex_skewness(X, centre, idx, (2, 4))
    with pytest.raises(RuntimeError, match=r"1 of 1 queries hold an index outside \[0, 50\)"):
        _lib.simplex_skewness(X, torch.tensor([50], dtype=torch.int64, device=DEV), idx[:1], (2, 4))


def test_non_finite_rows_are_reported_not_served():
    X = sc.data(60, 6, 4)
    X[7, 2], X[31, 0] = float('nan'), float('inf')
    centre = torch.tensor([0, 7, 31, 40], dtype=torch.int64, device=DEV)
    idx = torch.tensor([[1, 2, 3, 4], [8, 9, 10, 11], [30, 32, 33, 34], [41, 42, 43, 7]], dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match=r"3 have a neighbourhood that is not finite"):
        _lib.simplex_skewness(X.to(DEV), centre, idx, (2, 4))
    ess = _lib.simplex_skewness(X.to(DEV), centre[:1], idx[:1], (2, 4)).cpu().numpy()      # a clean query of the same data
    ref, bound = sc.oracle(X, idx[:1].cpu().numpy(), (2, 4), centre=centre[:1].cpu().numpy())
    assert sc.worst_ratio(ess, ref, bound) <= 1.0


REFUSALS = [(dict(k=1, scales=(1,)), "k = 1 outside 2..64"), (dict(k=65, scales=(2,)), "k = 65 outside 2..64"),
            (dict(scales=()), "S = 0 scales outside 1..16"), (dict(k=64, scales=tuple(range(2, 19))), "S = 17 scales outside 1..16"),
            (dict(scales=(2, 5)), "scales[1] = 5 outside 2..k = 4"), (dict(scales=(3, 2)), "ascend strictly")] + \
           [(dict(null=n), "null pointer") for n in ('X', 'centre', 'idx', 'scales', 'ess', 'status')]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_raw_call_refusals(case):
    """Each with real device buffers of the sizes named, so that a call that were NOT refused would stay inside them."""
    kwargs, message = REFUSALS[case]
    k, scales, null = kwargs.get('k', 4), kwargs.get('scales', (2, 4)), kwargs.get('null')
    N, D, Q = 80, 3, 2
    X = torch.zeros(N, D, device=DEV)
    centre = torch.zeros(Q, dtype=torch.int64, device=DEV)
    idx = torch.ones(Q, max(k, 1), dtype=torch.int64, device=DEV)
    out = torch.full((Q, max(len(scales), 1), 3), 7.0, dtype=torch.float64, device=DEV)
    status = torch.full((Q,), -1, dtype=torch.int32, device=DEV)
    buf = (ctypes.c_int * max(len(scales), 1))(*scales)
    ptr = dict(X=X.data_ptr(), centre=centre.data_ptr(), idx=idx.data_ptr(), scales=ctypes.cast(buf, ctypes.c_void_p).value,
               ess=out.data_ptr(), status=status.data_ptr())
    if null:
        ptr[null] = 0
    rc = _lib.lib().idiff_simplex_skewness_f64(ptr['X'], N, D, ptr['centre'], ptr['idx'], Q, k, ptr['scales'], len(scales),
                                               ptr['ess'], ptr['status'], 0)
    text = _lib.lib().idiff_last_error().decode()
    torch.cuda.synchronize()
    assert rc == 1001 and text.startswith("simplex_skewness: ") and message in text, (rc, text)
    assert bool((out == 7.0).all()) and bool((status == -1).all())                    # nothing was launched
    if not null:
        with pytest.raises(RuntimeError, match="simplex_skewness"):
            _lib.simplex_skewness(X, centre, idx, scales)


# ------------------------------------------------------------------------------------------- acceptance on two spheres
@functools.lru_cache(maxsize=None)
def _spheres():
    X = sc.two_spheres()
    ess, idx = simplex.skewness(torch.from_numpy(X).to(DEV), simplex.SCALES)
    idx = idx.cpu().numpy()
    return X, ess.cpu().numpy(), idx, simplex.skewness_host(X, idx, simplex.SCALES)


def test_scale_curve_on_two_spheres():
    X, ess, idx, host = _spheres()
    curve = simplex.scale_curve(torch.from_numpy(X).to(DEV))
    assert curve.shape == (2048, 7) and curve.dtype == np.float64 and np.isfinite(curve).all()
    assert np.array_equal(curve, simplex.dims_from_skewness(ess[..., 0], 'a'))
    # the rounded readings are the host's, except where the host's value lies within the bound of a half-integer
    _, bound = sc.oracle_cached(X, idx, simplex.SCALES)
    want = simplex.dims_from_skewness(host[..., 0], 'a')
    n = np.floor(want).astype(np.int64)
    slope = simplex.reference(n + 1, 'a') - simplex.reference(n, 'a')
    near = np.abs(want - np.floor(want) - 0.5) <= bound[..., 0] / slope
    print(f"{int(near.sum())} of {near.size} host readings within the bound of a half-integer")
    assert near.sum() <= 4
    assert np.array_equal(np.rint(curve)[~near], np.rint(want)[~near])
    two = {k: int((np.rint(curve[:1024, s]) == 2).sum()) for s, k in enumerate(simplex.SCALES)}
    four = {k: int((np.rint(curve[1024:, s]) == 4).sum()) for s, k in enumerate(simplex.SCALES)}
    print(f"2-sphere reads 2: {two}; 4-sphere reads 4: {four}")
    print("mean reading: " + ", ".join(f"k={k}: {curve[:1024, s].mean():.2f} / {curve[1024:, s].mean():.2f}"
                                       for s, k in enumerate(simplex.SCALES)))
    assert all(two[k] >= 1016 for k in (12, 16, 24, 32, 48, 64))
    assert four[48] >= 1016 and four[64] >= 1016 and four[32] >= 940 and four[16] >= 780
    stable = simplex.stable_dims(curve, simplex.SCALES)
    s2, s4 = int((stable[:1024] == 2).sum()), int((stable[1024:] == 4).sum())
    print(f"stable_dims: {s2} of 1024 read 2, {s4} of 1024 read 4")
    assert s2 >= 1000 and s4 >= 1000


def test_local_dims_and_variant_b():
    X, ess, _, _ = _spheres()
    Xd = torch.from_numpy(X).to(DEV)
    dims = simplex.local_dims(Xd, 32)
    assert dims.shape == (2048,) and dims.dtype == np.float64
    assert np.array_equal(dims, simplex.dims_from_skewness(ess[:, 4, 0], 'a'))        # k = 32 of the sweep, bit for bit
    b = simplex.local_dims(Xd, 64, ver='b')
    assert np.array_equal(b, simplex.dims_from_skewness(ess[:, 6, 1], 'b'))
    print(f"variant b at k = 64: {(np.rint(b[:1024]) == 2).sum()} read 2, {(np.rint(b[1024:]) == 4).sum()} read 4")
    assert (np.rint(b[1024:]) == 4).sum() >= 1016 and (np.rint(b[:1024]) == 2).sum() >= 1016
    with pytest.raises(ValueError):
        simplex.local_dims(Xd, 20, ver='c')


def test_run_writes_the_pickle(tmp_path, capsys):
    import pickle
    from id_diff_amd import benchmark
    from id_diff_amd.configs.utils import read_config
    cfg = read_config('configs/dimension_estimation/paper/euclidean_data/ksphere/union.py')
    cfg.data.ambient_dim, cfg.data.dim, cfg.data.shape = 16, 16, [16]
    cfg.data.manifold_dim, cfg.data.data_samples = [2, 4], 1024
    cfg.model.state_size = 16
    torch.manual_seed(5)
    dims = simplex.run(cfg, k=16, out_dir=str(tmp_path / 'one'))
    with open(tmp_path / 'one' / 'local_dims.pkl', 'rb') as f:
        saved = pickle.load(f)
    assert sorted(saved) == ['dims', 'k', 'skewness', 'ver'] and saved['k'] == 16 and saved['ver'] == 'a'
    assert saved['dims'].shape == (1638,) and saved['skewness'].shape == (1638, 1, 3) and np.array_equal(saved['dims'], dims)
    torch.manual_seed(5)                                # the train split, exactly as Benchmark.create_dataset takes it
    bm = benchmark.Benchmark(str(tmp_path / 'b.csv'), {'u': cfg})
    data = bm.create_dataset('u', cfg)
    assert np.array_equal(simplex.local_dims(data, 16), dims)
    bm.evaluate_estimator(data, 'ess_knn_16', 'u')
    assert bm.results.loc['ess_knn_16', 'u'] == dims.mean()
    out = capsys.readouterr().out
    assert 'dim   2:' in out and 'dim   4:' in out
    torch.manual_seed(5)
    sweep = simplex.run(cfg, ver='a', sweep=True, ks=(8, 16), out_dir=str(tmp_path / 'sweep'))
    with open(tmp_path / 'sweep' / 'local_dims.pkl', 'rb') as f:
        saved = pickle.load(f)
    assert sorted(saved) == ['dims', 'ks', 'skewness', 'ver'] and saved['ks'] == [8, 16]
    assert sweep.shape == (1638, 2) and np.array_equal(sweep[:, 1], dims)
    assert 'stable over k' in capsys.readouterr().out
