"""GPU: the exact self-kNN kernel (idiff_knn_f32) and the classical ID estimators built on it (mle.py, benchmark.py).

Oracle of the kNN: fp64 torch on the CPU.  Candidates from the fp64 Gram of the centred data, their distances again as
sum_d (x_id - x_jd)^2 in fp64, ordered by (distance, index); a row whose candidates are not provably enough under the
Gram's fp64 error is done by brute force over all N.
"""
import numpy as np
import pytest
import torch

import id_diff_amd
from id_diff_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _exact_row(X64, i, k):
    d2 = ((X64 - X64[i]) ** 2).sum(1)
    d2[i] = float("inf")
    order = np.lexsort((np.arange(len(d2)), d2.numpy()))[:k]
    return d2[order], torch.from_numpy(order)


def oracle_knn(X, k):
    X64 = X.double()
    N, D = X64.shape
    c = X64 - X64.mean(0)
    n = (c * c).sum(1)
    A = n[:, None] + n[None, :] - 2.0 * (c @ c.T)
    A.fill_diagonal_(float("inf"))
    m = min(N - 1, k + 32)
    Am, cand = torch.topk(A, m, dim=1, largest=False, sorted=True)
    a = n.sqrt()
    err = (D + 8) * 2.0 ** -52 * (a + a.max()) ** 2 * 4
    dist2 = torch.empty(N, k, dtype=torch.float64)
    idx = torch.empty(N, k, dtype=torch.int64)
    for r0 in range(0, N, 256):
        r1 = min(N, r0 + 256)
        d2 = ((X64[r0:r1, None, :] - X64[cand[r0:r1]]) ** 2).sum(-1)
        for r in range(r0, r1):
            order = np.lexsort((cand[r].numpy(), d2[r - r0].numpy()))[:k]
            dk, ik = d2[r - r0][order], cand[r][order]
            if m < N - 1 and not (float(Am[r, -1]) - float(err[r]) > float(dk[-1])):
                dk, ik = _exact_row(X64, r, k)
            dist2[r], idx[r] = dk, ik
    return dist2.sqrt(), idx


def check_knn(X, k):
    dist, idx, n_exact = _lib.knn(X.to(DEV).contiguous(), k)
    dist, idx = dist.cpu(), idx.cpu()
    ref_d, ref_i = oracle_knn(X, k)
    assert dist.shape == (X.shape[0], k) and dist.dtype == torch.float64 and idx.dtype == torch.int64
    bad = (idx != ref_i).any(1).nonzero().flatten()
    assert len(bad) == 0, f"{len(bad)} rows differ, first {int(bad[0])}: {idx[bad[0]].tolist()} vs {ref_i[bad[0]].tolist()}"
    np.testing.assert_allclose(dist.numpy(), ref_d.numpy(), rtol=1e-12, atol=0)
    return int(n_exact)


@pytest.mark.parametrize("N,D,k", [(2, 1, 1), (33, 3, 5), (1000, 100, 21), (4097, 784, 21), (3000, 1025, 64), (600, 12288, 20)])
def test_knn_exact_against_fp64(N, D, k):
    g = torch.Generator().manual_seed(N + D + k)
    X = torch.randn(N, D, generator=g)
    if D >= 100:                      # a low-dimensional structure, as the ID data have
        X[:, 20:] *= 0.05
    n_exact = check_knn(X, k)
    print(f"N={N} D={D} k={k}: {n_exact} rows by brute force")


def test_knn_large_common_offset():
    g = torch.Generator().manual_seed(7)
    X = torch.randn(1500, 64, generator=g) + 1e3
    check_knn(X, 10)


def test_knn_tight_clusters_take_the_exact_pass():
    g = torch.Generator().manual_seed(8)
    centres = torch.randn(20, 784, generator=g)
    centres = 10.0 * centres / centres.norm(dim=1, keepdim=True)
    X = centres.repeat_interleave(60, 0) + 1e-4 * torch.rand(1200, 784, generator=g) / 784 ** 0.5
    n_exact = check_knn(X, 21)
    assert n_exact > 0


def test_knn_lattice_ties_by_index():
    g = torch.Generator().manual_seed(9)
    X = torch.randint(-3, 4, (1500, 4), generator=g).float()
    X = torch.unique(X, dim=0)                        # distinct lattice points: every distance tie is exact
    X = X[torch.randperm(X.shape[0], generator=g)]
    check_knn(X, 12)
    Y = torch.randint(0, 3, (800, 6), generator=g).float()   # duplicates too: zero distances, ties among them by index
    check_knn(Y, 30)


@pytest.mark.parametrize("N,D,k,msg", [(1, 4, 1, "at least 2"), (10, 0, 1, "at least 1 dimension"), (10, 3, 0, "outside"),
                                       (100, 3, 65, "outside"), (10, 3, 10, "only N - 1")])
def test_knn_refusals(N, D, k, msg):
    X = torch.zeros(max(N, 1), max(D, 1), device=DEV)[:N, :D].contiguous()
    with pytest.raises(RuntimeError, match=msg):
        _lib.knn(X, k)


def test_knn_refuses_cpu_and_other_dtypes():
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.knn(torch.zeros(10, 3), 2)
    with pytest.raises(RuntimeError, match="dtype"):
        _lib.knn(torch.zeros(10, 3, dtype=torch.float64, device=DEV), 2)


# ------------------------------------------------------------------------------------------ the estimators on the GPU
from id_diff_amd import benchmark, mle  # noqa: E402

SETS = ("a", "b")


@pytest.fixture(scope="module")
def sets(golden):
    """The two fixture sets, rebuilt from the project's generators and checked against the sums stored with them."""
    import golden.make_classical_id as mk
    z = golden("classical_id.npz")
    out = mk.make_sets()
    for s, X in out.items():
        sums, head = mk.pin(X)
        np.testing.assert_allclose(sums, z[f"{s}::sums"], rtol=1e-12)
        np.testing.assert_array_equal(head, z[f"{s}::head"])
    return out


@pytest.mark.parametrize("s", SETS)
def test_knn_against_the_ball_tree_fixture(golden, sets, s):
    z = golden("classical_id.npz")
    dist, idx, _ = _lib.knn(torch.from_numpy(sets[s]).to(DEV), 20)
    np.testing.assert_allclose(dist.cpu().numpy(), z[f"{s}::dist"], rtol=1e-12)
    assert np.array_equal(idx.cpu().numpy(), z[f"{s}::ind"])


@pytest.mark.parametrize("s", SETS)
def test_mle_on_the_gpu_against_the_reference(golden, sets, s):
    import pandas as pd
    z = golden("classical_id.npz")
    X = sets[s]
    np.testing.assert_allclose(mle.intrinsic_dim_sample_wise(X, k=5), z[f"{s}::sw5"], rtol=1e-9)
    np.testing.assert_allclose(mle.intrinsic_dim_scale_interval(torch.from_numpy(X).to(DEV), 10, 20), z[f"{s}::si"], rtol=1e-9)
    res, Rs = mle.bootstrap_intrinsic_dim_scale_interval(pd.DataFrame(X), nb_iter=10, random_state=0)
    np.testing.assert_allclose(res, z[f"{s}::boot_F"], rtol=1e-9)
    np.testing.assert_allclose(Rs, z[f"{s}::Rs"], rtol=1e-9)
    mean, _ = mle.bootstrap_intrinsic_dim_scale_interval(torch.from_numpy(X), nb_iter=10, random_state=0, average=True)
    np.testing.assert_allclose(mean, z[f"{s}::boot_T"], rtol=1e-9)


@pytest.mark.parametrize("s", SETS)
def test_pca_estimators_on_the_gpu_against_the_fixture(golden, sets, s):
    z = golden("classical_id.npz")
    X = torch.from_numpy(sets[s]).to(DEV)
    ev = z[f"{s}::ppca_ev"]
    lam = benchmark.covariance_eigenvalues(X)
    keep = ev > 1e-6 * ev[0]
    np.testing.assert_allclose(lam[keep], ev[keep], rtol=1e-6)
    assert benchmark.ppca_dim(X) == int(z[f"{s}::ppca_n"])
    assert benchmark.pca_fo_dim(X) == benchmark.pca_fo_count(ev)


def test_one_knn_launch_per_scale_interval(sets, monkeypatch):
    calls = []
    orig = _lib.knn

    def counted(*a, **k):
        calls.append(a[1])
        return orig(*a, **k)
    monkeypatch.setattr(_lib, "knn", counted)
    mle.intrinsic_dim_scale_interval(sets["a"], 10, 20)
    assert calls == [20]
    mle.bootstrap_intrinsic_dim_scale_interval(sets["a"], nb_iter=3, random_state=1)
    assert calls == [20, 20]


def test_mle_refuses_duplicate_points():
    X = torch.randn(50, 4)
    X[7] = X[3]
    with pytest.raises(ValueError, match="1 points have a zero distance|2 points have a zero distance"):
        mle.intrinsic_dim_sample_wise(X, k=5)


def test_benchmark_writes_the_four_rows_and_skips_filled_cells(tmp_path, capsys):
    import pandas as pd
    from id_diff_amd.configs.config_dict import ConfigDict
    cfg = ConfigDict()
    cfg.data = ConfigDict(datamodule="KSphere", data_samples=1500, n_spheres=1, ambient_dim=20, manifold_dim=5,
                          noise_std=0.01, embedding_type='random_isometry', split=[0.8, 0.1, 0.1])
    cfg.training = ConfigDict(batch_size=256)
    path = str(tmp_path / "classical.csv")
    torch.manual_seed(0)
    benchmark.Benchmark(path, {"ksphere5": cfg}).run()
    df = pd.read_csv(path, index_col="method")
    assert list(df.index) == ["mle_5", "mle_20", "lpca", "ppca"] and list(df.columns) == ["ksphere5"]
    v = df["ksphere5"]
    assert 4.0 < v["mle_5"] < 6.0 and 4.0 < v["mle_20"] < 6.0
    assert v["lpca"] == 6 and v["ppca"] == 6            # a 5-sphere spans 6 linear dimensions
    capsys.readouterr()
    benchmark.Benchmark(path, {"ksphere5": cfg}).run()
    out = capsys.readouterr().out
    assert "was already benchmarked" in out and " START\n" not in out
    pd.testing.assert_frame_equal(pd.read_csv(path, index_col="method"), df)
