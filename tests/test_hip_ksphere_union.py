"""GPU tests of the union of k-spheres: the fused kernel (csrc/ksphere_union.hip) element-wise against ``reference_score`` (fp64 numpy,
itself held to a Bessel-free oracle in test_ksphere_union_host.py), its refusals, and the intrinsic dimension of single points of a
union through the score-matrix builder, the spectrum kernel and the whole driver."""
import ctypes
import math

import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd import _lib, dim_reduction, sde_lib
from id_diff_amd.configs.config_dict import ConfigDict
from id_diff_amd.configs.utils import read_config
from id_diff_amd.lightning_data_modules import KSphereDataset as ksd
from id_diff_amd.models import ksphere_union_exact as ku
from id_diff_amd.models import utils as mutils
from oracle import dim as odim

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _table(frames, log_weights=None):
    off, rows = 0, []
    for j, (Q, R) in enumerate(frames):
        rows.append([off, Q.shape[1], R, -math.log(len(frames)) if log_weights is None else log_weights[j]])
        off += Q.shape[1]
    return np.array(rows, dtype=np.float64)


def _random_union(n, ps, seed):
    """Frames in general position (their spans overlap), radii from {0.5, 1, 2}."""
    rng = np.random.default_rng(seed)
    return [(np.linalg.qr(rng.standard_normal((n, p)))[0], float(rng.choice([0.5, 1.0, 2.0]))) for p in ps]


def _rows_near(frames, B, seed):
    """B rows: a uniform point of a random component plus sigma * noise, sigma spread over 0.01 .. 0.05 row by row."""
    rng = np.random.default_rng(seed + 1)
    n = frames[0][0].shape[0]
    sigma = rng.uniform(0.01, 0.05, B).astype(np.float32)
    x = np.empty((B, n))
    for b in range(B):
        Q, R = frames[rng.integers(len(frames))]
        y = rng.standard_normal(Q.shape[1])
        x[b] = R * Q @ (y / np.linalg.norm(y)) + sigma[b] * rng.standard_normal(n)
    return x.astype(np.float32), sigma


def _launch(x, sigma, frames, mult=None):
    q = torch.from_numpy(np.ascontiguousarray(np.concatenate([Q for Q, _ in frames], axis=1))).to(DEV)
    out, refused = _lib.ksphere_union_score(torch.from_numpy(x).to(DEV), q, _table(frames), torch.from_numpy(sigma).to(DEV),
                                            None if mult is None else torch.from_numpy(mult).to(DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(refused.item())


def _compare(x, sigma, frames, mult, what):
    """|out - ref| <= 2^-23 |ref| + 1e-9 max|ref_row|: the fp32 rounding of an fp64 result, nothing else."""
    score, w, refused = ku.reference_score(x, sigma, frames)
    s2 = sigma.astype(np.float64) ** 2
    ref = score * s2[:, None] * (1.0 if mult is None else mult.astype(np.float64)[:, None])
    out, count = _launch(x, sigma, frames, mult)
    assert out.shape == x.shape and out.dtype == np.float32
    assert count == int(refused.sum()), f"{what}: {count} rows refused on the device, {int(refused.sum())} by the oracle"
    assert np.array_equal(np.isnan(out).all(axis=1), refused) and np.array_equal(np.isnan(out).any(axis=1), refused)
    good = ~refused
    bound = 2.0 ** -23 * np.abs(ref[good]) + 1e-9 * np.abs(ref[good]).max(axis=1, keepdims=True)
    err = np.abs(out[good].astype(np.float64) - ref[good])
    worst = float((err / bound).max()) if good.any() else 0.0
    print(f"{what}: {int(refused.sum())} of {len(x)} rows refused, worst |out - ref| / bound = {worst:.3f}, "
          f"max |ref| = {np.abs(ref[good]).max() if good.any() else 0.0:.3e}")
    assert (err <= bound).all(), f"{what}: worst |out - ref| / bound = {worst:.3f}"
    return w, refused


CASES = [  # B, n, widths p_j, mult given
    (1, 5, [2], False),
    (63, 5, [2, 3, 4], True),
    (65, 23, [11, 4], False),
    (257, 23, [2, 3, 4, 11, 2, 3, 4, 11], True),
    (65, 48, [31, 11, 3], True),
    (257, 48, [4], False),
    (63, 100, [11, 31], True),
    (257, 100, [2, 3, 4, 11, 31, 2, 3, 4], False),
    (1, 100, [31], True),
]


@pytest.mark.parametrize("B,n,ps,with_mult", CASES, ids=[f"B{c[0]}-n{c[1]}-J{len(c[2])}-P{sum(c[2])}-{'mult' if c[3] else 'nomult'}" for c in CASES])
def test_kernel_against_reference_score(B, n, ps, with_mult):
    seed = 1000 * n + 10 * len(ps) + B
    frames = _random_union(n, ps, seed)
    x, sigma = _rows_near(frames, B, seed)
    mult = (-1.0 / sigma ** 2 * np.random.default_rng(seed).uniform(0.5, 2.0, B)).astype(np.float32) if with_mult else None
    w, refused = _compare(x, sigma, frames, mult, f"B={B} n={n} p={ps}")
    assert refused.mean() <= 0.25                          # the comparison above is not about refused rows


def _intersection_rows(B=257, seed=7):
    """`along_axis`, dims [3, 3] in R^16: the 3-spheres of coordinates 0..3 and 1..4 share the unit sphere of coordinates 1..3.  Rows
    around the common point e_1, pushed along coordinates 0 and 4 (the two directions that tell the spheres apart)."""
    cfg = ConfigDict()
    cfg.data = ConfigDict(n_spheres=2, ambient_dim=16, manifold_dim=[3, 3], noise_std=0.0, embedding_type='along_axis')
    frames = ksd.frames(cfg)
    rng = np.random.default_rng(seed)
    sigma = np.linspace(0.01, 0.05, B).astype(np.float32)
    x = np.zeros((B, 16))
    x[:, 1] = 1.0
    x += sigma[:, None] * rng.standard_normal((B, 16))
    x[:, 0] *= 3.0
    x[:, 4] *= 3.0
    return x.astype(np.float32), sigma, frames


def test_intersection_of_two_spheres_mixes_for_real():
    x, sigma, frames = _intersection_rows()
    score, w, refused = ku.reference_score(x, sigma, frames)
    assert not refused.any()
    assert w[:, 0].min() < 0.01 and w[:, 0].max() > 0.99 and ((w[:, 0] > 0.2) & (w[:, 0] < 0.8)).sum() >= 16
    _compare(x, sigma, frames, None, "intersection")


def test_concentric_spheres_mix_three_ways():
    """Three 3-spheres of radii 1, 1.03 and 1.06 in ONE subspace of R^23 plus an 11-sphere elsewhere: rows between the shells."""
    rng = np.random.default_rng(11)
    Q = np.linalg.qr(rng.standard_normal((23, 4)))[0]
    frames = [(Q, 1.0), (Q, 1.03), (np.linalg.qr(rng.standard_normal((23, 12)))[0], 1.0), (Q, 1.06)]
    B = 65
    sigma = rng.uniform(0.01, 0.03, B).astype(np.float32)
    y = rng.standard_normal((B, 4))
    x = (np.linspace(0.98, 1.08, B)[:, None] * y / np.linalg.norm(y, axis=1, keepdims=True)) @ Q.T + sigma[:, None] * rng.standard_normal((B, 23))
    x = x.astype(np.float32)
    score, w, refused = ku.reference_score(x, sigma, frames)
    assert not refused.any()
    assert all(((w[:, j] > 0.1) & (w[:, j] < 0.9)).sum() >= 4 for j in (0, 1, 3))
    mult = (-1.0 / sigma).astype(np.float32)
    _compare(x, sigma, frames, mult, "concentric")


def _union_config(n, dims, radii, noise_std=0.0, emb='random_isometry'):
    cfg = read_config('configs/dimension_estimation/paper/euclidean_data/ksphere/union.py')
    cfg.data.ambient_dim, cfg.data.dim, cfg.data.shape = n, n, [n]
    cfg.data.manifold_dim, cfg.data.radii, cfg.data.noise_std, cfg.data.embedding_type = dims, radii, noise_std, emb
    cfg.data.data_samples = 8
    cfg.model.state_size = n
    cfg.device = DEV
    return cfg


def test_refused_rows_are_nan_and_counted_and_the_model_raises():
    frames = _random_union(48, [4, 11], 5)
    x, sigma = _rows_near(frames, 65, 5)
    x[17] = 0.0                                            # the origin: no component's series applies
    score, w, refused = ku.reference_score(x, sigma, frames)
    assert refused.sum() == 1 and refused[17]
    out, count = _launch(x, sigma, frames)
    assert count == 1
    assert np.isnan(out[17]).all() and np.isfinite(np.delete(out, 17, axis=0)).all()
    cfg = _union_config(48, [3, 10], [1, 2])
    model = mutils.create_model(cfg).to(DEV)
    torch.manual_seed(0)
    pts = ksd.KSphereDataset(cfg).data[:6].clone()
    labels = torch.zeros(6, device=DEV)
    assert torch.isfinite(model(pts.to(DEV), labels)).all()
    pts[2] = 0.0
    with pytest.raises(NotImplementedError, match="1 of 6 rows refused"):
        model(pts.to(DEV), labels)


def test_unserved_shapes_are_refused_before_any_launch():
    x = torch.zeros(4, 512, device=DEV)
    q = torch.zeros(512, 400, device=DEV, dtype=torch.float64)
    sigma = torch.full((4,), 0.01, device=DEV)
    table = [[50 * j, 50, 1.0, -math.log(8)] for j in range(8)]
    assert not _lib.ksphere_union_ok(512, 8, 400)
    with pytest.raises(RuntimeError, match="is not served"):
        _lib.ksphere_union_score(x, q, table, sigma)
    # the entry point itself: more than 8 components, a frame wider than 128, a table that does not tile [0, P)
    out, refused = torch.full((4, 48), 7.0, device=DEV), torch.zeros(1, device=DEV, dtype=torch.int32)
    x, q = torch.zeros(4, 48, device=DEV), torch.zeros(48, 12, device=DEV, dtype=torch.float64)
    call = lambda tab, n, J, P: _lib.lib().idiff_ksphere_union_score_f32(
        x.data_ptr(), q.data_ptr(), np.ascontiguousarray(tab, dtype=np.float64).ctypes.data, sigma.data_ptr(), None, out.data_ptr(),
        refused.data_ptr(), 4, n, J, P, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    lw = -math.log(2)
    assert call([[j, 1, 1.0, lw] for j in range(9)], 48, 9, 9) == 1001
    assert call([[0, 129, 1.0, 0.0]], 300, 1, 129) == 1001
    assert call([[0, 4, 1.0, lw], [5, 7, 1.0, lw]], 48, 2, 12) == 1001           # a gap
    assert call([[0, 4, 1.0, lw], [4, 9, 1.0, lw]], 48, 2, 12) == 1001           # past P
    assert call([[0, 4, -1.0, lw], [4, 8, 1.0, lw]], 48, 2, 12) == 1001          # a radius that is not positive
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(refused.item()) == 0


def _builder(cfg):
    model = mutils.create_model(cfg).to(DEV).eval()
    sde, eps = sde_lib.configure_sde(cfg)
    score_fn = mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=True)
    return model, dim_reduction.ScoreMatrixBuilder(score_fn, sde, eps, torch.device(DEV))


@pytest.mark.parametrize("n,dims,radii,noise_std", [(48, [3, 10], [1, 2], 0.0), (100, [10, 30], [1, 1], 0.0)],
                         ids=["3-10-in-R48", "10-30-in-R100"])
def test_id_of_one_point_per_component(n, dims, radii, noise_std):
    """A point of each sphere of the union reports the dimension of ITS sphere (batch size 500, as the paper's configs)."""
    cfg = _union_config(n, dims, radii, noise_std)
    torch.manual_seed(5)
    data = ksd.KSphereDataset(cfg).data                    # 8 points of sphere 0, then 8 of sphere 1
    model, builder = _builder(cfg)
    with torch.no_grad():
        for comp, point in ((0, 0), (1, 8)):
            S = builder.build(data[point].to(DEV), 500, seed=1234 + comp)
            assert S.shape == (1501, n) and bool(torch.isfinite(S).all())
            sv = _lib.spectrum(S).cpu()
            got = odim.estimate_dim(sv.tolist())
            print(f"union {dims} in R^{n}: point of sphere {comp}: ID {got}")
            assert got == dims[comp]


def test_union_config_end_to_end(tmp_path):
    """`get_manifold_dimension` on configs/.../ksphere/union.py (10- and 30-sphere in R^100): every point's ID is the k of its nearest
    sphere, and every spectrum is that of the oracle's score matrix on the same perturbed rows."""
    cfg = read_config('configs/dimension_estimation/paper/euclidean_data/ksphere/union.py')
    cfg.data.data_samples = 2000
    cfg.device = DEV
    cfg.logging.log_path = str(tmp_path)
    svd, dims = dim_reduction.get_manifold_dimension(cfg, return_svd=True, return_dims=True)
    # the points the driver visited, in its order (dim_reduction.py: the seed, the data module, collect_points)
    seed = int(cfg.get('seed', 42))
    torch.manual_seed(seed)
    DataModule, pl_module, score_fn, device = dim_reduction.setup_model(cfg)
    points = dim_reduction.collect_points(DataModule.train_dataloader(), dim_reduction._num_datapoints(cfg))
    assert len(points) == len(dims) == len(svd['singular_values']) == 4
    frames = pl_module.score_model.frames()
    builder = dim_reduction.ScoreMatrixBuilder(score_fn, pl_module.sde, pl_module.sampling_eps, device)
    sigma = float(pl_module.sde.marginal_prob(torch.zeros(()), torch.tensor(pl_module.sampling_eps))[1])
    for p, (x, batchsize) in enumerate(points):
        xd = x.double().numpy()
        dist = [abs(np.linalg.norm(xd @ Q) - R) + np.linalg.norm(xd - Q @ (Q.T @ xd)) for Q, R in frames]
        k = cfg.data.manifold_dim[int(np.argmin(dist))]
        assert dims[p] == odim.estimate_dim(svd['singular_values'][p]) == k, f"point {p}: ID {dims[p]}, nearest sphere has k = {k}"
        rows = dim_reduction.batching(tuple(x.shape), batchsize)[2]
        batch, _ = builder._perturbed([x.to(device).reshape(-1).contiguous()], builder.eps, 0, rows, seeds=[seed + 1000003 * (p + 1)])
        score, w, refused = ku.reference_score(batch[0].cpu().numpy(), np.float32(sigma), frames)
        assert not refused.any()
        ref = odim.spectrum_f64(torch.from_numpy(score.astype(np.float32))).numpy()
        sv = np.array(svd['singular_values'][p])
        keep = ref > 1e-5 * ref[0]
        np.testing.assert_allclose(sv[keep], ref[keep], rtol=1e-4)
