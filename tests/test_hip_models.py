"""GPU parity of the score networks and of the whole ID pipeline against the oracle / the reference's golden outputs."""
import numpy as np
import pytest
import torch

import id_diff_amd
from helpers import (beatgans_config, ddpm_config, fcn_config, fill_from_seed, ncsnpp_config, overrides_from_golden,
                     rel_err, replay_conditional_noise, state_dict_from_golden, weight_abs_sums)
from id_diff_amd import _lib, dim_reduction, plot_utils, sde_lib
from id_diff_amd.configs.utils import read_config
from id_diff_amd.models import utils as mutils
from oracle import dim as odim, ksphere as oks, models as omodels, sde as osde

pytestmark = pytest.mark.gpu
DEV = "cuda"
# fp32 networks evaluated with a different (but exact-fp32) summation order than ATen's CPU kernels.  Measured on the
# 16x16 nf=8 NCSN++ (scripts/relerr_probe.py): HIP vs oracle 1.2e-6; HIP vs an fp64 evaluation of the same weights
# 1.0e-6, the oracle's own fp32 vs fp64 9.7e-7 -- the HIP path is as close to the exact network as the reference path is.
NET_RTOL = 2e-5


def test_fcn_tiny_golden(golden):
    z = golden("fcn_tiny.npz")
    model = mutils.create_model(fcn_config(hidden_nodes=64))
    model.load_state_dict(state_dict_from_golden(z))
    model.to(DEV)
    score_fn = mutils.get_score_fn(sde_lib.VESDE(1e-2, 4, 1000), model, conditional=False, train=False, continuous=True)
    y = score_fn(torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV))
    assert rel_err(y.cpu(), z["score"]) < NET_RTOL


def test_fcn_full_size_golden(golden):
    z = golden("fcn_full_seed0.npz")
    torch.manual_seed(0)
    model = mutils.create_model(fcn_config(hidden_nodes=2048))   # same nn.Linear construction order as the reference
    sums = np.array([float(v.double().abs().sum()) for v in model.state_dict().values()])
    np.testing.assert_allclose(sums, z["weight_abs_sums"], rtol=1e-12)
    model.to(DEV)
    score_fn = mutils.get_score_fn(sde_lib.VESDE(1e-2, 4, 1000), model)
    y = score_fn(torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV))
    assert rel_err(y.cpu(), z["score"]) < NET_RTOL


@pytest.mark.parametrize("variant", ["bench_init0", "bench_init1", "ddpm_outskip", "biggan_nofir", "biggan_outskip_sum"])
def test_ncsnpp_golden(golden, variant):
    z = golden(f"ncsnpp_{variant}.npz")
    model = mutils.create_model(ncsnpp_config(**overrides_from_golden(z)))
    model.load_state_dict(state_dict_from_golden(z))
    model.to(DEV)
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    raw = model(x, t * 999)
    assert rel_err(raw.cpu(), z["model_out"]) < NET_RTOL
    y = mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)(x, t)
    assert rel_err(y.cpu(), z["score"]) < NET_RTOL


@pytest.mark.parametrize("variant", ["paper_like", "plain_resample"])
def test_beatgans_golden(golden, variant):
    z = golden(f"beatgans_{variant}.npz")
    model = mutils.create_model(beatgans_config(**overrides_from_golden(z)))
    model.load_state_dict(state_dict_from_golden(z))
    model.to(DEV)
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    raw = model(x, t * 999)
    assert rel_err(raw.cpu(), z["model_out"]) < NET_RTOL
    y = mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)(x, t)
    assert rel_err(y.cpu(), z["score"]) < NET_RTOL


@pytest.mark.parametrize("variant", ["mnist_like", "pool_resample"])
def test_ddpm_golden(golden, variant):
    z = golden(f"ddpm_{variant}.npz")
    model = mutils.create_model(ddpm_config(**overrides_from_golden(z)))
    assert len(model.all_modules) == int(z["n_modules"])
    model.load_state_dict(state_dict_from_golden(z))
    model.to(DEV)
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    raw = model(x, t * 999)
    assert rel_err(raw.cpu(), z["model_out"]) < NET_RTOL
    y = mutils.get_score_fn(sde_lib.VESDE(0.009, 50, 1000), model)(x, t)
    assert rel_err(y.cpu(), z["score"]) < NET_RTOL


def test_beatgans_config5_architecture_vs_oracle():
    """BASELINE config 5 network (64x64x3, model_channels 128, mult (1,1,2,3,4)) at B=2, zero-initialised convs
    replaced by random values so that every branch contributes."""
    cfg = read_config('configs/dimension_estimation/extra_experiments/styleGAN/style_gan_64d_BeatGAN.py')
    torch.manual_seed(0)
    ref_model = omodels.create_model(cfg)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for prm in ref_model.parameters():
            if float(prm.abs().sum()) == 0.0:
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.02)
    model = mutils.create_model(cfg)
    assert sum(p.numel() for p in model.parameters()) == sum(p.numel() for p in ref_model.parameters())
    model.load_state_dict(ref_model.state_dict())
    model.to(DEV)
    x, t = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)), torch.tensor([1e-5, 0.3])
    with torch.no_grad():
        ref = osde.get_score_fn(osde.VESDE(0.01, 50, 1000), ref_model)(x, t)
    y = mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)(x.to(DEV), t.to(DEV))
    assert rel_err(y.cpu(), ref) < NET_RTOL


def test_ncsnpp_benchmark_width_vs_oracle():
    """nf=128 benchmark architecture with every branch active, B=4."""
    cfg = read_config('configs/dimension_estimation/paper/image_data/cifar_shaped/ncsnpp.py')
    cfg.model.init_scale = 1.0
    torch.manual_seed(0)
    ref_model = omodels.create_model(cfg)
    model = mutils.create_model(cfg)
    model.load_state_dict(ref_model.state_dict())
    model.to(DEV)
    g = torch.Generator().manual_seed(1)
    x, t = torch.rand(4, 3, 32, 32, generator=g), torch.tensor([1e-5, 1e-5, 0.1, 0.5])
    with torch.no_grad():
        ref = osde.get_score_fn(osde.VESDE(0.01, 50, 1000), ref_model)(x, t)
    y = mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)(x.to(DEV), t.to(DEV))
    assert rel_err(y.cpu(), ref) < NET_RTOL


def test_batch_size_is_not_observable():
    """Rows are independent samples: evaluating 5 rows at once or one by one gives the same scores (design premise
    of the inflight batching in dim_reduction.py)."""
    z_cfg = ncsnpp_config(**{"model.init_scale": 1.0})
    torch.manual_seed(3)
    model = mutils.create_model(z_cfg).to(DEV)
    x, t = torch.rand(5, 3, 32, 32, device=DEV), torch.full((5,), 1e-5 * 999, device=DEV)
    full = model(x, t)
    for i in range(5):
        assert rel_err(model(x[i:i + 1].contiguous(), t[i:i + 1].contiguous()).cpu(), full[i:i + 1].cpu()) < 1e-5


def _pipeline_pair(score_fn_hip, score_fn_cpu, sde_hip, sde_cpu, x, batchsize, eps):
    num_batches, _, rows = odim.batching(tuple(x.shape), batchsize)
    g = torch.Generator().manual_seed(7)
    noise = torch.randn(num_batches, batchsize, *x.shape, generator=g)
    S_ref = odim.score_matrix(score_fn_cpu, sde_cpu, x, batchsize, eps, noise=noise)
    builder = dim_reduction.ScoreMatrixBuilder(score_fn_hip, sde_hip, eps, torch.device(DEV))
    flat_noise = noise.reshape(num_batches * batchsize, *x.shape)[:rows].to(DEV)
    S = builder.build(x.to(DEV), batchsize, noise=flat_noise)
    return S, S_ref


def test_score_matrix_and_spectrum_fcn_vs_oracle():
    """BASELINE config 2 recipe (50-sphere, fcn 2048x5, B=500 -> S 1501x100) end to end on identical noise."""
    torch.manual_seed(0)
    cfg = fcn_config(hidden_nodes=2048)
    ref_model = omodels.create_model(cfg)
    model = mutils.create_model(cfg)
    model.load_state_dict(ref_model.state_dict())
    model.to(DEV)
    torch.manual_seed(42)
    x = oks.ksphere_data(4, 100, 50)[1]
    sde_c, sde_h = osde.VESDE(1e-2, 4, 1000), sde_lib.VESDE(1e-2, 4, 1000)
    S, S_ref = _pipeline_pair(mutils.get_score_fn(sde_h, model), osde.get_score_fn(sde_c, ref_model), sde_h, sde_c, x, 500, 1e-5)
    assert S.shape == (1501, 100) and rel_err(S.cpu(), S_ref) < NET_RTOL
    sv = _lib.spectrum(S).cpu()
    # same input -> the 1e-4 criterion of north_star
    np.testing.assert_allclose(sv.numpy(), odim.spectrum(S.cpu()).numpy(), rtol=1e-4)
    # end to end the two score matrices differ by fp32 summation order; singular values then differ by at most
    # ||S - S_ref||_2 (Weyl), and the integer ID must agree
    ref = odim.spectrum(S_ref)
    bound = float(torch.linalg.matrix_norm(S.cpu().double() - S_ref.double(), ord=2))
    assert float((sv.double() - ref.double()).abs().max()) <= 1.5 * bound + 1e-6 * float(ref[0])
    assert plot_utils.estimate_dim(sv.tolist()) == odim.estimate_dim(ref.tolist())


def test_score_matrix_and_spectrum_ncsnpp_small_vs_oracle():
    """Image recipe at reduced width (nf=8) and B=32 -> S 1056... rows x 3072 cols needs M >= D, so use 16x16 images."""
    cfg = ncsnpp_config(**{"model.init_scale": 1.0, "model.attn_resolutions": (8,), "data.image_size": 16,
                           "data.effective_image_size": 16, "data.shape": [3, 16, 16], "model.num_res_blocks": 1})
    torch.manual_seed(0)
    ref_model = omodels.create_model(cfg)
    model = mutils.create_model(cfg)
    model.load_state_dict(ref_model.state_dict())
    model.to(DEV)
    x = torch.rand(3, 16, 16, generator=torch.Generator().manual_seed(1))
    sde_c, sde_h = osde.VESDE(0.01, 50, 1000), sde_lib.VESDE(0.01, 50, 1000)
    S, S_ref = _pipeline_pair(mutils.get_score_fn(sde_h, model), osde.get_score_fn(sde_c, ref_model), sde_h, sde_c, x, 100, 1e-5)
    assert S.shape == (1156, 768) and rel_err(S.cpu(), S_ref) < NET_RTOL   # (256//100+1)*4=12 batches, extra 56
    sv = _lib.spectrum(S).cpu()
    ref64 = odim.spectrum_f64(S.cpu())
    keep = ref64 > 2e-5 * ref64[0]
    np.testing.assert_allclose(sv.numpy()[keep], odim.spectrum(S.cpu()).numpy()[keep], rtol=1e-4)
    bound = float(torch.linalg.matrix_norm(S.cpu().double() - S_ref.double(), ord=2))
    assert float((sv.double() - odim.spectrum(S_ref).double()).abs().max()) <= 1.5 * bound + 1e-6 * float(ref64[0])


@pytest.mark.parametrize("k", [10, 50])
def test_id_recovered_on_ksphere_end_to_end(k, tmp_path):
    """North-star acceptance: the drop-in driver on the GPU recovers ID = k on the k-sphere in R^100."""
    cfg = read_config(f'configs/dimension_estimation/paper/euclidean_data/ksphere/{k}dim.py')
    cfg.model.name = 'ksphere_exact'
    cfg.data.data_samples = 2000
    cfg.device = DEV
    cfg.logging.log_path = str(tmp_path)
    svd = dim_reduction.get_manifold_dimension(cfg, return_svd=True)
    assert len(svd['singular_values']) == 4 and len(svd['singular_values'][0]) == 100   # svd_points=5 -> 4 points
    assert plot_utils.plot_dims(svd)[1] == [k] * 4
    # pickle layout of the non-returning form (dim_reduction.py:206-211)
    dim_reduction.get_manifold_dimension(cfg, name='svd_test')
    import pickle, os
    with open(os.path.join(str(tmp_path), cfg.logging.log_name, 'svd', 'svd_test.pkl'), 'rb') as f:
        again = pickle.load(f)
    assert again['singular_values'] == svd['singular_values']          # per-point seeds: reproducible


def test_exact_score_vs_oracle():
    cfg = read_config('configs/dimension_estimation/paper/euclidean_data/ksphere/10dim.py')
    cfg.model.name = 'ksphere_exact'
    model = mutils.create_model(cfg).to(DEV)
    torch.manual_seed(42)
    x = (oks.ksphere_data(64, 100, 10) + 0.01 * torch.randn(64, 100)).contiguous()
    t = torch.full((64,), 1e-5)
    ref = osde.get_score_fn(osde.VESDE(1e-2, 4, 1000), oks.KSphereExact(100, 10, 1e-2, 4))(x, t)
    y = mutils.get_score_fn(sde_lib.VESDE(1e-2, 4, 1000), model)(x.to(DEV), t.to(DEV))
    assert rel_err(y.cpu(), ref) < 1e-4


def test_conditional_manifold_dimension_layout(tmp_path):
    """get_conditional_manifold_dimension (dim_reduction.py:12-114): 12 noise levels, label==1 points only, three
    pickles per level."""
    import os, pickle
    cfg = ncsnpp_config(**{"model.init_scale": 1.0, "model.attn_resolutions": (8,), "data.image_size": 16,
                           "data.effective_image_size": 16, "data.shape": [3, 16, 16], "model.num_res_blocks": 1})
    cfg.data.datamodule = 'image_synthetic'
    cfg.data.data_samples = 200
    cfg.data.latent_dim = 4
    cfg.training.batch_size = 100
    cfg.training.lightning_module = 'base'
    cfg.validation = type(cfg)(batch_size=100)
    cfg.model.checkpoint_path = None
    cfg.model.allow_random_init = True          # no trained checkpoint ships with the reference
    cfg.logging = type(cfg)(log_path=str(tmp_path), log_name='cond')
    cfg.dim_estimation = type(cfg)(num_datapoints=3)
    cfg.device = DEV
    cfg.seed = 7
    dim_reduction.get_conditional_manifold_dimension(cfg)
    root = os.path.join(str(tmp_path), 'cond', 'svd')
    levels = sorted(os.listdir(root))
    assert len(levels) == 12 and levels[0] == '0.000' and levels[-1] == '0.300'
    first = None
    for lv in levels:
        with open(os.path.join(root, lv, 'labels_svd.pkl'), 'rb') as f:
            sv = pickle.load(f)['singular_values']
        with open(os.path.join(root, lv, 'labels.pkl'), 'rb') as f:
            labels = pickle.load(f)['labels']
        with open(os.path.join(root, lv, 'images.pkl'), 'rb') as f:
            imgs = pickle.load(f)['images']
        assert labels == [1, 1] and len(sv) == 2 and imgs.shape == (2, 16, 16, 3)   # num_datapoints=3 -> 2 points
        # the validation split has 20 items, so the loader batch (= rows per score batch) is 20:
        # ambient 256 -> (256 // 20 + 1) * 4 = 52 batches, 51 * 20 + 16 = 1036 rows >= 768 columns
        assert all(len(s) == 768 for s in sv)
        assert all(s[i] >= s[i + 1] for s in sv for i in range(len(s) - 1))
        first = first or sv
    assert first != sv     # the spectrum depends on the noise level


def test_score_matrix_does_not_depend_on_launch_set_size():
    """In-kernel Philox noise is indexed by the element's position in the point's noise matrix and every kernel is
    free of atomics, so cutting the rows of a point into different launch sets changes nothing observable."""
    cfg = ncsnpp_config(**{"model.init_scale": 1.0})
    torch.manual_seed(5)
    model = mutils.create_model(cfg).to(DEV)
    sde = sde_lib.VESDE(0.01, 50, 1000)
    score_fn = mutils.get_score_fn(sde, model)
    x = torch.rand(3, 32, 32, device=DEV)
    mats = []
    for inflight in (None, 96, 1000):
        b = dim_reduction.ScoreMatrixBuilder(score_fn, sde, 1e-5, torch.device(DEV), inflight_rows=inflight)
        mats.append(b.build(x, 700, seed=99))                    # (1024 // 700 + 1) * 4 = 8 batches, extra 324 -> 5224 rows
    assert mats[0].shape == (5224, 3072)
    for other in mats[1:]:
        assert rel_err(other.cpu(), mats[0].cpu()) < 2e-6


def _rows_driver_worker(rank, world, port, log_path, q):
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    import id_diff_amd  # noqa: F401
    from id_diff_amd import dim_reduction as dr
    from id_diff_amd.configs.utils import read_config as rc
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    torch.cuda.set_device(0)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    cfg = rc('configs/dimension_estimation/paper/euclidean_data/ksphere/10dim.py')
    cfg.model.name = 'ksphere_exact'
    cfg.data.data_samples = 2000
    cfg.device = "cuda"
    cfg.logging.log_path = log_path
    cfg.dim_estimation = type(cfg)(shard='rows')
    svd = dr.get_manifold_dimension(cfg, return_svd=True)
    q.put((rank, svd['singular_values']))
    dist.barrier()
    dist.destroy_process_group()


def test_driver_row_sharded_matches_point_sharded(tmp_path):
    """`config.dim_estimation.shard = 'rows'`: two ranks split the rows of every point; spectra
    and IDs equal the ordinary single-process run (per-row Philox noise does not depend on the split)."""
    import os
    import torch.multiprocessing as mp
    cfg = read_config('configs/dimension_estimation/paper/euclidean_data/ksphere/10dim.py')
    cfg.model.name = 'ksphere_exact'
    cfg.data.data_samples = 2000
    cfg.device = DEV
    cfg.logging.log_path = str(tmp_path)
    ref = dim_reduction.get_manifold_dimension(cfg, return_svd=True)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_rows_driver_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank in (0, 1):
        np.testing.assert_allclose(np.array(got[rank]), np.array(ref['singular_values']), rtol=2e-5, atol=1e-5)
        assert plot_utils.plot_dims({'singular_values': got[rank]})[1] == [10] * 4
    # not only the HIP path against itself: point 0's score matrix rebuilt here (driver's data order and per-point seed)
    # and handed to the oracle's CPU SVD -- the row-sharded spectrum holds 1e-4 against it, and the oracle's ID is 10 too
    torch.manual_seed(int(cfg.get('seed', 42)))
    DataModule, pl_module, score_fn, device = dim_reduction.setup_model(cfg)
    points = dim_reduction.collect_points(DataModule.train_dataloader(), dim_reduction._num_datapoints(cfg))
    builder = dim_reduction.ScoreMatrixBuilder(score_fn, pl_module.sde, pl_module.sampling_eps, device)
    S0 = builder.build(points[0][0].to(DEV), points[0][1], seed=int(cfg.get('seed', 42)) + 1000003).cpu()
    ref32, ref64 = odim.spectrum(S0), odim.spectrum_f64(S0)
    for rank in (0, 1):
        sv0 = np.array(got[rank][0])
        np.testing.assert_allclose(sv0, ref32.numpy(), rtol=1e-4)
        np.testing.assert_allclose(sv0, ref64.numpy(), rtol=1e-4)
    assert odim.estimate_dim(ref32.tolist()) == 10


def test_winograd_and_implicit_gemm_paths_agree_on_the_spectrum():
    """The benchmark network (nf = 128) on one data point, 3x3 convs once through Winograd F(2x2,3x3) and once through
    the implicit GEMM (IDIFF_NO_WINOGRAD): score matrix, singular values (the 1e-4 bar of the north star) and ID."""
    cfg = read_config('configs/dimension_estimation/paper/image_data/cifar_shaped/ncsnpp.py')
    torch.manual_seed(0)
    model = mutils.create_model(cfg).to(DEV).eval()
    sde, eps = sde_lib.configure_sde(cfg)
    builder = dim_reduction.ScoreMatrixBuilder(mutils.get_score_fn(sde, model), sde, eps, torch.device(DEV))
    x = torch.rand(3, 32, 32, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        S_w = builder.build(x, 128, seed=9)
        assert _lib.set_option("IDIFF_NO_WINOGRAD", True) is False
        try:
            S_d = builder.build(x, 128, seed=9)
        finally:
            _lib.set_option("IDIFF_NO_WINOGRAD", False)
    assert S_w.shape == (4480, 3072)
    assert not torch.equal(S_w, S_d)                      # different arithmetic ...
    assert rel_err(S_w.cpu(), S_d.double().cpu()) < 2e-5  # ... same numbers
    sv_w, sv_d = _lib.spectrum(S_w), _lib.spectrum(S_d)
    big = sv_d > 1e-3 * sv_d[0]                          # the part of the spectrum the estimator can see
    assert float(((sv_w - sv_d).abs() / sv_d)[big].max()) < 1e-4
    assert plot_utils.estimate_dim(sv_w.tolist()) == plot_utils.estimate_dim(sv_d.tolist())


# ---------------------------------------------------------------------------------------------- round-2 parity holes
def test_wide_ncsnpp_golden(golden):
    """nf = 128 against REFERENCE output (weights from the seed recipe of make_golden.fill_from_seed): the GroupNorm
    32-group cap and the Winograd-eligible 3x3 convs (Cin % 8 == 0, Cout % 64 == 0) are now pinned to the reference,
    not only to the oracle."""
    z = golden("ncsnpp_wide.npz")
    model = mutils.create_model(ncsnpp_config(**overrides_from_golden(z)))
    assert len(model.all_modules) == int(z["n_modules"])
    fill_from_seed(model, int(z["seed"]))
    np.testing.assert_allclose(weight_abs_sums(model), z["weight_abs_sums"], rtol=1e-12)
    model.to(DEV)
    model._invalidate()
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    raw = model(x, t * 999)
    assert rel_err(raw.cpu(), z["model_out"]) < NET_RTOL
    y = mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)(x, t)
    assert rel_err(y.cpu(), z["score"]) < NET_RTOL


@pytest.fixture
def wino43_everywhere(monkeypatch):
    """Send every eligible 3x3 convolution of 8x8 maps and larger through the F(4x4, 3x3) kernel, also at test batch sizes (the
    executor keeps launches of fewer than 512 workgroups on the 2x2 form: a speed rule, not a correctness one)."""
    from id_diff_amd.models import nhwc as hip_nhwc
    monkeypatch.setattr(hip_nhwc, "WINO43_MIN_WORKGROUPS", 1)
    monkeypatch.setattr(hip_nhwc, "WINO43_PAIRS_MIN_WORKGROUPS", 1)
    calls = {"n": 0, "pairs": 0, "gemm_pairs": 0}
    orig = _lib.conv2d_winograd43

    def counted(*a, **k):
        calls["n"] += 1
        calls["pairs"] += bool(k.get("pairs"))
        return orig(*a, **k)
    monkeypatch.setattr(_lib, "conv2d_winograd43", counted)
    # ... and the attention blocks' projections of a GroupNorm's output through the fp16-pair GEMM (from 256 tiles on in production)
    orig_gp = _lib.gemm_pairs

    def counted_gp(*a, **k):
        calls["gemm_pairs"] += 1
        return orig_gp(*a, **k)
    monkeypatch.setattr(_lib, "gemm_pairs", counted_gp)
    prev = _lib.set_option("IDIFF_PAIRS_MIN_TILES", 1)
    yield calls
    _lib.set_option("IDIFF_PAIRS_MIN_TILES", prev)


def test_wide_ncsnpp_golden_through_winograd43(golden, wino43_everywhere):
    """The nf = 128 NCSN++ against the REFERENCE's output with every eligible convolution on F(4x4, 3x3) (the form the benchmark
    runs): same NET_RTOL as the 2x2 form -- the gate of DESIGN.md 7.3 (rel_err(S) <= 2e-5), measured ~5e-6."""
    z = golden("ncsnpp_wide.npz")
    model = mutils.create_model(ncsnpp_config(**overrides_from_golden(z)))
    fill_from_seed(model, int(z["seed"]))
    model.to(DEV)
    model._invalidate()
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    raw = model(x, t * 999)
    assert wino43_everywhere["n"] >= 8, wino43_everywhere            # the 3x3 convs of the levels of 8x8 pixels and larger
    assert wino43_everywhere["pairs"] >= 8, wino43_everywhere        # ... all fed by a GroupNorm: contraction on fp16 pairs
    assert wino43_everywhere["gemm_pairs"] >= 2, wino43_everywhere   # q|k and V^T of every attention block
    assert rel_err(raw.cpu(), z["model_out"]) < NET_RTOL
    y = mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)(x, t)
    assert rel_err(y.cpu(), z["score"]) < NET_RTOL
    # the same network with the contraction on the fp32 matrix cores (IDIFF_NO_WINO43H): same bar
    before = dict(wino43_everywhere)
    model._invalidate()
    with _lib.thread_option("IDIFF_NO_WINO43H", 1):
        raw32 = model(x, t * 999)
    assert wino43_everywhere["n"] - before["n"] >= 8 and wino43_everywhere["pairs"] == before["pairs"], wino43_everywhere
    assert rel_err(raw32.cpu(), z["model_out"]) < NET_RTOL


@pytest.fixture
def wino1d_everywhere(monkeypatch, wino43_everywhere):
    """... and the GroupNorm-fed 3x3 convolutions of 8 x 8 maps and larger through the row-wise F(4, 3) pair kernel, at test batch sizes."""
    from id_diff_amd.models import nhwc as hip_nhwc
    monkeypatch.setattr(hip_nhwc, "WINO1D_MIN_WORKGROUPS", 1)
    calls = {"n": 0}
    orig = _lib.conv2d_wino1d

    def counted(*a, **k):
        calls["n"] += 1
        return orig(*a, **k)
    monkeypatch.setattr(_lib, "conv2d_wino1d", counted)
    return calls


def test_wide_networks_golden_through_wino1d(golden, wino1d_everywhere):
    """The nf = 128 NCSN++ and the BeatGANs U-Net against the REFERENCE's outputs with the GroupNorm-fed 3x3 convolutions on the row-wise F(4, 3)
    pair kernel (the form the benchmark runs on its 16 x 16 and 32 x 32 levels): NET_RTOL, as every other route; IDIFF_NO_WINO1D puts the same
    layers back on the 2-D pair kernel."""
    z = golden("ncsnpp_wide.npz")
    model = mutils.create_model(ncsnpp_config(**overrides_from_golden(z)))
    fill_from_seed(model, int(z["seed"]))
    model.to(DEV)
    model._invalidate()
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    raw = model(x, t * 999)
    assert wino1d_everywhere["n"] >= 8, wino1d_everywhere
    assert rel_err(raw.cpu(), z["model_out"]) < NET_RTOL
    n1 = wino1d_everywhere["n"]
    model._invalidate()
    with _lib.thread_option("IDIFF_NO_WINO1D", 1):
        raw2 = model(x, t * 999)
    assert wino1d_everywhere["n"] == n1                                  # the switch took them off the row-wise kernel
    assert rel_err(raw2.cpu(), z["model_out"]) < NET_RTOL
    assert rel_err(raw.cpu(), raw2.cpu()) < 1e-5 and not torch.equal(raw, raw2)     # two different kernels, the same function
    zb = golden("beatgans_wide.npz")
    mb = mutils.create_model(beatgans_config(**overrides_from_golden(zb)))
    fill_from_seed(mb, int(zb["seed"]))
    mb.to(DEV)
    mb._invalidate()
    before = wino1d_everywhere["n"]
    out = mb(torch.from_numpy(zb["x"]).to(DEV), torch.from_numpy(zb["t"]).to(DEV) * 999)
    assert wino1d_everywhere["n"] - before >= 4, wino1d_everywhere
    assert rel_err(out.cpu(), zb["model_out"]) < NET_RTOL


def _scaled_gamma_pair(z, factor, which="GroupNorm_1.weight"):
    """(oracle model, HIP model on the GPU, name) of the nf = 128 golden configuration with ONE GroupNorm's gamma multiplied by `factor`."""
    cfg = ncsnpp_config(**overrides_from_golden(z))
    ref_model = omodels.create_model(cfg)
    fill_from_seed(ref_model, int(z["seed"]))
    sd = ref_model.state_dict()
    name = next(k for k in sd if k.endswith(which))
    with torch.no_grad():
        sd[name].mul_(factor)
    ref_model.load_state_dict(sd)
    ref_model.eval()
    model = mutils.create_model(cfg)
    model.load_state_dict(sd)
    return cfg, ref_model, model.to(DEV).eval(), name


def test_out_of_range_groupnorm_is_routed_to_fp32_at_pack_time(golden, wino43_everywhere, factor=500.0):
    """VERDICT r4 #2 / ADVICE: the fp16-pair route is taken per LAYER only when that layer's gamma / beta keep the transformed input
    inside fp16's range (base.HipScoreModel.pairs_admissible).  A checkpoint with one GroupNorm's gamma x 500 gets exactly that
    layer's convolution on the fp32 contraction, with a warning, and the score agrees with the oracle's at NET_RTOL -- the reference evaluates any checkpoint in fp32 (models/layerspp.py:242-274)."""
    z = golden("ncsnpp_wide.npz")
    x, t = torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    _, ref_plain, model_plain, _ = _scaled_gamma_pair(z, 1.0)
    model_plain(x.to(DEV), (t * 999).to(DEV))
    plain = dict(wino43_everywhere)
    cfg, ref_model, model, name = _scaled_gamma_pair(z, factor)
    with pytest.warns(UserWarning, match="runs on the fp32 route"):
        raw = model(x.to(DEV), (t * 999).to(DEV))
    scaled = {k: wino43_everywhere[k] - plain[k] for k in plain}
    assert scaled["n"] == plain["n"] and scaled["pairs"] == plain["pairs"] - 1, (plain, scaled, name)   # one layer moved, same kernel family
    with torch.no_grad():
        ref = ref_model(x, t * 999)
    assert bool(torch.isfinite(raw).all()) and rel_err(raw.cpu(), ref) < NET_RTOL
    # a second forward does not warn again (decided once per layer, kept in the pack)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model(x.to(DEV), (t * 999).to(DEV))
    # the rule itself: bound = (sqrt(group elements) max|gamma| + max|beta|) x FIR gain x 29.34 (transform) < 60000, tensor scale >= 2^-6
    from id_diff_amd.models import base
    def gn_with(gamma):                                     # the verdict is kept per module in the pack: a fresh module per question
        g = torch.nn.GroupNorm(32, 128).to(DEV)
        with torch.no_grad():
            g.weight.fill_(gamma)
        return g
    gn = gn_with(1.0)
    assert model.pairs_admissible(gn, 4 * 1024) and model.pairs_admissible(gn, 16 * 1024, gain=1.0)       # gamma 1: 29.34 x 128 = 3756
    gn = gn_with(17.0)
    with pytest.warns(UserWarning):
        assert not model.pairs_admissible(gn, 16 * 1024)                                                   # 29.34 x 128 x 17 = 63.8k
    assert model.pairs_admissible(gn, 16 * 1024, transform=False) and model.pairs_admissible(gn_with(17.0), 16 * 1024, modulated=True)
    with pytest.warns(UserWarning):
        assert not model.pairs_admissible(gn_with(1e-3), 4 * 1024)                                         # the whole tensor below 2^-6
    assert abs(base.F43_INPUT_GAIN - 29.34) < 0.01


def test_non_finite_point_is_rebuilt_on_the_fp32_route(golden, wino43_everywhere, monkeypatch):
    """The second line of defence (the modulated norms of BeatGANs have no pack-time bound): with the bound check switched OFF, a
    gamma x 1e5 layer overflows the pair kernel, the point's S comes back NaN, and SpectrumPipeline builds the point ONCE more under
    IDIFF_NO_WINO43H / IDIFF_NO_PAIRS (ScoreMatrixBuilder.build(safe=True)) instead of raising: finite spectrum, a warning, rows equal
    to the oracle's at NET_RTOL."""
    from id_diff_amd.models import base
    monkeypatch.setattr(base, "PAIRS_BOUND_CHECK", False)
    z = golden("ncsnpp_wide.npz")
    cfg, ref_model, model, _ = _scaled_gamma_pair(z, 1e5)
    sde = sde_lib.VESDE(0.01, 50, 1000)
    builder = dim_reduction.ScoreMatrixBuilder(mutils.get_score_fn(sde, model), sde, 1e-5, torch.device(DEV))
    x0 = torch.from_numpy(z["x"])[0].to(DEV)
    B = 16                                                             # 3x8x8 sample: 64 // 16 + 1 = 5 -> 20 batches, 304 rows
    with torch.no_grad():
        S_bad = builder.build(x0, B, seed=77)
        assert not bool(torch.isfinite(S_bad).all())                   # the documented failure of the pair kernel: NaN, never finite-wrong
        pipe = dim_reduction.SpectrumPipeline(torch.device(DEV))
        pipe.submit(S_bad, rebuild=lambda: builder.build(x0, B, seed=77, safe=True))
        with pytest.warns(UserWarning, match="fp32 route"):
            (sv,) = pipe.results()
        assert pipe.rebuilt == 1 and bool(torch.isfinite(sv).all())
        S_ok = builder.build(x0, B, seed=77, safe=True)
        np.testing.assert_allclose(_lib.spectrum(S_ok, full=True).cpu().numpy(), sv.cpu().numpy(), rtol=1e-6)
        # rows of the safe build against the oracle on the same draws
        n = 8
        vec_t = torch.full((n,), 1e-5, device=DEV)
        _, std = sde.marginal_prob(torch.ones((), device=DEV), vec_t)
        batch, zz = torch.empty(n, x0.numel(), device=DEV), torch.empty(n, x0.numel(), device=DEV)
        _lib.perturb_randn(x0.reshape(-1).contiguous(), std.contiguous(), None, batch, n, x0.numel(), 0, 77, z_out=zz)
        ref_rows = osde.get_score_fn(osde.VESDE(0.01, 50, 1000), ref_model)(batch.cpu().view(n, *x0.shape), vec_t.cpu())
    assert rel_err(S_ok[:n].cpu(), ref_rows.reshape(n, -1)) < NET_RTOL
    # without a rebuild closure the old contract holds: a non-finite score matrix is an error, not a spectrum
    pipe2 = dim_reduction.SpectrumPipeline(torch.device(DEV))
    pipe2.submit(S_bad)
    with pytest.raises(RuntimeError, match="non-finite"):
        pipe2.results()


def test_wide_beatgans_golden_through_winograd43(golden, wino43_everywhere):
    z = golden("beatgans_wide.npz")
    model = mutils.create_model(beatgans_config(**overrides_from_golden(z)))
    fill_from_seed(model, int(z["seed"]))
    model.to(DEV)
    model._invalidate()
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    raw = model(x, t * 999)
    assert wino43_everywhere["n"] >= 4 and wino43_everywhere["pairs"] >= 4, wino43_everywhere
    assert rel_err(raw.cpu(), z["model_out"]) < NET_RTOL


def test_score_matrix_spectrum_and_id_through_winograd43(wino43_everywhere):
    """One whole point of the image recipe at nf = 64 (Winograd-eligible widths), 16x16 images, B = 100 -> S 1156 x 768, with the
    3x3 convolutions on F(4x4, 3x3): S against the oracle network on identical noise (NET_RTOL), spectrum against the oracle's
    fp32 SVD of the GPU's S at 1e-4, same integer ID as the oracle end to end."""
    cfg = ncsnpp_config(**{"model.init_scale": 1.0, "model.nf": 64, "model.attn_resolutions": (8,), "data.image_size": 16,
                           "data.effective_image_size": 16, "data.shape": [3, 16, 16], "model.num_res_blocks": 1})
    torch.manual_seed(0)
    ref_model = omodels.create_model(cfg)
    model = mutils.create_model(cfg)
    model.load_state_dict(ref_model.state_dict())
    model.to(DEV)
    x = torch.rand(3, 16, 16, generator=torch.Generator().manual_seed(1))
    sde_c, sde_h = osde.VESDE(0.01, 50, 1000), sde_lib.VESDE(0.01, 50, 1000)
    S, S_ref = _pipeline_pair(mutils.get_score_fn(sde_h, model), osde.get_score_fn(sde_c, ref_model), sde_h, sde_c, x, 100, 1e-5)
    assert wino43_everywhere["n"] > 0
    assert S.shape == (1156, 768) and rel_err(S.cpu(), S_ref) < NET_RTOL
    sv = _lib.spectrum(S).cpu()
    ref64 = odim.spectrum_f64(S.cpu())
    keep = ref64 > 2e-5 * ref64[0]
    np.testing.assert_allclose(sv.numpy()[keep], odim.spectrum(S.cpu()).numpy()[keep], rtol=1e-4)
    assert plot_utils.estimate_dim(sv.tolist()) == odim.estimate_dim(odim.spectrum(S_ref).tolist())


def test_wide_beatgans_golden(golden):
    z = golden("beatgans_wide.npz")
    model = mutils.create_model(beatgans_config(**overrides_from_golden(z)))
    fill_from_seed(model, int(z["seed"]))
    np.testing.assert_allclose(weight_abs_sums(model), z["weight_abs_sums"], rtol=1e-12)
    model.to(DEV)
    model._invalidate()
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    raw = model(x, t * 999)
    assert rel_err(raw.cpu(), z["model_out"]) < NET_RTOL
    y = mutils.get_score_fn(sde_lib.VESDE(0.01, 50, 1000), model)(x, t)
    assert rel_err(y.cpu(), z["score"]) < NET_RTOL


def test_vp_score_fn_golden(golden):
    """VP branch of get_score_fn (models/utils.py:238-255) on the GPU against the reference's output, and the VP
    perturbation (mean coefficient path of idiff_perturb_f32) against the reference's mean + std * z."""
    z = golden("ncsnpp_vp.npz")
    w = golden(str(z["weights_of"]))
    cfg = ncsnpp_config(**overrides_from_golden(w))
    cfg.training.sde = "vpsde"
    cfg.model.beta_min, cfg.model.beta_max = 0.1, 20.
    model = mutils.create_model(cfg)
    model.load_state_dict(state_dict_from_golden(w))
    model.to(DEV)
    sde, eps = sde_lib.configure_sde(cfg)
    assert isinstance(sde, sde_lib.VPSDE) and eps == 1e-3
    t = torch.from_numpy(z["t"]).to(DEV)
    y = mutils.get_score_fn(sde, model)(torch.from_numpy(z["perturbed"]).to(DEV), t)
    assert rel_err(y.cpu(), z["score"]) < NET_RTOL
    # the driver's perturbation of ONE sample repeated over the rows (dim_reduction.py:167, 180-182), VP: mean = coeff * x
    x0 = torch.from_numpy(z["x"][0]).to(DEV)
    noise = torch.from_numpy(z["z"]).to(DEV).reshape(4, -1).contiguous()
    mean_unit, std = sde.marginal_prob(torch.ones((), device=DEV), t)
    out = torch.empty(4, x0.numel(), device=DEV)
    _lib.perturb(x0.reshape(-1).contiguous(), noise, std.contiguous(), mean_unit.reshape(-1).contiguous(), out, 4, x0.numel())
    ref_mean, ref_std = osde.VPSDE(0.1, 20., 1000).marginal_prob(torch.from_numpy(z["x"][:1]).repeat(4, 1, 1, 1), t.cpu())
    ref = ref_mean + ref_std[:, None, None, None] * torch.from_numpy(z["z"])
    torch.testing.assert_close(out.cpu().reshape(ref.shape), ref, rtol=2e-6, atol=2e-6)


def test_snr_score_fn_golden(golden):
    """SNR branch of get_score_fn (models/utils.py:270-277) on the GPU against the REFERENCE's output
    (tests/golden/ncsnpp_snr.npz), and the driver's SNR perturbation mean = alpha(t) x (sde_lib.py:175-180) through the
    mean-coefficient path of idiff_perturb_f32 against the reference's mean + std * z."""
    z = golden("ncsnpp_snr.npz")
    w = golden(str(z["weights_of"]))
    cfg = ncsnpp_config(**overrides_from_golden(w))
    cfg.training.sde = "snrsde"
    model = mutils.create_model(cfg)
    model.load_state_dict(state_dict_from_golden(w))
    model.to(DEV)
    sde, eps = sde_lib.configure_sde(cfg)
    assert type(sde) is sde_lib.SNRSDE and eps == 1e-3
    t = torch.from_numpy(z["t"]).to(DEV)
    y = mutils.get_score_fn(sde, model)(torch.from_numpy(z["perturbed"]).to(DEV), t)
    assert rel_err(y.cpu(), z["score"]) < NET_RTOL
    for i in range(4):                       # row i: sample i perturbed at t[i], as the driver does for one point's rows
        x0 = torch.from_numpy(z["x"][i]).to(DEV)
        noise = torch.from_numpy(z["z"][i:i + 1]).to(DEV).reshape(1, -1).contiguous()
        mean_unit, std = sde.marginal_prob(torch.ones((), device=DEV), t[i:i + 1])
        out = torch.empty(1, x0.numel(), device=DEV)
        _lib.perturb(x0.reshape(-1).contiguous(), noise, std.contiguous(), mean_unit.reshape(-1).contiguous(), out, 1, x0.numel())
        torch.testing.assert_close(out.cpu().reshape(z["perturbed"][i].shape), torch.from_numpy(z["perturbed"][i]), rtol=2e-6, atol=2e-6)


def test_snr_score_matrix_and_spectrum_vs_oracle(golden):
    """The whole per-point recipe under the SNR SDE at its sampling_eps = 1e-3: HIP score matrix against the oracle's on
    identical noise, spectrum at the 1e-4 bar, same integer ID."""
    z = golden("conditional.npz")                                  # 16x16 nf=8 NCSN++ with stored weights
    cfg = ncsnpp_config(**overrides_from_golden(z))
    ref_model = omodels.create_model(cfg)
    ref_model.load_state_dict(state_dict_from_golden(z))
    model = mutils.create_model(cfg)
    model.load_state_dict(state_dict_from_golden(z))
    model.to(DEV)
    x = torch.from_numpy(z["val_images"][2])
    sde_c, sde_h = osde.SNRSDE(1000), sde_lib.SNRSDE(1000)
    S, S_ref = _pipeline_pair(mutils.get_score_fn(sde_h, model), osde.get_score_fn(sde_c, ref_model), sde_h, sde_c, x, 100, 1e-3)
    assert S.shape == (1156, 768) and rel_err(S.cpu(), S_ref) < NET_RTOL
    sv = _lib.spectrum(S).cpu()
    ref64 = odim.spectrum_f64(S.cpu())
    keep = ref64 > 2e-5 * ref64[0]
    np.testing.assert_allclose(sv.numpy()[keep], odim.spectrum(S.cpu()).numpy()[keep], rtol=1e-4)
    assert plot_utils.estimate_dim(sv.tolist()) == odim.estimate_dim(odim.spectrum(S_ref).tolist())


def test_concurrent_launch_sets_give_the_same_score_matrix(golden):
    """ScoreMatrixBuilder(concurrent_sets=2) (opt-in): the launch sets of a point on two worker streams -- same kernels on
    the same inputs, so S is the sequential S bit for bit (in-kernel noise keyed by the row, explicit noise by index)."""
    cfg = ncsnpp_config(init_scale=1.)               # init_scale = 0 would zero the output conv: a score matrix of zeros
    cfg.model.allow_random_init = True
    torch.manual_seed(3)
    model = mutils.create_model(cfg).to(DEV)
    sde, eps = sde_lib.configure_sde(cfg)
    score_fn = mutils.get_score_fn(sde, model)
    x = torch.rand(cfg.data.num_channels, cfg.data.image_size, cfg.data.image_size, device=DEV)
    seq = dim_reduction.ScoreMatrixBuilder(score_fn, sde, eps, torch.device(DEV), inflight_rows=48, concurrent_sets=1)
    con = dim_reduction.ScoreMatrixBuilder(score_fn, sde, eps, torch.device(DEV), inflight_rows=48, concurrent_sets=2)
    ref = seq.build(x, 32, seed=11)
    con.build(x, 32, seed=5)                        # the first point of a builder warms the lazily made banks on one stream
    assert con._warmed and torch.equal(con.build(x, 32, seed=11), ref) and con._workers is not None
    noise = torch.randn(ref.shape, device=DEV)
    assert torch.equal(con.build(x, 32, noise=noise), seq.build(x, 32, noise=noise))


def test_subvp_score_fn_vs_oracle(golden):
    """config.training.sde = 'subvpsde' (BaseSdeGenerativeModel.py:33-35): the VP branch of get_score_fn with
    std = 1 - exp(2 log_mean_coeff); the oracle's restatement is pinned by the reference's own marginal_prob
    (tests/golden/sde_extra.npz), the network by the stored reference weights."""
    z = golden("ncsnpp_vp.npz")
    w = golden(str(z["weights_of"]))
    cfg = ncsnpp_config(**overrides_from_golden(w))
    cfg.training.sde = "subvpsde"
    cfg.model.beta_min, cfg.model.beta_max = 0.1, 20.
    model = mutils.create_model(cfg)
    model.load_state_dict(state_dict_from_golden(w))
    ref_model = omodels.create_model(cfg)
    ref_model.load_state_dict(state_dict_from_golden(w))
    sde, eps = sde_lib.configure_sde(cfg)
    assert type(sde) is sde_lib.subVPSDE and eps == 1e-3
    model.to(DEV)
    x, t = torch.from_numpy(z["perturbed"]), torch.from_numpy(z["t"])
    y = mutils.get_score_fn(sde, model)(x.to(DEV), t.to(DEV))
    with torch.no_grad():
        ref = osde.get_score_fn(osde.make_sde(cfg)[0], ref_model)(x, t)
    assert rel_err(y.cpu(), ref) < NET_RTOL


def test_vp_score_matrix_and_spectrum_vs_oracle(golden):
    """The whole per-point recipe under the VP SDE at its sampling_eps = 1e-3 (BaseSdeGenerativeModel.py:44-47): HIP
    score matrix against the oracle's on identical noise, spectrum at the 1e-4 bar, same integer ID."""
    z = golden("conditional.npz")                                  # 16x16 nf=8 NCSN++ with stored weights
    cfg = ncsnpp_config(**overrides_from_golden(z))
    ref_model = omodels.create_model(cfg)
    ref_model.load_state_dict(state_dict_from_golden(z))
    model = mutils.create_model(cfg)
    model.load_state_dict(state_dict_from_golden(z))
    model.to(DEV)
    x = torch.from_numpy(z["val_images"][2])
    sde_c, sde_h = osde.VPSDE(0.1, 20., 1000), sde_lib.VPSDE(0.1, 20., 1000)
    S, S_ref = _pipeline_pair(mutils.get_score_fn(sde_h, model), osde.get_score_fn(sde_c, ref_model), sde_h, sde_c, x, 100, 1e-3)
    assert S.shape == (1156, 768) and rel_err(S.cpu(), S_ref) < NET_RTOL
    sv = _lib.spectrum(S).cpu()
    ref64 = odim.spectrum_f64(S.cpu())
    keep = ref64 > 2e-5 * ref64[0]
    np.testing.assert_allclose(sv.numpy()[keep], odim.spectrum(S.cpu()).numpy()[keep], rtol=1e-4)
    assert plot_utils.estimate_dim(sv.tolist()) == odim.estimate_dim(odim.spectrum(S_ref).tolist())


def test_conditional_manifold_dimension_vs_reference(golden):
    """get_conditional_manifold_dimension (dim_reduction.py:12-114) against the REFERENCE's own function: same model,
    same labelled validation batch, and the same noise -- the reference consumed torch's global CPU generator in the
    order (level, point, batch); the test replays that stream and hands it to the HIP driver.  Three of the twelve
    levels (first, middle, last), both label-1 points: spectra within 1e-4, integer IDs equal."""
    z = golden("conditional.npz")
    cfg = ncsnpp_config(**overrides_from_golden(z))
    model = mutils.create_model(cfg)
    model.load_state_dict(state_dict_from_golden(z))
    model.to(DEV)
    sde = sde_lib.VESDE(0.01, 50, 1000)
    builder = dim_reduction.ScoreMatrixBuilder(mutils.get_score_fn(sde, model), sde, 1e-5, torch.device(DEV))
    images, labels = torch.from_numpy(z["val_images"]), torch.from_numpy(z["val_labels"])
    B = images.shape[0]
    num_batches, _, rows = odim.batching(tuple(images.shape[1:]), B)
    levels = (0, 5, 11)
    noise = replay_conditional_noise(int(z["seed"]), 12, 2, num_batches, (B, *images.shape[1:]), rows, levels)
    out = dim_reduction.conditional_spectra(builder, [(images, labels)], int(z["num_datapoints"]), levels=levels,
                                            noise=lambda level, point: noise[(level, point)])
    assert [lv["level"] for lv in out] == list(levels)
    for lv in out:
        ref = z["singular_values"][lv["level"]]
        assert '%.3f' % lv["t"] == str(z["level_dirs"][lv["level"]])
        assert lv["labels"] == z["labels"][lv["level"]].tolist()
        np.testing.assert_array_equal(lv["images"], z["images_pkl"])
        got = np.array(lv["singular_values"])
        assert got.shape == ref.shape == (2, 768)
        # 1e-4 relative (north star) above the floor of the reference's own arithmetic: its fp32 gesdd is only good to
        # ~3e-7 * sigma_max absolute (measured on this fixture against an fp64 SVD of the same S: 2.7e-7), and the
        # two fp32 networks differ by summation order (a 5e-6 elementwise change of S moves the smallest singular
        # values by up to 8e-4 relative) -- the same-input 1e-4 bar is held by tests/test_hip_spectrum.py
        for a, b in zip(got, ref):
            np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6 * b[0])
            assert plot_utils.estimate_dim(a.tolist()) == odim.estimate_dim(b.tolist())
    # one (level, point) with the perturbation made explicit: the oracle's S on the same draws, then Weyl's bound
    ref_model = omodels.create_model(cfg)
    ref_model.load_state_dict(state_dict_from_golden(z))
    sde_c = osde.VESDE(0.01, 50, 1000)
    lvl, t_lvl = levels[1], float(odim.conditional_times(1e-5)[levels[1]])
    pts = dim_reduction.collect_labelled_points([(images, labels)], int(z["num_datapoints"]))
    x0 = pts[0][0]
    nz = noise[(lvl, 0)]
    pad = torch.zeros(num_batches * B - rows, *x0.shape)
    S_ref = odim.score_matrix(osde.get_score_fn(sde_c, ref_model), sde_c, x0, B, t_lvl,
                              noise=torch.cat([nz, pad]).reshape(num_batches, B, *x0.shape))
    S = builder.build(x0.to(DEV), B, t=t_lvl, noise=nz.to(DEV))
    assert rel_err(S.cpu(), S_ref) < NET_RTOL
    bound = float(torch.linalg.matrix_norm(S.cpu().double() - S_ref.double(), ord=2))
    sv = _lib.spectrum(S).cpu().double()
    assert float((sv - odim.spectrum_f64(S_ref)).abs().max()) <= 1.5 * bound + 1e-7 * float(sv[0])
