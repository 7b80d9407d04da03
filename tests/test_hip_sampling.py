"""GPU tests of the sampling feature: the two kernels of csrc/sampler.hip element-wise against fp64, the generated noise bit for bit
against idiff_perturb_randn_f32, every trajectory of the reference's sampler (tests/golden/sampling.npz) replayed on both execution
paths, reverse diffusion through the exact empirical score landing on the cloud, and a trained fcn generating the sphere it learnt."""
import os

import numpy as np
import pytest
import torch

import sampling_cases as sc
from id_diff_amd import _lib, sampling, sde_lib, train
from id_diff_amd.configs.config_dict import ConfigDict
from id_diff_amd.configs.utils import read_config
from id_diff_amd.models.fcn import FCN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SMALL_CONFIG = 'configs/dimension_estimation/paper/euclidean_data/ksphere/train_small.py'


@pytest.fixture(scope="module")
def fx():
    return sc.load()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


def padded(rows, pitch):
    """[B, D] -> a sentinel-filled [B, pitch] device buffer holding the rows in its first D columns."""
    buf = np.full((rows.shape[0], pitch), sc.SENTINEL, dtype=np.float32)
    buf[:, :rows.shape[1]] = rows
    return dev(buf)


def generated(B, D, seed, row0=0):
    """What FcnTrainer.draw gets from the library's generator for [B, pad4(D)]: the z the step kernel must reproduce, [B, D]."""
    D4 = (D + 3) // 4 * 4
    zeros, ones = torch.zeros(1, D4, device=DEV), torch.ones(B, device=DEV)
    scratch, z = torch.empty(B, D4, device=DEV), torch.empty(B, D4, device=DEV)
    _lib.perturb_randn(zeros, ones, None, scratch, B, D4, row0, seed, z_out=z)
    return z[:, :D].contiguous()


# ---------------------------------------------------------------------------------------------- 1. the step kernel
@pytest.mark.parametrize("with_mean", [True, False], ids=["mean", "nomean"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("shape", sc.STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_kernel_against_fp64(shape, in_place, with_mean):
    B, D, pitch = shape
    rng = np.random.default_rng([3, B, D, pitch])
    x, s, z = (rng.standard_normal((B, D)).astype(np.float32) * k for k in (np.float32(3.0), np.float32(0.5), np.float32(1.0)))
    a, b, c = 0.9371, -0.4182, 1.2345
    xd, sd, zd = padded(x, pitch), padded(s, pitch), padded(z, pitch)
    out = xd if in_place else padded(np.full((B, D), sc.SENTINEL, dtype=np.float32), pitch)
    mean = padded(np.full((B, D), sc.SENTINEL, dtype=np.float32), pitch) if with_mean else None
    label_col = D if pitch > D else -1
    _lib.sampler_step(xd, sd, a, b, c, z=zd, out=out, mean_out=mean, D=D, label_col=label_col, label_value=38.5)
    ax, bs, cz = a * x.astype(np.float64), b * s.astype(np.float64), c * z.astype(np.float64)
    want_m, want = ax + bs, ax + bs + cz
    got = out.cpu().numpy()
    share = float((np.abs(got[:, :D] - want) / sc.step_bound(want, ax, bs, cz)).max())
    if with_mean:
        gm = mean.cpu().numpy()
        share = max(share, float((np.abs(gm[:, :D] - want_m) / sc.step_bound(want_m, ax, bs, 0 * cz)).max()))
        assert np.all(gm[:, D:] == np.float32(sc.SENTINEL))                   # the mean's pad columns are nobody's
    print(f"step {shape} inplace={in_place} mean={with_mean}: {share:.3f} of the bound")
    assert share <= 1.0
    pad = got[:, D:]
    if label_col >= 0:
        assert np.all(pad[:, 0] == np.float32(38.5))                          # written in every row
        pad = pad[:, 1:]
    assert np.all(pad == np.float32(sc.SENTINEL))                             # and nothing else in the pad columns touched
    assert np.array_equal(sd.cpu().numpy()[:, :D], s) and np.array_equal(zd.cpu().numpy()[:, :D], z)
    if not in_place:
        assert np.array_equal(xd.cpu().numpy()[:, :D], x)


# ---------------------------------------------------------------------------------------------- 2. generated noise
@pytest.mark.parametrize("D", [6, 100])
def test_generated_noise_is_the_library_s_stream(D):
    B, seed = 64, 0x1234_5678_9ABC
    zeros = torch.zeros(B, D, device=DEV)
    out = torch.full((B, D), sc.SENTINEL, device=DEV)
    _lib.sampler_step(zeros, zeros, 0.0, 0.0, 1.0, out=out, seed=seed)
    want = generated(B, D, seed)
    assert torch.equal(out, want)
    # 64 rows in one launch = 2 x 32 rows with row0 = 0, 32
    halves = torch.full((B, D), sc.SENTINEL, device=DEV)
    for r0 in (0, 32):
        _lib.sampler_step(zeros[r0:r0 + 32], zeros[r0:r0 + 32], 0.0, 0.0, 1.0, out=halves[r0:r0 + 32], seed=seed, row0=r0)
    assert torch.equal(halves, out)
    assert torch.equal(generated(32, D, seed, row0=32), out[32:])
    other = torch.empty(B, D, device=DEV)
    _lib.sampler_step(zeros, zeros, 0.0, 0.0, 1.0, out=other, seed=seed + 1)
    assert not torch.equal(other, out)
    z = out.double()
    assert abs(float(z.mean())) < 5 / np.sqrt(B * D) and abs(float(z.var()) - 1) < 0.2


def test_no_noise_without_a_coefficient_for_it():
    B, D = 33, 100
    g = torch.Generator(device=DEV).manual_seed(5)
    x, s = torch.randn(B, D, device=DEV, generator=g), torch.randn(B, D, device=DEV, generator=g)
    out, mean = torch.empty(B, D, device=DEV), torch.empty(B, D, device=DEV)
    _lib.sampler_step(x, s, 0.75, 0.3, 0.0, out=out, mean_out=mean, seed=9)                    # nothing drawn
    assert torch.equal(out, mean)
    poisoned = torch.full((B, D), float('nan'), device=DEV)
    out2 = torch.empty(B, D, device=DEV)
    _lib.sampler_step(x, s, 0.75, 0.3, 0.0, z=poisoned, out=out2)                              # and a given z is not read
    assert torch.equal(out2, mean)
    want = 0.75 * x.double() + 0.3 * s.double()
    assert float(((mean.double() - want).abs() / (sc.U * want.abs() + 2.0 ** -149)).max()) <= 1.0 + 2.0 ** -20


# ---------------------------------------------------------------------------------------------- 3. the noise norm and the Langevin form
@pytest.mark.parametrize("shape", sc.NORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_noise_norm_and_langevin_form(shape):
    B, D = shape
    rng = np.random.default_rng([4, B, D])
    z = rng.standard_normal((B, D)).astype(np.float32)
    want = np.sqrt((z.astype(np.float64) ** 2).sum(axis=1)).mean()
    got = float(_lib.sampler_noise_norm(dev(z)).cpu())
    print(f"noise norm {shape}: explicit {abs(got - want) / want / sc.norm_rtol(B, D):.3f} of the bar")
    assert abs(got - want) <= sc.norm_rtol(B, D) * want
    zp = padded(z, D + 3)                                                                       # a pitch that is not D
    assert float(_lib.sampler_noise_norm(zp, D=D).cpu()) == got
    seed = 77
    zg = generated(B, D, seed).cpu().numpy()
    want_g = np.sqrt((zg.astype(np.float64) ** 2).sum(axis=1)).mean()
    nn = _lib.sampler_noise_norm(None, B=B, D=D, seed=seed, device=torch.device(DEV))
    got_g = float(nn.cpu())
    print(f"noise norm {shape}: regenerated {abs(got_g - want_g) / want_g / sc.norm_rtol(B, D):.3f} of the bar")
    assert abs(got_g - want_g) <= sc.norm_rtol(B, D) * want_g
    # the Langevin form reads that device double: a = 1, b = lang_scale nn^2 score_scale, c = sqrt(2 lang_scale nn^2)
    x, s = rng.standard_normal((B, D)).astype(np.float32), rng.standard_normal((B, D)).astype(np.float32)
    lang_scale, score_scale = 2 * 0.93 * 0.15 ** 2, -1.7
    for zz, zdev in ((zg, None), (z, dev(z))):
        nn_dev = nn if zdev is None else _lib.sampler_noise_norm(zdev)
        n = float(nn_dev.cpu())
        out, mean = torch.empty(B, D, device=DEV), torch.empty(B, D, device=DEV)
        _lib.sampler_step(dev(x), dev(s), 5.0, 5.0, 5.0, z=zdev, out=out, mean_out=mean, seed=seed, noise_norm=nn_dev,
                          lang_scale=lang_scale, score_scale=score_scale)
        b, c = lang_scale * n * n * score_scale, np.sqrt(2 * lang_scale * n * n)
        ax, bs, cz = x.astype(np.float64), b * s.astype(np.float64), c * zz.astype(np.float64)
        assert float((np.abs(out.cpu().numpy() - (ax + bs + cz)) / sc.step_bound(ax + bs + cz, ax, bs, cz)).max()) <= 1.0
        assert float((np.abs(mean.cpu().numpy() - (ax + bs)) / sc.step_bound(ax + bs, ax, bs, 0 * cz)).max()) <= 1.0


# ---------------------------------------------------------------------------------------------- 4. trajectories against the reference
def fixture_model(fx, kind):
    model = FCN(sc.fcn_config(kind))
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sc.weights(fx).items()})
    return model.to(DEV).eval()


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_trajectories_follow_the_reference(fx, case):
    """Both paths replay the fixture's draws; per time step the state stays within max(16 x the fixture's own |fp32 - fp64|,
    2^-20 max|x|) of the fp64 trajectory, the samples likewise, and the two paths agree within the same bar.  Measured: states at most
    0.160 of the bar (ve-reverse_diffusion-langevin), samples 0.139, the two paths 0.096 apart."""
    kind, pred, corr, pf = case
    sde, tr = sc.make_sde(kind), sc.trajectory(fx, case)
    model = fixture_model(fx, kind)
    sampler = sampling.get_pc_sampler(sde, (sc.B, sc.D), sampling.get_predictor(pred), sampling.get_corrector(corr), sc.SNR, n_steps=1,
                                      probability_flow=pf, continuous=True, denoise=True, eps=sc.EPS[kind])
    ks = [k for k, (_, which) in enumerate(sc.updates(case)) if which == 'predictor']
    gap = np.abs(tr['x32'].astype(np.float64) - tr['x64']).max(axis=(1, 2))[ks]
    bar = np.maximum(sc.TRAJ_FACTOR * gap, sc.TRAJ_FLOOR * np.abs(tr['x64'][ks]).max(axis=(1, 2)))
    gap_m = np.abs(tr['xm32'][-1].astype(np.float64) - tr['xm64'][-1]).max()
    bar_m = max(sc.TRAJ_FACTOR * gap_m, sc.TRAJ_FLOOR * np.abs(tr['xm64'][-1]).max())
    runs = {}
    for name, fast in (('generic', False), ('fcn', True)):
        samples, info = sampler(model, show_evolution=True, noise=(fx["prior_z"], tr['draws']), fast=fast)
        evo = info['evolution'].numpy().astype(np.float64)
        assert evo.shape == (sc.N_STEPS, sc.B, sc.D) and info['steps'] == sc.N_STEPS * 2 and len(info['times']) == sc.N_STEPS
        assert np.isfinite(evo).all()
        share = float((np.abs(evo - tr['x64'][ks]).max(axis=(1, 2)) / bar).max())
        share_m = float(np.abs(samples.cpu().numpy().astype(np.float64) - tr['xm64'][-1]).max() / bar_m)
        print(f"{sc.case_id(case)} {name}: states {share:.3f}, samples {share_m:.3f} of the bar")
        assert share <= 1.0 and share_m <= 1.0
        runs[name] = (evo, samples.cpu().numpy().astype(np.float64))
    between = float((np.abs(runs['generic'][0] - runs['fcn'][0]).max(axis=(1, 2)) / bar).max())
    print(f"{sc.case_id(case)} generic vs fcn: {between:.3f} of the bar")
    assert between <= 1.0 and np.abs(runs['generic'][1] - runs['fcn'][1]).max() <= bar_m


@pytest.mark.parametrize("fast", [True, False], ids=["fcn", "generic"])
def test_no_host_synchronisation_inside_the_sampler(fx, fast):
    """A second call of a sampler (its time grid and buffers are in place) with generated noise and the Langevin corrector, whose step
    size depends on the noise drawn: torch's synchronisation check stays silent on both paths, and the bits repeat."""
    model = fixture_model(fx, 've')
    sampler = sampling.get_pc_sampler(sc.make_sde('ve'), (33, sc.D), 'reverse_diffusion', 'langevin', sc.SNR, n_steps=2, continuous=True,
                                      eps=sc.EPS['ve'])
    first, _ = sampler(model, seed=3, fast=fast)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again, info = sampler(model, seed=3, fast=fast)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert info['steps'] == sc.N_STEPS * 3 and bool(torch.isfinite(again).all()) and torch.equal(again, first)


# ---------------------------------------------------------------------------------------------- 5. acceptance without a checkpoint
def test_reverse_diffusion_through_the_exact_score_lands_on_the_cloud(fx):
    """empirical_exact is exact at every noise level, so the sampler must end on the cloud: every sample within 3 x the largest
    nearest-point distance the reference's sampler reached on this cloud (an extreme of 128 draws, other noise), which is below half
    the neighbour spacing.  The prior alone sits at sigma_max sqrt(8) = 5.7.  Measured: 2.00e-3 at worst against a bar of 5.95e-3."""
    from id_diff_amd.models.empirical_exact import EmpiricalExact
    cloud = fx["emp::cloud"]
    sigma_min, sigma_max, N, n = (float(v) for v in fx["emp::params"])
    bar = 3.0 * float(fx["emp::max_dist"])
    assert bar < 0.5 * float(fx["emp::spacing"])
    config = ConfigDict()
    config.model = ConfigDict(name='empirical_exact', sigma_min=sigma_min, sigma_max=sigma_max, num_scales=int(N))
    config.data = ConfigDict(noise_std=0.0, shape=[cloud.shape[1]])
    config.training = ConfigDict(sde='vesde', continuous=True)
    model = EmpiricalExact(config, data=cloud).to(DEV)
    model.ess_warn = 0                                   # below the spacing one point holds all the weight: that is the test
    sde = sde_lib.VESDE(sigma_min=sigma_min, sigma_max=sigma_max, N=int(N))
    sampler = sampling.get_pc_sampler(sde, (int(n), cloud.shape[1]), sampling.get_predictor('reverse_diffusion'), None, 0.15,
                                      continuous=True, denoise=True, eps=1e-5)
    samples, info = sampler(model, seed=0)
    got = samples.cpu().numpy()
    assert got.shape == (int(n), cloud.shape[1]) and np.isfinite(got).all()
    dist = sc.nearest_distance(got, cloud)
    print(f"nearest-point distance: max {dist.max():.3e}, mean {dist.mean():.3e}; bar {bar:.3e}; reference max {float(fx['emp::max_dist']):.3e}")
    assert dist.max() <= bar
    assert len(np.unique(np.argmin(((got[:, None] - cloud[None]) ** 2).sum(-1), axis=1))) > 32        # spread over the circle


# ---------------------------------------------------------------------------------------------- 6. it generates what it learnt
def test_trained_network_generates_the_sphere(tmp_path):
    """train_small for 8000 steps, then --mode generate's code path: the norms of 512 samples are finite with a mean in (0.5, 1.5)
    (the untouched prior has mean norm sigma_max sqrt(8) = 5.7, a collapsed sampler 0), and the same seed gives the same bits.
    Measured: min 0.738, mean 1.040, max 1.590."""
    config = read_config(SMALL_CONFIG)
    config.device = DEV
    config.logging.log_path = str(tmp_path)
    train.train(config, log_path=str(tmp_path), n_iters=8000, log=None)
    ckpt = train.last_checkpoint_path(config, str(tmp_path))
    lines = []
    samples, info = sampling.generate(config, checkpoint_path=ckpt, num_samples=512, seed=1, log_path=str(tmp_path), log=lines.append)
    print(lines[-1])
    assert samples.shape == (512, 8) and bool(torch.isfinite(samples).all())
    assert all(np.isfinite(info[k]) for k in ('min_norm', 'max_norm', 'mean_norm'))
    assert 0.5 < info['mean_norm'] < 1.5
    import pickle
    with open(info['path'], 'rb') as f:
        saved = pickle.load(f)
    assert saved['samples'].dtype == np.float32 and saved['samples'].shape == (512, 8) and saved['steps'] == 2000
    assert saved['mean_norm'] == info['mean_norm'] and len(saved['times']) == 1000
    again, _ = sampling.generate(config, checkpoint_path=ckpt, num_samples=512, seed=1, log_path=str(tmp_path), log=None)
    assert torch.equal(again, samples)
    other, _ = sampling.generate(config, checkpoint_path=ckpt, num_samples=512, seed=2, log_path=str(tmp_path), log=None)
    assert not torch.equal(other, samples)
    # the generic path draws the same stream and runs the same network through FCN.forward
    from id_diff_amd.lightning_modules.BaseSdeGenerativeModel import BaseSdeGenerativeModel
    module = BaseSdeGenerativeModel(config).load_from_checkpoint(ckpt).to(DEV).eval()
    module.configure_sde(config)
    sampler = sampling.get_sampling_fn(config, module.sde, [512, 8], module.sampling_eps)
    generic, _ = sampler(module.score_model, seed=1, fast=False)
    norms = sampling.ksphere_evaluation(generic)
    print(f"generic path: min {norms['min_norm']:.4f} mean {norms['mean_norm']:.4f} max {norms['max_norm']:.4f}")
    assert 0.5 < norms['mean_norm'] < 1.5


def test_fit_with_eval_every_logs_and_leaves_training_alone(tmp_path):
    config = read_config(SMALL_CONFIG)
    config.device = DEV
    config.logging.log_path = str(tmp_path)
    lines = []
    a = train.FcnTrainer(config, DEV)
    a.fit(200, checkpoint_path=str(tmp_path / "checkpoints" / "last.ckpt"), eval_every=100, log=lines.append)
    evals = [l for l in lines if 'mean_norm' in l]
    print("\n".join(evals))
    assert len(evals) == 2 and [s for s, _ in a.evaluations] == [100, 200]
    for _, e in a.evaluations:
        assert sorted(e) == ['dim', 'max_norm', 'mean_norm', 'min_norm'] and all(np.isfinite(v) for v in e.values())
    assert os.path.exists(str(tmp_path / "checkpoints" / "last.ckpt"))
    b = train.FcnTrainer(read_config(SMALL_CONFIG), DEV)
    b.fit(200, log=None)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and b.evaluations == []
