"""Host side of the sampling feature (no GPU): the (a, b, c) of id_diff_amd.sampling restate every predictor and corrector of the
reference (checked update by update against the fixture's fp64 trajectory), the table indices are the reference's, what the reference
cannot do is refused by name, the defaults of a config without a ``sampling`` section, the refusals of the two entry points before any
device call, and the argument handling of ``--mode generate``."""
import numpy as np
import pytest

import sampling_cases as sc
from id_diff_amd import _lib, main, run_lib, sampling, sde_lib
from id_diff_amd.configs.utils import read_config

SMALL_CONFIG = 'configs/dimension_estimation/paper/euclidean_data/ksphere/train_small.py'
COEFF_RTOL = 1e-6            # the reference forms its coefficients in fp32: 2^-24 = 6e-8 each, a handful per update


@pytest.fixture(scope="module")
def fx():
    return sc.load()


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_coefficients_reproduce_every_update_of_the_reference(fx, case):
    """x_mean = a x + b s, x = x_mean + c z in fp64 numpy from the fixture's own previous state, its draw and the fp64 score of its
    network: within 1e-6 max|x| of the fixture's fp64 x and x_mean of that update.  Measured largest share of the bar: 0.070
    (vp-ancestral_sampling, with and without langevin)."""
    kind, pred, corr, pf = case
    sde, w, tr = sc.make_sde(kind), sc.weights(fx), sc.trajectory(fx, case)
    times = fx[f"times::{kind}"]
    prev, worst = sc.prior_state(fx, kind), 0.0
    for k, (i, which) in enumerate(sc.updates(case)):
        t = float(times[i])
        z = tr['draws'][k].astype(np.float64)
        if which == 'predictor':
            a, b, c = sampling.predictor_coefficients(sde, pred, t, pf)
        else:
            nn = float(np.sqrt((z * z).sum(axis=1)).mean())
            a, b, c = sampling.corrector_coefficients(sde, corr, t, sc.SNR, noise_norm=nn)
        assert all(isinstance(v, float) for v in (a, b, c))
        s = sc.score64(w, sde, prev, t)
        xm = a * prev + b * s
        x = xm + c * z
        bar = COEFF_RTOL * np.abs(tr['x64'][k]).max()
        worst = max(worst, np.abs(x - tr['x64'][k]).max() / bar, np.abs(xm - tr['xm64'][k]).max() / bar)
        prev = tr['x64'][k]
    print(f"{sc.case_id(case)}: {worst:.3f} of the bar")
    assert worst <= 1.0


@pytest.mark.parametrize("kind", sorted(sc.SDE_PARAMS))
def test_table_indices_are_the_reference_s(fx, kind):
    sde = sc.make_sde(kind)
    grid = sampling.time_grid(sde, sc.EPS[kind])
    assert grid.dtype == np.float32 and np.array_equal(grid, fx[f"times::{kind}"])
    assert [sampling.table_index(sde, t) for t in grid] == fx[f"index::{kind}"].tolist()


def test_predictors_agree_where_the_reference_s_do():
    """SDE.discretize is Euler-Maruyama for VE and subVP, so reverse_diffusion and euler_maruyama are one update there; on VP they differ."""
    for kind in ('ve', 'subvp'):
        sde = sc.make_sde(kind)
        assert sampling.predictor_coefficients(sde, 'reverse_diffusion', 0.37) == pytest.approx(
            sampling.predictor_coefficients(sde, 'euler_maruyama', 0.37), rel=1e-15)
    vp = sc.make_sde('vp')
    assert sampling.predictor_coefficients(vp, 'reverse_diffusion', 0.37) != sampling.predictor_coefficients(vp, 'euler_maruyama', 0.37)
    a, b, c = sampling.predictor_coefficients(vp, 'euler_maruyama', 0.37, probability_flow=True)
    a1, b1, c1 = sampling.predictor_coefficients(vp, 'euler_maruyama', 0.37)
    assert (a, b, c) == (a1, 0.5 * b1, 0.0) and c1 > 0
    assert sampling.predictor_coefficients(vp, 'none', 0.5) == (1.0, 0.0, 0.0) == sampling.corrector_coefficients(vp, 'none', 0.5, 0.15)


def test_refusals():
    ve, vp, sub = (sc.make_sde(k) for k in ('ve', 'vp', 'subvp'))
    with pytest.raises(NotImplementedError, match="subVPSDE"):
        sampling.predictor_coefficients(sub, 'ancestral_sampling', 0.5)
    with pytest.raises(NotImplementedError, match="langevin.*subVPSDE"):
        sampling.corrector_coefficients(sub, 'langevin', 0.5, 0.15, noise_norm=2.0)
    with pytest.raises(NotImplementedError, match="ald.*subVPSDE"):
        sampling.corrector_coefficients(sub, 'ald', 0.5, 0.15)
    with pytest.raises(NotImplementedError, match="subVPSDE"):
        sampling.get_pc_sampler(sub, (4, 6), sampling.get_predictor('reverse_diffusion'), sampling.get_corrector('langevin'), 0.15)
    for sde in (ve, vp):
        with pytest.raises(ValueError, match="[Pp]robability flow"):
            sampling.predictor_coefficients(sde, 'ancestral_sampling', 0.5, probability_flow=True)
    with pytest.raises(ValueError, match="N = 12"):
        sampling.get_pc_sampler(sc.make_sde('vp', N=12), (4, 6), sampling.get_predictor('reverse_diffusion'), None, 0.15)
    with pytest.raises(ValueError, match="N = 12"):
        sampling.predictor_coefficients(sc.make_sde('vp', N=12), 'ancestral_sampling', 0.5)
    sampling.get_pc_sampler(sc.make_sde('vp', N=21), (4, 6), sampling.get_predictor('reverse_diffusion'), None, 0.15)
    with pytest.raises(ValueError, match="noise_norm"):
        sampling.corrector_coefficients(ve, 'langevin', 0.5, 0.15)
    for name, get in (('heun', sampling.get_predictor), ('mala', sampling.get_corrector), ('conditional_langevin', sampling.get_corrector)):
        with pytest.raises(NotImplementedError):
            get(name)
    with pytest.raises(KeyError):
        sampling.get_predictor('no_such_predictor')
    config = read_config(SMALL_CONFIG)
    from id_diff_amd.configs.config_dict import ConfigDict
    config.sampling = ConfigDict(method='ode')
    with pytest.raises(NotImplementedError, match="ode"):
        sampling.get_sampling_fn(config, sde_lib.configure_sde(config)[0], [4, 8], 1e-5)
    config.sampling.method = 'nonsense'
    with pytest.raises(ValueError, match="unknown"):
        sampling.get_sampling_fn(config, sde_lib.configure_sde(config)[0], [4, 8], 1e-5)
    from id_diff_amd.lightning_modules.BaseSdeGenerativeModel import BaseSdeGenerativeModel
    with pytest.raises(NotImplementedError, match="ode"):
        BaseSdeGenerativeModel(read_config(SMALL_CONFIG)).sample(ode=True)


def test_sampling_config_defaults():
    config = read_config(SMALL_CONFIG)
    assert config.get('sampling') is None                     # the configs here carry no sampling section
    assert sampling.sampling_config(config) == dict(method='pc', predictor='reverse_diffusion', corrector='none', n_steps_each=1,
                                                    noise_removal=True, probability_flow=False, snr=0.15)
    from id_diff_amd.configs.config_dict import ConfigDict
    config.sampling = ConfigDict(corrector='langevin', snr=0.2)
    got = sampling.sampling_config(config)
    assert got['corrector'] == 'langevin' and got['snr'] == 0.2 and got['predictor'] == 'reverse_diffusion'
    assert callable(sampling.get_sampling_fn(config, sde_lib.configure_sde(config)[0], [4, 8], 1e-5))


def test_ksphere_evaluation():
    import torch
    x = torch.tensor([[3.0, 4.0], [0.0, 1.0], [0.0, -3.0]])
    assert sampling.ksphere_evaluation(x) == dict(min_norm=1.0, max_norm=5.0, mean_norm=3.0)


# ---------------------------------------------------------------------------------------------- entry points refuse before any device call
A16 = 0x10000            # fabricated, 16-byte aligned: never dereferenced, the launchers refuse first


def _step(x=A16, ldx=8, s=A16, lds=8, z=0, ldz=0, out=A16, ldo=8, mean=0, ldm=0, B=4, D=6, nn=0, row0=0, label_col=-1):
    return _lib.lib().idiff_sampler_step_f32(x, ldx, s, lds, z, ldz, out, ldo, mean, ldm, B, D, 1.0, 1.0, 1.0, nn, 0.0, 1.0, 7, row0,
                                             label_col, 0.0, None)


def _norm(z=0, ldz=0, B=4, D=6, row0=0, ws=A16, out=A16):
    return _lib.lib().idiff_sampler_noise_norm_f32(z, ldz, B, D, 7, row0, ws, out, None)


REFUSALS = [
    ("sampler_step: ", lambda: _step(x=0)), ("sampler_step: ", lambda: _step(s=0)), ("sampler_step: ", lambda: _step(out=0)),
    ("sampler_step: ", lambda: _step(B=-1)), ("sampler_step: ", lambda: _step(D=0)), ("sampler_step: ", lambda: _step(ldx=5)),
    ("sampler_step: ", lambda: _step(lds=5)), ("sampler_step: ", lambda: _step(ldo=4)), ("sampler_step: ", lambda: _step(z=A16, ldz=5)),
    ("sampler_step: ", lambda: _step(mean=A16, ldm=3)), ("sampler_step: ", lambda: _step(x=A16 + 2)),
    ("sampler_step: ", lambda: _step(nn=A16 + 4)), ("sampler_step: ", lambda: _step(label_col=3)),
    ("sampler_step: ", lambda: _step(label_col=8)), ("sampler_step: ", lambda: _step(row0=-1)),
    ("sampler_noise_norm: ", lambda: _norm(B=0)), ("sampler_noise_norm: ", lambda: _norm(D=0)), ("sampler_noise_norm: ", lambda: _norm(ws=0)),
    ("sampler_noise_norm: ", lambda: _norm(out=0)), ("sampler_noise_norm: ", lambda: _norm(out=A16 + 4)),
    ("sampler_noise_norm: ", lambda: _norm(z=A16, ldz=5)), ("sampler_noise_norm: ", lambda: _norm(z=A16 + 1, ldz=8)),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_sampler_entry_points_refuse_before_any_device_call(case):
    prefix, call = REFUSALS[case]
    assert call() == 1001
    msg = _lib.lib().idiff_last_error().decode()
    assert msg.startswith(prefix), msg


def test_sampler_step_with_no_rows_does_nothing():
    assert _step(B=0) == 0


# ---------------------------------------------------------------------------------------------- drivers
def test_mode_generate_argument_handling(monkeypatch):
    flags = main.parse(["--config", SMALL_CONFIG, "--mode", "generate", "--num_samples", "64", "--seed=3"])
    assert flags.num_samples == 64 and flags.seed == 3 and flags.eval_every == 0
    seen = {}
    monkeypatch.setattr(run_lib, "generate", lambda config, **kw: seen.update(kw, name=config.model.name))
    main.main(["--config", SMALL_CONFIG, "--mode", "generate", "--num_samples", "64", "--seed", "3", "--checkpoint_path", "/x/last.ckpt",
               "--log_path", "/y", "--log_name", "run"])
    assert seen == dict(name='fcn', checkpoint_path="/x/last.ckpt", num_samples=64, seed=3, log_path="/y", log_name="run")
    seen.clear()
    main.main(["--config", SMALL_CONFIG, "--mode", "generate"])
    assert seen['num_samples'] is None and seen['seed'] is None and seen['checkpoint_path'] is None and seen['log_path'] == 'logs/ksphere/'
    with pytest.raises(SystemExit, match="one GPU"):
        main.main(["--config", SMALL_CONFIG, "--mode", "generate", "--gpus", "2"])
    with pytest.raises(SystemExit, match="--num_samples"):
        main.main(["--config", SMALL_CONFIG, "--mode", "generate", "--num_samples", "0"])
    with pytest.raises(SystemExit, match="must not be negative"):
        main.main(["--config", SMALL_CONFIG, "--mode", "train", "--n_iters", "5", "--eval_every", "-1"])


def test_mode_sample_is_still_outside_the_scope():
    with pytest.raises(SystemExit, match="outside the scope"):
        main.main(["--config", SMALL_CONFIG, "--mode", "sample"])


def test_mode_train_passes_eval_every_only_when_asked(monkeypatch):
    seen = {}
    monkeypatch.setattr(run_lib, "train", lambda config, **kw: seen.update(kw))
    main.main(["--config", SMALL_CONFIG, "--mode", "train", "--n_iters", "5"])
    assert 'eval_every' not in seen
    main.main(["--config", SMALL_CONFIG, "--mode", "train", "--n_iters", "5", "--eval_every", "100"])
    assert seen['eval_every'] == 100
