"""GPU tests of the likelihood and of the probability-flow ODE sampler: every case of tests/golden/likelihood.npz with both divergences
(nfe equal; z and bpd within 8 x the fixture's fp32-CPU deviation from its fp64 run), Hutchinson's estimate with unit probes against the
exact trace of the same launch, the round trip data -> z -> data, the generic ``score_fn`` path on the circle cloud, a trained network
against the oracle, reproducibility, and the three entry points' pickles.

Measured on the MI355X (share of the bar, worst over the batch): see DESIGN.md 4.10."""
import pickle

import numpy as np
import pytest
import torch

import ode_cases as oc
import sampling_cases as sc
from id_diff_amd import likelihood, sampling, sde_lib, train
from id_diff_amd.configs.config_dict import ConfigDict
from id_diff_amd.configs.utils import read_config
from id_diff_amd.models.fcn import FCN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SMALL_CONFIG = 'configs/dimension_estimation/paper/euclidean_data/ksphere/train_small.py'
DIVERGENCES = [('hutch', False), ('exact', True)]


@pytest.fixture(scope="module")
def fx():
    return oc.load()


def fixture_model(fx, case):
    model = FCN(oc.fcn_config(case))
    model.load_state_dict({k: torch.as_tensor(v) for k, v in oc.weights(fx, case).items()}, strict=True)
    return model.to(DEV).eval()


def share(got, want64, want32):
    """max |got - fp64| as a share of BAR x max |fp32 - fp64|."""
    return float(np.abs(np.asarray(got, dtype=np.float64) - want64).max() / (oc.BAR * np.abs(want32 - want64).max()))


# ---------------------------------------------------------------------------------------------- 1. the fixture, fast path
@pytest.mark.parametrize("name,exact", DIVERGENCES, ids=[d[0] for d in DIVERGENCES])
@pytest.mark.parametrize("case", oc.CASES, ids=oc.case_id)
def test_likelihood_of_the_fixture_cases(fx, case, name, exact):
    cid, kind = oc.case_id(case), case[0]
    model, sde = fixture_model(fx, case), oc.make_sde(kind)
    fn = likelihood.get_likelihood_fn(sde, exact=exact, eps=oc.EPS[kind], rtol=oc.RTOL, atol=oc.ATOL)
    bpd, z, nfe = fn(model, torch.as_tensor(fx[f"{cid}::data"]).to(DEV), epsilon=fx[f"{cid}::epsilon"])
    key = f"{cid}::{name}::"
    sz = share(z.cpu().numpy(), fx[key + "z64"], fx[key + "z32"])
    sb = share(bpd.cpu().numpy(), fx[key + "bpd64"], fx[key + "bpd32"])
    print(f"{cid} {name}: nfe {nfe} (fixture {int(fx[key + 'nfe'])}); share of the bar: z {sz:.3f}, bpd {sb:.3f}")
    assert nfe == int(fx[key + "nfe"])
    assert z.dtype == torch.float32 and tuple(z.shape) == (oc.B, oc.D) and tuple(bpd.shape) == (oc.B,)
    assert sz <= 1.0 and sb <= 1.0
    if kind == 've':                                                          # the reference's own numbers, recorded beside the oracle's
        assert np.abs(z.cpu().numpy() - fx[key + "ref_z"]).max() <= 2 * oc.BAR * np.abs(fx[key + "z32"] - fx[key + "z64"]).max()
        assert np.abs(bpd.cpu().numpy() - fx[key + "ref_bpd"]).max() <= 2 * oc.BAR * np.abs(fx[key + "bpd32"] - fx[key + "bpd64"]).max()


@pytest.mark.parametrize("case", oc.CASES, ids=oc.case_id)
def test_ode_sampler_of_the_fixture_cases_and_the_round_trip(fx, case):
    cid, kind = oc.case_id(case), case[0]
    model, sde = fixture_model(fx, case), oc.make_sde(kind)
    data = fx[f"{cid}::data"]
    sampler = sampling.get_ode_sampler(sde, (oc.B, oc.D), eps=oc.EPS[kind], rtol=oc.RTOL, atol=oc.ATOL)
    x, nfe = sampler(model, z=torch.as_tensor(fx[f"{cid}::exact::z64"]).float().to(DEV))
    s = share(x.cpu().numpy(), fx[f"{cid}::sample::x64"], fx[f"{cid}::sample::x32"])
    # the round trip: the latent code of the GPU's own likelihood, back to the data
    _, z, _ = likelihood.get_likelihood_fn(sde, exact=True, eps=oc.EPS[kind], rtol=oc.RTOL, atol=oc.ATOL)(model, torch.as_tensor(data).to(DEV))
    back, nfe_back = sampler(model, z=z)
    oracle_trip = np.abs(fx[f"{cid}::sample::x64"] - data).max()
    trip = np.abs(back.cpu().numpy().astype(np.float64) - data).max()
    print(f"{cid}: sampler nfe {nfe} (fixture {int(fx[f'{cid}::sample::nfe'])}), share of the bar {s:.3f}; round trip {trip:.2e} "
          f"(oracle {oracle_trip:.2e}, bar {oc.BAR * oracle_trip:.2e})")
    assert nfe == int(fx[f"{cid}::sample::nfe"]) and s <= 1.0
    assert trip <= oc.BAR * oracle_trip
    if kind == 've':
        assert np.abs(x.cpu().numpy() - fx[f"{cid}::sample::ref_x"]).max() <= \
            2 * oc.BAR * np.abs(fx[f"{cid}::sample::x32"] - fx[f"{cid}::sample::x64"]).max()


# ---------------------------------------------------------------------------------------------- 2. Hutchinson against exact
@pytest.mark.parametrize("case", oc.CASES, ids=oc.case_id)
def test_unit_probes_sum_to_the_exact_trace_of_the_same_launch(fx, case):
    """With epsilon = +-e_i the estimate is J_ii: over i it sums to the exact trace.  The two run different fp32 products (the
    vector-Jacobian product through idiff_gemm_nn_f32, the tangent rows through idiff_jvp_layer_f32), each a chain of fp32 fmas with
    |error| <= (K + 2) 2^-24 sum |a w| per layer and one rounding of ELU': against the product of the absolute matrices,
    |J_ii - exact| <= sum_layers (K_l + 4) 2^-24 |W_out| g |W| ... g |W_1| per path, twice (two paths), plus the fp64 kernel bounds."""
    cid, kind = oc.case_id(case), case[0]
    model, sde = fixture_model(fx, case), oc.make_sde(kind)
    D, B, t = oc.D, oc.B, 0.3
    x = torch.as_tensor(fx[f"{cid}::data"]).to(DEV)
    a, b, label, _ = sampling.flow_coefficients(sde, t)
    K = torch.zeros(7, B, D + 1, dtype=torch.float64, device=DEV)

    def launch(flow):
        flow.x32[:, :D] = x
        flow.x32[:, D] = label
        flow.rhs(0, t, K)
        return K[0, :, D].cpu().numpy().copy()
    exact_flow = likelihood.FcnFlow(model, sde, B, aug=1, exact=True)
    exact = launch(exact_flow)
    total = np.zeros(B)
    signs = np.where(np.arange(B) % 2 == 0, 1.0, -1.0).astype(np.float32)
    for i in range(D):
        eps = np.zeros((B, D), dtype=np.float32)
        eps[:, i] = signs
        total += launch(likelihood.FcnFlow(model, sde, B, aug=1, eps=torch.as_tensor(eps).to(DEV))) - a * D
    # the bound, from the weights and the ELU outputs of that launch
    ws = [w.cpu().numpy().astype(np.float64) for w in exact_flow.ws]
    g = [np.where(act.cpu().numpy() > 0, 1.0, act.cpu().numpy().astype(np.float64) + 1.0) for act in exact_flow.acts]
    path = np.broadcast_to(np.abs(ws[0][:, :D]), (B,) + ws[0][:, :D].shape)
    rel = 0.0
    for l, w in enumerate(ws):
        if l > 0:
            path = np.abs(w[:, :path.shape[1]])[None] @ path
            rel += (w.shape[1] + 4) * 2.0 ** -24
        if l < len(g):
            path = g[l][:, :path.shape[1], None] * path
    rel += (D + 1 + 4) * 2.0 ** -24
    bound = abs(b) * 2 * rel * np.trace(path, axis1=1, axis2=2) + 64 * 2.0 ** -53 * (abs(a) * D + np.abs(exact))
    dev_ = np.abs(total - (exact - a * D))
    print(f"{cid}: |sum_i J_ii - trace| at most {dev_.max():.2e}, {float((dev_ / bound).max()):.3f} of the bound; |b trace| up to {np.abs(exact - a * D).max():.2e}")
    assert (dev_ <= bound).all() and np.abs(exact - a * D).max() > 10 * bound.max()


# ---------------------------------------------------------------------------------------------- 3. the generic path
def test_ode_sampler_through_the_exact_score_lands_on_the_cloud(fx):
    """empirical_exact through ``score_fn``: every sample within 3 x the largest nearest-point distance the reference's ODE sampler
    reached on this cloud through the fp64 restatement of that score (as the PC sampler's acceptance test)."""
    from id_diff_amd.models.empirical_exact import EmpiricalExact
    e, cloud = sc.EMP, sc.empirical_cloud()
    bar = 3.0 * float(fx["emp::max_dist"])
    assert bar < 0.5 * float(fx["emp::spacing"])
    config = ConfigDict()
    config.model = ConfigDict(name='empirical_exact', sigma_min=e['sigma_min'], sigma_max=e['sigma_max'], num_scales=e['N'])
    config.data = ConfigDict(noise_std=0.0, shape=[cloud.shape[1]])
    config.training = ConfigDict(sde='vesde', continuous=True)
    model = EmpiricalExact(config, data=cloud).to(DEV)
    model.ess_warn = 0
    sde = sde_lib.VESDE(sigma_min=e['sigma_min'], sigma_max=e['sigma_max'], N=e['N'])
    samples, nfe = sampling.get_ode_sampler(sde, (e['samples'], cloud.shape[1]), eps=1e-5)(model, seed=0)
    got = samples.cpu().numpy()
    assert got.shape == (e['samples'], cloud.shape[1]) and np.isfinite(got).all()
    dist = sc.nearest_distance(got, cloud)
    print(f"generic path: nfe {nfe}, nearest-point distance max {dist.max():.3e}, mean {dist.mean():.3e}; bar {bar:.3e}")
    assert dist.max() <= bar
    assert len(np.unique(np.argmin(((got[:, None] - cloud[None]) ** 2).sum(-1), axis=1))) > 32        # spread over the circle


# ---------------------------------------------------------------------------------------------- 4. a trained network
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    root = tmp_path_factory.mktemp("likelihood")
    config = read_config(SMALL_CONFIG)
    config.device = DEV
    config.logging.log_path = str(root)
    train.train(config, log_path=str(root), n_iters=8000, log=None)
    return config, train.last_checkpoint_path(config, str(root)), root


def _module(config, ckpt):
    from id_diff_amd.lightning_modules.BaseSdeGenerativeModel import BaseSdeGenerativeModel
    module = BaseSdeGenerativeModel(config).load_from_checkpoint(ckpt).to(DEV).eval()
    module.configure_sde(config)
    return module


@pytest.mark.parametrize("name,exact", DIVERGENCES, ids=[d[0] for d in DIVERGENCES])
def test_trained_network_against_the_oracle(trained, name, exact):
    """train_small after 8000 steps: 64 points on the sphere and 64 at radius 2, against the oracle on the same checkpoint, within 8 x the
    deviation of the oracle's own fp32 run from its fp64 run."""
    config, ckpt, _ = trained
    module = _module(config, ckpt)
    params = dict(sigma_min=float(config.model.sigma_min), sigma_max=float(config.model.sigma_max))
    w = {k: v.detach().cpu().numpy() for k, v in module.score_model.state_dict().items()}
    on = train.data_split(config, 'test')[:64].numpy()
    data = np.concatenate([on, 2.0 * on]).astype(np.float32)
    epsilon = (np.random.default_rng(5).integers(0, 2, data.shape) * 2 - 1).astype(np.float32)
    kw = dict(eps=module.sampling_eps, N=module.sde.N, params=params)
    r64 = oc.oracle_likelihood(w, 've', data, torch.float64, exact, epsilon, **kw)
    r32 = oc.oracle_likelihood(w, 've', data, torch.float32, exact, epsilon, **kw)
    fn = likelihood.get_likelihood_fn(module.sde, exact=exact, eps=module.sampling_eps)
    bpd, z, nfe = fn(module, torch.as_tensor(data).to(DEV), epsilon=epsilon)
    sz, sb = share(z.cpu().numpy(), r64['z'], r32['z']), share(bpd.cpu().numpy(), r64['bpd'], r32['bpd'])
    print(f"trained {name}: nfe {nfe} (oracle {r64['nfe']} fp64, {r32['nfe']} fp32); share of the bar: z {sz:.3f}, bpd {sb:.3f}; "
          f"bpd on the sphere {float(bpd[:64].mean()):.3f}, at radius 2 {float(bpd[64:].mean()):.3f}")
    assert nfe == r64['nfe']
    assert sz <= 1.0 and sb <= 1.0
    assert float(bpd[:64].mean()) < float(bpd[64:].mean())                    # the data are likelier than points off the sphere


# ---------------------------------------------------------------------------------------------- 5. reproducibility, entry points
def test_the_same_seed_gives_the_same_bits(fx):
    case = oc.CASES[1]
    model, sde = fixture_model(fx, case), oc.make_sde(case[0])
    data = torch.as_tensor(fx[f"{oc.case_id(case)}::data"]).to(DEV)
    for htype in ('Rademacher', 'Gaussian'):
        fn = likelihood.get_likelihood_fn(sde, hutchinson_type=htype)
        a, b, c = fn(model, data, seed=3), fn(model, data, seed=3), fn(model, data, seed=4)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
        assert not torch.equal(a[0], c[0])
    p = likelihood.probes('Rademacher', 64, 6, 3, DEV)
    assert bool((p.abs() == 1).all()) and 0.2 < float((p > 0).float().mean()) < 0.8
    sampler = sampling.get_ode_sampler(sde, (16, oc.D))
    x, y, z = sampler(model, seed=1), sampler(model, seed=1), sampler(model, seed=2)
    assert torch.equal(x[0], y[0]) and x[1] == y[1] and not torch.equal(x[0], z[0])
    d = sampling.get_ode_sampler(sde, (16, oc.D), denoise=True)(model, seed=1)
    assert bool(torch.isfinite(d[0]).all()) and not torch.equal(d[0], x[0]) and float((d[0] - x[0]).abs().max()) < 0.1


def test_entry_points_write_their_pickles(trained):
    from id_diff_amd import main
    config, ckpt, root = trained
    module = _module(config, ckpt)
    samples, nfe = module.ode_sample(num_samples=64, seed=1)
    norms = sampling.ksphere_evaluation(samples)
    print(f"ode_sample: nfe {nfe}, norms min {norms['min_norm']:.3f} mean {norms['mean_norm']:.3f} max {norms['max_norm']:.3f}")
    assert samples.shape == (64, 8) and 0.5 < norms['mean_norm'] < 1.5
    back, _ = module.ode_sample(z=samples)
    assert back.shape == (64, 8)
    cfg = "id-diff_amd/" + SMALL_CONFIG
    main.main(["--config", cfg, "--mode", "generate", "--sampler", "ode", "--num_samples", "32", "--seed", "2", "--checkpoint_path", ckpt,
               "--log_path", str(root), "--log_name", "gen"])
    with open(root / "gen" / "samples" / "samples.pkl", 'rb') as f:
        saved = pickle.load(f)
    assert saved['samples'].shape == (32, 8) and saved['nfe'] > 0 and 0.5 < saved['mean_norm'] < 1.5 and 'steps' not in saved
    for extra, exact in ((["--exact"], True), ([], False)):
        main.main(["--config", cfg, "--mode", "likelihood", "--num_samples", "16", "--checkpoint_path", ckpt, "--log_path", str(root),
                   "--log_name", "lik"] + extra)
        with open(root / "lik" / "likelihood" / "likelihood.pkl", 'rb') as f:
            saved = pickle.load(f)
        assert saved['bpd'].shape == (16,) and saved['z'].shape == (16, 8) and saved['nfe'] > 0 and saved['exact'] is exact
        assert np.isfinite(saved['bpd']).all()
