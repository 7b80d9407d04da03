"""CPU tests of the probability-flow ODE feature: the fp64 restatement of scipy's RK45 bit for bit against scipy, the three guards, the
flow coefficients and priors against the fixture and closed forms, an fp64 replay of each kernel's expression inside its stated bound (and
three mutations outside it), the argument handling of ``--mode likelihood`` and ``--sampler ode``, and the refusals."""
import math

import numpy as np
import pytest
import torch
from scipy import integrate

import ode_cases as oc
import sampling_cases as sc
from id_diff_amd import likelihood, main, ode, run_lib, sampling, sde_lib
from id_diff_amd.configs.config_dict import ConfigDict

SMALL_CONFIG = "id-diff_amd/configs/dimension_estimation/paper/euclidean_data/ksphere/train_small.py"


@pytest.fixture(scope="module")
def fx():
    return oc.load()


# ---------------------------------------------------------------------------------------------- 1. the restatement of scipy's RK45
_LIN = np.array([[-0.5, 2.0, 0.0], [-2.0, -0.5, 0.3], [0.1, 0.0, -1.5]])
PROBLEMS = {
    'linear': (lambda t, y: _LIN @ y, 0.0, 3.0, [1.0, 0.0, -1.0], 1e-6, 1e-8),
    'stiffish': (lambda t, y: -50.0 * (y - np.cos(t)), 0.0, 1.5, [0.0], 1e-4, 1e-7),
    'backward': (lambda t, y: _LIN @ y + np.sin(t), 2.0, 0.25, [0.3, -0.2, 0.9], 1e-5, 1e-5),
    'tight_rtol': (lambda t, y: np.array([y[1], -y[0]]), 0.0, 1.0, [1.0, 0.0], 1e-15, 1e-12),
}


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_rk45_host_equals_scipy_bit_for_bit(name):
    f, t0, t1, y0, rtol, atol = PROBLEMS[name]
    with oc.recorded_error_norms() as norms, pytest.warns(UserWarning) if rtol < 1e-13 else _nothing():
        sol = integrate.solve_ivp(f, (t0, t1), y0, method='RK45', rtol=rtol, atol=atol)
    y, nfev, steps, rejected, error_norms = ode.rk45_host(f, t0, t1, y0, rtol=rtol, atol=atol)
    assert sol.status == 0
    assert np.array_equal(y, sol.y[:, -1]) and nfev == sol.nfev
    assert steps == len(sol.t) - 1 and steps + rejected == len(error_norms) and error_norms == norms
    assert nfev == 2 + 6 * (steps + rejected)


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _numpy_flow(w, kind, data, exact, epsilon):
    """The fixture's flow with its divergence in fp64 numpy, flat as the reference lays it out: [B D rows, then B log p]."""
    sde = oc.make_sde(kind)
    keys = sorted({int(k.split('.')[1]) for k in w})
    Ws = [w[f"mlp.{i}.weight"].astype(np.float64) for i in keys]
    bs = [w[f"mlp.{i}.bias"].astype(np.float64) for i in keys]
    Bn, Dn = data.shape

    def f(t, v):
        x = v[:-Bn].reshape(Bn, Dn)
        a, b, label, _ = sampling.flow_coefficients(sde, t)
        h, J = np.concatenate([x, np.full((Bn, 1), label)], axis=1), None
        for j, (W, bias) in enumerate(zip(Ws, bs)):
            pre = h @ W.T + bias
            J = np.broadcast_to(W[:, :Dn], (Bn,) + W[:, :Dn].shape) if J is None else W[None] @ J
            if j < len(Ws) - 1:
                h = sc.elu(pre)
                J = np.where(pre > 0, 1.0, np.exp(np.minimum(pre, 0)))[:, :, None] * J
            else:
                h = pre
        tr = np.trace(J, axis1=1, axis2=2) if exact else np.einsum('bi,bij,bj->b', epsilon, J, epsilon)
        return np.concatenate([(a * x + b * h).reshape(-1), a * Dn + b * tr])
    return f


@pytest.mark.parametrize("case", oc.CASES, ids=oc.case_id)
@pytest.mark.parametrize("exact", [False, True], ids=['hutch', 'exact'])
def test_rk45_host_equals_scipy_on_the_fixture_network(fx, case, exact):
    cid = oc.case_id(case)
    data, epsilon = fx[f"{cid}::data"].astype(np.float64), fx[f"{cid}::epsilon"].astype(np.float64)
    f = _numpy_flow(oc.weights(fx, case), case[0], data, exact, epsilon)
    y0 = np.concatenate([data.reshape(-1), np.zeros(len(data))])
    sol = integrate.solve_ivp(f, (oc.EPS[case[0]], 1.0), y0, method='RK45', rtol=oc.RTOL, atol=oc.ATOL)
    y, nfev, steps, rejected, norms = ode.rk45_host(f, oc.EPS[case[0]], 1.0, y0, rtol=oc.RTOL, atol=oc.ATOL)
    assert np.array_equal(y, sol.y[:, -1]) and nfev == sol.nfev
    # the numpy flow is the oracle's flow with the coefficients and the label at the fp32 value of t (2^-24 relative in t moves b by
    # up to 4e-7 relative): the same steps, and the fixture's latent code and log p to 1e-6
    name = 'exact' if exact else 'hutch'
    assert nfev == int(fx[f"{cid}::{name}::nfe"])
    Bn = len(data)
    assert np.abs(y[:-Bn].reshape(data.shape) - fx[f"{cid}::{name}::z64"]).max() < 1e-6
    assert np.abs(y[-Bn:] - fx[f"{cid}::{name}::delta_logp64"]).max() < 1e-6


# ---------------------------------------------------------------------------------------------- 2. the guards
def test_guard_non_finite_error_norm():
    with pytest.raises(RuntimeError, match=r"error norm is nan at t = .*h = "):
        ode.rk45_host(lambda t, y: y * (np.nan if t > 0.5 else 1.0), 0.0, 1.0, [1.0])
    with pytest.raises(RuntimeError, match=r"error norm is .* at t = .*h = "):
        ode.rk45_host(lambda t, y: np.full_like(y, np.inf), 0.0, 1.0, [1.0])


def test_guard_step_below_ten_ulp():
    with pytest.raises(RuntimeError, match=r"below 10 ulp\(t\) at t = .*h = "):
        ode.rk45_host(lambda t, y: 1.0 / (1.0 - t) ** 2 * np.ones_like(y), 0.0, 2.0, [1.0], rtol=1e-10, atol=1e-12)


def test_guard_max_steps():
    with pytest.raises(RuntimeError, match=r"more than max_steps = 7 attempted steps at t = .*h = "):
        ode.rk45_host(lambda t, y: np.array([y[1], -400.0 * y[0]]), 0.0, 10.0, [1.0, 0.0], rtol=1e-8, atol=1e-10, max_steps=7)


def test_the_loop_ends_at_equal_end_points():
    y, nfev, steps, rejected, norms = ode.rk45_host(lambda t, y: y, 1.0, 1.0, [2.0])
    assert (y[0], nfev, steps, rejected, norms) == (2.0, 1, 0, 0, [])


# ---------------------------------------------------------------------------------------------- 3. flow coefficients, priors
@pytest.mark.parametrize("case", oc.CASES, ids=oc.case_id)
def test_flow_coefficients_match_the_fixture_drift(fx, case):
    """a x + b raw in fp64 against the recorded drift (the reference's rsde.sde for VE, the oracle's for VP and subVP), within
    4 x 2^-53 relative to |a x| + |b raw|.  The reference's VESDE.marginal_prob makes its two sigmas fp32 tensors
    (``torch.tensor(sigma_min)``) whatever the dtype of the run, while its VESDE.sde keeps them fp64: the std under its fp64 score is
    the std of sigma_min = fl32(0.01), 2e-8 away.  The comparison divides that one factor out of b; g and the formula are as they are."""
    cid, sde = oc.case_id(case), oc.make_sde(case[0])
    quirk = None
    if case[0] == 've':
        quirk = sde_lib.VESDE(sigma_min=float(np.float32(sde.sigma_min)), sigma_max=float(np.float32(sde.sigma_max)), N=sde.N)
    x = fx[f"{cid}::data"].astype(np.float64)
    for k, t in enumerate(oc.DRIFT_TIMES):
        a, b, label, std = sampling.flow_coefficients(sde, t)
        raw, want = fx[f"{cid}::raw"][k], fx[f"{cid}::drift"][k]
        if quirk is not None:
            b = b * (std / sampling.marginal_std(quirk, t))
        got = a * x + b * raw
        rel = np.abs(got - want) / (np.abs(a * x) + np.abs(b * raw))
        print(f"{cid} t = {t}: max relative deviation {rel.max() / 2.0 ** -53:.2f} x 2^-53")
        assert rel.max() <= 4 * 2.0 ** -53
        assert label == t * (sde.N - 1) and std == sampling.marginal_std(sde, t)


def test_flow_coefficients_use_the_schedule_expressions():
    for kind in ('ve', 'vp', 'subvp'):
        sde = sc.make_sde(kind)
        for t in (1e-3, 0.3, 1.0):
            t32 = float(np.float32(t))                                        # the time the label carries
            a, b, label, std = sampling.flow_coefficients(sde, t)
            d, g = sampling._drift_diffusion(sde, t32)
            assert (a, b, label, std) == (d, 0.5 * g * g / sampling.marginal_std(sde, t32), sampling.label_of(sde, t),
                                          sampling.marginal_std(sde, t32))
    with pytest.raises(NotImplementedError):
        sampling.flow_coefficients(sde_lib.SNRSDE(N=10), 0.5)


def test_prior_logp_closed_forms():
    rng = np.random.default_rng(0)
    z = torch.as_tensor(rng.standard_normal((5, 6)))
    s = 4.0
    want_ve = np.array([sum(-0.5 * math.log(2 * math.pi * s * s) - v * v / (2 * s * s) for v in row) for row in z.tolist()])
    want_vp = np.array([sum(-0.5 * math.log(2 * math.pi) - v * v / 2 for v in row) for row in z.tolist()])
    assert np.allclose(sde_lib.VESDE(sigma_min=0.01, sigma_max=s).prior_logp(z).numpy(), want_ve, rtol=1e-14, atol=0)
    for cls in (sde_lib.VPSDE, sde_lib.subVPSDE):
        assert np.allclose(cls().prior_logp(z).numpy(), want_vp, rtol=1e-14, atol=0)
        # all non-batch dimensions are summed: [B, D] and [B, C, H, W] rows alike (the reference's VP versions raise on [B, D])
        assert torch.equal(cls().prior_logp(z.reshape(5, 1, 2, 3)), cls().prior_logp(z))
    assert torch.equal(sde_lib.VESDE(sigma_max=s).prior_logp(z.reshape(5, 3, 2)), sde_lib.VESDE(sigma_max=s).prior_logp(z))


# ---------------------------------------------------------------------------------------------- 4. the kernels' expressions in fp64
def _problem(Bn, Dn, aug, seed=0):
    rng = np.random.default_rng(seed)
    W = Dn + aug
    return dict(y=rng.standard_normal((Bn, W)), K=rng.standard_normal((7, Bn, W)), y_new=rng.standard_normal((Bn, W)),
                x32=rng.standard_normal((Bn, Dn)).astype(np.float32), v=rng.standard_normal((Bn, Dn)).astype(np.float32),
                eps=(rng.integers(0, 2, (Bn, Dn)) * 2 - 1).astype(np.float32), u=rng.standard_normal((Bn, Dn)).astype(np.float32))


def _stage64(y, K, c):
    acc = np.zeros_like(y)
    for j, cj in enumerate(c):
        acc = cj * K[j] + acc
    return y + acc


def _error64(K, e, y, y_new, atol, rtol, pick=np.maximum):
    err = np.zeros_like(y)
    for j, ej in enumerate(e):
        err = ej * K[j] + err
    q = err / (atol + rtol * pick(np.abs(y), np.abs(y_new)))
    return float((q * q).sum())


@pytest.mark.parametrize("shape", oc.SHAPES[:4])
def test_fp64_replay_of_the_kernels_stays_inside_the_bounds_and_mutations_leave(shape):
    Bn, Dn, aug = shape
    p, h = _problem(Bn, Dn, aug), 0.37
    for s in range(1, 7):
        c = [h * a for a in (ode.A[s][:s] if s < 6 else ode.B)]
        ref, bound = oc.stage_ref(p['y'], p['K'], c)
        assert (np.abs(_stage64(p['y'], p['K'], c) - ref) <= bound).all()
    # mutation 1: a wrong tableau entry
    c = [h * a for a in ode.A[4][:4]]
    ref, bound = oc.stage_ref(p['y'], p['K'], c)
    bad = list(c); bad[2] = h * 64448 / 6651
    assert (np.abs(_stage64(p['y'], p['K'], bad) - ref) > bound).any()
    e = [h * v for v in ode.E]
    ref, bound = oc.error_ref(p['K'], e, p['y'], p['y_new'], 1e-5, 1e-3)
    assert abs(_error64(p['K'], e, p['y'], p['y_new'], 1e-5, 1e-3) - float(ref)) <= bound
    # mutation 2: min for max in the scale
    assert abs(_error64(p['K'], e, p['y'], p['y_new'], 1e-5, 1e-3, pick=np.minimum) - float(ref)) > bound
    a, b = -0.7, 1.3
    for kw in (dict(eps=p['eps'], u=p['u']), dict(q=p['y'][:, 0])) if aug else (dict(),):
        ref, bound = oc.rhs_ref(p['x32'], p['v'], a, b, Dn, aug, **kw)
        got = a * p['x32'].astype(np.float64) + b * p['v'].astype(np.float64)
        if aug:
            q = kw['q'] if 'q' in kw else (p['eps'].astype(np.float64) * p['u'].astype(np.float64)).sum(1)
            got = np.concatenate([got, (a * Dn + b * q)[:, None]], axis=1)
            # mutation 3: the a D term missing from the log p column
            assert (np.abs(got - oc.rhs_ref(p['x32'], p['v'], a, b, Dn, aug, a_term=False, **kw)[0]) > bound)[:, Dn].all()
        assert (np.abs(got - ref) <= bound).all()
    T, Wo = np.random.default_rng(1).standard_normal((3, Dn, 5)).astype(np.float32), p['v'][:1].T @ np.ones((1, 5), dtype=np.float32)
    ref, bound = oc.trace_ref(T, Wo[:Dn])
    assert (np.abs((T.astype(np.float64) * Wo[None, :Dn]).sum((1, 2)) - ref) <= bound).all()


def test_dormand_prince_tableau_is_scipys():
    from scipy.integrate._ivp.rk import RK45
    assert np.array_equal(ode.A, RK45.A) and np.array_equal(ode.B, RK45.B) and np.array_equal(ode.C, RK45.C) and np.array_equal(ode.E, RK45.E)


# ---------------------------------------------------------------------------------------------- 5. the entry points' arguments
def test_mode_likelihood_argument_handling(monkeypatch):
    seen = {}
    monkeypatch.setattr(run_lib, "likelihood", lambda config, **kw: seen.update(kw, name=config.model.name))
    main.main(["--config", SMALL_CONFIG, "--mode", "likelihood", "--num_samples", "64", "--exact", "--seed", "3", "--checkpoint_path",
               "/x/last.ckpt", "--log_path", "/tmp/l", "--log_name", "n"])
    assert seen == dict(name='fcn', checkpoint_path="/x/last.ckpt", num_samples=64, exact=True, seed=3, log_path="/tmp/l", log_name="n")
    seen.clear()
    main.main(["--config", SMALL_CONFIG, "--mode", "likelihood"])
    assert seen['num_samples'] is None and seen['exact'] is False and seen['seed'] is None
    with pytest.raises(SystemExit, match="one GPU"):
        main.main(["--config", SMALL_CONFIG, "--mode", "likelihood", "--gpus", "2"])
    with pytest.raises(SystemExit, match="positive"):
        main.main(["--config", SMALL_CONFIG, "--mode", "likelihood", "--num_samples", "0"])


def test_mode_generate_sampler_flag_reaches_generate_only_when_given(monkeypatch):
    seen = {}
    monkeypatch.setattr(run_lib, "generate", lambda config, **kw: seen.update(kw))
    main.main(["--config", SMALL_CONFIG, "--mode", "generate", "--sampler", "ode", "--num_samples", "8"])
    assert seen['sampler'] == 'ode' and seen['num_samples'] == 8 and len(seen) == 6
    seen.clear()
    main.main(["--config", SMALL_CONFIG, "--mode", "generate", "--num_samples", "8"])
    assert sorted(seen) == ['checkpoint_path', 'log_name', 'log_path', 'num_samples', 'seed']
    with pytest.raises(SystemExit):
        main.parse(["--config", SMALL_CONFIG, "--mode", "generate", "--sampler", "heun"])


def test_run_lib_generate_passes_the_sampler_on_only_when_given(monkeypatch):
    seen = {}
    monkeypatch.setattr(sampling, "generate", lambda config, **kw: seen.update(kw))
    run_lib.generate(ConfigDict(), num_samples=4)
    assert 'sampler' not in seen
    run_lib.generate(ConfigDict(), num_samples=4, sampler='ode')
    assert seen['sampler'] == 'ode'


# ---------------------------------------------------------------------------------------------- 6. the refusals, before the GPU
def _config(name='fcn', dropout=0.0):
    c = sc.fcn_config('ve')
    c.model.name, c.model.dropout = name, dropout
    return c


def test_refusals_before_the_gpu_is_touched(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("the GPU was asked for")))
    sde = sc.make_sde('ve')
    with pytest.raises(NotImplementedError, match="RK45"):
        likelihood.get_likelihood_fn(sde, method='RK23')
    with pytest.raises(NotImplementedError, match="RK45"):
        sampling.get_ode_sampler(sde, (4, 6), method='RK23')
    with pytest.raises(NotImplementedError, match="Hutchinson type"):
        likelihood.get_likelihood_fn(sde, hutchinson_type='Cauchy')
    with pytest.raises(NotImplementedError, match="likelihood serves model.name == 'fcn' only"):
        likelihood.check_config(_config(name='ddpm'))
    with pytest.raises(NotImplementedError, match="dropout"):
        likelihood.check_config(_config(dropout=0.1))
    with pytest.raises(NotImplementedError, match="not yet supported"):
        likelihood.get_likelihood_fn(sde_lib.SNRSDE(N=10))
    fn = likelihood.get_likelihood_fn(sde)
    with pytest.raises(NotImplementedError, match="'fcn' network only"):
        fn(torch.nn.Linear(3, 3), torch.zeros(2, 3))
    from id_diff_amd.models.fcn import FCN
    with pytest.raises(NotImplementedError, match="dropout"):
        fn(FCN(_config(dropout=0.25)), torch.zeros(2, 6))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fn(FCN(_config()), torch.zeros(2, 6))


def test_mode_likelihood_refuses_other_networks_with_the_scope_message(monkeypatch):
    monkeypatch.setattr(run_lib, "likelihood", lambda *a, **k: (_ for _ in ()).throw(AssertionError("reached the driver")))
    with pytest.raises(NotImplementedError, match="fcn"):
        main.main(["--config", "id-diff_amd/configs/dimension_estimation/paper/euclidean_data/line/empirical.py", "--mode", "likelihood"])


# ---------------------------------------------------------------------------------------------- 7. the launchers refuse on the host
def test_launchers_refuse_bad_geometry_before_any_device_call():
    """Made-up addresses: a launcher that touched them, or launched, would fault; each call returns IDIFF_EINVAL with its own message."""
    from id_diff_amd import _lib
    lib = _lib.lib()
    P, c7 = 0x10000, (_lib.c_d * 7)(*([1.0] * 7))
    calls = {
        "rk_stage: a row pitch": lambda: lib.idiff_rk_stage_f64(P, 6, P, 8, 64, c7, 2, P, 8, P, 8, 4, 6, 1, 1.0, None),
        "rk_stage: ldx": lambda: lib.idiff_rk_stage_f64(P, 8, P, 8, 64, c7, 2, P, 8, P, 6, 4, 6, 1, 1.0, None),
        "rk_stage: ns = 7": lambda: lib.idiff_rk_stage_f64(P, 8, P, 8, 64, c7, 7, P, 8, P, 8, 4, 6, 1, 1.0, None),
        "rk_stage: strideK": lambda: lib.idiff_rk_stage_f64(P, 8, P, 8, 16, c7, 2, P, 8, P, 8, 4, 6, 1, 1.0, None),
        "rk_stage: y, K and y_out must be 8-byte": lambda: lib.idiff_rk_stage_f64(P + 4, 8, P, 8, 64, c7, 2, P, 8, P, 8, 4, 6, 1, 1.0, None),
        "rk_stage: null": lambda: lib.idiff_rk_stage_f64(P, 8, None, 8, 64, c7, 2, P, 8, P, 8, 4, 6, 1, 1.0, None),
        "rk_error: a row pitch": lambda: lib.idiff_rk_error_f64(P, 6, 64, c7, P, 8, P, 8, 4, 7, 1e-5, 1e-5, P, P, None),
        "rk_error: strideK": lambda: lib.idiff_rk_error_f64(P, 8, 8, c7, P, 8, P, 8, 4, 7, 1e-5, 1e-5, P, P, None),
        "rk_error: every pointer": lambda: lib.idiff_rk_error_f64(P, 8, 64, c7, P, 8, P, 8, 4, 7, 1e-5, 1e-5, P + 4, P, None),
        "rk_error: atol": lambda: lib.idiff_rk_error_f64(P, 8, 64, c7, P, 8, P, 8, 4, 7, -1.0, 1e-5, P, P, None),
        "flow_rhs: a row pitch": lambda: lib.idiff_flow_rhs_f64(P, 8, P, 8, 1.0, 1.0, P, 6, 4, 6, 1, None, 0, None, 0, P, None),
        "flow_rhs: aug = 1 needs": lambda: lib.idiff_flow_rhs_f64(P, 8, P, 8, 1.0, 1.0, P, 8, 4, 6, 1, P, 8, None, 0, None, None),
        "flow_rhs: pass q, or": lambda: lib.idiff_flow_rhs_f64(P, 8, P, 8, 1.0, 1.0, P, 8, 4, 6, 1, P, 8, P, 8, P, None),
        "flow_rhs: x32, v, eps and u must be": lambda: lib.idiff_flow_rhs_f64(P + 2, 8, P, 8, 1.0, 1.0, P, 8, 4, 6, 0, None, 0, None, 0, None, None),
        "jvp_trace: T and Wout must be 16-byte": lambda: lib.idiff_jvp_trace_f64(P + 4, 16, 96, P, 16, P, 2, 6, 16, None),
        "jvp_trace: ldt": lambda: lib.idiff_jvp_trace_f64(P, 14, 96, P, 16, P, 2, 6, 16, None),
        "jvp_trace: ldt = 12": lambda: lib.idiff_jvp_trace_f64(P, 12, 96, P, 16, P, 2, 6, 14, None),
        "jvp_trace: strideT": lambda: lib.idiff_jvp_trace_f64(P, 16, 32, P, 16, P, 2, 6, 16, None),
    }
    for start, call in calls.items():
        assert call() != 0, start
        msg = lib.idiff_last_error().decode()
        assert msg.startswith(start.split(":")[0] + ": ") and start.split(": ", 1)[1].split(" = ")[0] in msg, (start, msg)
