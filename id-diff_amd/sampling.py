"""Sampling from a score model: the unconditional predictor-corrector sampler of the reference (sampling/predictors.py,
sampling/correctors.py, sampling/unconditional.py:133-199) on one HIP kernel per update.

All rows of a sampling step share one time, so every predictor and corrector of the reference is

    x_mean = a x + b s,      x = x_mean + c z,      z ~ N(0, I)

with s the score and (a, b, c) three scalars of (SDE, method, t).  ``predictor_coefficients`` / ``corrector_coefficients`` state them
in fp64 (host arithmetic, importable without a GPU); ``idiff_sampler_step_f32`` applies them.  The Langevin corrector's step size
(snr mean_r |z_r|)^2 2 alpha depends on the noise just drawn: ``idiff_sampler_noise_norm_f32`` leaves that mean on the device and the
step kernel forms b and c from it, so nothing inside the loop reads the device back.  (a, b, c) per SDE:

    reverse_diffusion   VE, subVP   a = 1 - d / N,   b = k g^2 / N,   c = g / sqrt(N)      (SDE.discretize: Euler-Maruyama; the SMLD
                        VP          a = 2 - sqrt(1 - beta_i),  b = k beta_i,  c = sqrt(beta_i)      form of VESDE is commented out)
    euler_maruyama      all         a = 1 - d / N,   b = k g^2 / N,   c = g / sqrt(N)
    ancestral_sampling  VE          a = 1,  b = s_i^2 - s_{i-1}^2,  c = sqrt(s_{i-1}^2 (s_i^2 - s_{i-1}^2) / s_i^2)     (s_{-1} = 0)
                        VP          a = 1 / sqrt(1 - beta_i),  b = beta_i / sqrt(1 - beta_i),  c = sqrt(beta_i)
    langevin            VE, VP      a = 1,  b = 2 alpha (snr mean_r |z_r|)^2,  c = sqrt(2 b)        alpha = 1 (VE), 1 - beta_i (VP)
    ald                 VE, VP      a = 1,  b = 2 alpha (snr std(t))^2,        c = sqrt(2 b)

d x and g are drift and diffusion of the forward SDE at t (d = 0 for VE, -beta(t) / 2 otherwise), k = 1/2 and c = 0 under
``probability_flow``, i = long(t (N - 1) / T) the table index formed in fp32 as the reference forms it.

Two execution paths behind ``pc_sampler``: any model ``mutils.get_score_fn`` accepts runs ``score_fn`` + one step launch per update;
``models.fcn.FCN`` keeps the state in the padded input rows of its first layer and runs ``hidden_layers + 2`` idiff_gemm_f32 launches
and one step launch that reads the raw output (score = -out / std rides in b), updates the state in place and writes the next time
feature.  Out of scope: ``heun``, ``mala``, the conditional samplers, inpainting, EMA weights, several GPUs.

The probability-flow ODE sampler (``get_ode_sampler``) arrives through its own name and ``generate(sampler='ode')`` /
``BaseSdeGenerativeModel.ode_sample``; ``sampling.method = 'ode'`` in ``get_sampling_fn`` and ``sample(ode=True)`` still refuse.
"""
import math

import numpy as np
import torch

from . import sde_lib

SAMPLING_DEFAULTS = dict(method='pc', predictor='reverse_diffusion', corrector='none', n_steps_each=1, noise_removal=True,
                         probability_flow=False, snr=0.15)
SALT_PRIOR, SALT_CORRECTOR, SALT_PREDICTOR = 11, 12, 13          # train.stream_key salts; training draws use 0 .. 4
FCN_FAST_PATH = True              # scripts/sample_bench.py: the fast path is the faster one at the paper's shape

_PREDICTORS = ('none', 'reverse_diffusion', 'euler_maruyama', 'ancestral_sampling')
_CORRECTORS = ('none', 'langevin', 'ald')
_OUT_OF_SCOPE = {'heun': "the 'heun' predictor drives a second score evaluation per step and is not built",
                 'mala': "the 'mala' corrector needs the model's energy and an accept/reject pass and is not built"}


# ---------------------------------------------------------------------------------------------- names
class _Method:
    """What ``get_predictor`` / ``get_corrector`` return: the reference hands classes around, and only their identity is used."""
    kind = name = None

    def __init__(self, *args, **kwargs):
        raise TypeError(f"{self.kind} {self.name!r} is a name here: pass it to get_pc_sampler")


def _method(kind, name, table):
    name = str(name).lower()
    if name in _OUT_OF_SCOPE:
        raise NotImplementedError(_OUT_OF_SCOPE[name])
    if name.startswith('conditional_'):
        raise NotImplementedError(f"{kind} {name!r}: the conditional samplers are not built")
    if name not in table:
        raise KeyError(f"unknown {kind} {name!r} (have: {', '.join(table)})")
    return type(name, (_Method,), dict(kind=kind, name=name))


def get_predictor(name):
    return _method('predictor', name, _PREDICTORS)


def get_corrector(name):
    return _method('corrector', name, _CORRECTORS)


def _name_of(method, kind):
    if method is None:
        return 'none'
    if isinstance(method, str):
        return _method(kind, method, _PREDICTORS if kind == 'predictor' else _CORRECTORS).name
    return method.name


def sampling_config(config):
    """The ``sampling`` section of a config with the defaults of the reference's Euclidean configs filled in."""
    out = dict(SAMPLING_DEFAULTS)
    section = config.get('sampling') if hasattr(config, 'get') else None
    if section is not None:
        for k in out:
            v = section.get(k)
            if v is not None:
                out[k] = v
    return out


# ---------------------------------------------------------------------------------------------- the SDE at one time, fp64
def _kind(sde):
    if isinstance(sde, sde_lib.VESDE):
        return 've'
    if isinstance(sde, sde_lib.subVPSDE):
        return 'subvp'
    if isinstance(sde, sde_lib.VPSDE):
        return 'vp'
    raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")


def time_grid(sde, eps):
    """torch.linspace(T, eps, N) in fp32, as unconditional.py:178 forms it; fp32 numpy [N]."""
    return torch.linspace(float(sde.T), float(eps), int(sde.N), dtype=torch.float32).numpy()


def table_index(sde, t):
    """long(t (N - 1) / T) in the reference's arithmetic: t and the product are fp32."""
    return int(np.float32(np.float32(t) * np.float32(sde.N - 1)) / np.float32(sde.T))


def label_of(sde, t):
    """The network's time feature t (N - 1), the fp32 product get_score_fn forms."""
    return float(np.float32(t) * np.float32(sde.N - 1))


def marginal_std(sde, t):
    t = float(t)
    if _kind(sde) == 've':
        return float(sde.sigma_min) * (float(sde.sigma_max) / float(sde.sigma_min)) ** t
    lmc = -0.25 * t * t * (sde.beta_1 - sde.beta_0) - 0.5 * t * sde.beta_0
    v = 1.0 - math.exp(2.0 * lmc)
    return v if _kind(sde) == 'subvp' else math.sqrt(v)


def _drift_diffusion(sde, t):
    """(d, g): drift d x and diffusion g of the forward SDE at t."""
    t, kind = float(t), _kind(sde)
    if kind == 've':
        ratio = float(sde.sigma_max) / float(sde.sigma_min)
        return 0.0, float(sde.sigma_min) * ratio ** t * math.sqrt(2.0 * math.log(ratio))
    beta_t = sde.beta_0 + t * (sde.beta_1 - sde.beta_0)
    if kind == 'vp':
        return -0.5 * beta_t, math.sqrt(beta_t)
    discount = 1.0 - math.exp(-2.0 * sde.beta_0 * t - (sde.beta_1 - sde.beta_0) * t * t)
    return -0.5 * beta_t, math.sqrt(beta_t * discount)


def check_vp_table(sde):
    """torch.linspace(beta_min / N, beta_max / N, N) must stay below 1: 1 - beta_i is under a square root."""
    if _kind(sde) == 'vp' and float(sde.beta_1) / sde.N >= 1.0:
        raise ValueError(f"VPSDE with N = {sde.N} steps has discrete beta_i = beta_max / N = {float(sde.beta_1) / sde.N:g} >= 1 "
                         f"(needs N > beta_max = {sde.beta_1:g}): sqrt(1 - beta_i) is not a number there")


def _discrete_beta(sde, i):
    check_vp_table(sde)
    n = sde.N
    lo, hi = float(sde.beta_0) / n, float(sde.beta_1) / n
    return lo + (hi - lo) * i / (n - 1) if n > 1 else lo


def _discrete_sigma(sde, i):
    n = sde.N
    lo, hi = math.log(float(sde.sigma_min)), math.log(float(sde.sigma_max))
    return math.exp(lo + (hi - lo) * i / (n - 1) if n > 1 else lo)


def predictor_coefficients(sde, name, t, probability_flow=False):
    """(a, b, c) of one predictor update at time ``t``: x_mean = a x + b score, x = x_mean + c z."""
    name, kind = _name_of(name, 'predictor'), _kind(sde)
    k = 0.5 if probability_flow else 1.0
    n = float(sde.N)
    if name == 'none':
        return 1.0, 0.0, 0.0
    if name == 'ancestral_sampling':
        if kind == 'subvp':
            raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported by ancestral_sampling.")
        if probability_flow:
            raise ValueError("Probability flow not supported by ancestral sampling")
        i = table_index(sde, t)
        if kind == 've':
            s2 = _discrete_sigma(sde, i) ** 2
            a2 = 0.0 if i == 0 else _discrete_sigma(sde, i - 1) ** 2
            return 1.0, s2 - a2, math.sqrt(a2 * (s2 - a2) / s2)
        beta = _discrete_beta(sde, i)
        return 1.0 / math.sqrt(1.0 - beta), beta / math.sqrt(1.0 - beta), math.sqrt(beta)
    if name == 'reverse_diffusion' and kind == 'vp':
        beta = _discrete_beta(sde, table_index(sde, t))
        return 2.0 - math.sqrt(1.0 - beta), k * beta, 0.0 if probability_flow else math.sqrt(beta)
    d, g = _drift_diffusion(sde, t)          # reverse_diffusion through SDE.discretize and euler_maruyama with dt = -1 / N agree
    return 1.0 - d / n, k * g * g / n, 0.0 if probability_flow else g * math.sqrt(1.0 / n)


def langevin_scale(sde, t, snr):
    """2 alpha snr^2: the Langevin step size is this times (mean_r |z_r|)^2."""
    kind = _kind(sde)
    if kind == 'subvp':
        raise NotImplementedError("corrector 'langevin' on subVPSDE: the reference reads sde.alphas, which subVPSDE does not have")
    alpha = 1.0 if kind == 've' else 1.0 - _discrete_beta(sde, table_index(sde, t))
    return 2.0 * alpha * float(snr) ** 2


def corrector_coefficients(sde, name, t, snr, noise_norm=None):
    """(a, b, c) of one corrector update at time ``t``.  'langevin' needs ``noise_norm`` = mean_r |z_r| of the noise of that update
    (on the device the step kernel reads it from idiff_sampler_noise_norm_f32's result)."""
    name = _name_of(name, 'corrector')
    if name == 'none':
        return 1.0, 0.0, 0.0
    if name == 'langevin':
        scale = langevin_scale(sde, t, snr)
        if noise_norm is None:
            raise ValueError("corrector 'langevin': the step size depends on the noise drawn; pass noise_norm")
        b = scale * float(noise_norm) ** 2
        return 1.0, b, math.sqrt(2.0 * b)
    if _kind(sde) == 'subvp':
        raise NotImplementedError("corrector 'ald' on subVPSDE: the reference reads sde.alphas, which subVPSDE does not have")
    alpha = 1.0 if _kind(sde) == 've' else 1.0 - _discrete_beta(sde, table_index(sde, t))
    b = (float(snr) * marginal_std(sde, t)) ** 2 * 2.0 * alpha
    return 1.0, b, math.sqrt(2.0 * b)


def prior_std(sde):
    if _kind(sde) == 've':
        if getattr(sde, 'diffused_mean', None) is not None:
            raise NotImplementedError("a VESDE prior around the data mean is not built")
        return float(sde.sigma_max)
    return 1.0


def build_schedule(sde, predictor, corrector, snr, n_steps, probability_flow, eps):
    """Everything the loop needs, before the first launch: per time step (t, label, std, corrector entry, predictor (a, b, c)).  The
    corrector entry is None, ('abc', a, b, c) or ('langevin', 2 alpha snr^2)."""
    check_vp_table(sde)
    pname, cname = _name_of(predictor, 'predictor'), _name_of(corrector, 'corrector')
    steps = []
    for t in time_grid(sde, eps):
        t = float(t)
        if cname == 'none' or n_steps < 1:
            corr = None
        elif cname == 'langevin':
            corr = ('langevin', langevin_scale(sde, t, snr))
        else:
            corr = ('abc',) + corrector_coefficients(sde, cname, t, snr)
        pred = None if pname == 'none' else predictor_coefficients(sde, pname, t, probability_flow)
        steps.append(dict(t=t, label=label_of(sde, t), std=marginal_std(sde, t), corrector=corr, predictor=pred))
    return steps


# ---------------------------------------------------------------------------------------------- the sampler
def _stream_key(seed, index, salt):
    from .train import stream_key
    return stream_key(seed, index, salt)


class _Noise:
    """Where an update's z comes from: the caller's draws in the reference's order of consumption, or the kernel's own stream."""

    def __init__(self, noise, seed, B, D, device):
        self.seed, self.B, self.D = seed, B, D
        self.prior, self.draws, self.used = None, None, 0
        if noise is not None:
            prior, draws = noise
            self.prior = torch.as_tensor(prior, dtype=torch.float32).reshape(B, D).to(device).contiguous()
            self.draws = torch.as_tensor(draws, dtype=torch.float32).reshape(-1, B, D).to(device).contiguous()

    def next(self, index, salt):
        """(z or None, key) for the update ``index`` of the stream ``salt``."""
        if self.draws is None:
            return None, _stream_key(self.seed, index, salt)
        if self.used >= self.draws.shape[0]:
            raise ValueError(f"noise=: {self.draws.shape[0]} draws given, the sampler needs more")
        z = self.draws[self.used]
        self.used += 1
        return z, 0


def _fcn_buffers(model, B):
    """Allocated once per (model, B): the padded input rows (the state), one activation buffer per hidden layer, the raw output, the
    mean, and the epilogues of the layers."""
    from . import _lib
    pk = model.packed()
    cache = pk.setdefault("sampler_buffers", {})
    if B not in cache:
        dev = pk["w"][0].device
        z = lambda r, c: torch.zeros(r, c, device=dev, dtype=torch.float32)
        last = len(pk["w"]) - 1
        cache[B] = dict(h=[z(B, pk["kpad"])] + [z(B, w.shape[0]) for w in pk["w"][:-1]], out=z(B, pk["w"][-1].shape[0]),
                        mean=z(B, pk["w"][-1].shape[0]),
                        ep=[_lib.make_epilogue(bias=b, act=None if i == last else "elu") for i, b in enumerate(pk["b"])])
    return pk, cache[B]


def get_pc_sampler(sde, shape, predictor, corrector, snr, n_steps=1, probability_flow=False, continuous=False, denoise=True, eps=1e-3):
    """unconditional.py:133-199.  Returns ``pc_sampler(model, show_evolution=False, *, seed=None, noise=None, fast=None)`` ->
    ``(samples, sampling_info)``; ``noise=(prior, draws)`` replays explicit N(0, 1) draws (prior [B, ...], draws [n, B, ...] in the
    reference's order: per time step the corrector's ``n_steps`` draws, then the predictor's one), otherwise the kernels draw from the
    streams of ``seed``.  ``fast`` forces (True) or forbids (False) the fcn path."""
    from . import _lib
    from .models import utils as mutils
    from .models.fcn import FCN
    shape = [int(v) for v in shape]
    B, D = shape[0], int(np.prod(shape[1:]))
    pname, cname = _name_of(predictor, 'predictor'), _name_of(corrector, 'corrector')
    n_steps = int(n_steps)
    schedule = build_schedule(sde, pname, cname, snr, n_steps, probability_flow, eps)
    has_corr = cname != 'none' and n_steps >= 1
    p_std = prior_std(sde)
    grids = {}                    # device -> the time grid there: uploaded once, so that a later call makes no blocking copy

    def pc_sampler(model, show_evolution=False, *, seed=None, noise=None, fast=None):
        device = model.device
        if device.type != 'cuda':
            raise RuntimeError(f"pc_sampler: the model is on {device}; id-diff_amd samples on the MI355X only (no CPU path)")
        use_fast = isinstance(model, FCN) and len(shape) == 2 and (FCN_FAST_PATH if fast is None else bool(fast))
        if fast and not use_fast:
            raise RuntimeError("pc_sampler: fast=True needs a models.fcn.FCN and [B, D] samples")
        if seed is None:
            seed = 42
        src = _Noise(noise, int(seed), B, D, device)
        if device not in grids:
            grids[device] = torch.from_numpy(time_grid(sde, eps)).to(device)
        times = grids[device]
        evolution = []
        ws = _lib.reduce_workspace(device) if cname == 'langevin' else None
        nn = torch.zeros((), device=device, dtype=torch.float64) if cname == 'langevin' else None

        with torch.no_grad():
            if use_fast:
                pk, buf = _fcn_buffers(model, B)
                x, raw, mean, ep = buf['h'][0], buf['out'], buf['mean'], buf['ep']
                x.zero_()
                layers = list(zip(pk["w"], ep))
                acts = buf['h'][1:] + [raw]
                ld_in = [x.stride(0)] + [a.stride(0) for a in buf['h'][1:]]
                label_col = D

                def evaluate(step):
                    src_rows = x
                    for (w, e), dst, lda in zip(layers, acts, ld_in):
                        _lib.gemm(src_rows, w, out=dst, epilogue=e, M=B, N=w.shape[0], K=w.shape[1], lda=lda, ldb=w.shape[1],
                                  ldc=dst.stride(0))
                        src_rows = dst
                    return raw, -1.0 / step['std']
            else:
                score_fn = mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=True)
                x = torch.zeros(B, D, device=device, dtype=torch.float32)
                mean = torch.zeros(B, D, device=device, dtype=torch.float32)
                ones = torch.ones(B, device=device, dtype=torch.float32)
                label_col = -1

                def evaluate(step):
                    return score_fn(x.view(shape), ones * times[step['i']]).reshape(B, D), 1.0

            def update(step, coef, z, key, label):
                s, scale = evaluate(step)
                if coef[0] == 'langevin':
                    _lib.sampler_noise_norm(z, B=B, D=D, seed=key, out=nn, workspace=ws, device=device)
                    _lib.sampler_step(x, s, 1.0, 0.0, 0.0, z=z, mean_out=mean, D=D, seed=key, noise_norm=nn, lang_scale=coef[1],
                                      score_scale=scale, label_col=label_col, label_value=label)
                else:
                    _lib.sampler_step(x, s, coef[1], coef[2], coef[3], z=z, mean_out=mean, D=D, seed=key, score_scale=scale,
                                      label_col=label_col, label_value=label)

            # the prior: x = p_std z (s = x is read as zeros), and the first time feature
            z, key = (src.prior, 0) if src.prior is not None else (None, _stream_key(src.seed, 0, SALT_PRIOR))
            _lib.sampler_step(x, x, 0.0, 0.0, p_std, z=z, D=D, seed=key, label_col=label_col, label_value=schedule[0]['label'])
            mean_is_x = True
            for i, step in enumerate(schedule):
                step['i'] = i
                nxt = schedule[i + 1]['label'] if i + 1 < len(schedule) else step['label']
                if has_corr:
                    for j in range(n_steps):
                        z, key = src.next(i * n_steps + j, SALT_CORRECTOR)
                        update(step, step['corrector'], z, key, step['label'])
                    mean_is_x = False
                if step['predictor'] is not None:
                    z, key = src.next(i, SALT_PREDICTOR)
                    update(step, ('abc',) + step['predictor'], z, key, nxt)
                    mean_is_x = False
                else:
                    mean_is_x = True                              # NonePredictor returns (x, x)
                if show_evolution:
                    evolution.append(x[:, :D].reshape(shape).cpu())
            samples = (x if mean_is_x or not denoise else mean)[:, :D].reshape(shape).clone()

        info = {'times': times.clone(), 'steps': sde.N * (n_steps + 1)}
        if show_evolution:
            info['evolution'] = torch.stack(evolution)
        return samples, info

    return pc_sampler


# ---------------------------------------------------------------------------------------------- the probability-flow ODE
def flow_coefficients(sde, t):
    """``(a, b, label, std)`` as fp64 host scalars: the reverse SDE's ``probability_flow=True`` drift at time t is a x + b raw with raw
    the fcn output (score = -raw / std): a = d, b = g^2 / (2 std), with d, g and std the fp64 expressions of the schedule evaluated at
    the fp32 value of t, the time the network's label carries (the reference's ``vec_t`` is fp32 too), and label the fp32 product
    ``label_of`` forms.  Coefficients at the unrounded t beside a label at the rounded one cost the VE sampler of the fixture ten times
    its deviation from the fp64 oracle."""
    t32 = float(np.float32(t))
    d, g = _drift_diffusion(sde, t32)
    std = marginal_std(sde, t32)
    return d, 0.5 * g * g / std, label_of(sde, t), std


def get_ode_sampler(sde, shape, denoise=False, rtol=1e-5, atol=1e-5, method='RK45', eps=1e-3):
    """unconditional.py:66-131 of the reference.  Returns ``ode_sampler(model, z=None, *, seed=None) -> (x, nfe)``: the
    probability-flow ODE integrated from sde.T to eps by ``ode.rk45`` (scipy's RK45 step control on the host, the state in fp64 on the
    device), from the latent code ``z`` or a draw of the prior from the stream of ``seed``.  A ``models.fcn.FCN`` with [B, D] samples runs
    its own launches (likelihood.FcnFlow); any other model ``get_score_fn`` accepts runs through its ``score_fn``.  ``denoise``: one
    noise-free reverse-diffusion step at eps."""
    from . import _lib, likelihood, ode
    from .models import utils as mutils
    from .models.fcn import FCN
    likelihood.check_method(method)
    _kind(sde)
    shape = [int(v) for v in shape]
    B, D = shape[0], int(np.prod(shape[1:]))
    p_std = prior_std(sde)
    eps = float(eps)

    def ode_sampler(model, z=None, *, seed=None):
        device = model.device
        if device.type != 'cuda':
            raise RuntimeError(f"ode_sampler: the model is on {device}; id-diff_amd samples on the MI355X only (no CPU path)")
        fast = isinstance(model, FCN) and len(shape) == 2
        with torch.no_grad():
            y = likelihood.state_buffer(B, D, device)
            if z is None:
                x0 = torch.zeros(B, D, device=device, dtype=torch.float32)
                _lib.sampler_step(x0, x0, 0.0, 0.0, p_std, D=D, seed=_stream_key(42 if seed is None else int(seed), 0, SALT_PRIOR))
            else:
                x0 = torch.as_tensor(z, dtype=torch.float32).to(device).reshape(B, D)
            y.copy_(x0.double())
            if fast:
                flow = likelihood.FcnFlow(likelihood.fcn_of(model), sde, B, aug=0)
                x32, rhs = flow.x32, flow.rhs

                def score_at_eps():
                    return flow.forward(), -1.0 / marginal_std(sde, eps)
            else:
                score_fn = mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=True)
                x32 = torch.zeros(B, (D + 1 + 3) // 4 * 4, device=device, dtype=torch.float32)
                ones = torch.ones(B, device=device, dtype=torch.float32)

                def score(t):
                    return score_fn(x32[:, :D].contiguous().view(shape), ones * float(np.float32(t))).reshape(B, D).contiguous()

                def rhs(stage, t, K, v=None):
                    d, g = _drift_diffusion(sde, float(np.float32(t)))
                    _lib.flow_rhs(x32, score(t), d, -0.5 * g * g, K[stage], D, 0)

                def score_at_eps():
                    return score(eps), 1.0
            K = torch.zeros(7, B, y.stride(0), device=device, dtype=torch.float64)[:, :, :D]
            nfe, _, _, _ = ode.rk45(rhs, float(sde.T), eps, y, x32, D, lambda t: label_of(sde, t), rtol=rtol, atol=atol, K=K)
            x = y.float()
            if denoise:
                _lib.rk_stage(y, K, [], x32, D, label_of(sde, eps))
                s, scale = score_at_eps()
                a, b, _ = predictor_coefficients(sde, 'reverse_diffusion', eps, False)
                mean = torch.zeros_like(x)
                _lib.sampler_step(x, s, a, b, 0.0, mean_out=mean, D=D, score_scale=scale)
                x = mean
            return x.reshape(shape).contiguous(), nfe

    return ode_sampler


def get_sampling_fn(config, sde, shape, eps):
    """unconditional.py:13-49; ``method == 'ode'`` (scipy's RK45 driven from the host) is not built."""
    s = sampling_config(config)
    method = str(s['method']).lower()
    if method == 'ode':
        raise NotImplementedError("sampling.method = 'ode': the probability-flow ODE sampler is not built (use method = 'pc')")
    if method != 'pc':
        raise ValueError(f"Sampler name {s['method']} unknown.")
    return get_pc_sampler(sde=sde, shape=shape, predictor=get_predictor(s['predictor']), corrector=get_corrector(s['corrector']),
                          snr=s['snr'], n_steps=s['n_steps_each'], probability_flow=s['probability_flow'],
                          continuous=bool(config.training.get('continuous', True)), denoise=s['noise_removal'], eps=eps)


def ksphere_evaluation(samples):
    """The numbers of the reference's KSphereEvaluation callback: minimum, maximum and mean of the samples' norms."""
    norms = torch.linalg.norm(torch.as_tensor(samples).reshape(len(samples), -1).double(), dim=1)
    return dict(min_norm=float(norms.min()), max_norm=float(norms.max()), mean_norm=float(norms.mean()))


def generate(config, checkpoint_path=None, num_samples=None, seed=None, log_path=None, log_name=None, log=print, sampler=None):
    """``--mode generate``: draw ``num_samples`` (default 1000, the callback's number) samples from the config's model on one GPU and
    write ``<log_path>/<log_name>/samples/samples.pkl`` = {samples, times, steps, min_norm, max_norm, mean_norm}.  ``sampler='ode'``
    draws them with the probability-flow ODE sampler instead of the config's (``--sampler ode``); the pickle then holds
    {samples, nfe, min_norm, max_norm, mean_norm}."""
    import os
    import pickle
    from .lightning_modules.utils import create_lightning_module
    device = torch.device(config.get('device', 'cuda:0'))
    module = create_lightning_module(config)
    module = module.load_from_checkpoint(checkpoint_path if checkpoint_path is not None else config.model.get('checkpoint_path'))
    module.configure_sde(config)
    module.to(device).eval()
    n = 1000 if num_samples is None else int(num_samples)
    if sampler not in (None, 'pc', 'ode'):
        raise ValueError(f"generate: sampler {sampler!r} unknown (have: 'pc', the config's sampler, and 'ode')")
    if sampler == 'ode':
        samples, nfe = module.ode_sample(num_samples=n, seed=seed)
        info = {'nfe': int(nfe)}
    else:
        samples, info = module.sample(num_samples=n, seed=seed)
    norms = ksphere_evaluation(samples)
    log_path = log_path if log_path is not None else (config.logging.get('log_path') or './')
    log_name = log_name if log_name is not None else (config.logging.get('log_name') or 'generate')
    path = os.path.join(log_path, log_name, 'samples', 'samples.pkl')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    record = dict(nfe=info['nfe']) if sampler == 'ode' else dict(times=info['times'].cpu().numpy(), steps=int(info['steps']))
    with open(path, 'wb') as f:
        pickle.dump(dict(samples=samples.cpu().numpy().astype(np.float32), **record, **norms), f)
    if log is not None:
        log(f"{n} samples: min_norm {norms['min_norm']:.6g} max_norm {norms['max_norm']:.6g} mean_norm {norms['mean_norm']:.6g}; wrote {path}")
    return samples, dict(info, **norms, path=path)
