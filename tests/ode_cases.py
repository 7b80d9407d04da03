"""What tests/golden/make_likelihood.py, tests/test_ode_host.py, tests/test_hip_ode.py and tests/test_hip_likelihood.py share: the cases
of the likelihood fixture, the oracle, and the shapes and bounds of the kernel tests.

The oracle is ``scipy.integrate.solve_ivp(method='RK45')`` driving a torch CPU copy of the network, the divergence by autograd, with
the SDE's drift, diffusion and std restated below in torch: it uses neither the reference nor the code under test.  Run in fp64 it is the
truth; run in fp32 (model, state rows, times, as the reference runs) its distance to the fp64 run is the yardstick: the GPU result must lie
within ``BAR`` of those deviations, per quantity, maximum over the batch (the convention of DESIGN.md 4.7 and 4.9).

The fixture (tests/golden/likelihood.npz) holds arrays only.  Per case ``<kind>-<hidden_layers>`` and divergence (``hutch`` / ``exact``):
the oracle's fp64 and fp32 runs (z, delta_logp, bpd, nfe), for VE the reference's own ``get_likelihood_fn`` (z, bpd, nfe); the same
for the ODE sampler from the fp64 latent code; the flow drift and the raw network output at three times; the data, the Rademacher draw
and the weights.
"""
import contextlib
import math
import os

import numpy as np

import sampling_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "likelihood.npz")

D, HIDDEN, B = sc.D, sc.HIDDEN, 8
RTOL = ATOL = 1e-5
BAR = 8.0
CASES = [('ve', 0), ('ve', 1), ('vp', 1), ('subvp', 1)]          # (SDE, model.hidden_layers: one or two hidden layers of 16)
DATA_SEED = {('ve', 0): 200, ('ve', 1): 201, ('vp', 1): 202, ('subvp', 1): 203}
DRIFT_TIMES = (0.125, 0.5, 1.0)                                   # exact in fp32: the rounding of t to fp32 changes nothing
EPS = sc.EPS
BAND = (0.95, 1.05)               # no attempted step's error norm may lie in here: only then is "equal nfe" a fair demand


def case_id(case):
    return f"{case[0]}-{case[1]}"


def make_sde(kind):
    return sc.make_sde(kind)


def fcn_config(case):
    c = sc.fcn_config(case[0])
    c.model.hidden_layers = case[1]
    return c


def load():
    return np.load(GOLDEN, allow_pickle=False)


def weights(fx, case):
    pre = f"{case_id(case)}::sd::"
    return {k[len(pre):]: fx[k] for k in fx.files if k.startswith(pre)}


def make_weights(case):
    """The case's network: nn.Linear's default initialisation under a fixed seed, the last layer scaled by 0.05 (sampling_cases)."""
    import torch
    widths = [D + 1] + [HIDDEN] * (case[1] + 1)
    gen = torch.Generator().manual_seed(300 + CASES.index(case))
    out, idx = {}, 0
    dims = list(zip(widths[:-1], widths[1:])) + [(HIDDEN, D)]
    for j, (a, b) in enumerate(dims):
        bound = 1.0 / math.sqrt(a)
        scale = sc.LAST_LAYER_SCALE if j == len(dims) - 1 else 1.0
        out[f"mlp.{idx}.weight"] = ((torch.rand(b, a, generator=gen) * 2 - 1) * bound * scale).numpy()
        out[f"mlp.{idx}.bias"] = ((torch.rand(b, generator=gen) * 2 - 1) * bound * scale).numpy()
        idx += 3
    return out


def make_data(case):
    rng = np.random.default_rng(DATA_SEED[case])
    x = rng.standard_normal((B, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), (rng.integers(0, 2, (B, D)) * 2 - 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the oracle
def torch_net(w, dtype):
    import torch
    keys = sorted({int(k.split('.')[1]) for k in w})
    layers = []
    for j, i in enumerate(keys):
        W = torch.as_tensor(np.asarray(w[f"mlp.{i}.weight"]))
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(W); lin.bias.copy_(torch.as_tensor(np.asarray(w[f"mlp.{i}.bias"])))
        layers.append(lin)
        if j < len(keys) - 1:
            layers.append(torch.nn.ELU())
    return torch.nn.Sequential(*layers).to(dtype).eval()


def sde_terms(kind, t, params=None):
    """(d, g, std) of the forward SDE at the torch times t, in t's dtype (``params``: other than sampling_cases' SDE parameters)."""
    import torch
    p = sc.SDE_PARAMS[kind] if params is None else params
    if kind == 've':
        lo, hi = p['sigma_min'], p['sigma_max']
        sigma = lo * (hi / lo) ** t
        return torch.zeros_like(t), sigma * math.sqrt(2 * math.log(hi / lo)), sigma
    b0, b1 = p['beta_min'], p['beta_max']
    beta = b0 + t * (b1 - b0)
    lmc = -0.25 * t ** 2 * (b1 - b0) - 0.5 * t * b0
    if kind == 'vp':
        return -0.5 * beta, torch.sqrt(beta), torch.sqrt(1. - torch.exp(2. * lmc))
    discount = 1. - torch.exp(-2 * b0 * t - (b1 - b0) * t ** 2)
    return -0.5 * beta, torch.sqrt(beta * discount), 1 - torch.exp(2. * lmc)


def flow_drift(net, kind, N, x, t, params=None):
    """(drift, raw) of the probability-flow ODE at the rows x and the times t [B]: d x - g^2 score / 2, score = -raw / std."""
    import torch
    d, g, std = sde_terms(kind, t, params)
    raw = net(torch.cat([x, (t * (N - 1))[:, None]], dim=1))
    score = -raw / std[:, None]
    return d[:, None] * x - 0.5 * g[:, None] ** 2 * score, raw


def prior_logp(kind, z, params=None):
    s2 = (sc.SDE_PARAMS['ve'] if params is None else params)['sigma_max'] ** 2 if kind == 've' else 1.0
    return -z.shape[1] / 2. * math.log(2 * math.pi * s2) - (z ** 2).sum(1) / (2 * s2)


@contextlib.contextmanager
def recorded_error_norms():
    """Every error norm scipy's RK45 computes inside the block, in order."""
    from scipy.integrate._ivp import rk
    seen, orig = [], rk.RungeKutta._estimate_error_norm

    def wrapped(self, K, h, scale):
        v = orig(self, K, h, scale)
        seen.append(float(v))
        return v
    rk.RungeKutta._estimate_error_norm = wrapped
    try:
        yield seen
    finally:
        rk.RungeKutta._estimate_error_norm = orig


def oracle_likelihood(w, kind, data, dtype, exact, epsilon=None, eps=None, N=sc.N_STEPS, rtol=RTOL, atol=ATOL, params=None):
    """dict(z, delta_logp, bpd [fp64 numpy, computed in ``dtype`` as the reference computes them], nfe, error_norms): the reference's
    likelihood_fn restated: state [B D rows, then B log p] flat in fp64 numpy, rows and times cast to ``dtype`` per evaluation."""
    import torch
    from scipy import integrate
    net = torch_net(w, dtype)
    data = torch.as_tensor(np.asarray(data)).to(dtype)
    Bn, Dn = data.shape
    e = None if exact else torch.as_tensor(np.asarray(epsilon)).to(dtype)
    eps = EPS[kind] if eps is None else eps

    def ode_func(t, x):
        sample = torch.from_numpy(x[:-Bn].reshape(Bn, Dn)).to(dtype).requires_grad_(True)
        vec_t = torch.ones(Bn, dtype=dtype) * t
        with torch.enable_grad():
            drift, _ = flow_drift(net, kind, N, sample, vec_t, params)
            if exact:
                div = sum(torch.autograd.grad(drift[:, i].sum(), sample, retain_graph=True)[0][:, i] for i in range(Dn))
            else:
                div = (torch.autograd.grad((drift * e).sum(), sample)[0] * e).sum(1)
        return np.concatenate([drift.detach().numpy().reshape(-1), div.detach().numpy().reshape(-1)]).astype(np.float64)

    init = np.concatenate([data.numpy().reshape(-1).astype(np.float64), np.zeros(Bn)])
    with recorded_error_norms() as norms:
        sol = integrate.solve_ivp(ode_func, (eps, 1.0), init, rtol=rtol, atol=atol, method='RK45')
    zp = sol.y[:, -1]
    z = torch.from_numpy(zp[:-Bn].reshape(Bn, Dn)).to(dtype)
    delta = torch.from_numpy(zp[-Bn:].copy()).to(dtype)
    bpd = -(prior_logp(kind, z, params) + delta)
    return dict(z=z.double().numpy(), delta_logp=delta.double().numpy(), bpd=bpd.double().numpy(), nfe=int(sol.nfev),
                error_norms=list(norms), z64=zp[:-Bn].reshape(Bn, Dn).copy())


def oracle_sample(w, kind, z, dtype, eps=None, N=sc.N_STEPS, rtol=RTOL, atol=ATOL, params=None):
    """dict(x, nfe, error_norms): the reference's ode_sampler restated, from the latent code z, T -> eps."""
    import torch
    from scipy import integrate
    net = torch_net(w, dtype)
    z = np.asarray(z)
    Bn, Dn = z.shape
    eps = EPS[kind] if eps is None else eps

    def ode_func(t, x):
        with torch.no_grad():
            drift, _ = flow_drift(net, kind, N, torch.from_numpy(x.reshape(Bn, Dn)).to(dtype), torch.ones(Bn, dtype=dtype) * t, params)
        return drift.numpy().reshape(-1).astype(np.float64)

    with recorded_error_norms() as norms:
        sol = integrate.solve_ivp(ode_func, (1.0, eps), torch.as_tensor(z).to(dtype).numpy().reshape(-1).astype(np.float64), rtol=rtol,
                                  atol=atol, method='RK45')
    x = torch.from_numpy(sol.y[:, -1].reshape(Bn, Dn)).to(dtype)
    return dict(x=x.double().numpy(), nfe=int(sol.nfev), error_norms=list(norms))


def outside_band(norms):
    return all(not (BAND[0] <= v <= BAND[1]) for v in norms)


def same_steps(a, b):
    """Two runs took the same steps: the same attempts, each accepted or rejected alike."""
    return len(a) == len(b) and all((u < 1) == (v < 1) for u, v in zip(a, b))


# ---------------------------------------------------------------------------------------------- kernel tests
SHAPES = [(1, 1, 1), (5, 6, 0), (5, 6, 1), (33, 7, 1), (130, 100, 1)]                  # (B, D, aug)
TRACE_SHAPES = [(1, 1, 4), (3, 6, 16), (5, 100, 132)]                                     # (P, D, H)
# (B, W) of the reduction: below one block's share; a ragged last block; more blocks' worth than the workspace holds doubles
REDUCE_SHAPES = [(7, 9), (37, 101), (4100, 257)]
U32, U64 = 2.0 ** -24, 2.0 ** -53


def sum_bound(terms):
    """|computed - exact| of a sum of ``terms`` [n, ...] evaluated in fp64 with one rounding per operation: (n + 1) 2^-53 sum |terms|."""
    terms = np.abs(np.asarray(terms, dtype=np.longdouble))
    return np.asarray((terms.shape[0] + 1) * U64 * terms.sum(0), dtype=np.float64)


LD = np.longdouble


def stage_ref(y, K, c):
    """(v, bound) of rk_stage in longdouble: v = y + sum_j c_j K_j, |computed - v| <= (ns + 2) 2^-53 (|y| + sum_j |c_j K_j|)."""
    terms = np.stack([np.asarray(y, dtype=LD)] + [LD(cj) * np.asarray(K[j], dtype=LD) for j, cj in enumerate(c)])
    return terms.sum(0), sum_bound(terms)


def error_ref(K, e, y, y_new, atol, rtol, scale_fn=np.maximum):
    """(sum, bound) of rk_error in longdouble.  Per element the numerator is a sum of 7 terms, the scale costs three roundings, the
    quotient one and the square one; the sum of n squares goes through at most ``path`` additions (a lane's share, two trees)."""
    terms = np.stack([LD(ej) * np.asarray(K[j], dtype=LD) for j, ej in enumerate(e)])
    err = terms.sum(0)
    scale = LD(atol) + LD(rtol) * scale_fn(np.abs(np.asarray(y, dtype=LD)), np.abs(np.asarray(y_new, dtype=LD)))
    q = err / scale
    dq = sum_bound(terms) / scale + 4 * U64 * np.abs(q)
    n = err.size
    per = -(-n // min(1024, max(1, -(-n // 1024))))
    path = -(-per // 256) + 8 + 4 + 8 + 2
    total = (q * q).sum()
    return total, float((2 * np.abs(q) * dq + 2 * U64 * q * q).sum() + path * U64 * total)


def rhs_ref(x32, v, a, b, Dn, aug, eps=None, u=None, q=None, a_term=True):
    """(K_s [B, D + aug], bound) of flow_rhs in longdouble; ``a_term=False`` drops a D from the log p column (a mutation)."""
    x, vv = np.asarray(x32, dtype=LD)[:, :Dn], np.asarray(v, dtype=LD)[:, :Dn]
    ref = LD(a) * x + LD(b) * vv
    bound = np.asarray(3 * U64 * (np.abs(LD(a) * x) + np.abs(LD(b) * vv)), dtype=np.float64)
    if aug:
        if q is None:
            prod = np.asarray(eps, dtype=LD)[:, :Dn] * np.asarray(u, dtype=LD)[:, :Dn]
            qq, qb = prod.sum(1), sum_bound(prod.T)
        else:
            qq, qb = np.asarray(q, dtype=LD), 0.0
        last = (LD(a) * Dn if a_term else LD(0)) + LD(b) * qq
        lb = 3 * U64 * (abs(LD(a) * Dn) + np.abs(LD(b) * qq)) + abs(LD(b)) * qb
        ref = np.concatenate([ref, last[:, None]], axis=1)
        bound = np.concatenate([bound, np.asarray(lb, dtype=np.float64)[:, None]], axis=1)
    return ref, bound


def trace_ref(T, W):
    """(tr [P], bound) of jvp_trace in longdouble: T [P, D, N], W [D, N]."""
    prod = np.asarray(T, dtype=LD) * np.asarray(W, dtype=LD)[None]
    flat = prod.reshape(prod.shape[0], -1)
    return flat.sum(1), sum_bound(flat.T)
