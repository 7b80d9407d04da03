"""Generate tests/golden/sampling.npz by RUNNING the reference's sampler on the CPU.

Run once, where the reference checkout that make_golden.py imports from exists::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sampling.py

The reference's sampling.predictors, sampling.correctors and sampling.unconditional are imported as they are (make_golden.py supplies
the stand-ins for the packages they import at module level).  Nothing of the reference is copied: the file holds arrays only.

Per case of tests/sampling_cases.py (a tiny fcn, D = 6, one hidden layer of 16, 40 steps, 5 rows; last layer scaled by 0.05):
the N(0, 1) draws in the order consumed (torch.randn_like is patched to record), the state x and x_mean after every corrector and
predictor update of the reference in fp32, and the same loop re-run with model, state and times in fp64 on the same draws (stored as
fp32 differences to the fp32 arrays, sampling_cases.trajectory).  The loop is unconditional.py:175-189 driven update by update so that
the intermediate states can be recorded; the fp32 result is checked bit for bit against the reference's own ``get_pc_sampler`` on
the same draws.  Also: the weights, the prior draw, the fp32 time grids, the table indices long(t (N - 1) / T), and the largest
nearest-point distance of 128 samples the reference's ``get_pc_sampler`` draws through an fp64 restatement of the empirical score of
the circle cloud (the bar of the acceptance test).
"""
import copy
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

for _missing in ("tqdm", "scipy"):
    try:
        __import__(_missing)
    except Exception:
        _m = types.ModuleType(_missing)
        _m.tqdm = lambda it, *a, **k: it
        _m.integrate = types.ModuleType("scipy.integrate")
        sys.modules[_missing] = _m
        sys.modules["scipy.integrate"] = _m.integrate

import make_golden as mg  # noqa: E402  (installs the stand-ins, puts the reference on sys.path)
import sampling_cases as sc  # noqa: E402

from sampling import predictors as ref_pred, correctors as ref_corr, unconditional as ref_unc  # noqa: E402  (reference)

ref_unc.tqdm = lambda it, *a, **k: it
sde_lib, mutils = mg.sde_lib, mg.mutils


def ref_sde(kind, N=sc.N_STEPS):
    p = sc.SDE_PARAMS[kind]
    if kind == 've':
        return sde_lib.VESDE(sigma_min=p['sigma_min'], sigma_max=p['sigma_max'], N=N)
    return (sde_lib.VPSDE if kind == 'vp' else sde_lib.subVPSDE)(beta_min=p['beta_min'], beta_max=p['beta_max'], N=N)


def ref_model():
    cfg = mg.ConfigDict()
    cfg.model = mg.ConfigDict(name="fcn", state_size=sc.D, hidden_layers=sc.HIDDEN_LAYERS, hidden_nodes=sc.HIDDEN, dropout=0.0)
    torch.manual_seed(0)
    model = mutils.create_model(cfg)
    with torch.no_grad():
        last = [m for m in model.mlp if isinstance(m, torch.nn.Linear)][-1]
        last.weight.mul_(sc.LAST_LAYER_SCALE); last.bias.mul_(sc.LAST_LAYER_SCALE)
    return model.eval()


class Draws:
    """torch.randn_like patched: records fresh fp32 draws, or replays given ones, in the dtype of the state."""

    def __init__(self, seed=None, replay=None):
        self.gen = None if seed is None else torch.Generator().manual_seed(seed)
        self.replay, self.taken = replay, []

    def __call__(self, x, *a, **k):
        z = torch.randn(x.shape, generator=self.gen) if self.replay is None else self.replay[len(self.taken)]
        self.taken.append(z)
        return z.to(x.dtype)

    def __enter__(self):
        self.orig = torch.randn_like
        torch.randn_like = self
        return self

    def __exit__(self, *exc):
        torch.randn_like = self.orig


def run_case(case, model, prior_z, dtype, replay=None, seed=None):
    kind, pred, corr, pf = case
    sde = ref_sde(kind)
    model = copy.deepcopy(model).to(dtype)
    P, C = ref_pred.get_predictor(pred), ref_corr.get_corrector(corr)
    times = torch.linspace(sde.T, sc.EPS[kind], sde.N)
    x = (prior_z.to(dtype) * (sc.SDE_PARAMS['ve']['sigma_max'] if kind == 've' else 1.0))
    xs, xms = [], []
    with Draws(seed=seed, replay=replay) as draws, torch.no_grad():
        for i in range(sde.N):
            vec_t = torch.ones(sc.B, dtype=dtype) * times[i].to(dtype)
            x, xm = ref_unc.shared_corrector_update_fn(x, vec_t, sde=sde, model=model, corrector=C, continuous=True, snr=sc.SNR, n_steps=1)
            if corr != 'none':
                xs.append(x); xms.append(xm)
            x, xm = ref_unc.shared_predictor_update_fn(x, vec_t, sde=sde, model=model, predictor=P, probability_flow=pf, continuous=True)
            xs.append(x); xms.append(xm)
    assert all(v.dtype == dtype for v in xs + xms), case
    return torch.stack(draws.taken), torch.stack(xs), torch.stack(xms)


def check_against_pc_sampler(case, model, prior_z, draws, want):
    """The reference's own get_pc_sampler on the same draws gives the recorded fp32 samples bit for bit."""
    kind, pred, corr, pf = case
    sde = ref_sde(kind)
    sampler = ref_unc.get_pc_sampler(sde, (sc.B, sc.D), ref_pred.get_predictor(pred), ref_corr.get_corrector(corr), sc.SNR, n_steps=1,
                                     probability_flow=pf, continuous=True, denoise=True, eps=sc.EPS[kind])
    orig = torch.randn
    torch.randn = lambda *a, **k: prior_z.clone()
    try:
        with Draws(replay=draws):
            got, info = sampler(model)
    finally:
        torch.randn = orig
    assert torch.equal(got, want), case
    assert info['steps'] == sde.N * 2


class EmpiricalTorch(torch.nn.Module):
    """fp64 restatement of the empirical score in the model convention score = -out / std: out = -sigma (sum_i w_i x_i - x) / sigma^2."""

    def __init__(self, cloud, sigma_min, sigma_max, N):
        super().__init__()
        self.cloud = torch.nn.Parameter(torch.as_tensor(cloud, dtype=torch.float64), requires_grad=False)
        self.lo, self.hi, self.N = sigma_min, sigma_max, N

    @property
    def device(self):
        return self.cloud.device

    def forward(self, x, labels):
        t = labels.double() / (self.N - 1)
        sigma = self.lo * (self.hi / self.lo) ** t
        d = self.cloud[None] - x.double()[:, None]
        w = torch.softmax(-(d * d).sum(-1) / (2 * sigma[:, None] ** 2), dim=1)
        return (-(w[..., None] * d).sum(1) / sigma[:, None]).to(x.dtype)


def gen_empirical(out):
    e = sc.EMP
    cloud = sc.empirical_cloud()
    sde = sde_lib.VESDE(sigma_min=e['sigma_min'], sigma_max=e['sigma_max'], N=e['N'])
    sampler = ref_unc.get_pc_sampler(sde, (e['samples'], e['ambient']), ref_pred.get_predictor('reverse_diffusion'),
                                     ref_corr.get_corrector('none'), 0.15, n_steps=1, probability_flow=False, continuous=True,
                                     denoise=True, eps=1e-5)
    torch.manual_seed(e['seed'])
    samples, _ = sampler(EmpiricalTorch(cloud, e['sigma_min'], e['sigma_max'], e['N']))
    dist = sc.nearest_distance(samples.numpy(), cloud)
    spacing = float(np.linalg.norm(cloud[1].astype(np.float64) - cloud[0].astype(np.float64)))
    print(f"empirical: max nearest-point distance {dist.max():.3e} (mean {dist.mean():.3e}), neighbour spacing {spacing:.3e}, "
          f"bar 3 x = {3 * dist.max():.3e} vs half spacing {spacing / 2:.3e}")
    assert np.isfinite(dist).all() and 3 * dist.max() < spacing / 2, "lower EMP['sigma_min']"
    out["emp::cloud"], out["emp::max_dist"], out["emp::spacing"] = cloud, np.array(dist.max()), np.array(spacing)
    out["emp::params"] = np.array([e['sigma_min'], e['sigma_max'], e['N'], e['samples']], dtype=np.float64)


def main():
    torch.set_num_threads(4)
    model = ref_model()
    out = mg.sd_arrays(model)
    prior_z = torch.randn(sc.B, sc.D, generator=torch.Generator().manual_seed(100))
    out["prior_z"] = prior_z.numpy()
    for kind in sc.SDE_PARAMS:
        sde = ref_sde(kind)
        t32 = torch.linspace(sde.T, sc.EPS[kind], sde.N)
        idx32 = (t32 * (sde.N - 1) / sde.T).long()
        assert torch.equal(idx32, (t32.double() * (sde.N - 1) / sde.T).long()), "the fp64 re-run would read other table entries"
        out[f"times::{kind}"], out[f"index::{kind}"] = t32.numpy(), idx32.numpy()
    for n, case in enumerate(sc.CASES):
        cid = sc.case_id(case)
        draws, x32, xm32 = run_case(case, model, prior_z, torch.float32, seed=1000 + n)
        again, x64, xm64 = run_case(case, model, prior_z, torch.float64, replay=list(draws))
        assert torch.equal(draws, again) and len(draws) == len(sc.updates(case)) == len(x32)
        check_against_pc_sampler(case, model, prior_z, list(draws), xm32[-1])
        assert torch.isfinite(x32).all() and torch.isfinite(x64).all(), cid
        gap = (x32.double() - x64).abs().amax(dim=(1, 2))
        print(f"{cid:44s} updates {len(draws):3d}  max|x| {float(x64.abs().max()):9.3f}  fp32-fp64 gap at the end {float(gap[-1]):.2e}")
        out[f"{cid}::draws"], out[f"{cid}::x32"], out[f"{cid}::xm32"] = draws.numpy(), x32.numpy(), xm32.numpy()
        out[f"{cid}::dx64"] = (x64 - x32.double()).float().numpy()
        out[f"{cid}::dxm64"] = (xm64 - xm32.double()).float().numpy()
    gen_empirical(out)
    mg.save("sampling.npz", **out)


if __name__ == "__main__":
    main()
