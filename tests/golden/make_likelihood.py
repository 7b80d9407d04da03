"""Generate tests/golden/likelihood.npz by RUNNING the reference's likelihood and ODE sampler on the CPU, and the oracle beside them.

Run once, where the reference checkout that make_golden.py imports from exists::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_likelihood.py

The reference's ``likelihood.get_likelihood_fn`` and ``sampling.unconditional.get_ode_sampler`` are imported as they are (make_golden.py
supplies the stand-ins for the packages they import at module level).  Nothing of the reference is copied: the file holds arrays only.

Per case of tests/ode_cases.py (a tiny fcn, D = 6, one or two hidden layers of 16, last layer scaled by 0.05, 8 rows on the unit sphere)
and per divergence (Hutchinson with a recorded Rademacher draw, exact): the oracle of ode_cases in fp64 and in fp32; for the VE cases
also the reference's own result (its VP and subVP ``prior_logp`` sum dim=(1, 2, 3) and raise on [B, D] rows).  The same for the ODE
sampler started from the fp64 latent code.  The flow drift and the raw network output at three times in fp64: the reference's
``rsde.sde`` for VE, the oracle's for VP and subVP.  The largest nearest-point distance of 128 samples the reference's
``get_ode_sampler`` draws through the fp64 restatement of the empirical score of the circle cloud (the bar of the generic-path test).

Asserted here, so that "equal nfe" is a fair demand on the GPU: no attempted step of any run, fp64 or fp32, has an error norm in
ode_cases.BAND, the two runs take the same steps, and the reference takes as many evaluations as the oracle.  If a case misses this,
change its data seed in ode_cases.DATA_SEED; do not loosen the band.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

import make_golden as mg  # noqa: E402  (installs the stand-ins, puts the reference on sys.path)
import make_sampling as ms  # noqa: E402  (the fp64 empirical score, the reference's SDEs)
import ode_cases as oc  # noqa: E402
import sampling_cases as sc  # noqa: E402

import likelihood as ref_lik  # noqa: E402  (reference)
from sampling import unconditional as ref_unc  # noqa: E402  (reference)

sde_lib, mutils = mg.sde_lib, mg.mutils


def ref_model(case, w):
    cfg = mg.ConfigDict()
    cfg.model = mg.ConfigDict(name="fcn", state_size=oc.D, hidden_layers=case[1], hidden_nodes=oc.HIDDEN, dropout=0.0)
    model = mutils.create_model(cfg)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in w.items()}, strict=True)
    return model.eval()


class FixedRademacher:
    """torch.randint_like patched so that the reference's ``randint_like(...).float() * 2 - 1`` is the recorded draw."""

    def __init__(self, epsilon):
        self.bits = (torch.as_tensor(epsilon) + 1) / 2

    def __enter__(self):
        self.orig = torch.randint_like
        torch.randint_like = lambda x, *a, **k: self.bits.to(x.dtype)

    def __exit__(self, *exc):
        torch.randint_like = self.orig


def check_runs(cid, r64, r32):
    assert oc.outside_band(r64['error_norms']) and oc.outside_band(r32['error_norms']), \
        (cid, "an error norm inside the band: change the data seed", r64['error_norms'], r32['error_norms'])
    assert oc.same_steps(r64['error_norms'], r32['error_norms']) and r64['nfe'] == r32['nfe'], (cid, "the fp32 run takes other steps")


def gen_case(case, out):
    kind, cid = case[0], oc.case_id(case)
    w = oc.make_weights(case)
    data, epsilon = oc.make_data(case)
    for k, v in w.items():
        out[f"{cid}::sd::{k}"] = v
    out[f"{cid}::data"], out[f"{cid}::epsilon"] = data, epsilon
    sde = ms.ref_sde(kind)
    model = ref_model(case, w) if kind == 've' else None
    for name, exact in (('hutch', False), ('exact', True)):
        r64 = oc.oracle_likelihood(w, kind, data, torch.float64, exact, epsilon)
        r32 = oc.oracle_likelihood(w, kind, data, torch.float32, exact, epsilon)
        check_runs(f"{cid}::{name}", r64, r32)
        for q in ('z', 'delta_logp', 'bpd'):
            out[f"{cid}::{name}::{q}64"], out[f"{cid}::{name}::{q}32"] = r64[q], r32[q]
        out[f"{cid}::{name}::nfe"] = np.array(r64['nfe'])
        line = f"{cid:10s} {name:5s} nfe {r64['nfe']:3d} steps {len(r64['error_norms']):2d}  fp32-fp64: z {np.abs(r32['z'] - r64['z']).max():.1e} " \
               f"logp {np.abs(r32['delta_logp'] - r64['delta_logp']).max():.1e} bpd {np.abs(r32['bpd'] - r64['bpd']).max():.1e}"
        if model is not None:
            with FixedRademacher(epsilon):
                bpd, z, nfe = ref_lik.get_likelihood_fn(sde, exact=exact, eps=oc.EPS[kind], rtol=oc.RTOL, atol=oc.ATOL)(model, torch.as_tensor(data))
            assert nfe == r64['nfe'], (cid, name, "the reference takes other steps than the oracle", nfe, r64['nfe'])
            out[f"{cid}::{name}::ref_bpd"], out[f"{cid}::{name}::ref_z"] = bpd.numpy(), z.numpy()
            line += f"  reference-oracle32: z {np.abs(z.numpy() - r32['z']).max():.1e} bpd {np.abs(bpd.numpy() - r32['bpd']).max():.1e}"
        print(line)
    # the sampler back from the fp64 latent code of the exact run
    z64 = out[f"{cid}::exact::z64"]
    s64, s32 = oc.oracle_sample(w, kind, z64, torch.float64), oc.oracle_sample(w, kind, z64, torch.float32)
    check_runs(f"{cid}::sample", s64, s32)
    out[f"{cid}::sample::x64"], out[f"{cid}::sample::x32"], out[f"{cid}::sample::nfe"] = s64['x'], s32['x'], np.array(s64['nfe'])
    line = f"{cid:10s} sample nfe {s64['nfe']:3d}  fp32-fp64 {np.abs(s32['x'] - s64['x']).max():.1e}  round trip {np.abs(s64['x'] - data).max():.1e}"
    if model is not None:
        x, nfe = ref_unc.get_ode_sampler(sde, (oc.B, oc.D), eps=oc.EPS[kind], rtol=oc.RTOL, atol=oc.ATOL)(model, torch.as_tensor(z64).float())
        assert nfe == s64['nfe'], (cid, "the reference's sampler takes other steps than the oracle", nfe, s64['nfe'])
        out[f"{cid}::sample::ref_x"] = x.numpy()
        line += f"  reference-oracle32 {np.abs(x.numpy() - s32['x']).max():.1e}"
    print(line)
    # the drift at three times, fp64
    x = torch.as_tensor(data).double()
    drifts, raws = [], []
    for t in oc.DRIFT_TIMES:
        vec_t = torch.ones(oc.B, dtype=torch.float64) * t
        if model is not None:
            m64 = ref_model(case, w).double()
            with torch.no_grad():
                score_fn = mutils.get_score_fn(sde, m64, train=False, continuous=True)
                drifts.append(sde.reverse(score_fn, probability_flow=True).sde(x, vec_t)[0].numpy())
                raws.append(m64(x, vec_t * (sde.N - 1)).numpy())
        else:
            with torch.no_grad():
                dr, raw = oc.flow_drift(oc.torch_net(w, torch.float64), kind, sde.N, x, vec_t)
            drifts.append(dr.numpy()); raws.append(raw.numpy())
    out[f"{cid}::drift"], out[f"{cid}::raw"] = np.stack(drifts), np.stack(raws)


def gen_empirical(out):
    e = sc.EMP
    cloud = sc.empirical_cloud()
    sde = sde_lib.VESDE(sigma_min=e['sigma_min'], sigma_max=e['sigma_max'], N=e['N'])
    sampler = ref_unc.get_ode_sampler(sde, (e['samples'], e['ambient']), eps=1e-5, rtol=oc.RTOL, atol=oc.ATOL)
    torch.manual_seed(e['seed'])
    samples, nfe = sampler(ms.EmpiricalTorch(cloud, e['sigma_min'], e['sigma_max'], e['N']))
    dist = sc.nearest_distance(samples.numpy(), cloud)
    spacing = float(np.linalg.norm(cloud[1].astype(np.float64) - cloud[0].astype(np.float64)))
    print(f"empirical (ode): nfe {nfe}, max nearest-point distance {dist.max():.3e} (mean {dist.mean():.3e}), bar 3 x = {3 * dist.max():.3e} "
          f"vs half spacing {spacing / 2:.3e}")
    assert np.isfinite(dist).all() and 3 * dist.max() < spacing / 2
    out["emp::max_dist"], out["emp::spacing"] = np.array(dist.max()), np.array(spacing)


def main():
    torch.set_num_threads(4)
    out = {}
    for case in oc.CASES:
        gen_case(case, out)
    gen_empirical(out)
    mg.save("likelihood.npz", **out)


if __name__ == "__main__":
    main()
