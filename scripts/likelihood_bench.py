"""Time the likelihood of an fcn network (csrc/ode.hip, ode.py, likelihood.py) beside the reference's formulation on the same card.

    python scripts/likelihood_bench.py --case paper|small --arm hip|torch [--reps 3] [--out profiles/likelihood_bench.txt]

One (case, arm) a process: start the arms in fresh processes, interleaved, each under its own time limit, and nothing after one that
failed; the lines are APPENDED to --out.  Cases: paper = the paper's k-sphere shape (configs/.../ksphere/10dim.py: D = 100,
Linear(101, 2048), 5 x Linear(2048, 2048), Linear(2048, 100)), small = configs/.../ksphere/train_small.py (D = 8, 128 x 2).  Random
weights with the last layer scaled by 0.05 (the arithmetic does not depend on them; an untrained full-scale output makes the flow stiff),
B = 1000 points of the unit sphere, VE, rtol = atol = 1e-5, one Rademacher probe a row.

  hip     likelihood.get_likelihood_fn: whole call (wall clock around a synchronise) for Hutchinson and for the exact divergence, nfe,
          and one right-hand side of each kind alone (a window of back-to-back calls between two device events)
  torch   the reference's formulation: scipy.integrate.solve_ivp driving a torch nn.Sequential copy of the network on the same card,
          the state crossing to the host as a flat fp64 vector at every evaluation, the divergence by autograd (one backward for
          Hutchinson, D backwards for exact); whole call, nfe, and one right-hand side of each kind

Medians over --reps after one warm-up call.  The ratio is recorded whichever way it falls; it is not a pass condition.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import id_diff_amd  # noqa: E402,F401
from id_diff_amd import likelihood, sde_lib  # noqa: E402
from id_diff_amd.configs.utils import read_config  # noqa: E402
from id_diff_amd.models.fcn import FCN  # noqa: E402

KSPHERE = "configs/dimension_estimation/paper/euclidean_data/ksphere/"
CASES = {"paper": KSPHERE + "10dim.py", "small": KSPHERE + "train_small.py"}
B, RTOL, ATOL, EPS = 1000, 1e-5, 1e-5, 1e-5


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def torch_arm(model, sde, data, epsilon, exact, D):
    """The reference's likelihood_fn on a plain torch copy of the network: (whole-call function, one-rhs function)."""
    from scipy import integrate
    linears = [l for l in model.mlp if isinstance(l, torch.nn.Linear)]
    layers = []
    for i, l in enumerate(linears):
        layers.append(l)
        if i < len(linears) - 1:
            layers.append(torch.nn.ELU())
    net = torch.nn.Sequential(*layers)
    lo, hi, n = float(sde.sigma_min), float(sde.sigma_max), sde.N
    Bn = data.shape[0]

    def drift(x, t):
        sigma = lo * (hi / lo) ** t
        g2 = sigma * sigma * 2 * np.log(hi / lo)
        raw = net(torch.cat([x, (t * (n - 1))[:, None]], dim=1))
        return 0.5 * g2[:, None] * raw / sigma[:, None]

    def rhs(t, x):
        with torch.enable_grad():
            sample = torch.from_numpy(x[:-Bn].reshape(Bn, D)).to(data.device).float().requires_grad_(True)
            vec_t = torch.ones(Bn, device=data.device) * t
            dr = drift(sample, vec_t)
            if exact:
                div = sum(torch.autograd.grad(dr[:, i].sum(), sample, retain_graph=True)[0][:, i] for i in range(D))
            else:
                div = (torch.autograd.grad((dr * epsilon).sum(), sample)[0] * epsilon).sum(1)
        return np.concatenate([dr.detach().cpu().numpy().reshape(-1), div.detach().cpu().numpy().reshape(-1)]).astype(np.float64)

    init = np.concatenate([data.cpu().numpy().reshape(-1).astype(np.float64), np.zeros(Bn)])

    def whole():
        sol = integrate.solve_ivp(rhs, (EPS, 1.0), init, rtol=RTOL, atol=ATOL, method='RK45')
        return sol.nfev
    return whole, lambda: rhs(0.5, init)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=sorted(CASES))
    ap.add_argument("--arm", required=True, choices=("hip", "torch"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihood_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "likelihood_bench needs the MI355X"
    dev = torch.device("cuda:0")
    config = read_config(CASES[args.case])
    config.training.sde = 'vesde'
    D, H, L = config.model.state_size, config.model.hidden_nodes, config.model.hidden_layers
    lines = []

    def emit(obj):
        line = obj if isinstance(obj, str) else json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    torch.manual_seed(0)
    model = FCN(config).to(dev).eval()
    with torch.no_grad():
        last = [l for l in model.mlp if isinstance(l, torch.nn.Linear)][-1]
        last.weight.mul_(0.05); last.bias.mul_(0.05)
    sde, _ = sde_lib.configure_sde(config)
    x = torch.randn(B, D, generator=torch.Generator().manual_seed(1))
    data = (x / x.norm(dim=1, keepdim=True)).contiguous().to(dev)
    epsilon = (torch.randint(0, 2, (B, D), generator=torch.Generator().manual_seed(2)).float() * 2 - 1).to(dev)
    emit(f"case {args.case} arm {args.arm}: device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, B = {B}, D = {D}, "
         f"{L + 1} x Linear(., {H}) + ELU, VE sigma {sde.sigma_min} .. {sde.sigma_max}, rtol = atol = {RTOL}")
    for name, exact in (("hutchinson", False), ("exact", True)):
        if args.arm == "hip":
            fn = likelihood.get_likelihood_fn(sde, exact=exact, rtol=RTOL, atol=ATOL, eps=EPS)
            whole = lambda: fn(model, data, epsilon=epsilon)[2]
            flow = likelihood.FcnFlow(model, sde, B, aug=1, exact=exact, eps=None if exact else epsilon)
            flow.x32[:, :D] = data
            K = torch.zeros(7, B, D + 2, dtype=torch.float64, device=dev)[:, :, :D + 1]
            one = lambda: flow.rhs(0, 0.5, K)
            rhs_ms = lambda: window(one, 5)
        else:
            whole, one = torch_arm(model, sde, data, epsilon, exact, D)
            rhs_ms = lambda: wall(one)[0]
        whole_ms, rhs = [], []
        nfe = None
        for rep in range(1 + args.reps):
            ms, nfe = wall(whole)
            r = rhs_ms()
            if rep >= 1:
                whole_ms.append(ms); rhs.append(r)
        emit(dict(case=args.case, arm=args.arm, divergence=name, B=B, D=D, H=H, nfe=int(nfe), whole_call_ms=round(float(np.median(whole_ms)), 2),
                  whole_min_ms=round(min(whole_ms), 2), ms_per_rhs_alone=round(float(np.median(rhs)), 3),
                  whole_call_ms_per_nfe=round(float(np.median(whole_ms)) / nfe, 3)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
