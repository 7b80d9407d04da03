"""Time of one fcn training step at the paper's shape (ksphere/10dim.py: B = 500, D = 100, 5 hidden layers of 2048) -> profiles/train_bench.txt.

    python scripts/train_bench.py [--out profiles/train_bench.txt] [--steps 50]

Two arms on the same card, alternating: the HIP trainer (id_diff_amd/train.py) and a torch eager fp32 step of the same network
(autograd, torch.optim.Adam, clip_grad_norm_).  Time per step by device events over windows of ``--steps`` back-to-back steps on
explicit (x, t, z): the median of 5 windows after 2 warm-up windows.  Then the split of the HIP step over its phases (events between
the phases, summed over one window), the two new contractions alone against the 157 TFLOP/s fp32 matrix peak, and the launches a step
makes.  No host read-back inside a window.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import id_diff_amd  # noqa: E402,F401
from id_diff_amd import _lib, train  # noqa: E402
from id_diff_amd.configs.utils import read_config  # noqa: E402

PEAK_TFLOPS = 157.0


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps * 1e3          # us per call


def torch_arm(trainer, config, dev):
    lins = trainer.linears
    layers = []
    for i, l in enumerate(lins):
        lin = torch.nn.Linear(l.in_features, l.out_features).to(dev)
        with torch.no_grad():
            lin.weight.copy_(l.weight); lin.bias.copy_(l.bias)
        layers.append(lin)
        if i < len(lins) - 1:
            layers.append(torch.nn.ELU())
    net = torch.nn.Sequential(*layers)
    o = trainer.optim
    opt = torch.optim.Adam(net.parameters(), lr=o['lr'], betas=(o['beta1'], 0.999), eps=o['eps'], weight_decay=o['weight_decay'])
    sde, lw = trainer.sde, trainer.likelihood_weighting

    def step(x, t, z):
        labels, std, mean_coeff, weight = train.sde_terms(sde, t, lw)
        mean = x if mean_coeff is None else mean_coeff[:, None] * x
        out = net(torch.cat([mean + std[:, None] * z, labels[:, None]], dim=1))
        losses = 0.5 * torch.sum(torch.square(z - out), dim=-1)
        if weight is not None:
            losses = losses * weight
        loss = losses.mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), o['grad_clip'])
        opt.step()
        return loss
    return step


def phase_split(trainer, x, t, z, steps):
    """us per step of each phase of the HIP step: the body of FcnTrainer.loss_and_grad / step with events between the phases."""
    names = ["sde terms + input + forward", "loss + dL/dout", "weight/bias gradients (gemm_tn)", "data gradients (gemm_nn)",
             "norm + Adam"]
    marks = []
    B = x.shape[0]
    buf = trainer._buffers(B)
    for _ in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * len(names))]
        k = 0
        ev[k].record(); k += 1
        weight = trainer._forward(x, t, z, buf)
        ev[k].record(); k += 1
        ev[k].record(); k += 1
        _lib.dsm_loss_grad(buf['out'], z, weight=weight, reduce_mean=trainer.reduce_mean, grad=buf['G'], loss=trainer.loss, workspace=trainer.ws)
        ev[k].record(); k += 1
        h, dAs, dA = buf['h'], [buf['G']], buf['G']
        tn0, tn1, nn0, nn1 = ev[4], ev[5], ev[6], ev[7]
        # the backward chain alternates the two kernels: time it twice, once per kind, on the same buffers (the values do not matter)
        for i in range(len(trainer.layers) - 1, 0, -1):
            dAs.append(buf['dA'][i - 1])
        tn0.record()
        for j, i in enumerate(range(len(trainer.layers) - 1, -1, -1)):
            L = trainer.layers[i]
            _lib.gemm_tn(dAs[j], h[i], out=trainer.gW[i], colsum=trainer.gb[i], M=L['n'], N=L['kp'], K=B, lda=dAs[j].stride(0),
                         ldb=h[i].stride(0), ldc=L['kp'])
        tn1.record()
        nn0.record()
        for j, i in enumerate(range(len(trainer.layers) - 1, 0, -1)):
            L = trainer.layers[i]
            _lib.gemm_nn(dAs[j], trainer.W[i], out=dAs[j + 1], elu_out=h[i], M=B, N=L['k'], K=L['n'], lda=dAs[j].stride(0), ldb=L['kp'],
                         ldc=dAs[j + 1].stride(0), ldp=h[i].stride(0))
        nn1.record()
        ev[8].record()
        sumsq = _lib.grad_sumsq(trainer.grad, out=trainer.sumsq, workspace=trainer.ws)
        _lib.adam_step(trainer.theta, trainer.grad, trainer.m, trainer.v, trainer.global_step + 1, 0.0, sumsq=sumsq, max_norm=1.0)
        ev[9].record()
        marks.append(ev)
    torch.cuda.synchronize()
    return [(n, sum(e[2 * i].elapsed_time(e[2 * i + 1]) for e in marks) / steps * 1e3) for i, n in enumerate(names)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_bench.txt"))
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    config = read_config('configs/dimension_estimation/paper/euclidean_data/ksphere/10dim.py')
    config.device = dev
    trainer = train.FcnTrainer(config, dev)
    B, D = trainer.batch_size, trainer.D
    g = torch.Generator(dev).manual_seed(0)
    x = torch.randn(B, D, device=dev, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    t = torch.rand(B, device=dev, generator=g) * (1 - 1e-5) + 1e-5
    z = torch.randn(B, D, device=dev, generator=g)
    hip = lambda: trainer.step(x, t, z)
    tstep = torch_arm(trainer, config, dev)
    ref = lambda: tstep(x, t, z)
    times = {"hip": [], "torch": []}
    for w in range(7):                                   # 2 warm-up windows, then 5 measured, arms alternating
        for name, fn in (("hip", hip), ("torch", ref)):
            us = window(fn, args.steps)
            if w >= 2:
                times[name].append(us)
    lines = [f"fcn training step, B = {B}, D = {D}, {config.model.hidden_layers} hidden layers of {config.model.hidden_nodes}, fp32, "
             f"{torch.cuda.get_device_name(0)}",
             f"windows of {args.steps} back-to-back steps, median of 5 after 2 warm-up windows, arms alternating (us per step)"]
    for name in ("hip", "torch"):
        lines.append(f"  {name:5s} median {statistics.median(times[name]):9.1f}   windows " + " ".join(f"{v:.1f}" for v in times[name]))
    lines.append(f"  torch / hip = {statistics.median(times['torch']) / statistics.median(times['hip']):.2f}")
    n_lin = len(trainer.layers)
    flops = sum(2.0 * B * L['n'] * L['kp'] for L in trainer.layers) * 3 - 2.0 * B * trainer.layers[0]['n'] * trainer.layers[0]['kp']
    lines.append(f"matrix work per step {flops / 1e12:.4f} TFLOP -> {flops / statistics.median(times['hip']) / 1e6:.1f} TFLOP/s over the whole HIP step")
    lines.append("split of the HIP step (events between the phases, us per step; the backward's two kernel kinds timed apart):")
    split = phase_split(trainer, x, t, z, args.steps)
    for n, us in split:
        lines.append(f"  {n:36s} {us:9.1f}")
    lines.append(f"  {'sum':36s} {sum(us for _, us in split):9.1f}")
    # the two new contractions alone at the hidden-layer shape
    H = config.model.hidden_nodes
    a = torch.randn(B, H, device=dev); w = torch.randn(H, H, device=dev); p = torch.randn(B, H, device=dev)
    o1, o2, cs = torch.empty(B, H, device=dev), torch.empty(H, H, device=dev), torch.empty(H, device=dev)
    fl = 2.0 * B * H * H
    for name, fn in (("gemm_nn  [500 x 2048] . [2048 x 2048] (*) ELU'", lambda: _lib.gemm_nn(a, w, out=o1, elu_out=p)),
                     ("gemm_tn  [500 x 2048]^T . [500 x 2048] + colsum", lambda: _lib.gemm_tn(a, p, out=o2, colsum=cs)),
                     ("gemm (forward) [500 x 2048] . [2048 x 2048]^T + bias + ELU",
                      lambda: _lib.gemm(a, w, out=o1, epilogue=_lib.make_epilogue(bias=cs, act="elu")))):
        window(fn, 20)
        us = statistics.median(window(fn, args.steps) for _ in range(5))
        lines.append(f"{name}: {us:.1f} us = {fl / us / 1e6:.1f} TFLOP/s = {100 * fl / us / 1e6 / PEAK_TFLOPS:.1f} % of {PEAK_TFLOPS:.0f}")
    lines.append(f"library launches per step: 1 input + {n_lin} forward gemm + 2 loss + {n_lin} gemm_tn + {n_lin - 1} gemm_nn + 2 norm + 1 Adam = "
                 f"{1 + n_lin + 2 + n_lin + n_lin - 1 + 2 + 1} kernels (+ the [B]-sized torch elementwise ops of the SDE scalars; with drawn "
                 "(t, z): + 1 uniform draw, 1 perturb_randn, 1 index_select)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
