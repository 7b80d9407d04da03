"""What tests/test_fcn_flipd_host.py and tests/test_hip_fcn_flipd.py share: FLIPD of an fcn score network by torch autograd on the CPU,

    flipd(x) = D + std(t)^2 [ tr grad_y s(y) + |s(y)|^2 ],     y = mean(t) x,   s(y) = -net([y, label]) / std(t)

in fp64 (the reference) and in fp32 (the yardstick of the bar), with the exact trace or with Hutchinson's eps^T (grad s) eps for given
probe rows.  The bar is the project's usual one, measured and not fixed: 8 x the deviation of the fp32 evaluation from the fp64 one --
the largest over the points of a case, because a single scalar per point can agree by accident where a whole matrix cannot.
"""
import numpy as np
import torch

import fcn_jacobian_cases as jcases
from fcn_jacobian_cases import net_config, net_points, sde_scalars  # noqa: F401

NET_SHAPES = jcases.NET_SHAPES                                           # (D, H, hidden_layers): (8, 128, 2), (100, 256, 3)
NET_SDES = ('vesde', 'vpsde', 'subvpsde')
MARGIN = 8.0


def autograd_flipd(state_dict, sde, xs, t, dtype, probes=None):
    """float64 numpy [P] of a ``dtype`` computation on the CPU.  ``probes`` [K, P, D]: the mean over k of eps_k^T (grad s) eps_k in place
    of the trace."""
    net = jcases.sequential(state_dict, dtype)
    mean, std, label = sde_scalars(sde, t)
    lab = torch.full((1,), label, dtype=dtype)
    D = xs.shape[1]

    def score(y):
        return -net(torch.cat([y, lab])[None, :])[0] / std

    out = []
    for p, x in enumerate(xs):
        y = (mean * x.to(torch.float64)).to(dtype)
        J = torch.autograd.functional.jacobian(score, y)                 # [j, i] = d s_j / d y_i
        s = score(y).detach()
        if probes is None:
            tr = torch.trace(J)
        else:
            e = torch.as_tensor(probes[:, p, :], dtype=dtype)            # [K, D]
            tr = ((e @ J.T) * e).sum(dim=1).mean()                       # sum_ij e_i (d s_j / d y_i) e_j
        out.append(float(D + std * std * (tr + (s * s).sum())))
    return np.asarray(out, dtype=np.float64)


def bar(f32, f64, margin=MARGIN):
    """margin x the largest |fp32 - fp64| over the points of the case."""
    return margin * float(np.abs(np.asarray(f32) - np.asarray(f64)).max())
