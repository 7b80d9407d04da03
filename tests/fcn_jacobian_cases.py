"""What tests/test_fcn_jacobian_host.py and tests/test_hip_fcn_jacobian.py share: the cases, the numpy restatements of the order of
operations of csrc/fcn_jacobian.hip, the fp64 references and the bounds.  u = 2^-24 throughout (fp32 unit roundoff).

Layer kernel.  v_mfma_f32_32x32x2_f32 is a k-ordered chain of fp32 fmas: the chain's result v is within K u sum_k |a_k w_k| of the exact
sum (to first order in u, as fcn_train_cases.gemm_reference has it).  The kernel then forms g = fl(a + 1) (one rounding; exactly 1 for
a > 0) and fl(v g) (one more), so the chain's error is scaled by g <= 1 and two roundings of the result are added:

    |C - ref| <= g K u sum_k |a_k w_k| + 2 u |ref|          (act given)          |C - ref| <= K u sum_k |a_k w_k|          (act = NULL)

with ref and g = (a > 0 ? 1 : a + 1) evaluated in fp64 from the fp32 inputs.

Seed kernel.  One fp32 multiply of two fp32 numbers, W1[n, i] and fl(a + 1): the product is exact in fp64, so rounding the fp64 product
to fp32 once IS the kernel's result -- the kernel is held bit-equal to it.

Whole Jacobian.  The bar is measured, not fixed: 8 x the max-norm error of the fp32 CPU torch autograd Jacobian against the fp64 one, per
matrix and relative to max |J|.  8 because the kernel's chain order differs from torch's blocked sums, up to K = 2048.
"""
import numpy as np
import torch

import fcn_train_cases as tc
from fcn_train_cases import net_config, padded, sequential  # noqa: F401  (the GPU and host tests take them from here)

U = tc.U

LAYER_SHAPES = [(1, 1, 1, 1), (3, 7, 5, 3), (3, 33, 65, 17), (3, 8, 128, 128), (2, 100, 256, 2048), (2, 100, 2048, 104)]   # (P, R, N, K)
LAYER_PADDED = (3, 33, 65, 17)          # also run with every leading dimension and both point strides larger than needed
SEED_SHAPES = [(1, 1, 1, 4), (3, 8, 128, 12), (2, 100, 2048, 104), (3, 7, 5, 8)]                                           # (P, D, N, ldw)
NET_SHAPES = [(8, 128, 2), (100, 256, 3)]                                                                                  # (D, H, hidden_layers)
NET_SDES = ('vesde', 'vpsde')
NET_POINTS = 5
NET_MARGIN = 8.0
SV_RTOL = 1e-4                          # singular values within this of sigma_max: the project's contract for them


def act_case(P, N, rng):
    """ELU outputs [P, N] that differ between the points: about half positive, the rest in (-1, 0), and -- placed at a different offset in
    every point -- 0, -0.0, a tiny negative value and two values next to -1."""
    a = rng.uniform(0.0, 1.0, (P, N)).astype(np.float32)
    neg = rng.uniform(size=(P, N)) < 0.5
    a[neg] = -a[neg] * np.float32(0.999)
    special = np.array([0.0, -0.0, -1e-10, -1.0 + 2.0 ** -20, -0.99999], dtype=np.float32)
    for p in range(P):
        for s, v in enumerate(special):
            a[p, (3 * p + 2 * s) % N] = v
    return a


def layer_case(P, R, N, K, seed=0):
    """A [P, R, K] and W [N, K] uniform in [-1, 1), act [P, N] of ``act_case``."""
    rng = np.random.default_rng([seed, P, R, N, K])
    A = rng.uniform(-1, 1, (P, R, K)).astype(np.float32)
    W = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    return A, W, act_case(P, N, rng)


def slope64(act):
    a = np.asarray(act, dtype=np.float64)
    return np.where(a > 0, 1.0, a + 1.0)


def slope32(act):
    """g as the kernels form it: 1 for a > 0, else fl(a + 1)."""
    a = np.asarray(act, dtype=np.float32)
    return np.where(a > 0, np.float32(1.0), (a + np.float32(1.0)).astype(np.float32)).astype(np.float32)


def layer_reference(A, W, act=None):
    """(ref, bound) [P, R, N] in fp64."""
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    K = W.shape[1]
    ref = A64 @ W64.T
    bound = K * U * (np.abs(A64) @ np.abs(W64).T)
    if act is not None:
        g = slope64(act)[:, None, :]
        ref = ref * g
        bound = g * bound + 2 * U * np.abs(ref)
    return ref, bound


def layer_restated(A, W, act=None):
    """The kernel's order in numpy fp32: acc = fma(a_k, w_k, acc) for k = 0, 1, ..., then one multiply by g = fl(a + 1)."""
    acc = np.zeros((A.shape[0], A.shape[1], W.shape[0]), dtype=np.float32)
    Wt = np.ascontiguousarray(W.T)
    for k in range(W.shape[1]):
        acc = tc.fma32(A[:, :, k:k + 1], Wt[None, k:k + 1, :], acc)
    if act is not None:
        acc = (acc * slope32(act)[:, None, :]).astype(np.float32)
    return acc


def seed_case(P, D, N, ldw, seed=0):
    """W1 [N, ldw] with NaN from column D on (the time column and the pads: a kernel that reads them shows) and act [P, N]."""
    rng = np.random.default_rng([seed, P, D, N, ldw, 7])
    W1 = np.full((N, ldw), np.nan, dtype=np.float32)
    W1[:, :D] = rng.uniform(-1, 1, (N, D)).astype(np.float32)
    return W1, act_case(P, N, rng)


def seed_reference(W1, act, D):
    """T [P, D, N] fp32: the exact (fp64) product of W1[n, i] and fl(a + 1), rounded once."""
    g = slope32(act).astype(np.float64)
    return (W1[:, :D].astype(np.float64).T[None, :, :] * g[:, None, :]).astype(np.float32)


def seed_restated(W1, act, D):
    """The kernel's arithmetic in numpy fp32: one multiply."""
    return (np.ascontiguousarray(W1[:, :D].T)[None, :, :] * slope32(act)[:, None, :]).astype(np.float32)


def share(got, ref, bound):
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) / bound).max())


# ---------------------------------------------------------------------------------------------- whole network
def net_points(D, P=NET_POINTS, seed=5):
    """P points of the unit sphere in R^D, fp32 CPU."""
    x = torch.randn(P, D, generator=torch.Generator().manual_seed(seed))
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def sde_scalars(sde, t):
    """(mean coefficient, std, label) of the SDE at time t, as Python floats from an fp64 evaluation."""
    tt = torch.full((1,), float(t), dtype=torch.float64)
    mean, std = sde.marginal_prob(torch.ones(1, 1, dtype=torch.float64), tt)
    return float(mean.reshape(-1)[0]), float(std.reshape(-1)[0]), float(t) * (sde.N - 1)


def autograd_jacobians(state_dict, sde, xs, t, dtype):
    """J [P, D, D] (numpy fp64 copy of a ``dtype`` computation on the CPU), J[p][i, j] = d score_j / d x_i of
    score(x) = -net([x, label]) / std(t) at x = mean(t) xs[p]: torch.autograd.functional.jacobian of the reference's Sequential."""
    net = sequential(state_dict, dtype)
    mean, std, label = sde_scalars(sde, t)
    lab = torch.full((1,), label, dtype=dtype)

    def score(x):
        return -net(torch.cat([x, lab])[None, :])[0] / std

    out = []
    for x in xs:
        J = torch.autograd.functional.jacobian(score, (mean * x.to(torch.float64)).to(dtype))       # [j, i]
        out.append(J.T.double().numpy())
    return np.stack(out)


def measured_bars(J32, J64, margin=NET_MARGIN):
    """Per matrix: margin x max |J32 - J64| / max |J64|."""
    return np.array([margin * np.abs(a - b).max() / np.abs(b).max() for a, b in zip(J32, J64)])


def relative_errors(J, J64):
    return np.array([np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max() for a, b in zip(J, J64)])


def network_restated(state_dict, sde, xs, t, mutate=None):
    """jacobian.network_jacobians in numpy fp32, kernel by kernel (forward in fp64 rounded to fp32 per layer: the activations are inputs
    of the kernels under test, not their work).  ``mutate``: None, 'no_scale' (the -1 / std left out) or 'time_column' (the seed reads
    the columns 1 .. D of W1, the time column among them)."""
    keys = sorted({int(k.split('.')[1]) for k in state_dict})
    Ws = [state_dict[f'mlp.{i}.weight'].detach().cpu().numpy().astype(np.float32) for i in keys]
    bs = [state_dict[f'mlp.{i}.bias'].detach().cpu().numpy().astype(np.float32) for i in keys]
    mean, std, label = sde_scalars(sde, t)
    P, D = xs.shape
    h = np.concatenate([(np.float32(mean) * xs.numpy()).astype(np.float32), np.full((P, 1), label, dtype=np.float32)], axis=1)
    acts = []
    for W, b in zip(Ws[:-1], bs[:-1]):
        pre = h.astype(np.float64) @ W.astype(np.float64).T + b
        h = np.where(pre > 0, pre, np.expm1(pre)).astype(np.float32)
        acts.append(h)
    W1 = Ws[0][:, 1:D + 1] if mutate == 'time_column' else Ws[0]
    T = seed_restated(W1, acts[0], D)
    for i, W in enumerate(Ws[1:], start=1):
        T = layer_restated(T, W, acts[i] if i < len(acts) else None)
    if mutate == 'no_scale':
        return T
    return (T * np.float32(-1.0 / np.float32(std))).astype(np.float32)
