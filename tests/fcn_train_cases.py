"""What tests/test_fcn_train_host.py and tests/test_hip_fcn_train.py share: the cases, the numpy restatements of the order of operations
of csrc/fcn_train.hip, the fp64 references and the bounds the kernels are held to.  u = 2^-24 throughout (fp32 unit roundoff).

Contractions.  v_mfma_f32_32x32x2_f32 is a k-ordered chain of fp32 fmas, so for ANY order of the K terms
    |C - ref| <= gamma_K sum_k |a_k b_k| <= (K + 2) u sum_k |a_k b_k|.
With the ELU' mask the kernel forms v (a + 1) as ONE fma of the chain's result v, so the chain's error is scaled by g = a + 1 <= 1 and
one rounding u |ref| is added:  |C - ref| <= g (K + 2) u sum_k |a_k b_k| + u |ref|.   colsum is a chain of K - 1 fp32 additions:
(K + 1) u sum_k |a_k|.

Loss.  G = fl32(s w (out - z)) evaluated in fp64: one rounding, held to 4 u |ref|.  The loss is an fp64 sum rounded once: 2^-23 |ref|.

Adam.  The kernel evaluates torch.optim.Adam behind clip_grad_norm_ in fp64 from the fp32 state and rounds m, v, theta once each.  The
reference is the same update in fp64 numpy, run for 5 steps WITHOUT rounding its state (the trajectory).  At every step the kernel is
given that state rounded to fp32, and is compared with the fp64 update OF THAT ROUNDED STATE: the bounds (m, v: 4 u relative + 2^-149;
theta: u |theta| + 8 u |delta_ref|) are statements about one step's arithmetic, and a comparison with the update of the unrounded
state would add the input's own rounding u |theta| to theta, which no arithmetic can take back.
"""
import numpy as np
import torch

U = 2.0 ** -24

GEMM_SHAPES = [(1, 1, 1), (7, 5, 3), (33, 65, 17), (130, 257, 100), (257, 104, 500), (500, 2048, 100), (100, 104, 2048)]
GEMM_PADDED = (33, 65, 17)           # also run with lda, ldb, ldc (and ldp) larger than the row


def pad4(n):
    return (n + 3) // 4 * 4


def padded(a, extra=0, fill=np.nan):
    """[rows, cols] -> a [rows, ld] array (ld = pad4(cols) + extra, the pad filled with NaN: a kernel that reads it shows) and ld."""
    ld = pad4(a.shape[1]) + extra
    out = np.full((a.shape[0], ld), fill, dtype=np.float32)
    out[:, :a.shape[1]] = a
    return out, ld


def gemm_case(kind, M, N, K, seed=0):
    """Operands uniform in [-1, 1); kind 'nn': A [M, K], Bm [K, N], P [M, N] with half its entries negative (in (-1, 0]);
    kind 'tn': At [K, M], Bm [K, N]."""
    rng = np.random.default_rng([seed, M, N, K, 0 if kind == 'nn' else 1])
    A = rng.uniform(-1, 1, (M, K) if kind == 'nn' else (K, M)).astype(np.float32)
    Bm = rng.uniform(-1, 1, (K, N)).astype(np.float32)
    P = None
    if kind == 'nn':
        P = rng.uniform(0, 1, (M, N)).astype(np.float32)
        neg = rng.permutation(M * N).reshape(M, N) < (M * N + 1) // 2
        P[neg] = -P[neg]
    return A, Bm, P


def elu_grad_from_output(P):
    P = np.asarray(P, dtype=np.float64)
    return np.where(P > 0, 1.0, P + 1.0)


def gemm_reference(kind, A, Bm, P=None):
    """(ref, bound) in fp64, and for 'tn' also (colsum_ref, colsum_bound)."""
    A64, B64 = A.astype(np.float64), Bm.astype(np.float64)
    L = A64 if kind == 'nn' else A64.T
    K = B64.shape[0]
    ref, mag = L @ B64, np.abs(L) @ np.abs(B64)
    bound = (K + 2) * U * mag
    if P is not None:
        g = elu_grad_from_output(P)
        ref = ref * g
        bound = g * bound + U * np.abs(ref)
    if kind == 'nn':
        return ref, bound
    return ref, bound, A64.sum(axis=0), (K + 1) * U * np.abs(A64).sum(axis=0)


def fma32(a, b, c):
    """fl32(a b + c) for fp32 arrays: the product of two fp32 numbers is exact in fp64 and the sum is rounded to fp64 before fp32, which
    differs from a true fma in rare double roundings of half an fp32 ulp -- 2^-29 of the bound, and the host test says what it measures."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def gemm_restated(kind, A, Bm, P=None):
    """The kernel's order in numpy fp32: acc = fma(a_k, b_k, acc) for k = 0, 1, ..., then v (a + 1) as one fma; colsum sequential."""
    L = A if kind == 'nn' else np.ascontiguousarray(A.T)
    acc = np.zeros((L.shape[0], Bm.shape[1]), dtype=np.float32)
    for k in range(Bm.shape[0]):
        acc = fma32(L[:, k:k + 1], Bm[k:k + 1, :], acc)
    if P is not None:
        acc = np.where(P > 0, acc, fma32(acc, P, acc))
    if kind == 'nn':
        return acc
    cs = np.zeros(A.shape[1], dtype=np.float32)
    for k in range(A.shape[0]):
        cs = (cs + A[k]).astype(np.float32)
    return acc, cs


# ---------------------------------------------------------------------------------------------- loss
LOSS_B, LOSS_D = (1, 7, 500), (1, 5, 100)


def loss_case(B, D, weighted, seed=0):
    rng = np.random.default_rng([seed, B, D, int(weighted)])
    out = rng.standard_normal((B, D)).astype(np.float32)
    z = rng.standard_normal((B, D)).astype(np.float32)
    w = rng.uniform(0.1, 30.0, B).astype(np.float32) if weighted else None
    return out, z, w


def loss_reference(out, z, w, reduce_mean):
    """(loss, G) in fp64 of losses.py's reduction: mean_b w_b reduce_d (z - out)^2, reduce = mean or half the sum."""
    B, D = out.shape
    o, zz = out.astype(np.float64), z.astype(np.float64)
    ww = np.ones(B) if w is None else w.astype(np.float64)
    r = ((zz - o) ** 2).mean(axis=1) if reduce_mean else 0.5 * ((zz - o) ** 2).sum(axis=1)
    s = 2.0 / (B * D) if reduce_mean else 1.0 / B
    return float((ww * r).mean()), s * ww[:, None] * (o - zz)


def loss_restated(out, z, w, reduce_mean, blocks_of=1024, lanes=256):
    """The kernel's order: workgroup ranges of ceil(total / nb) elements, 256 strided lane sums in fp64, a pairwise tree, then the
    partials in index order per lane and the same tree; G = fl32(s w d) from fp64."""
    B, D = out.shape
    total = B * D
    nb = min(max(-(-total // blocks_of), 1), 1024)
    per = -(-total // nb)
    o, zz = out.astype(np.float64).ravel(), z.astype(np.float64).ravel()
    ww = np.ones(B) if w is None else w.astype(np.float64)
    om = np.repeat(ww, D)
    d = o - zz
    terms = om * d * d

    def tree(v):
        v = v.copy()
        s = lanes // 2
        while s:
            v[:s] += v[s:2 * s]
            s //= 2
        return v[0]

    def block(x):
        lane = np.zeros(lanes)
        for i in range(0, len(x), lanes):
            seg = x[i:i + lanes]
            lane[:len(seg)] += seg
        return tree(lane)

    partial = np.array([block(terms[b * per:min(total, (b + 1) * per)]) for b in range(-(-total // per))])
    tot = block(partial)
    s = 2.0 / (B * D) if reduce_mean else 1.0 / B
    scale = 1.0 / (B * D) if reduce_mean else 0.5 / B
    return np.float32(scale * tot), (s * om * d).astype(np.float32).reshape(B, D)


# ---------------------------------------------------------------------------------------------- Adam
ADAM_N = (1, 1000, 2 ** 20 + 3)
ADAM_CASES = {                       # name -> (grad scale, max_norm or None, weight_decay, warmup)
    'clip_active': (1.0, 1.0, 0.0, 0),
    'clip_inactive': (1e-4, 1.0, 0.0, 0),
    'no_clip_decay': (1.0, None, 0.01, 0),
    'clip_decay_warmup': (1.0, 1.0, 0.01, 3),      # warm-up 3: the first step has lr 0
}
ADAM_LR, ADAM_BETAS, ADAM_EPS, ADAM_STEPS = 1e-3, (0.9, 0.999), 1e-8, 5


def adam_case(n, name, seed=0):
    scale = ADAM_CASES[name][0]
    rng = np.random.default_rng([seed, n, sorted(ADAM_CASES).index(name)])
    theta = rng.standard_normal(n).astype(np.float32)
    grad = (scale * rng.standard_normal(n)).astype(np.float32)
    return theta, grad


def warmup_lr(lr, steps_taken, warmup):
    return lr if warmup <= 0 else lr * min(steps_taken / warmup, 1.0)


def adam_update(theta, m, v, grad, step, lr, max_norm, weight_decay, betas=ADAM_BETAS, eps=ADAM_EPS):
    """One step of clip_grad_norm_(max_norm) + torch.optim.Adam in fp64 numpy (``step`` >= 1); returns the new (theta, m, v)."""
    theta, m, v, g = (np.asarray(a, dtype=np.float64) for a in (theta, m, v, grad))
    if max_norm is not None:
        norm = np.sqrt((g * g).sum())
        g = g * min(1.0, max_norm / (norm + 1e-6))
    g = g + weight_decay * theta
    m = m + (1.0 - betas[0]) * (g - m)                       # exp_avg.lerp_(grad, 1 - beta1)
    v = betas[1] * v + (1.0 - betas[1]) * g * g
    bc1, bc2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    return theta - (lr / bc1) * (m / denom), m, v


def adam_bounds(theta_in, target_theta, target_m, target_v):
    delta = np.abs(target_theta - np.asarray(theta_in, dtype=np.float64))
    return (U * np.abs(target_theta) + 8 * U * delta, 4 * U * np.abs(target_m) + 2.0 ** -149, 4 * U * np.abs(target_v) + 2.0 ** -149)


# ---------------------------------------------------------------------------------------------- whole network
NET_SHAPES = [(5, 32, 2, 33), (100, 256, 2, 130), (100, 512, 1, 500)]          # (D, H, hidden_layers, B)
NET_MODES = {'ve': ('vesde', False), 've_lw': ('vesde', True), 'vp': ('vpsde', False)}
TRAJ_SHAPE = (100, 256, 2, 130)
NET_FACTOR, NET_FLOOR, LOSS_RTOL = 16.0, 2.0 ** -22, 2.0 ** -20


def net_config(D, H, hidden_layers, B, sde='vesde', likelihood_weighting=True, reduce_mean=False, seed=42, **optim):
    from id_diff_amd.configs.default import get_default_configs
    from id_diff_amd.configs.config_dict import ConfigDict
    config = get_default_configs()
    config.seed = seed
    config.device = 'cuda:0'
    config.logging = ConfigDict(log_path='logs/', log_name='fcn-train-test', svd_points=4)
    config.training.batch_size = B
    config.training.sde = sde
    config.training.continuous = True
    config.training.likelihood_weighting = likelihood_weighting
    config.training.reduce_mean = reduce_mean
    config.data = ConfigDict(datamodule='KSphere', create_dataset=False, split=[0.8, 0.1, 0.1], data_samples=1024, use_data_mean=False,
                             n_spheres=1, ambient_dim=D, manifold_dim=min(2, D - 1), noise_std=0.0, embedding_type='random_isometry',
                             dim=D, num_channels=0, shape=[D])
    config.model = ConfigDict(checkpoint_path=None, sigma_max=4.0, sigma_min=1e-2, beta_min=0.1, beta_max=20.0, name='fcn', state_size=D,
                              hidden_layers=hidden_layers, hidden_nodes=H, dropout=0.0, num_scales=1000)
    o = dict(weight_decay=0.0, optimizer='Adam', lr=1e-3, beta1=0.9, eps=1e-8, warmup=5, grad_clip=1.0)
    o.update(optim)
    config.optim = ConfigDict(o)
    return config


def batch(D, B, seed):
    """(x, t, z) fp32 CPU tensors: points of a unit sphere's neighbourhood, times in [1e-5, 1], standard normal noise."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    t = torch.rand(B, generator=g) * (1 - 1e-5) + 1e-5
    z = torch.randn(B, D, generator=g)
    return x, t, z


def sequential(state_dict, dtype):
    """The reference's nn.Sequential (Linear, ELU, ..., Linear; Dropout(0) left out) with the given weights, on the CPU."""
    keys = sorted({int(k.split('.')[1]) for k in state_dict})
    layers = []
    for j, i in enumerate(keys):
        w, b = state_dict[f'mlp.{i}.weight'], state_dict[f'mlp.{i}.bias']
        lin = torch.nn.Linear(w.shape[1], w.shape[0]).to(dtype)
        with torch.no_grad():
            lin.weight.copy_(w.detach().cpu().to(dtype)); lin.bias.copy_(b.detach().cpu().to(dtype))
        layers.append(lin)
        if j < len(keys) - 1:
            layers.append(torch.nn.ELU())
    return torch.nn.Sequential(*layers)


def torch_loss(net, x, t, z, terms, likelihood_weighting, reduce_mean, dtype):
    """losses.py:172-188 word for word (score = -out / std), in ``dtype`` on the CPU; ``terms`` = (labels, std, mean_coeff, g2)
    as the trainer computed them for these times (fp32), so both sides see the same SDE scalars."""
    labels, std, mean_coeff, g2 = (None if a is None else a.detach().cpu().to(dtype) for a in terms)
    x, z = x.to(dtype), z.to(dtype)
    mean = x if mean_coeff is None else mean_coeff[:, None] * x
    perturbed = mean + std[:, None] * z
    out = net(torch.cat([perturbed, labels[:, None]], dim=1))
    score = -out / std[:, None]
    reduce_op = torch.mean if reduce_mean else (lambda *a, **k: 0.5 * torch.sum(*a, **k))
    if not likelihood_weighting:
        losses = reduce_op(torch.square(score * std[:, None] + z), dim=-1)
    else:
        losses = reduce_op(torch.square(score + z / std[:, None]), dim=-1) * g2
    return torch.mean(losses)


def sde_terms_for_reference(trainer, t_dev):
    """(labels, std, mean_coeff, g2) for ``torch_loss`` from the trainer's own device computation: weight = g2 / std^2."""
    from id_diff_amd import train
    labels, std, mean_coeff, weight = train.sde_terms(trainer.sde, t_dev, trainer.likelihood_weighting)
    g2 = None if weight is None else weight.double() * std.double() ** 2
    return labels, std, mean_coeff, g2


def torch_grads(state_dict, x, t, z, terms, likelihood_weighting, reduce_mean, dtype):
    net = sequential(state_dict, dtype)
    loss = torch_loss(net, x, t, z, terms, likelihood_weighting, reduce_mean, dtype)
    loss.backward()
    names = [k for k in state_dict]
    params = dict(zip([f'mlp.{i}.{p}' for i in sorted({int(k.split(".")[1]) for k in state_dict}) for p in ('weight', 'bias')],
                      [p for l in net if isinstance(l, torch.nn.Linear) for p in (l.weight, l.bias)]))
    return float(loss.detach().double()), {k: params[k].grad.detach().double() for k in names}


def torch_trajectory(state_dict, batches, terms_list, config, dtype, steps):
    """The reference's training loop on the CPU: Adam, clip_grad_norm_, LambdaLR warm-up; returns the per-step losses (before the update)."""
    o = config.optim
    net = sequential(state_dict, dtype)
    opt = torch.optim.Adam(net.parameters(), lr=o.lr, betas=(o.beta1, 0.999), eps=o.eps, weight_decay=o.weight_decay)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: min(s / o.warmup, 1.0) if o.warmup > 0 else 1.0)
    losses = []
    for i in range(steps):
        x, t, z = batches[i]
        opt.zero_grad()
        loss = torch_loss(net, x, t, z, terms_list[i], config.training.likelihood_weighting, config.training.reduce_mean, dtype)
        loss.backward()
        if o.grad_clip >= 0:
            torch.nn.utils.clip_grad_norm_(net.parameters(), o.grad_clip)
        opt.step()
        sched.step()
        losses.append(float(loss.detach().double()))
    return losses
