"""Training the ``fcn`` score network on the MI355X (``--mode train`` for the Euclidean configs).

Denoising score matching as /root/reference/losses.py:164-188 states it, with Adam, global-norm gradient clipping and the linear
learning-rate warm-up of the reference's optimiser set-up.  Every pass over the batch is a HIP kernel of libidiff_hip.so:

    forward    idiff_fcn_train_input_f32 (perturb + append the time), one idiff_gemm_f32 per layer with bias + ELU in its epilogue
    loss       idiff_dsm_loss_grad_f32: the loss (fp64 sum, fixed order) and dL/dout
    backward   per layer idiff_gemm_tn_f32 (dW = dA^T H, db = column sums) and idiff_gemm_nn_f32 (dH = dA W through ELU')
    update     idiff_grad_sumsq_f32 + idiff_adam_step_f32 over ONE flat parameter buffer

ELU' is written in terms of the ELU output (a > 0 ? 1 : a + 1), so the activations kept for the backward pass are the ones the forward
produced anyway.  Nothing inside a step reads the device back; the same (seed, step) gives the same bits, also across a resume.

Scope: ``model.name == 'fcn'``, unconditional, continuous, VE / VP / subVP, one GPU, no dropout, no EMA (the estimator evaluates the
raw weights, checkpoint_io.score_model_state_dict).  The flat buffer holds, per Linear, the weight as [out, in rounded up to 4]
(zero pad columns, whose gradients are zero because the matching input columns are) and the bias (rounded up to 4 likewise), so every
row any kernel touches is 16-byte aligned; the module's parameters are views into it and ``state_dict()`` keeps the reference's keys.
"""
import math
import os

import torch
import torch.nn as nn

from . import _lib, sde_lib
from .models.fcn import FCN

SCOPE = ("--mode train covers model.name == 'fcn' (unconditional, continuous, VE / VP / subVP, one GPU); "
         "use the reference to train any other network")
T_EPS = 1e-5          # smallest training time, losses.py:54
OPTIM_DEFAULTS = dict(weight_decay=0.0, optimizer='Adam', lr=2e-4, beta1=0.9, eps=1e-8, warmup=5000, grad_clip=1.0)
_MASK63 = 0x7FFFFFFFFFFFFFFF


def pad4(n):
    return (n + 3) // 4 * 4


def warmup_lr(lr, steps_taken, warmup):
    """lr * min(s / warmup, 1) with s the number of optimiser steps already taken (the reference's LambdaLR: the first step has lr 0)."""
    if warmup is None or warmup <= 0:
        return float(lr)
    return float(lr) * min(float(steps_taken) / float(warmup), 1.0)


def stream_key(seed, index, salt=0):
    """63-bit key of the random stream (seed, index); ``salt`` separates the streams a step draws (t, z) and the epoch permutation."""
    x = (int(seed) * 0x9E3779B97F4A7C15 + int(index) * 0xBF58476D1CE4E5B9 + int(salt) * 0x94D049BB133111EB + 0x2545F4914F6CDD1D)
    x &= 0xFFFFFFFFFFFFFFFF
    x ^= x >> 31
    x = (x * 0xD6E8FEB86659FD93) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 32
    return x & _MASK63


def check_scope(config):
    """Refuse what is not trained here: another network keeps the mode's SystemExit, dropout is a NotImplementedError."""
    if config.model.get('name') != 'fcn':
        raise SystemExit(f"model.name = {config.model.get('name')!r} is outside the scope of id-diff_amd's training: {SCOPE}")
    if float(config.model.get('dropout', 0.0) or 0.0) > 0:
        raise NotImplementedError("model.dropout > 0 is not trained here (the forward kernels fuse bias + ELU and have no dropout mask); "
                                  "set model.dropout = 0")
    if not bool(config.training.get('continuous', True)):
        raise NotImplementedError("training.continuous = False is not trained here")
    kind = str(config.training.sde).lower()
    if kind not in ('vesde', 'vpsde', 'subvpsde'):
        raise NotImplementedError(f"training.sde = {config.training.sde!r}: training covers vesde, vpsde and subvpsde")


def optim_config(config):
    out = dict(OPTIM_DEFAULTS)
    for k in out:
        v = config.get('optim.' + k)
        if v is not None:
            out[k] = v
    if str(out['optimizer']).lower() != 'adam':
        raise NotImplementedError(f"optim.optimizer = {out['optimizer']!r}: only Adam is implemented")
    return out


def plain(obj):
    """A config as plain nested builtins (what ``torch.load(weights_only=True)`` accepts)."""
    if isinstance(obj, dict):
        return {str(k): plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [plain(v) for v in obj]
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    return str(obj)


def diffusion(sde, t):
    """g(t) of the forward SDE (sde_lib.py of the reference: VE :336-340, VP :244-248, subVP :293-298)."""
    if isinstance(sde, sde_lib.VESDE):
        sigma = sde.sigma_min * (sde.sigma_max / sde.sigma_min) ** t
        return sigma * math.sqrt(2.0 * (math.log(sde.sigma_max) - math.log(sde.sigma_min)))
    if isinstance(sde, sde_lib.subVPSDE):
        beta_t = sde.beta_0 + t * (sde.beta_1 - sde.beta_0)
        discount = 1. - torch.exp(-2 * sde.beta_0 * t - (sde.beta_1 - sde.beta_0) * t ** 2)
        return torch.sqrt(beta_t * discount)
    if isinstance(sde, sde_lib.VPSDE):
        return torch.sqrt(sde.beta_0 + t * (sde.beta_1 - sde.beta_0))
    raise NotImplementedError(f"SDE class {sde.__class__.__name__} has no diffusion coefficient here")


def sde_terms(sde, t, likelihood_weighting):
    """(labels, std, mean_coeff or None, weight or None) [B] each for the times ``t``: what get_score_fn and the loss read of the SDE.
    score = -out / std, so both weightings of losses.py are weight * reduce (z - out)^2 with weight = 1 or g(t)^2 / std^2."""
    labels = t * (sde.N - 1)
    ones = torch.ones(t.shape[0], 1, device=t.device, dtype=t.dtype)
    mean, std = sde.marginal_prob(ones, t)
    mean_coeff = None if isinstance(sde, sde_lib.VESDE) else mean.reshape(-1).contiguous()
    weight = None
    if likelihood_weighting:
        g = diffusion(sde, t)
        weight = (g * g / (std * std)).contiguous()
    return labels.contiguous(), std.contiguous(), mean_coeff, weight


def data_split(config, name='train'):
    """Rows [N, D] fp32 of one split of the config's data set, as the drivers split it (seeded with config.seed, global RNG untouched)."""
    from .lightning_data_modules.utils import create_lightning_datamodule
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(config.get('seed', 42)))
        dm = create_lightning_datamodule(config)
        dm.setup()
        part = {'train': dm.train_data, 'val': dm.valid_data, 'valid': dm.valid_data, 'test': dm.test_data}[name]
        if hasattr(part.dataset, 'data'):
            rows = torch.as_tensor(part.dataset.data)[torch.as_tensor(part.indices)]
        else:
            rows = torch.stack([torch.as_tensor(part[i][0] if isinstance(part[i], (list, tuple)) else part[i]) for i in range(len(part))])
    if rows.ndim != 2:
        raise NotImplementedError(f"training takes data modules that yield [B, D] rows; {config.data.datamodule} gives {tuple(rows.shape[1:])}")
    return rows.to(torch.float32).contiguous()


def checkpoint_dict(state_dict, config, global_step, epoch, m, v):
    """The file layout: Lightning's keys, plain containers and tensors only (loads with ``weights_only=True``)."""
    return {'state_dict': {'score_model.' + k: t.detach().cpu().clone().contiguous() for k, t in state_dict.items()},
            'hyper_parameters': {'config': plain(config)},
            'global_step': int(global_step), 'epoch': int(epoch),
            'optimizer_states': [{'m': m.detach().cpu().clone(), 'v': v.detach().cpu().clone()}]}


def write_checkpoint(path, ckpt):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + '.tmp'
    torch.save(ckpt, tmp)
    os.replace(tmp, path)


class FcnTrainer:
    def __init__(self, config, device=None):
        check_scope(config)
        self.config = config
        self.device = torch.device(device if device is not None else config.get('device', 'cuda:0'))
        if self.device.type != 'cuda':
            raise RuntimeError(f"FcnTrainer: device {self.device}; id-diff_amd trains on the MI355X only (no CPU path)")
        _lib.lib()
        self.seed = int(config.get('seed', 42))
        self.sde, _ = sde_lib.configure_sde(config)
        self.likelihood_weighting = bool(config.training.get('likelihood_weighting', True))
        self.reduce_mean = bool(config.training.get('reduce_mean', False))
        self.optim = optim_config(config)
        self.batch_size = int(config.training.batch_size)
        self.global_step, self.epoch = 0, 0
        self._pos = 0                 # batches of the current epoch already taken
        self._perm = None
        self._train = None
        self._bufs = {}

        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(self.seed)
            self.model = FCN(config)
        self.D = int(config.model.state_size)
        self.linears = [l for l in self.model.mlp if isinstance(l, nn.Linear)]
        # flat layout: W_i [out_i, pad4(in_i)] then b_i [pad4(out_i)]
        self.layers, off = [], 0
        for lin in self.linears:
            n, k = lin.out_features, lin.in_features
            kp = pad4(k)
            self.layers.append(dict(n=n, k=k, kp=kp, w=off, b=off + n * kp))
            off += n * kp + pad4(n)
        self.n_params = off
        self.theta = torch.zeros(off, device=self.device, dtype=torch.float32)
        self.grad = torch.zeros_like(self.theta)
        self.m = torch.zeros_like(self.theta)
        self.v = torch.zeros_like(self.theta)
        self.W, self.b, self.gW, self.gb = [], [], [], []
        for lin, L in zip(self.linears, self.layers):
            n, k, kp = L['n'], L['k'], L['kp']
            W = self.theta[L['w']:L['w'] + n * kp].view(n, kp)
            b = self.theta[L['b']:L['b'] + n]
            W[:, :k].copy_(lin.weight.detach())
            b.copy_(lin.bias.detach())
            lin.weight.data = W[:, :k]           # the parameters ARE the flat buffer from here on
            lin.bias.data = b
            self.W.append(W); self.b.append(b)
            self.gW.append(self.grad[L['w']:L['w'] + n * kp].view(n, kp))
            self.gb.append(self.grad[L['b']:L['b'] + n])
        self.model._invalidate()
        self.kpad = self.layers[0]['kp']
        self.ws = _lib.reduce_workspace(self.device)
        self.sumsq = torch.zeros((), device=self.device, dtype=torch.float64)
        self.loss = torch.zeros((), device=self.device, dtype=torch.float32)
        self._gen = torch.Generator(device=self.device)
        self.evaluations = []         # [(global_step, {min_norm, max_norm, mean_norm, dim})] of fit(eval_every=)

    # ---------------------------------------------------------------------------------------- state
    def state_dict(self):
        return self.model.state_dict()

    def load_state_dict(self, state):
        """Copies into the flat buffer through the parameter views (their storage does not move)."""
        self.model.load_state_dict(state, strict=True)

    def _buffers(self, B):
        if B not in self._bufs:
            z = lambda r, c: torch.zeros(r, c, device=self.device, dtype=torch.float32)
            acts = [z(B, self.kpad)] + [z(B, pad4(L['n'])) for L in self.layers[:-1]]
            self._bufs[B] = dict(h=acts, out=z(B, self.D), G=z(B, pad4(self.D)),
                                 dA=[z(B, pad4(L['n'])) for L in self.layers[:-1]],
                                 zfull=z(B, pad4(self.D)), zeros=z(1, pad4(self.D)), ones=torch.ones(B, device=self.device),
                                 scratch=z(B, pad4(self.D)))
        return self._bufs[B]

    # ---------------------------------------------------------------------------------------- one batch
    def _forward(self, x, t, z, buf):
        labels, std, mean_coeff, weight = sde_terms(self.sde, t, self.likelihood_weighting)
        B = x.shape[0]
        h = buf['h']
        _lib.fcn_train_input(x, z, std, mean_coeff, labels, h[0])
        last = len(self.layers) - 1
        for i, L in enumerate(self.layers):
            ep = _lib.make_epilogue(bias=self.b[i], act=None if i == last else "elu")
            dst = buf['out'] if i == last else h[i + 1]
            _lib.gemm(h[i], self.W[i], out=dst, epilogue=ep, M=B, N=L['n'], K=L['kp'], lda=h[i].stride(0), ldb=L['kp'],
                      ldc=dst.stride(0))
        return weight

    def _check_batch(self, x, t, z):
        for a, name in ((x, 'x'), (t, 't'), (z, 'z')):
            _lib._dev(a, name)
        if x.ndim != 2 or x.shape[1] != self.D or z.shape != x.shape or t.shape != (x.shape[0],):
            raise RuntimeError(f"FcnTrainer: x {tuple(x.shape)}, t {tuple(t.shape)}, z {tuple(z.shape)} for state_size {self.D}")

    def loss_and_grad(self, x, t, z):
        """The loss of the clean batch ``x`` [B, D] perturbed at the times ``t`` [B] with the noise ``z`` [B, D], as a device float, and
        its gradient with respect to every parameter in ``self.grad`` (flat; ``self.gW[i]`` / ``self.gb[i]`` are the layers' views)."""
        self._check_batch(x, t, z)
        B = x.shape[0]
        buf = self._buffers(B)
        weight = self._forward(x, t, z, buf)
        _lib.dsm_loss_grad(buf['out'], z, weight=weight, reduce_mean=self.reduce_mean, grad=buf['G'], loss=self.loss, workspace=self.ws)
        h = buf['h']
        dA = buf['G']
        for i in range(len(self.layers) - 1, -1, -1):
            L = self.layers[i]
            _lib.gemm_tn(dA, h[i], out=self.gW[i], colsum=self.gb[i], M=L['n'], N=L['kp'], K=B, lda=dA.stride(0), ldb=h[i].stride(0),
                         ldc=L['kp'])
            if i > 0:
                nxt = buf['dA'][i - 1]
                _lib.gemm_nn(dA, self.W[i], out=nxt, elu_out=h[i], M=B, N=L['k'], K=L['n'], lda=dA.stride(0), ldb=L['kp'],
                             ldc=nxt.stride(0), ldp=h[i].stride(0))
                dA = nxt
        return self.loss

    def eval_batch(self, x, t, z):
        """The loss alone (no gradient) of one batch, as a device float."""
        self._check_batch(x, t, z)
        buf = self._buffers(x.shape[0])
        weight = self._forward(x, t, z, buf)
        loss, _ = _lib.dsm_loss_grad(buf['out'], z, weight=weight, reduce_mean=self.reduce_mean, want_grad=False, workspace=self.ws)
        return loss

    def draw(self, B, index, salt=0):
        """(t, z) of the stream (seed, index): t uniform on [eps, T], z standard normal [B, D] from the library's counter-based generator."""
        buf = self._buffers(B)
        self._gen.manual_seed(stream_key(self.seed, index, 1 + 2 * salt))
        t = torch.rand(B, device=self.device, dtype=torch.float32, generator=self._gen) * (self.sde.T - T_EPS) + T_EPS
        D4 = pad4(self.D)
        _lib.perturb_randn(buf['zeros'], buf['ones'], None, buf['scratch'], B, D4, 0, stream_key(self.seed, index, 2 + 2 * salt),
                           z_out=buf['zfull'])
        z = buf['zfull'] if D4 == self.D else buf['zfull'][:, :self.D].contiguous()
        return t, z

    def current_lr(self):
        return warmup_lr(self.optim['lr'], self.global_step, self.optim['warmup'])

    def step(self, x, t=None, z=None):
        """One optimiser step on the clean batch ``x``; ``t`` / ``z`` given (both) are used as they are, otherwise they are the draws of
        the stream (seed, global_step).  Returns the device loss of the batch BEFORE the update; no host read-back."""
        if (t is None) != (z is None):
            raise ValueError("step: pass both t and z, or neither")
        if t is None:
            t, z = self.draw(x.shape[0], self.global_step)
        loss = self.loss_and_grad(x, t, z)
        o = self.optim
        clip = float(o['grad_clip'])
        sumsq = None
        if clip >= 0:
            sumsq = _lib.grad_sumsq(self.grad, out=self.sumsq, workspace=self.ws)
        _lib.adam_step(self.theta, self.grad, self.m, self.v, self.global_step + 1, self.current_lr(), betas=(o['beta1'], 0.999),
                       eps=o['eps'], weight_decay=o['weight_decay'], sumsq=sumsq, max_norm=clip)
        self.global_step += 1
        self.model._invalidate()          # FCN.packed() caches a padded copy of the first weight: never leave a stale one behind
        return loss

    # ---------------------------------------------------------------------------------------- data
    def train_data(self):
        if self._train is None:
            self._train = data_split(self.config, 'train').to(self.device)
            if self._train.shape[1] != self.D:
                raise RuntimeError(f"data rows have {self._train.shape[1]} columns, model.state_size is {self.D}")
        return self._train

    def _epoch_perm(self, epoch):
        n = self.train_data().shape[0]
        self._gen.manual_seed(stream_key(self.seed, epoch, 0))
        return torch.randperm(n, device=self.device, generator=self._gen)

    def batches_per_epoch(self):
        return max(1, self.train_data().shape[0] // self.batch_size)

    def next_batch(self):
        """The next batch of the seeded epoch permutation (whole batches only; a split smaller than a batch is one batch)."""
        data = self.train_data()
        per = self.batches_per_epoch()
        self.epoch, self._pos = divmod(self.global_step, per)
        if self._perm is None or self._perm[0] != self.epoch:
            self._perm = (self.epoch, self._epoch_perm(self.epoch))
        idx = self._perm[1][self._pos * self.batch_size:(self._pos + 1) * self.batch_size]
        return data.index_select(0, idx)

    def evaluate(self, checkpoint_path, num_samples=1000, log=print):
        """The two callbacks the Euclidean configs name, as numbers: min / max / mean norm of ``num_samples`` samples drawn from the
        current weights (KSphereEvaluation) and ``dim``, the mean estimated dimension over ``logging.svd_points`` points (default 5) of
        the checkpoint written to ``checkpoint_path`` (ScoreSpectrumVisualization).  The sampler draws from streams of its own
        (sampling.SALT_*), so training goes on exactly as it would have."""
        import copy
        from . import dim_reduction, sampling
        _, eps = sde_lib.configure_sde(self.config)
        shape = [int(num_samples)] + list(self.config.data.shape)
        samples, _ = sampling.get_sampling_fn(self.config, self.sde, shape, eps)(self.model, seed=stream_key(self.seed, self.global_step, 5))
        out = sampling.ksphere_evaluation(samples)
        self.save_checkpoint(checkpoint_path)
        config = copy.deepcopy(self.config)
        config.model.checkpoint_path = checkpoint_path
        config.device = str(self.device)
        if config.get('dim_estimation.num_datapoints') is None and config.get('logging.svd_points') is None:
            config.logging.svd_points = 5
        _, dims = dim_reduction.get_manifold_dimension(config, return_svd=True, return_dims=True)
        dims = [int(d) for d in dims if int(d) >= 0]
        out['dim'] = float(sum(dims)) / len(dims) if dims else float('nan')
        self.evaluations.append((self.global_step, out))
        if log is not None:
            log(f"step {self.global_step} min_norm {out['min_norm']:.6g} max_norm {out['max_norm']:.6g} mean_norm {out['mean_norm']:.6g} "
                f"dim {out['dim']:.3g}")
        return out

    def fit(self, n_iters, log_every=0, checkpoint_every=0, checkpoint_path=None, log=print, eval_every=0, num_samples=1000):
        """Steps until ``global_step == n_iters``.  The loss is fetched every ``log_every`` steps (0: only at the end) and a checkpoint
        written every ``checkpoint_every`` steps (0: never here).  Returns [(step, loss)] of the fetched losses; the first entry is the
        loss of the first step taken and the last that of the last.  ``eval_every`` K > 0 (needs ``checkpoint_path``): every K steps
        and at the end ``evaluate`` logs the sample norms and the estimated dimension; its results collect in ``self.evaluations``."""
        if eval_every and not checkpoint_path:
            raise ValueError("fit: eval_every needs checkpoint_path (the dimension is read from the checkpoint just written)")
        history, first = [], self.global_step
        while self.global_step < n_iters:
            at = self.global_step
            loss = self.step(self.next_batch())
            fetch = at == first or (log_every and (at + 1) % log_every == 0) or at + 1 == n_iters
            if fetch:
                value = float(loss)
                history.append((at, value))
                if log is not None and (log_every or at + 1 == n_iters):
                    log(f"step {at + 1}/{n_iters} epoch {self.epoch} lr {warmup_lr(self.optim['lr'], at, self.optim['warmup']):.3e} loss {value:.6g}")
            if checkpoint_every and checkpoint_path and self.global_step % checkpoint_every == 0 and self.global_step < n_iters:
                self.save_checkpoint(checkpoint_path)
            if eval_every and (self.global_step % eval_every == 0 or self.global_step == n_iters):
                self.evaluate(checkpoint_path, num_samples=num_samples, log=log)
        return history

    def eval_loss(self, split='val', max_batches=None):
        """Mean loss over whole batches of ``validation.batch_size`` rows of a split, with the draws of the streams (seed, batch, salt 1):
        the same number for the same weights.  One read-back at the end."""
        rows = data_split(self.config, split).to(self.device)
        bs = int(self.config.get('validation.batch_size', self.batch_size))
        bs = min(bs, rows.shape[0])
        n = rows.shape[0] // bs
        if max_batches is not None:
            n = min(n, int(max_batches))
        total = torch.zeros((), device=self.device, dtype=torch.float64)
        for i in range(n):
            x = rows[i * bs:(i + 1) * bs].contiguous()
            t, z = self.draw(bs, i, salt=1)
            total += self.eval_batch(x, t, z).double()
        return float(total) / n

    # ---------------------------------------------------------------------------------------- checkpoints
    def save_checkpoint(self, path):
        write_checkpoint(path, checkpoint_dict(self.state_dict(), self.config, self.global_step, self.epoch, self.m, self.v))
        return path

    def load_checkpoint(self, path):
        from .lightning_modules import checkpoint_io
        ckpt = checkpoint_io.load_checkpoint(path)
        self.load_state_dict(checkpoint_io.score_model_state_dict(ckpt))
        states = ckpt.get('optimizer_states') or []
        if states and 'm' in states[0] and 'v' in states[0]:
            if states[0]['m'].numel() != self.n_params:
                raise RuntimeError(f"{path}: optimizer state of {states[0]['m'].numel()} entries, this network has {self.n_params}")
            self.m.copy_(states[0]['m']); self.v.copy_(states[0]['v'])
        else:
            self.m.zero_(); self.v.zero_()
        self.global_step = int(ckpt.get('global_step', 0))
        self.epoch = int(ckpt.get('epoch', 0))
        self._perm = None
        self.model._invalidate()
        return self


def last_checkpoint_path(config, log_path=None, log_name=None):
    log_path = log_path if log_path is not None else (config.logging.get('log_path') or './')
    log_name = log_name if log_name is not None else (config.logging.get('log_name') or 'train')
    return os.path.join(log_path, log_name, 'checkpoints', 'last.ckpt')


def train(config, log_path=None, checkpoint_path=None, n_iters=None, log_every=0, checkpoint_every=0, log_name=None, log=print,
          eval_every=0):
    """``--mode train``: resume from ``checkpoint_path`` (or ``config.model.checkpoint_path``) when given, train to ``n_iters`` steps,
    write ``<log_path>/<log_name>/checkpoints/last.ckpt`` every ``checkpoint_every`` steps and at the end.  Returns (trainer, history)."""
    check_scope(config)
    trainer = FcnTrainer(config, config.get('device', 'cuda:0'))
    resume = checkpoint_path if checkpoint_path is not None else config.model.get('checkpoint_path')
    if resume:
        trainer.load_checkpoint(resume)
    if n_iters is None:
        n_iters = config.get('training.n_iters')
    if n_iters is None:
        raise ValueError("train: pass --n_iters (the configs carry no usable step count)")
    n_iters = int(min(float(n_iters), 2 ** 62))
    out = last_checkpoint_path(config, log_path, log_name)
    history = trainer.fit(n_iters, log_every=log_every, checkpoint_every=checkpoint_every, checkpoint_path=out, log=log,
                          eval_every=eval_every)
    trainer.save_checkpoint(out)
    if log is not None:
        log(f"wrote {out} at global_step {trainer.global_step}")
    return trainer, history
