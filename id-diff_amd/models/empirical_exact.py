"""Score of the EMPIRICAL distribution of a data set: the acceptance model for data with no closed-form score (the 'Line' curve, a
user's own [N, D] array).  Not part of the reference.

The N points x_i, each with weight 1 / N, convolved with N(0, sigma^2 I), have the score

    w_i(x) = softmax_i(-|x - x_i|^2 / (2 sigma^2)),      score(x) sigma^2 = sum_i w_i(x) x_i - x

which is exact for any finite data set and needs no training.  ``forward`` is one launch of csrc/empirical_score.hip (attention with
the cloud as keys and values, fp64 from the first difference to the final rounding, no [B, N] buffer); ``reference_score`` restates
it in fp64 numpy with direct differences for the tests.

The noise level follows the other exact models: sigma(t) = sigma_min (sigma_max / sigma_min)^t, widened by ``data.noise_std``.  The
drivers evaluate the score at t = sampling_eps, so **``model.sigma_min`` is the kernel bandwidth of the estimate**: the spectrum of the
score matrix is that of the cloud seen at the scale sigma_min.  The estimate means something only where the effective sample size
ESS = 1 / sum_i w_i^2 is well above 1: with sigma below the spacing of the data one point holds all the weight, the score points at
that point from every direction, and the reported dimension is that of the ambient space (on the line at sigma = 0.01 the ESS is 1.5
and points report 96 and 98).  The forward therefore asks the kernel for the ESS of every row and warns, once per model, when the
median of a call falls below ``ess_warn`` (4.0; 0 disables the check, and with it the call's one read-back).

A sample-based score needs N to grow exponentially in the intrinsic dimension d (the ball of radius sigma around a point must hold
several neighbours in d dimensions): the Gaussian blobs (d = 10, 4000 points) are out of reach of ANY bandwidth, and with D = 1024
they are refused by the kernel's cap on D anyway.
"""
import warnings

import numpy as np
import torch

from .. import _lib
from ..lightning_data_modules.utils import create_lightning_datamodule
from . import utils
from .base import HipScoreModel

W_FLOOR = 2.0 ** -60        # reference_score: the radius r_b spans the points with at least this weight


def reference_score(x, sigma, X):
    """fp64 numpy with DIRECT differences (not the kernel's centred, expanded form): rows x [B, D], levels sigma [B] (or a scalar),
    cloud X [N, D] -> ``(score sigma^2 [B, D], ess [B], r [B])`` with d_i = x_i - x_b, w = softmax_i(-|d_i|^2 / (2 sigma_b^2)),
    score sigma^2 = sum_i w_i d_i, ess = 1 / sum_i w_i^2 and r_b = max{|d_i| : w_i >= 2^-60}.  The arithmetic runs in the dtype of
    ``X`` when that is wider than fp64 (``np.longdouble`` for the tests' oracle)."""
    dt = np.longdouble if np.asarray(X).dtype == np.longdouble else np.float64
    x, X = np.asarray(x, dtype=dt), np.asarray(X, dtype=dt)
    x, X = x.reshape(x.shape[0], -1), X.reshape(X.shape[0], -1)
    B = x.shape[0]
    sigma = np.broadcast_to(np.asarray(sigma, dtype=dt), (B,))
    out, ess, r = np.empty_like(x), np.empty(B, dtype=dt), np.empty(B, dtype=dt)
    for b in range(B):
        d = X - x[b]
        d2 = (d * d).sum(axis=1)
        lg = -d2 / (2 * sigma[b] * sigma[b])
        w = np.exp(lg - lg.max())
        w = w / w.sum()
        out[b] = (w[:, None] * d).sum(axis=0)
        ess[b] = 1 / (w * w).sum()
        r[b] = np.sqrt(d2[w >= W_FLOOR].max())
    return out, ess, r


def train_split(config):
    """The whole train split of the config's data set, [N, D] fp32, as ``get_manifold_dimension`` will split it: the driver seeds
    torch with ``config.seed`` immediately before it builds its data module, so the same seed inside ``fork_rng`` gives the same
    data and the same split row for row -- and leaves the global stream the driver goes on to use as it was."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(config.get('seed', 42)))
        dm = create_lightning_datamodule(config)
        dm.setup()
        part = dm.train_data
        if hasattr(part.dataset, 'data'):
            rows = torch.as_tensor(part.dataset.data)[torch.as_tensor(part.indices)]
        else:
            rows = torch.stack([torch.as_tensor(part[i][0] if isinstance(part[i], (list, tuple)) else part[i]) for i in range(len(part))])
    return rows.reshape(rows.shape[0], -1).to(torch.float32)


@utils.register_model(name='empirical_exact')
class EmpiricalExact(HipScoreModel):
    def __init__(self, config, data=None):
        super().__init__()
        self.noise_std = float(config.data.get('noise_std', 0.0) or 0.0)
        self.sigma_min, self.sigma_max, self.N = config.model.sigma_min, config.model.sigma_max, config.model.num_scales
        self.ess_warn = 4.0
        self._ess_warned = False
        self.last_ess = None                                         # [B] fp32 on the device: the ESS of the last forward's rows
        if data is None:
            data = train_split(config)
        data = torch.as_tensor(np.asarray(data) if not isinstance(data, torch.Tensor) else data.detach())
        if data.ndim < 2 or data.shape[0] < 1:
            raise ValueError(f"empirical_exact: data must be [N >= 1, ...], got {tuple(data.shape)}")
        data = data.reshape(data.shape[0], -1).to(torch.float32).contiguous()
        n, D = data.shape
        if not _lib.empirical_score_ok(n, D):
            raise NotImplementedError(f"empirical_exact: a cloud of {n} points in R^{D}: the kernel keeps a row's fp64 output in "
                                      "registers and serves D <= 192 (idiff_empirical_score_ok); wider data needs output slices "
                                      "with recomputed logits, which is not built")
        self.cloud = torch.nn.Parameter(data.clone(), requires_grad=False)        # [N, D] fp32: .to() moves it, _pack rebuilds

    def _pack(self):
        return _lib.empirical_pack(self.cloud.detach().contiguous())

    def forward(self, x, labels, out_rowscale=None):
        x, labels = self._check_inputs(x, labels)
        pk = self.packed()
        shape = x.shape
        x = x.reshape(shape[0], -1)
        if x.shape[1] != pk["D"]:
            raise RuntimeError(f"empirical_exact: x {tuple(shape)} for a cloud in R^{pk['D']}")
        t = labels / (self.N - 1)
        lo = torch.tensor(self.sigma_min).type_as(t)
        hi = torch.tensor(self.sigma_max).type_as(t)
        sigma = lo * (hi / lo) ** t                                  # [B]
        eff2 = sigma * sigma + self.noise_std ** 2                   # the data's own noise widens every level
        # model output convention: score = -out / std  ->  out = -sigma score = (-sigma / sigma_eff^2) (sum_i w_i x_i - x)
        mult = -sigma / eff2
        if out_rowscale is not None:
            mult = mult * out_rowscale
        out, ess = _lib.empirical_score(x, pk, torch.sqrt(eff2).contiguous(), mult.contiguous())
        self.last_ess = ess
        if self.ess_warn > 0 and not self._ess_warned and ess.numel():
            median = float(ess.float().nanmedian().item())           # the one synchronisation of the call (none once warned)
            if median < self.ess_warn:
                self._ess_warned = True
                warnings.warn(f"id-diff_amd: empirical_exact: the median effective sample size of a call is {median:.2f} at sigma = "
                              f"{float(torch.sqrt(eff2).median().item()):.4g} (below ess_warn = {self.ess_warn:g}): the bandwidth is "
                              "below the spacing of the data and the spectrum of such scores says nothing about the dimension; "
                              "raise model.sigma_min (empirical.sigma_from_knn gives a starting value)")
        return out.view(shape)
