"""Analytic score of a noised UNION of k-spheres of different dimension (the acceptance model for "each point reports the dimension
of the sphere it lies on"; not part of the reference, as ``ksphere_exact`` is not).

Component j: radius R_j, orthonormal frame Q_j [n, p_j], p_j = k_j + 1, weight pi_j = 1 / J; its data is uniform on R_j S^{k_j}
inside span Q_j (lightning_data_modules/KSphereDataset.py: frames).  At noise level sigma, with a_j = Q_j^T x, r_j = |a_j|,
kappa_j = r_j R_j / sigma^2, nu_j = p_j / 2 - 1, and dropping what all components share:

    E_j = log pi_j - R_j^2 / (2 sigma^2) + lgamma(p_j / 2) + nu_j log(2 / kappa_j) + log I_nu_j(kappa_j)
    w   = softmax_j(E_j),   A_j = I_{nu_j + 1}(kappa_j) / I_nu_j(kappa_j)
    score(x) sigma^2 = -x + sum_j w_j (R_j A_j / r_j) Q_j a_j

The Bessel functions come from the Hankel series H_nu(kappa) = sum_m (-1)^m prod_{i <= m} (4 nu^2 - (2 i - 1)^2) / (m! (8 kappa)^m),
64 terms:  log I_nu = kappa - log(2 pi kappa) / 2 + log H_nu,  A = H_{nu + 1} / H_nu,  which match scipy's ``ive`` to rounding for
p <= 129 wherever kappa >= kappa_min(p) = max(32, p^2 / 16).  Below that nothing is guessed: the component is bounded by
U_j = log pi_j + kappa_j - R_j^2 / (2 sigma^2) >= E_j (Gamma(nu + 1) (2 / kappa)^nu I_nu(kappa) <= e^kappa), its weight is exactly
0 in fp64 where U_j < max(exact E) - 800, and a row where that does not hold -- or that has no exact component -- is REFUSED.
For a point on one sphere of a union the OTHER spheres are in that regime (the projection onto their subspace is short), which
is why ``ksphere_exact``'s blanket ``kappa >= 5e3`` cannot serve a union.

``forward`` is one launch of csrc/ksphere_union.hip (fp64 from the projection to the final rounding); ``reference_score`` restates
it in fp64 numpy for the tests.
"""
import math

import numpy as np
import torch

from .. import _lib
from ..lightning_data_modules.KSphereDataset import frames as dataset_frames
from . import utils
from .base import HipScoreModel

TERMS = 63          # terms of the Hankel series after the leading 1 (csrc/ksphere_union.hip: TERMS)
FAR = 800.0         # exp(-800) == 0 in fp64


def kappa_min(p):
    return max(32.0, p * p / 16.0)


def hankel(nu, kappa):
    """H_nu(kappa), the kernel's loop: ascending m, term_m = term_{m-1} ((2 m - 1)^2 - 4 nu^2) / (8 kappa m)."""
    kappa = np.asarray(kappa, dtype=np.float64)
    mu, inv = 4.0 * nu * nu, 1.0 / (8.0 * kappa)
    term = np.ones_like(kappa)
    total = np.ones_like(kappa)
    for m in range(1, TERMS + 1):
        term = term * (((2 * m - 1) ** 2 - mu) * (inv * (1.0 / m)))
        total = total + term
    return total


def log_bessel_i(nu, kappa):
    """log I_nu(kappa) for kappa >= kappa_min(2 nu + 2)."""
    return kappa - 0.5 * np.log(2.0 * np.pi * kappa) + np.log(hankel(nu, kappa))


def bessel_ratio(nu, kappa):
    """I_{nu + 1}(kappa) / I_nu(kappa) for kappa >= kappa_min(2 nu + 2)."""
    return hankel(nu + 1.0, kappa) / hankel(nu, kappa)


def reference_score(x, sigma, frames, log_weights=None):
    """fp64 numpy: (score [B, n], weights [B, J], refused [B] bool) of the noised union at rows x [B, n] and levels sigma [B] (or a
    scalar); frames = [(Q_j [n, p_j], R_j)].  Refused rows are NaN in ``score`` and in ``weights``."""
    x = np.asarray(x, dtype=np.float64)
    B, n = x.shape
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (B,))
    J = len(frames)
    lw = np.full(J, -math.log(J)) if log_weights is None else np.asarray(log_weights, dtype=np.float64)
    s2 = sigma * sigma
    E = np.empty((B, J))
    exact = np.empty((B, J), dtype=bool)
    back = np.empty((J, B, n))                      # R_j A_j / r_j  Q_j a_j
    with np.errstate(all="ignore"):
        for j, (Q, R) in enumerate(frames):
            Q = np.asarray(Q, dtype=np.float64)
            p = Q.shape[1]
            nu = 0.5 * p - 1.0
            a = x @ Q
            r = np.sqrt((a * a).sum(axis=1))
            kappa = r * R / s2
            exact[:, j] = kappa >= kappa_min(p)
            half = R * R / (2.0 * s2)
            H = hankel(nu, kappa)
            e = (lw[j] + math.lgamma(0.5 * p)) - half + nu * np.log(2.0 / kappa) + kappa - 0.5 * np.log(2.0 * np.pi * kappa) + np.log(H)
            E[:, j] = np.where(exact[:, j], e, lw[j] + kappa - half)
            back[j] = (R * (hankel(nu + 1.0, kappa) / H) / r)[:, None] * (a @ Q.T)
        top = np.where(exact, E, -np.inf).max(axis=1)
        refused = ~exact.any(axis=1) | (~exact & ~(E < (top - FAR)[:, None])).any(axis=1)
        w = np.where(exact, np.exp(E - top[:, None]), 0.0)
        w = w / w.sum(axis=1, keepdims=True)
        score = -x
        for j in range(J):
            score = score + np.where(exact[:, j:j + 1], w[:, j:j + 1] * back[j], 0.0)
        score = score / s2[:, None]
    score[refused] = np.nan
    w[refused] = np.nan
    return score, w, refused


@utils.register_model(name='ksphere_union_exact')
class KSphereUnionExact(HipScoreModel):
    def __init__(self, config):
        super().__init__()
        d = config.data
        if d.get('angle_std', -1) != -1:
            raise NotImplementedError("ksphere_union_exact: angle_std != -1 samples a non-uniform density on the spheres; the exact "
                                      "score is that of the uniform one")
        self.n = d.ambient_dim
        self.noise_std = float(d.get('noise_std', 0.0) or 0.0)
        self.sigma_min, self.sigma_max, self.N = config.model.sigma_min, config.model.sigma_max, config.model.num_scales
        fr = dataset_frames(config)
        self.radii = [R for _, R in fr]
        self.widths = [Q.shape[1] for Q, _ in fr]
        J, P = len(fr), sum(self.widths)
        if not (1 <= J <= 8 and max(self.widths) <= 128):
            raise NotImplementedError(f"ksphere_union_exact: {J} spheres of dimension up to {max(self.widths) - 1}: the kernel takes at "
                                      "most 8 of dimension at most 127")
        self.Qcat = torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(np.concatenate([Q for Q, _ in fr], axis=1))),
                                       requires_grad=False)                                  # [n, P] fp64
        off = np.concatenate([[0], np.cumsum(self.widths)[:-1]])
        self.comp = np.array([[off[j], self.widths[j], self.radii[j], -math.log(J)] for j in range(J)], dtype=np.float64)

    def frames(self):
        """[(Q_j fp64 numpy, R_j)] as the kernel holds them."""
        q = self.Qcat.detach().cpu().numpy()
        return [(q[:, int(o):int(o) + int(p)], float(R)) for o, p, R, _ in self.comp]

    def _pack(self):
        q = self.Qcat.detach().double().contiguous()
        J, P = len(self.widths), q.shape[1]
        if not _lib.ksphere_union_ok(self.n, J, P):
            raise NotImplementedError(f"ksphere_union_exact: frames of {P} columns in R^{self.n} do not fit the kernel's LDS "
                                      "(idiff_ksphere_union_ok)")
        return {"Q": q}

    def forward(self, x, labels, out_rowscale=None):
        x, labels = self._check_inputs(x, labels)
        pk = self.packed()
        t = labels / (self.N - 1)
        lo = torch.tensor(self.sigma_min).type_as(t)
        hi = torch.tensor(self.sigma_max).type_as(t)
        sigma = lo * (hi / lo) ** t                                  # [B]
        eff2 = sigma * sigma + self.noise_std ** 2                   # the data's own noise widens every level
        # model output convention: score = -out / std  ->  out = -sigma score = (-sigma / sigma_eff^2) (-x + ...)
        mult = -sigma / eff2
        if out_rowscale is not None:
            mult = mult * out_rowscale
        out, refused = _lib.ksphere_union_score(x, pk["Q"], self.comp, torch.sqrt(eff2).contiguous(), mult.contiguous())
        count = int(refused.item())                                  # the one synchronisation of the call
        if count:
            raise NotImplementedError(f"ksphere_union_exact: {count} of {x.shape[0]} rows refused: a component whose Bessel series "
                                      "does not apply (kappa < max(32, p^2 / 16)) could not be shown to have zero weight")
        return out
