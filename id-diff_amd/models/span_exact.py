"""Score of a flat density on the linear span of the fixed squares (acceptance model for "correct ID on the squares
manifolds", in the role ``ksphere_exact`` plays for the sphere).  Not part of the reference.

An image of ``FixedSquaresManifold`` is M c, M [S^2, K] the 0/1 masks of the squares and c uniform in [0, 1)^K: the
data lie in a K-cube inside span(M).  With Q an orthonormal basis of that span, this model returns

    out = (x - Q Q^T x) / sigma(t),        i.e.   score(x) = -(I - Q Q^T) x / sigma^2,

the VE score of a density that is FLAT on span(M): Gaussian in the normal directions, zero along the span.

What it is: the small-sigma limit of the true perturbed score at points away from the cube's faces, which is where the
ID estimator evaluates it (sigma = 1e-2 against coefficients of order 1), and the cleanest statement of what the
estimator should see: D - rank(M) large singular values, rank(M) vanishing ones.
What it is not: the score of the cube.  It ignores the faces (no restoring force for c outside [0, 1]), so it is wrong
within a few sigma of a face and at large sigma, and it is not a model of the blobs (whose manifold is curved).

Q comes from an fp64 SVD of M with a rank threshold (numpy's: max(S^2, K) eps sigma_max), not from a QR: the masks
need not be independent -- with seed 42 the hundred squares of ``squares/100`` have rank 99 -- and a QR would hand
back a basis vector for every column, the dependent column's being an arbitrary direction.  The two projections are
GEMMs on the MFMA path; the rest are the existing element-wise kernels.
"""
import numpy as np
import torch

from .. import _lib
from ..lightning_data_modules.SyntheticDataset import get_the_squares, square_rects
from . import utils
from .base import HipScoreModel


def mask_matrix(rects, S):
    """M [S^2, K] fp64: column k is the 0/1 mask of square k = (row0, col0, side), pixels in row-major order."""
    rects = np.asarray(rects, dtype=np.int64).reshape(-1, 3)
    M = np.zeros((S, S, len(rects)))
    for k, (r0, c0, side) in enumerate(rects):
        M[r0:r0 + side, c0:c0 + side, k] = 1.0
    return M.reshape(S * S, len(rects))


def span_basis(M):
    """(Q [D, r] fp64 with orthonormal columns spanning the columns of M, r = rank(M)) from the SVD, the rank by numpy's
    ``matrix_rank`` threshold max(M.shape) * eps * largest singular value."""
    U, s, _ = np.linalg.svd(M, full_matrices=False)
    tol = max(M.shape) * np.finfo(np.float64).eps * (s[0] if s.size else 0.0)
    r = int(np.count_nonzero(s > tol))
    return np.ascontiguousarray(U[:, :r]), r


@utils.register_model(name='span_exact')
class SpanExact(HipScoreModel):
    def __init__(self, config):
        super().__init__()
        d = config.data
        if d.get('dataset_type') != 'FixedSquaresManifold':
            raise NotImplementedError(f"span_exact is the flat-span score of FixedSquaresManifold; data.dataset_type is "
                                      f"{d.get('dataset_type')!r}")
        self.S = int(d.image_size)
        self.sigma_min, self.sigma_max, self.N = config.model.sigma_min, config.model.sigma_max, config.model.num_scales
        rects = square_rects(get_the_squares(config.seed, int(d.num_squares), list(d.square_range), self.S))
        Q, self.rank = span_basis(mask_matrix(rects, self.S))
        self.Q = torch.nn.Parameter(torch.from_numpy(Q), requires_grad=False)      # [S^2, rank] fp64

    def _pack(self):
        q = self.Q.detach().float()
        rp = (self.rank + 3) // 4 * 4
        qpad = torch.zeros(q.shape[0], rp, device=q.device)
        qpad[:, :self.rank] = q
        return {"Q": qpad.contiguous(), "Qt": qpad.t().contiguous()}

    def forward(self, x, labels, out_rowscale=None):
        x, labels = self._check_inputs(x, labels)
        pk = self.packed()
        B, D = x.shape[0], self.S * self.S
        if x.numel() != B * D:
            raise RuntimeError(f"span_exact: expected {B} images of {self.S} x {self.S}, got {tuple(x.shape)}")
        flat = x.view(B, D)
        t = labels / (self.N - 1)
        lo = torch.tensor(self.sigma_min).type_as(t)
        hi = torch.tensor(self.sigma_max).type_as(t)
        sigma = lo * (hi / lo) ** t                                  # [B]
        inv_sigma = (1.0 / sigma).contiguous()
        scale = inv_sigma if out_rowscale is None else (inv_sigma * out_rowscale).contiguous()
        a = _lib.gemm(flat, pk["Qt"])                                # a = x Q             [B, rp]
        proj = _lib.gemm(a, pk["Q"], epilogue=_lib.make_epilogue(out_scale=-1.0))   # -(Q a)  [B, D]
        diff = torch.empty_like(flat)
        _lib.add_scale(flat, proj, diff, flat.numel(), 1.0)          # x - Q Q^T x
        res = torch.empty_like(x)
        _lib.affine_act(diff, res, diff.numel(), 1.0, 0.0, None, scale, D)
        return res
