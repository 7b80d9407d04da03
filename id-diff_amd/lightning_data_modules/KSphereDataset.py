"""k-sphere data (drop-in for /root/reference/lightning_data_modules/KSphereDataset.py:7-135).

Uniform points on S^k in R^{k+1} (normalised Gaussians, :87-91), embedded in R^ambient by the Q factor of a
seed-0 Gaussian matrix (:38-44; restated with ``.numpy()`` because the reference's ``np.linalg.qr(Tensor)``
breaks under numpy 2), plus optional isotropic noise.  Host-side generation: it is a few MB, done once.

Several spheres (``n_spheres``, ``manifold_dim`` an int or a list, ``radii``) are concatenated, each placed by
``embedding_type``: 'random_isometry', 'first' (coordinates 0..k), 'separating' (:49-56: disjoint coordinate blocks) or
'along_axis' (:57-64: sphere i starts at coordinate i, so neighbours share all but one axis).  ``angle_std != -1`` samples
polar angles from N(0, angle_std^2) instead of the uniform law (:75-94).  ``frames(config)`` gives the same placement as
orthonormal frames, for the exact score model of the union (models/ksphere_union_exact.py).
"""
import numpy as np
import torch
from torch.utils.data import Dataset

from . import utils


class KSphereDataset(Dataset):
    def __init__(self, config):
        super().__init__()
        d = config.data
        self.data = self.generate_data(d.get('data_samples'), d.get('n_spheres'), d.get('ambient_dim'),
                                       d.get('manifold_dim'), d.get('noise_std'), d.get('embedding_type'),
                                       d.get('radii', []), d.get('angle_std', -1))

    @staticmethod
    def isometry(ambient_dim, manifold_dim):
        g = torch.Generator().manual_seed(0)
        a = torch.randn(size=(ambient_dim, manifold_dim + 1), generator=g)
        q, _ = np.linalg.qr(a.numpy())
        return torch.from_numpy(q)

    def generate_data(self, n_samples, n_spheres, ambient_dim, manifold_dim, noise_std, embedding_type, radii,
                      angle_std):
        if radii == []:
            radii = [1] * n_spheres
        dims = [manifold_dim] * n_spheres if isinstance(manifold_dim, int) else list(manifold_dim)
        chunks = []
        for i in range(n_spheres):
            k = dims[i]
            pts = self.sample_sphere(n_samples, k, angle_std)
            pts = pts * radii[i]
            if embedding_type == 'random_isometry':
                pts = (self.isometry(ambient_dim, k) @ pts.T).T
            elif embedding_type == 'first':
                pts = torch.cat([pts, torch.zeros([n_samples, ambient_dim - pts.shape[1]])], dim=1)
            elif embedding_type in ('separating', 'along_axis'):
                lead = first_axis(embedding_type, i, k, n_spheres, ambient_dim)
                pts = torch.cat([torch.zeros((n_samples, lead)), pts], dim=1)
                pts = torch.cat([pts, torch.zeros([n_samples, ambient_dim - pts.shape[1]])], dim=1)
            else:
                raise RuntimeError('Unknown embedding type.')
            pts = pts + noise_std * torch.randn_like(pts)
            chunks.append(pts)
        return torch.cat(chunks, dim=0)

    @staticmethod
    def sample_sphere(n_samples, manifold_dim, std=-1):
        """std == -1: uniform on S^k (:87-91).  Otherwise polar angles std * randn(n_samples, k) in ONE draw, as the reference
        makes it (:93), and x_i = sin(a_0) ... sin(a_{i-1}) cos(a_i), x_k = sin(a_0) ... sin(a_{k-1}) with the running product
        multiplied in the reference's order (:77-85) -- over all samples at once instead of row by row."""
        if std == -1:
            pts = torch.randn((n_samples, manifold_dim + 1))
            return pts / torch.linalg.norm(pts, dim=1)[:, None]
        angles = std * torch.randn((n_samples, manifold_dim))
        cos, sin = torch.cos(angles), torch.sin(angles)
        cols, sin_prod = [], 1
        for i in range(manifold_dim):
            cols.append(sin_prod * cos[:, i])
            sin_prod = sin_prod * sin[:, i]
        cols.append(sin_prod if manifold_dim else torch.ones(n_samples))
        return torch.stack(cols, dim=1)

    def __getitem__(self, index):
        return self.data[index]

    def __len__(self):
        return len(self.data)


def first_axis(embedding_type, i, k, n_spheres, ambient_dim):
    """First coordinate of sphere i of dimension k under the two axis-aligned placements, with the reference's two errors (:51-52,
    :59-60) and its quirk that 'separating' offsets by i * (k_i + 1) of the CURRENT sphere (:53)."""
    if embedding_type == 'separating':
        if n_spheres * (k + 1) > ambient_dim:
            raise RuntimeError('Cant fit that many spheres. Enusre that n_spheres * (manifold_dim + 1) <= ambient_dim')
        return i * (k + 1)
    if (n_spheres - 1) + (k + 1) > ambient_dim:
        raise RuntimeError('Cant fit that many spheres.')
    return i


def frames(config):
    """[(Q_j fp64 numpy [ambient_dim, k_j + 1] with orthonormal columns, R_j)]: sphere j of KSphereDataset(config) is
    R_j Q_j S^{k_j} (+ noise).  Data set and exact model both read the placement from here."""
    d = config.data
    n_spheres, n, embedding_type = d.get('n_spheres'), d.get('ambient_dim'), d.get('embedding_type')
    radii = d.get('radii', [])
    radii = [1] * n_spheres if radii == [] else list(radii)
    manifold_dim = d.get('manifold_dim')
    dims = [manifold_dim] * n_spheres if isinstance(manifold_dim, int) else list(manifold_dim)
    out = []
    for i in range(n_spheres):
        k = dims[i]
        if embedding_type == 'random_isometry':
            Q = KSphereDataset.isometry(n, k).numpy().astype(np.float64)      # the fp32 values the data set multiplies by
        elif embedding_type in ('first', 'separating', 'along_axis'):
            lead = 0 if embedding_type == 'first' else first_axis(embedding_type, i, k, n_spheres, n)
            if lead + k + 1 > n:
                raise RuntimeError(f"sphere {i}: coordinates {lead}..{lead + k} do not fit R^{n}")
            Q = np.zeros((n, k + 1))
            Q[lead + np.arange(k + 1), np.arange(k + 1)] = 1.0
        else:
            raise RuntimeError('Unknown embedding type.')
        out.append((Q, float(radii[i])))
    return out


@utils.register_lightning_datamodule(name='KSphere')
class KSphereDataModule(utils.SplitDataModule):
    def make_dataset(self):
        return KSphereDataset(self.config)
