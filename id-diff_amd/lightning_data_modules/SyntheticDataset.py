"""The paper's image manifolds of known dimension (drop-in for the reference's lightning_data_modules/SyntheticDataset.py,
data module 'Synthetic'): ``FixedSquaresManifold`` (:81-123) and ``FixedGaussiansManifold`` (:125-183), rendered on the GPU.

The reference paints every image with Python loops over pixels and draws from Python's ``random``.  Here

* the tables (which squares / which centres) come from ``random.Random(config.seed)`` with the reference's own calls, so
  they are the reference's tables;
* the per-image draws continue the SAME Mersenne-Twister stream: its state is transplanted into a
  ``numpy.random.RandomState`` whose ``random_sample`` returns, vectorised, bit for bit what ``random.random()`` would
  return call by call (both build a double from two 32-bit outputs as (a >> 5, b >> 6));
* the pixels are written by ``idiff_render_squares_f32`` / ``idiff_render_gaussians_f32`` (csrc/manifolds.hip) in slabs of
  images: the squares bit-equal to the reference, the blobs within (K + 4) 2^-24 max / (max - min) per image.

``.data`` is a CPU [N, 1, S, S] fp32 tensor as for every data module here; ``render(config)`` returns the same tensor
resident on the GPU.  The other ``dataset_type`` values of the reference are not used by the dimension-estimation configs.
"""
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import _lib
from . import utils

SLAB_IMAGES = 1 << 16          # images rendered per launch (256 MB of fp32 pixels at 32 x 32)


def transplanted_stream(rng):
    """A ``numpy.random.RandomState`` that continues the stream of ``rng`` (a ``random.Random``): its ``random_sample(n)`` equals
    the next n values of ``rng.random()``.  ``rng`` itself is not advanced."""
    version, state, _ = rng.getstate()
    if version != 3:
        raise RuntimeError(f"random.Random state version {version}: the Mersenne-Twister layout this transplant knows is 3")
    rs = np.random.RandomState()
    rs.set_state(('MT19937', np.array(state[:-1], dtype=np.uint32), state[-1]))
    return rs


def get_the_squares(seed, num_squares, square_range, img_size, rng=None):
    """[x, y, side] per square exactly as the reference draws them (:85-96); (x, y) is the pixel the square is centred on."""
    rng = rng or random.Random()
    rng.seed(seed)
    squares_info = []
    for _ in range(num_squares):
        side = rng.choice(square_range)
        start = (side + 1) // 2
        finish = img_size - (side + 1) // 2
        x = rng.choice(np.arange(start, finish))
        y = rng.choice(np.arange(start, finish))
        squares_info.append([int(x), int(y), int(side)])
    return squares_info


def square_rects(squares_info):
    """(row0, col0, side) of every square: the pixels the reference's ``paint_the_square`` touches (:118-123)."""
    info = np.asarray(squares_info, dtype=np.int64).reshape(-1, 3)
    off = (info[:, 2] + 1) // 2 - 1
    return np.stack([info[:, 0] - off, info[:, 1] - off, info[:, 2]], axis=1)


def get_the_gaussian_centers(seed, num_gaussians, std_range, img_size, rng=None):
    """[row, column] per blob, drawn without replacement exactly as the reference does (:129-140)."""
    rng = rng or random.Random()
    rng.seed(seed)
    pairs = [[i, j] for i in range(img_size) for j in range(img_size)]
    return rng.sample(pairs, k=num_gaussians)


def _plan(config):
    """(kind, table, draws -> per-image values on the host, K, S, N, stream) for ``config``."""
    d = config.data
    kind = d.get('dataset_type')
    S, N, seed = int(d.image_size), int(d.data_samples), config.seed
    rng = random.Random()
    if kind == 'FixedSquaresManifold':
        K = int(d.num_squares)
        table = square_rects(get_the_squares(seed, K, list(d.square_range), S, rng=rng))
        values = lambda u: u.astype(np.float32)                       # `img[i, j] += c` on an fp32 image rounds c first
    elif kind == 'FixedGaussiansManifold':
        K = int(d.num_gaussians)
        a, b = d.std_range[0], d.std_range[1]
        table = np.asarray(get_the_gaussian_centers(seed, K, list(d.std_range), S, rng=rng), dtype=np.int64)
        values = lambda u: a + (b - a) * u                            # random.uniform(a, b)
    else:
        raise NotImplementedError(f"data.dataset_type {kind!r}: the 'Synthetic' data module renders FixedSquaresManifold and "
                                  "FixedGaussiansManifold (the manifolds of the dimension-estimation configs)")
    return kind, table, values, K, S, N, transplanted_stream(rng)


def _device(config, device):
    dev = torch.device(device if device is not None else config.get('device', 'cuda'))
    if dev.type != 'cuda':
        if not torch.cuda.is_available():
            raise RuntimeError("the 'Synthetic' data module renders its images on the MI355X; no GPU is visible "
                               "(id-diff_amd has no CPU path)")
        dev = torch.device('cuda')
    return dev


def _slabs(config, device=None, slab=SLAB_IMAGES):
    """Yields (lo, hi, images [hi - lo, S, S] on the GPU) over the data set, in order."""
    kind, table, values, K, S, N, stream = _plan(config)
    dev = _device(config, device)
    fn = _lib.render_squares if kind == 'FixedSquaresManifold' else _lib.render_gaussians
    slab = max(1, min(int(slab), (2 ** 31 - 1) // (S * S)))
    for lo in range(0, N, slab):
        hi = min(N, lo + slab)
        u = stream.random_sample((hi - lo, K))                        # image-major, k inside: the reference's call order
        yield lo, hi, fn(torch.from_numpy(values(u)).to(dev), table, S)


def render(config, device=None, slab=SLAB_IMAGES):
    """The whole data set as one [N, 1, S, S] fp32 tensor on the GPU (for callers that want it there)."""
    S, N = int(config.data.image_size), int(config.data.data_samples)
    out = None
    for lo, hi, img in _slabs(config, device, slab):
        if lo == 0 and hi == N:
            return img.view(N, 1, S, S)
        if out is None:
            out = torch.empty(N, 1, S, S, device=img.device, dtype=torch.float32)
        out[lo:hi, 0] = img
    return out if out is not None else torch.empty(0, 1, S, S, device=_device(config, device))


class SyntheticDataset(Dataset):
    def __init__(self, config):
        super().__init__()
        self.return_labels = config.data.get('return_labels', False)
        self.data, self.labels = self.create_dataset(config)

    dataset_type = None

    def create_dataset(self, config):
        if config.data.get('dataset_type') != self.dataset_type:
            raise NotImplementedError(f"{type(self).__name__} renders data.dataset_type = {self.dataset_type!r}, the config "
                                      f"asks for {config.data.get('dataset_type')!r}")
        S, N = int(config.data.image_size), int(config.data.data_samples)
        data = torch.empty(N, 1, S, S, dtype=torch.float32)
        for lo, hi, img in _slabs(config):
            data[lo:hi, 0] = img.cpu()
        return data, []

    def __getitem__(self, index):
        if self.return_labels:
            return self.data[index], self.labels[index]
        return self.data[index]

    def __len__(self):
        return len(self.data)


class FixedSquaresManifold(SyntheticDataset):
    dataset_type = 'FixedSquaresManifold'
    get_the_squares = staticmethod(get_the_squares)


class FixedGaussiansManifold(SyntheticDataset):
    dataset_type = 'FixedGaussiansManifold'
    get_the_gaussian_centers = staticmethod(get_the_gaussian_centers)


_DATASETS = {c.dataset_type: c for c in (FixedSquaresManifold, FixedGaussiansManifold)}


@utils.register_lightning_datamodule(name='Synthetic')
class SyntheticDataModule(utils.SplitDataModule):
    def make_dataset(self):
        kind = self.config.data.get('dataset_type')
        if kind not in _DATASETS:
            raise NotImplementedError(f"data.dataset_type {kind!r}: the 'Synthetic' data module renders "
                                      f"{' and '.join(_DATASETS)} (the manifolds of the dimension-estimation configs)")
        return _DATASETS[kind](self.config)
