"""A curve in R^ambient_dim (drop-in for the reference's lightning_data_modules/LineDataset.py, data module 'Line'):
row = (sin x, sin 2x, ..., sin(ambient_dim x)) for 10^4 draws x = torch.rand (:28-29; the count is fixed there, whatever
``data.data_samples`` says), plus ``noise_std`` times a standard normal draw (:36, drawn even for noise_std = 0, which
keeps the torch stream where the reference leaves it).  The reference evaluates one sine per Python call (:30-35); here
the [10^4, ambient_dim] table is one vectorised fp32 expression on the host: the products (i + 1) x are the same fp32
values, the vectorised sine may differ from the scalar one in the last bit.  A few MB, made once: plumbing.
"""
import torch
from torch.utils.data import Dataset

from . import utils

N_POINTS = int(1e4)


class LineDataset(Dataset):
    def __init__(self, config):
        super().__init__()
        self.data = self.generate_data(config.data.get('ambient_dim', 100), config.data.get('noise_std', 0))

    def generate_data(self, ambient_dim, noise_std):
        x = torch.rand((N_POINTS,))
        freq = torch.arange(1, ambient_dim + 1, dtype=torch.float32)
        data = torch.sin(x[:, None] * freq[None, :])
        return data + noise_std * torch.randn_like(data)

    def __getitem__(self, index):
        return self.data[index]

    def __len__(self):
        return len(self.data)


@utils.register_lightning_datamodule(name='Line')
class LineDataModule(utils.SplitDataModule):
    def make_dataset(self):
        return LineDataset(self.config)
