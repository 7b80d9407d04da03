"""Fixed-Gaussians image manifold, K = 10 blobs on 32 x 32 (the ``ddpm`` score model on the 'Synthetic' data module,
``FixedGaussiansManifold``): K Gaussian bumps at fixed centres whose standard deviations are uniform in [1, 5], each
image scaled to [0, 1] -- a curved K-dimensional manifold.  Key names and values of the paper's
``image_data/gaussian_blobs/10.py`` (which asks for 5,000 images, 20.py too, 100.py for 50,000)."""
import importlib

from ......configs.default import get_default_configs
from ......configs.config_dict import ConfigDict

_squares = importlib.import_module(__name__.rsplit('.', 2)[0] + '.squares.10')


def get_config(num_gaussians=10, data_samples=5000, batch_size=128, val_batch_size=256, eval_batch_size=128, ema_rate=0.999):
    config = get_default_configs()
    config.logging = ConfigDict(log_path='logs/blobs', log_name=str(num_gaussians), top_k=5, every_n_epochs=1000,
                                svd_frequency=50, save_svd=False, svd_points=5)
    training = config.training
    training.batch_size = batch_size
    training.sde = 'vesde'
    training.continuous = True
    training.likelihood_weighting = False
    training.reduce_mean = True
    config.validation.batch_size = val_batch_size
    config.eval.batch_size = eval_batch_size
    config.data = ConfigDict(datamodule='Synthetic', dataset_type='FixedGaussiansManifold', create_dataset=False,
                             split=[0.8, 0.1, 0.1], data_samples=data_samples, image_size=32, effective_image_size=32,
                             centered=False, use_data_mean=False, num_gaussians=num_gaussians, std_range=[1, 5], mixtures=4,
                             return_labels=False, return_mixtures=False, shape=[1, 32, 32], num_channels=1)
    config.model = _squares.ddpm_32(ema_rate=ema_rate)
    config.seed = 42
    return config
