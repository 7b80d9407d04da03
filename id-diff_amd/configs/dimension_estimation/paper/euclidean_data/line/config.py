"""A curve in R^100 with the fcn score model: x -> (sin x, sin 2x, ..., sin 100x), x uniform in [0, 1) -- a manifold of
dimension 1 (the 'Line' data module).  Key names and values of the paper's ``euclidean_data/line/config.py``."""
from ......configs.default import get_default_configs
from ......configs.config_dict import ConfigDict


def get_config():
    config = get_default_configs()
    config.logging = ConfigDict(log_path='logs/line', log_name='sine_line', top_k=5, every_n_epochs=1000,
                                svd_frequency=50, save_svd=False, svd_points=5)
    training = config.training
    training.batch_size = 500
    training.sde = 'vesde'
    training.continuous = True
    training.likelihood_weighting = True
    config.validation.batch_size = 500
    config.data = ConfigDict(datamodule='Line', create_dataset=False, split=[0.8, 0.1, 0.1], data_samples=50000,
                             use_data_mean=False, ambient_dim=100, noise_std=0, dim=100, num_channels=0, shape=[100])
    config.model = ConfigDict(checkpoint_path=None, sigma_max=4, sigma_min=1e-2, name='fcn', state_size=100,
                              hidden_layers=5, hidden_nodes=2048, dropout=0.0, scale_by_sigma=False, num_scales=1000,
                              ema_rate=0.9999)
    config.seed = 42
    return config
