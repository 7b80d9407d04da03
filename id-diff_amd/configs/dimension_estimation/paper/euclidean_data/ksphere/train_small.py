"""A unit 2-sphere in R^8 with a small fcn: the configuration the end-to-end training test runs (train on the GPU, then
``manifold_dimension`` on the written checkpoint must read 2 at every point).  Not in the reference: its k-sphere configs are the
paper's 10- and 50-sphere in R^100 with five hidden layers of 2048, hours of training; this one learns the radial normal in 8000
steps of batch 256."""
from ......configs.default import get_default_configs
from ......configs.config_dict import ConfigDict


def get_config():
    config = get_default_configs()
    config.logging = ConfigDict(log_path='logs/ksphere/', log_name='2-sphere-small', top_k=5, svd_frequency=50, save_svd=False,
                                svd_points=8)
    training = config.training
    training.batch_size = 256
    training.sde = 'vesde'
    training.continuous = True
    training.likelihood_weighting = True
    training.reduce_mean = False
    config.validation.batch_size = 256
    config.data = ConfigDict(datamodule='KSphere', create_dataset=False, split=[0.8, 0.1, 0.1], data_samples=8192,
                             use_data_mean=False, n_spheres=1, ambient_dim=8, manifold_dim=2, noise_std=0.0,
                             embedding_type='random_isometry', dim=8, num_channels=0, shape=[8])
    config.model = ConfigDict(checkpoint_path=None, sigma_max=2.0, sigma_min=0.1, name='fcn', state_size=8, hidden_layers=2,
                              hidden_nodes=128, dropout=0.0, scale_by_sigma=False, num_scales=1000, ema_rate=0.9999)
    config.optim = ConfigDict(weight_decay=0.0, optimizer='Adam', lr=1e-3, beta1=0.9, eps=1e-8, warmup=100, grad_clip=1.0)
    return config
