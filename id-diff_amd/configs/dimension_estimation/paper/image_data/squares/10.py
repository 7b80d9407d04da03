"""Fixed-squares image manifold, K = 10 squares on 32 x 32 (the ``ddpm`` score model on the 'Synthetic' data module,
``FixedSquaresManifold``): an image is sum_k c_k 1[square k] with c uniform in [0, 1)^K, so the manifold is a K-cube
in a K-dimensional linear subspace (ID = rank of the squares' masks).  Key names and values of the paper's
``image_data/squares/10.py``; its 20.py and 100.py differ in the arguments of ``get_config`` only."""
from ......configs.default import get_default_configs
from ......configs.config_dict import ConfigDict


def ddpm_32(ema_rate=0.999):
    """The 32 x 32 x 1 ``ddpm`` model group shared by the squares and the blobs configs."""
    return ConfigDict(
        checkpoint_path=None, sigma_min=0.01, sigma_max=50, num_scales=1000, beta_min=0.1, beta_max=20., dropout=0.1,
        embedding_type='fourier', name='ddpm', input_channels=1, output_channels=1, scale_by_sigma=True, ema_rate=ema_rate,
        normalization='GroupNorm', nonlinearity='swish', nf=128, ch_mult=(1, 2, 2, 2), num_res_blocks=4,
        attn_resolutions=(16,), resamp_with_conv=True, conditional=True, fir=True, fir_kernel=[1, 3, 3, 1],
        skip_rescale=True, resblock_type='biggan', progressive='none', progressive_input='residual',
        progressive_combine='sum', attention_type='ddpm', init_scale=0., fourier_scale=16, conv_size=3)


def get_config(num_squares=10, batch_size=128):
    config = get_default_configs()
    config.logging = ConfigDict(log_path='logs/squares', log_name=str(num_squares), top_k=5, every_n_epochs=1000,
                                svd_frequency=50, save_svd=False, svd_points=5)
    training = config.training
    training.batch_size = batch_size
    training.sde = 'vesde'
    training.continuous = True
    training.likelihood_weighting = False
    training.reduce_mean = True
    config.validation.batch_size = batch_size
    config.eval.batch_size = batch_size
    config.data = ConfigDict(datamodule='Synthetic', dataset_type='FixedSquaresManifold', create_dataset=False,
                             split=[0.8, 0.1, 0.1], data_samples=500000, image_size=32, effective_image_size=32,
                             centered=False, use_data_mean=False, num_squares=num_squares, square_range=[3, 5], mixtures=4,
                             return_labels=False, return_mixtures=False, shape=[1, 32, 32], num_channels=1)
    config.model = ddpm_32()
    config.seed = 42
    return config
