"""Fixed-Gaussians image manifold with K = 100 blobs (the paper's 100.py: 50,000 images, batches of 256, EMA 0.9999)."""
import importlib

_ten = importlib.import_module(__name__.rsplit('.', 1)[0] + '.10')


def get_config():
    return _ten.get_config(num_gaussians=100, data_samples=50000, batch_size=256, val_batch_size=256, eval_batch_size=256,
                           ema_rate=0.9999)
