"""Fixed-Gaussians image manifold with K = 20 blobs (the paper's 20.py differs from 10.py in num_gaussians / log_name and
the validation / evaluation batch sizes)."""
import importlib

_ten = importlib.import_module(__name__.rsplit('.', 1)[0] + '.10')


def get_config():
    return _ten.get_config(num_gaussians=20, val_batch_size=128, eval_batch_size=256)
