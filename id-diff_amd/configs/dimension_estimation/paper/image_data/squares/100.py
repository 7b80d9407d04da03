"""Fixed-squares image manifold with K = 100 squares (the paper's 100.py differs from 10.py in num_squares / log_name and the
batch sizes (256)).  With seed 42 the hundred masks have rank 99: that, not 100, is the manifold's dimension."""
import importlib

_ten = importlib.import_module(__name__.rsplit('.', 1)[0] + '.10')


def get_config():
    return _ten.get_config(num_squares=100, batch_size=256)
