"""Fixed-squares image manifold with K = 20 squares (the paper's 20.py differs from 10.py in num_squares / log_name only)."""
import importlib

_ten = importlib.import_module(__name__.rsplit('.', 1)[0] + '.10')


def get_config():
    return _ten.get_config(num_squares=20, batch_size=128)
