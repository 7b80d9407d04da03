"""The 'Line' curve in R^100 (line/config.py) with the score of its own train split in place of a trained network
(models/empirical_exact.py): the first acceptance model for "ID 1 on the line".  ``sigma_min`` is the kernel bandwidth of the
estimate: 0.2 is inside the range (0.05 to 0.4) in which the 8000 points of the split report 1 at every point tried; at 0.01 it is
below their spacing and the model warns."""
import importlib

_line = importlib.import_module(__name__.rsplit('.', 1)[0] + '.config')


def get_config():
    config = _line.get_config()
    config.logging.log_name = 'sine_line_empirical'
    config.model.name = 'empirical_exact'
    config.model.sigma_min = 0.2
    return config
