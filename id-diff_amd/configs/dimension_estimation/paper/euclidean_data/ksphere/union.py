"""Union of a 10-sphere and a 30-sphere in R^100 (the paper's union-of-spheres experiment, figures/paper/union_of_spheres_*.png of
the reference).  The reference ships no config for it: these are 10dim.py's values with two spheres of different dimension, and the
exact score of the mixture (models/ksphere_union_exact.py) in place of a trained network, so every point can be held to the
dimension of the sphere it lies on without a checkpoint."""
import importlib

_ten = importlib.import_module(__name__.rsplit('.', 1)[0] + '.10dim')


def get_config():
    config = _ten.get_config()
    config.logging.log_name = 'union-10-30-spheres'
    config.data.n_spheres = 2
    config.data.manifold_dim = [10, 30]
    config.model.name = 'ksphere_union_exact'
    return config
