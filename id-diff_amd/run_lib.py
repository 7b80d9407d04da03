"""Dispatch layer (the two lines of /root/reference/run_lib.py:324-328 that are on the hot path, and ``train`` of :37-71 for the
fcn score network)."""
from . import dim_reduction


def get_manifold_dimension(config, name=None):
    dim_reduction.get_manifold_dimension(config, name)


def get_conditional_manifold_dimension(config, name=None):
    dim_reduction.get_conditional_manifold_dimension(config, name)


def train(config, log_path=None, checkpoint_path=None, n_iters=None, log_every=0, checkpoint_every=0, log_name=None, eval_every=0):
    """Train the fcn score network (train.py); resumes when ``checkpoint_path`` or ``config.model.checkpoint_path`` is set and writes
    ``<log_path>/<log_name>/checkpoints/last.ckpt``."""
    from . import train as _train
    return _train.train(config, log_path=log_path, checkpoint_path=checkpoint_path, n_iters=n_iters, log_every=log_every,
                        checkpoint_every=checkpoint_every, log_name=log_name, eval_every=eval_every)


def generate(config, checkpoint_path=None, num_samples=None, seed=None, log_path=None, log_name=None, sampler=None):
    """Draw samples from the config's score model (sampling.py) and write ``<log_path>/<log_name>/samples/samples.pkl``;
    ``sampler='ode'``: with the probability-flow ODE sampler."""
    from . import sampling
    return sampling.generate(config, checkpoint_path=checkpoint_path, num_samples=num_samples, seed=seed, log_path=log_path,
                             log_name=log_name, **({"sampler": sampler} if sampler is not None else {}))


def likelihood(config, checkpoint_path=None, num_samples=None, exact=False, seed=None, log_path=None, log_name=None):
    """Log-likelihood of the first points of the config's test split (likelihood.py); writes
    ``<log_path>/<log_name>/likelihood/likelihood.pkl``."""
    from . import likelihood as _likelihood
    return _likelihood.evaluate(config, checkpoint_path=checkpoint_path, num_samples=num_samples, exact=exact, seed=seed,
                                log_path=log_path, log_name=log_name)
