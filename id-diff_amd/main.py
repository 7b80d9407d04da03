"""CLI drop-in for ``python main.py --config <cfg.py|cfg.pkl> --mode manifold_dimension [--checkpoint_path ...]``
(/root/reference/main.py:17-71; absl is not installable here, argparse accepts the same flags incl. ``--flag=value``).

``--mode train --n_iters N`` trains the ``fcn`` score network of a Euclidean config on one GPU (train.py) and writes
``<log_path>/<log_name>/checkpoints/last.ckpt``, which ``--mode manifold_dimension --checkpoint_path`` then reads;
``--checkpoint_path`` with ``--mode train`` resumes; ``--eval_every K`` also logs, every K steps and at the end, the norms of 1000 samples
drawn from the current weights and the mean estimated dimension of the checkpoint just written.

``--mode generate [--checkpoint_path ...] [--num_samples M] [--seed S]`` draws samples from the config's score model with the
predictor-corrector sampler (sampling.py) on one GPU, writes ``<log_path>/<log_name>/samples/samples.pkl`` and prints the minimum,
maximum and mean of the samples' norms.

``--mode generate --sampler ode`` draws them with the probability-flow ODE sampler (adaptive RK45, ode.py) instead; the pickle then
holds ``nfe``.  ``--mode likelihood [--checkpoint_path ...] [--num_samples M] [--exact] [--seed S]`` evaluates the log-likelihood of the
first M (default 1000) points of the config's test split under an ``fcn`` score network on one GPU (likelihood.py), writes
``<log_path>/<log_name>/likelihood/likelihood.pkl`` = {bpd, z, nfe, exact} and prints the mean, minimum and maximum.

Run it from the repo root as ``python id-diff_amd/main.py ...`` or, for several GPUs of one node,
``python -m torch.distributed.run --nproc-per-node N id-diff_amd/main.py ...``.

``--mode manifold_dimension`` with the config key ``dim_estimation.save_tangent = True`` (not in the reference; default False, one
GPU only) also writes ``<log_path>/<log_name>/svd/<log_name>_tangent.pkl`` = ``{'tangent': [...], 'dims': [...]}``: per point the
[D, d] float32 basis of its estimated tangent space, or None (``dim_reduction.get_manifold_dimension``).

``--mode manifold_dimension`` with the config key ``dim_estimation.method = 'jacobian'`` (or ``--dim_method jacobian``; not in the
reference; default 'sampling') writes the same pickle for the same points from the score Jacobian of an ``fcn`` network in closed form
instead of the score matrix of a perturbed cloud (jacobian.py): no sampling noise, one GPU, ``model.dropout == 0``.
``dim_estimation.method = 'flipd'`` (``--dim_method flipd``; models ``fcn`` and ``empirical_exact``, one GPU) writes
``<log_name>_flipd.pkl`` = ``{'flipd': [P] float64, 'dims': rint of it, 't' or 'sigma'}`` instead: FLIPD, the real-valued
D + sigma^2 (tr grad s + |s|^2), from one score divergence a point and no spectrum.
``dim_estimation.save_flipd = True`` (``--sampled_flipd``; method 'sampling', EVERY model, one GPU) also writes
``<log_name>_flipd_sampled.pkl`` = ``{'flipd', 'stderr', 'plain', 'beta', 'dims', 't', 'sigma'}`` (float64 [P]) beside the unchanged
spectra: FLIPD of the score smoothed over the sampling ball, read off the score rows already evaluated (stein.py).
"""
import argparse
import os
import sys

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import id_diff_amd  # noqa: F401
    __package__ = "id_diff_amd"

from id_diff_amd import parallel, run_lib  # noqa: E402
from id_diff_amd.configs.utils import read_config  # noqa: E402
from id_diff_amd.lightning_modules.checkpoint_io import load_config_pickle  # noqa: E402

_HOT_MODES = ('manifold_dimension', 'conditional_manifold_dimension')


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", required=True, help="Training configuration path (.py or .pkl).")
    ap.add_argument("--checkpoint_path", default=None)
    ap.add_argument("--data_path", default=None)
    ap.add_argument("--log_path", default="./")
    ap.add_argument("--mode", required=True)
    ap.add_argument("--eval_folder", default="eval")
    ap.add_argument("--debug", action="store_true")
    ap.add_argument("--log_name", default=None)
    ap.add_argument("--gpus", type=int, default=None,
                    help="(not in the reference) shard the data points over this many GPUs of the node: without a launcher "
                         "this process starts one fresh rank process per GPU itself; under torch.distributed.run it must "
                         "equal WORLD_SIZE")
    ap.add_argument("--allow_random_init", action="store_true",
                    help="run on freshly initialised weights when no checkpoint is given (timing / plumbing only)")
    ap.add_argument("--n_iters", type=float, default=None,
                    help="(--mode train) train until this many optimiser steps have been taken in total (the configs say 1e20)")
    ap.add_argument("--log_every", type=int, default=0, help="(--mode train) fetch and print the loss every this many steps")
    ap.add_argument("--checkpoint_every", type=int, default=0, help="(--mode train) also write last.ckpt every this many steps")
    ap.add_argument("--eval_every", type=int, default=0,
                    help="(--mode train) every this many steps, and at the end, sample from the current weights and log the norms and the "
                         "estimated dimension (0: never)")
    ap.add_argument("--num_samples", type=int, default=None, help="(--mode generate) number of samples to draw (default 1000)")
    ap.add_argument("--seed", type=int, default=None, help="(--mode generate) seed of the noise streams (default: config.seed)")
    ap.add_argument("--sampler", default=None, choices=("pc", "ode"),
                    help="(--mode generate) 'ode': draw the samples with the probability-flow ODE sampler instead of the config's")
    ap.add_argument("--exact", action="store_true",
                    help="(--mode likelihood) the exact divergence instead of Hutchinson's estimator")
    ap.add_argument("--dim_method", default=None, choices=("sampling", "jacobian", "flipd"),
                    help="(--mode manifold_dimension) sets the config key dim_estimation.method: 'sampling' (default), 'jacobian', the "
                         "score Jacobian of an fcn network in closed form, or 'flipd', one score divergence a point (both one GPU)")
    ap.add_argument("--sampled_flipd", action="store_true",
                    help="(--mode manifold_dimension) sets the config key dim_estimation.save_flipd: beside the spectra, the real-valued "
                         "FLIPD reading of every point from the score rows already evaluated, for any model (one GPU)")
    return ap.parse_args(argv)


def run_train(flags, config):
    from id_diff_amd import train as _train
    _train.check_scope(config)           # before anything touches the GPU: another network exits with the scope message
    if flags.gpus is not None and flags.gpus > 1:
        raise SystemExit("--mode train runs on one GPU: --gpus must be 1 (or left out)")
    if flags.n_iters is None:
        raise SystemExit("--mode train needs --n_iters (the reference's configs train for 1e20 steps)")
    if flags.n_iters < 0 or flags.log_every < 0 or flags.checkpoint_every < 0 or flags.eval_every < 0:
        raise SystemExit("--n_iters, --log_every, --checkpoint_every and --eval_every must not be negative")
    log_path = flags.log_path if flags.log_path != "./" or not config.logging.get("log_path") else config.logging.log_path
    return run_lib.train(config, log_path=log_path, checkpoint_path=config.model.get("checkpoint_path"), n_iters=flags.n_iters,
                         log_every=flags.log_every, checkpoint_every=flags.checkpoint_every, log_name=flags.log_name,
                         **({"eval_every": flags.eval_every} if flags.eval_every else {}))


def run_generate(flags, config):
    if flags.gpus is not None and flags.gpus > 1:
        raise SystemExit("--mode generate runs on one GPU: --gpus must be 1 (or left out)")
    if flags.num_samples is not None and flags.num_samples < 1:
        raise SystemExit("--num_samples must be positive")
    log_path = flags.log_path if flags.log_path != "./" or not config.logging.get("log_path") else config.logging.log_path
    return run_lib.generate(config, checkpoint_path=config.model.get("checkpoint_path"), num_samples=flags.num_samples, seed=flags.seed,
                            log_path=log_path, log_name=flags.log_name, **({"sampler": flags.sampler} if flags.sampler else {}))


def run_likelihood(flags, config):
    from id_diff_amd import likelihood as _likelihood
    _likelihood.check_config(config)     # before anything touches the GPU: another network exits with the scope message
    if flags.gpus is not None and flags.gpus > 1:
        raise SystemExit("--mode likelihood runs on one GPU: --gpus must be 1 (or left out)")
    if flags.num_samples is not None and flags.num_samples < 1:
        raise SystemExit("--num_samples must be positive")
    log_path = flags.log_path if flags.log_path != "./" or not config.logging.get("log_path") else config.logging.log_path
    return run_lib.likelihood(config, checkpoint_path=config.model.get("checkpoint_path"), num_samples=flags.num_samples,
                              exact=flags.exact, seed=flags.seed, log_path=log_path, log_name=flags.log_name)


def main(argv=None):
    flags = parse(argv)
    if flags.config.endswith('pkl'):
        config = load_config_pickle(flags.config)      # ml_collections pickles load without ml_collections
    elif flags.config.endswith('py'):
        config = read_config(flags.config)
    else:
        raise RuntimeError('Unknown config extension. Provide a path to .py or .pkl file.')
    if flags.checkpoint_path is not None:
        config.model.checkpoint_path = flags.checkpoint_path
    if flags.allow_random_init:
        config.model.allow_random_init = True
    if flags.dim_method is not None:
        config['dim_estimation.method'] = flags.dim_method
    if flags.sampled_flipd:
        config['dim_estimation.save_flipd'] = True
    if flags.mode == 'train':
        run_train(flags, config)
        return
    if flags.mode == 'generate':
        run_generate(flags, config)
        return
    if flags.mode == 'likelihood':
        run_likelihood(flags, config)
        return
    if flags.mode not in _HOT_MODES:
        raise SystemExit(f"mode {flags.mode!r} is outside the scope of id-diff_amd (the MI355X build covers "
                         f"{', '.join(_HOT_MODES)}, and train for the fcn score network); use the reference for "
                         "sampling / evaluation and for training any other network")
    if flags.gpus is not None:
        need_devices = not str(getattr(config, "device", "cuda")).startswith("cpu")     # the same answer in the launcher and in the ranks
        if flags.gpus > 1 and not parallel.launched():
            # become the launcher: nothing in this process has touched the GPU; fresh rank processes, never an exec
            rc = parallel.launch_local_ranks(os.path.abspath(__file__), list(sys.argv[1:] if argv is None else argv), flags.gpus,
                                             need_devices=need_devices)
            if rc:
                raise SystemExit(rc)
            return
        if parallel.launched():
            parallel.check_world(flags.gpus, int(os.environ["WORLD_SIZE"]), need_devices=need_devices)
    rank, world, local_rank = parallel.init_from_env()
    if world > 1:
        config.device = f"cuda:{parallel.device_ordinal(local_rank)}"
    if flags.mode == 'manifold_dimension':
        run_lib.get_manifold_dimension(config, name=flags.log_name)
    else:
        run_lib.get_conditional_manifold_dimension(config, name=flags.log_name)


if __name__ == "__main__":
    main()
