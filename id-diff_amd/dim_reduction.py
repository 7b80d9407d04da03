"""ID driver: score matrix -> centred spectrum, per data point (drop-in for /root/reference/dim_reduction.py).

``get_manifold_dimension(config, name=None, return_svd=False)`` keeps the reference's contract (:116-215):
same config keys, same number of processed points (``idx + 1 >= num_datapoints`` stops one short, :159-164),
same per-point row count ``M = (num_batches - 1) * B + extra`` with ``ambient_dim = prod(x.shape[1:])`` of ONE
un-batched sample (:166-171), same output ``{'singular_values': [[...], ...]}`` returned or pickled to
``<log_path>/<log_name>/svd/<name>.pkl`` (:206-211).

What is different, by design for MI355X:
* nothing leaves the GPU inside the loop: the reference moves every score batch to the host (:183) and runs a
  full CPU SVD with U and V (:197); here rows are written straight into the device-resident S [M, D] and the
  spectrum comes from the fp64 Gram -> tridiagonal -> bisection kernels (csrc/spectrum.hip);
* rows that the reference computes and throws away (the tail of the last batch, :185-188) are not computed;
* score evaluations run ``inflight`` rows at a time (default: as many of the point's rows as fit the
  ``dim_estimation.inflight_rows`` budget) instead of B -- every row is an independent sample, GroupNorm is
  per-sample and the model is in eval mode, so the batch boundary is not observable;
* noise comes from an in-kernel Philox stream keyed by ``seed + 1000003 * (point_index + 1)`` and indexed by the
  element's position in the point's noise matrix (csrc/rng.hip), fused with the perturbation, so results depend
  neither on how points are distributed over GPUs nor on the launch-set size; points are sharded round-robin over the ranks of the process group and
  the spectra are combined by one all-gather (parallel.py).
"""
import contextlib
import dataclasses
import math
import os
import pickle
from pathlib import Path

import torch

from . import _lib, parallel
from .lightning_data_modules.utils import create_lightning_datamodule
from .lightning_modules.utils import create_lightning_module
from .models import utils as mutils
from .plot_utils import estimate_dim


def batching(sample_shape, batchsize):
    """(num_batches, extra_in_last_batch, rows_in_S) of dim_reduction.py:166-171."""
    ambient_dim = math.prod(sample_shape[1:])
    num_batches = (ambient_dim // batchsize + 1) * 4
    extra = ambient_dim - (ambient_dim // batchsize) * batchsize
    return num_batches, extra, (num_batches - 1) * batchsize + extra


def _num_datapoints(config):
    # dotted hasattr, as the reference does (dim_reduction.py:144-147)
    if hasattr(config, 'dim_estimation.num_datapoints'):
        return config.dim_estimation.num_datapoints
    elif hasattr(config, 'logging.svd_points'):
        return config.logging.svd_points
    raise NameError("num_datapoints: neither dim_estimation.num_datapoints nor logging.svd_points is set")


class ScoreMatrixBuilder:
    """Produces S for one point with all work on the device."""

    def __init__(self, score_fn, sde, sampling_eps, device, inflight_rows=None, concurrent_sets=None):
        self.score_fn, self.sde, self.eps, self.device = score_fn, sde, sampling_eps, device
        self.inflight_rows = inflight_rows
        # OPT-IN (IDIFF_CONCURRENT_SETS=2 / concurrent_sets=2): consecutive launch sets of a point go to two worker streams,
        # so the tail of every launch and the small-map layers of one forward fill up with the other forward's work
        # (two 2240-row NCSN++ forwards 476.6 -> 468 ms in round 3, scripts/two_stream_probe.py).  Same kernels, same bits.  Off by
        # default -- and since the convolutions moved to the one-workgroup-per-CU pair kernel it LOSES: round 5 re-measured
        # bench.py --concurrent-sets 2 at 10.4-14.2k evals/s (erratic: how the two streams' launches interleave) against 16.1k in
        # sequence (profiles/HISTORY_r05.md).  Kept for the parity test of the stream logic only.
        if concurrent_sets is None:
            concurrent_sets = int(os.environ.get("IDIFF_CONCURRENT_SETS", "1"))
        self.concurrent_sets = max(1, int(concurrent_sets))
        self._workers = None
        self._warmed = False

    def rows_per_launch(self, rows, sample_numel, vector=False):
        if self.inflight_rows:
            return max(1, min(rows, int(self.inflight_rows)))
        # default: all rows of a vector point (the k-sphere MLPs); for images 2240 rows of 32x32x3 (measured best of
        # 1120 / 2240 / 4480 on the nf=128 NCSN++: whole numbers of workgroups per CU at every level) scaled by the sample size
        if vector and rows <= 65536:
            return rows
        return min(rows, max(128, (2240 * 3072) // sample_numel))

    def build(self, x, batchsize, t=None, noise=None, generator=None, seed=None, row_range=None, safe=False):
        """x: one sample on the device; returns S [M, D] fp32 (rows in the reference's order), or only the rows
        ``row_range = (lo, hi)`` of it (row-sharded pipeline: with ``seed`` the draws of a row do not depend on who
        computes it).

        ``safe=True``: the same point with every contraction on the range-unlimited route (fp32-contraction Winograd, six-product
        GEMMs: ``IDIFF_NO_WINO43H`` / ``IDIFF_NO_PAIRS`` for this host thread's launches only).  The drivers call it ONCE for a
        point whose score matrix came back non-finite from the default fp16-pair route, before they give up on the point: the
        reference evaluates any checkpoint in fp32 (models/layerspp.py:242-274), so a range limit of ours must not turn into an error
        of the user's.  Position-keyed noise (``seed`` / ``noise``) makes the re-run the same matrix.

        Noise: ``noise`` (explicit draws, for parity tests) > ``seed`` (in-kernel Philox stream, the default of the
        drivers: independent of the launch-set size; for D % 4 != 0 a torch generator keyed by the seed, same property) >
        ``generator`` (torch.randn, consumed launch set by launch set: the caller owns reproducibility)."""
        if safe:
            with _lib.thread_option("IDIFF_NO_WINO43H", 1), _lib.thread_option("IDIFF_NO_PAIRS", 1):
                return self.build(x, batchsize, t=t, noise=noise, generator=generator, seed=seed, row_range=row_range)
        _, _, rows = batching(tuple(x.shape), batchsize)
        D = x.numel()
        t = self.eps if t is None else t
        r_lo, r_hi = (0, rows) if row_range is None else row_range
        if row_range is not None and noise is None and seed is None:
            raise RuntimeError("a row range needs position-keyed noise: pass `seed` or explicit `noise`")
        if noise is None and seed is not None and D % 4:
            noise = self._seeded_noise(rows, D, seed)
        S = torch.empty(r_hi - r_lo, D, device=self.device, dtype=torch.float32)
        step = self.rows_per_launch(rows, D, vector=x.ndim == 1)
        xf = x.reshape(-1).contiguous()
        workers, cur = (), None
        if (self.concurrent_sets > 1 and r_hi - r_lo > step and torch.device(self.device).type == "cuda" and self._warmed
                and (noise is not None or seed is not None)):      # torch-generator draws stay in sequential order
            # the launch sets of the point dealt round-robin to ``concurrent_sets`` worker streams; the caller's stream waits
            # for all of them before S is handed back
            if self._workers is None or len(self._workers) != self.concurrent_sets:
                self._workers = [torch.cuda.Stream(device=self.device) for _ in range(self.concurrent_sets)]
            workers, cur = self._workers, torch.cuda.current_stream()
            for w in workers:
                w.wait_stream(cur)
        self._warmed = True     # the first point runs on one stream: filter banks and constants are made lazily, once
        for i, lo in enumerate(range(r_lo, r_hi, step)):
            n = min(step, r_hi - lo)
            with torch.cuda.stream(workers[i % len(workers)]) if workers else contextlib.nullcontext():
                batch, vec_t = self._perturbed([xf], t, lo, n, noise=None if noise is None else [noise],
                                               seeds=None if seed is None else [seed], generator=generator)
                self._score_into(S[lo - r_lo:lo - r_lo + n], batch.view(n, *x.shape), vec_t)
        for w in workers:
            cur.wait_stream(w)
        return S

    def _seeded_noise(self, rows, D, seed):
        """The in-kernel Philox stream writes 16-byte groups (D % 4 == 0).  Other widths draw the point's WHOLE noise matrix
        [rows, D] from a generator keyed by the point seed and slice it: still a function of (seed, row, column) only, whatever
        the launch-set size, the row range or the number of ranks."""
        return torch.randn(rows, D, device=self.device, dtype=torch.float32,
                           generator=torch.Generator(device=self.device).manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF))

    def _perturbed(self, xfs, t, lo, n, noise=None, seeds=None, generator=None):
        """Rows [lo, lo + n) of the noise matrices of the P points ``xfs`` (flat, [D] each), perturbed at time ``t``:
        (batch [P, n, D], vec_t [n]); the level's std and mean coefficient are computed once for all P.  One noise source, in
        ``build``'s order of precedence: ``noise`` (per point its whole matrix), ``seeds`` (per point, in-kernel Philox: D % 4 == 0),
        ``generator``."""
        P, D = len(xfs), xfs[0].numel()
        vec_t = torch.full((n,), float(t), device=self.device, dtype=torch.float32)
        mean_unit, std = self.sde.marginal_prob(torch.ones((), device=self.device), vec_t)
        coeff = None if mean_unit.ndim == 0 else mean_unit.reshape(-1).contiguous()
        std = std.contiguous()
        batch = torch.empty(P, n, D, device=self.device, dtype=torch.float32)
        for i, xf in enumerate(xfs):
            if noise is None and seeds is not None:
                _lib.perturb_randn(xf, std, coeff, batch[i], n, D, lo, seeds[i])
            else:
                if noise is not None:
                    z = noise[i][lo:lo + n].reshape(n, D).contiguous()
                else:
                    z = torch.randn(n, D, device=self.device, dtype=torch.float32, generator=generator)
                _lib.perturb(xf, z, std, coeff, batch[i], n, D)
        return batch, vec_t

    def _score_into(self, rows, batch, vec_t):
        """Scores of ``batch`` into ``rows`` (a row block of S): written there by the network's last kernel when the model takes an
        output buffer (the image models), copied otherwise."""
        if getattr(self.score_fn, "accepts_out", False):
            self.score_fn(batch, vec_t, out=rows)
        else:
            rows.copy_(self.score_fn(batch, vec_t).reshape(rows.shape))


@dataclasses.dataclass(slots=True)
class _Pending:
    """A spectrum that has been launched.  ``S`` is held until the failure flag has been read -- a flagged spectrum is solved again
    from it -- and released then (None marks an entry that ``_reap`` is done with)."""
    sv: torch.Tensor
    S: torch.Tensor
    flag: torch.Tensor        # pinned host bool[1]: NaN in sv
    done: object              # event behind the flag's copy
    rebuild: object           # callable -> this point's S again on the safe route, or None


def _rank0_log():
    """``log`` for the eigensolver's fallback walk: the warning on rank 0, silence on the others."""
    return None if parallel.rank_world()[0] == 0 else (lambda msg: None)


class SpectrumPipeline:
    """Runs the spectrum of point p on a side HIP stream while the score evaluations of point p+1 fill the
    main stream: the tridiagonalisation is a chain of ~2D short bandwidth-bound launches that leaves most CUs
    idle, the convolutions are MFMA-bound -- the two overlap almost for free.

    The spectrum of a point is ENQUEUED one ``submit`` late, i.e. after the next point's score evaluations have been
    queued: its ~6000 launches do not fit the side stream's hardware queue, so the enqueueing host thread blocks until
    the spectrum is nearly done -- and while it did that right after point p, nothing of point p+1 had been queued yet and
    the main stream sat idle for the length of a spectrum at every point boundary (72 ms gaps in the rocprofv3 trace)."""

    def __init__(self, device, overlap=True):
        self.device = device
        # A stream of another priority class gets a hardware queue of its own.  A default-priority stream shares the
        # runtime's small pool of queues with every other stream of the process: once an RCCL communicator exists (its
        # streams were made first) this one landed on the main stream's queue and the spectrum ran BETWEEN the score
        # evaluations instead of beside them (+35 ms per point under torch.distributed.run, same kernels, same durations).
        prio = int(os.environ.get("IDIFF_SIDE_STREAM_PRIORITY", "-1"))
        self.side = torch.cuda.Stream(device=device, priority=prio) if overlap else None
        self.pending = []         # _Pending, in submit order
        self.deferred = None      # (S, ready event, rebuild) of the last submitted point, not yet enqueued
        self.resolved = 0         # spectra that needed a fallback form of the eigensolver (fail-soft, see _reap)
        self.rebuilt = 0          # points whose score matrix was non-finite on the default route and was built again on the safe one

    def _launch(self, S, ready, rebuild=None):
        stream = self.side if self.side is not None else torch.cuda.current_stream()
        if self.side is not None:
            self.side.wait_event(ready)                  # S is complete on the producing stream
        with torch.cuda.stream(stream):
            sv = _lib.spectrum(S, full=True)
            # the eigensolver reports trouble as NaN; one flag per spectrum goes to pinned host memory so that the check
            # costs no synchronisation: it is read once the event behind the copy has completed
            flag = torch.empty(1, dtype=torch.bool, pin_memory=True)
            flag.copy_(torch.isnan(sv).any().reshape(1), non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        if self.side is not None:
            S.record_stream(self.side)                   # keep S alive until the side stream is done with it
        self.pending.append(_Pending(sv, S, flag, done, rebuild))

    def _reap(self, block):
        """Reads the failure flags of the spectra that have completed (all of them with ``block``).  A flagged spectrum is
        solved again from its S -- still held for exactly this -- with the eigensolver's fallback forms
        (``_lib.resolve_failed_spectrum``: wavefront chase, then the one-stage sweep) in this process; only a matrix
        that defeats all three, or holds non-finite scores, raises."""
        for entry in self.pending:
            if entry.S is None:
                continue
            if block:
                entry.done.synchronize()
            elif not entry.done.query():
                break                                    # in stream order: later ones are not done either
            if bool(entry.flag[0]):
                stream = self.side if self.side is not None else torch.cuda.current_stream()
                S = entry.S
                if entry.rebuild is not None and not bool(torch.isfinite(S).all()):
                    # not the eigensolver: the score matrix itself is non-finite.  One re-run of the point on the range-unlimited
                    # route (ScoreMatrixBuilder.build(safe=True)), on the caller's stream like every build, before that becomes an error
                    warn_non_finite_point()
                    S = entry.rebuild()
                    self.rebuilt += 1
                    torch.cuda.current_stream().synchronize()   # the rare path: S (and any filter bank packed for it) is complete
                    with torch.cuda.stream(stream):
                        entry.sv = _lib.spectrum(S, full=True)
                with torch.cuda.stream(stream):
                    if bool(torch.isnan(entry.sv).any()):
                        entry.sv = _lib.resolve_failed_spectrum(S, full=True, log=_rank0_log())
                        self.resolved += 1
            entry.S = entry.rebuild = None

    def submit(self, S, rebuild=None):
        """``rebuild``: a callable returning this point's S again on the safe route (see ``_reap``); without it a non-finite S raises."""
        self._reap(block=False)
        if self.side is None:
            self._launch(S, None, rebuild)
            return
        ready = torch.cuda.Event()
        ready.record()
        previous, self.deferred = self.deferred, (S, ready, rebuild)
        if previous is not None:
            self._launch(*previous)

    def results(self):
        """All submitted spectra, in order, checked; joins the side stream into the current one."""
        if self.side is not None and self.deferred is not None:
            self._launch(*self.deferred)
            self.deferred = None
        self._reap(block=True)
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)
        out, self.pending = [e.sv for e in self.pending], []
        return out


def warn_non_finite_point():
    import warnings
    if parallel.rank_world()[0] == 0:
        warnings.warn("id-diff_amd: a point's score matrix came back non-finite from the default (fp16-pair) route; building the "
                      "point again with every contraction on the fp32 route (IDIFF_NO_WINO43H / IDIFF_NO_PAIRS for this re-run)")


def row_sharded_spectrum(S_local, total_rows, ops=None, block_rows=None, rebuild=None):
    """Singular values (descending, fp32, [D]) of the column-centred [total_rows, D] matrix whose rows are spread over
    the ranks of the default process group (this rank holds ``S_local``); every rank returns the full spectrum.

    SURVEY.md 8(f) rank 2 / DESIGN.md 6: two collectives -- all-reduce of the fp64 column sums [D], all-reduce of the
    fp64 centred Gram [D, D] -- then the eigensolve, run redundantly on every rank (cheaper than shipping the result).
    The Gram (75 MB at D = 3072, 1.2 GB at D = 12288: bandwidth-bound on the xGMI ring) goes in blocks of ``block_rows``
    rows of its upper triangle, each packed from its first diagonal tile onwards (0.6 GB in total at D = 12288): the
    all-reduce of block b is asynchronous and runs while the matrix cores compute block b + 1; the lower triangle is
    mirrored once at the end.  With one rank this is the same arithmetic as
    ``_lib.spectrum``.  ``ops`` = (column_sums, gram_rows, symmetrize, sym_eigvals) defaults to the HIP stages; the CPU
    process-group test injects plain-torch stand-ins to check the reduction logic without a GPU.  ``rebuild``: a callable that returns
    this rank's rows again on the safe route; used once, on every rank, when any rank's Gram comes out non-finite."""
    col_sums, gram_rows, symmetrize, eigvals = ops if ops is not None else (
        _lib.column_sums, _lib.centered_gram_rows, _lib.symmetrize_upper, _lib.sym_eigvals)
    D = S_local.shape[1]
    if total_rows < D:
        raise RuntimeError(f"row_sharded_spectrum: needs total_rows >= D (got {total_rows} x {D})")
    sums = parallel.all_reduce_sum(col_sums(S_local))
    mean = sums / float(total_rows)
    if block_rows is None:
        block_rows = max(64, ((D // 8 + 63) // 64) * 64)            # ~8 blocks: enough to hide all but the first Gram block
    grouped = parallel.is_grouped()

    def reduced_gram():
        G = torch.zeros(D, D, dtype=torch.float64, device=S_local.device)
        pending = []
        for r0 in range(0, D, block_rows):
            r1 = min(D, r0 + block_rows)
            gram_rows(S_local, mean, G, r0, r1)
            if not grouped:
                continue
            # only the columns from the block's first diagonal tile onwards carry data (the rest is mirrored afterwards):
            # reduce that trapezoid, packed, not whole rows -- about half the bytes of a bandwidth-bound collective
            c0 = (r0 // 128) * 128
            staging = G[r0:r1, c0:].contiguous()
            pending.append((parallel.all_reduce_sum_async(staging), staging, r0, r1, c0))
        for work, staging, r0, r1, c0 in pending:
            parallel.wait(work)
            G[r0:r1, c0:].copy_(staging)
        return symmetrize(G)

    def any_rank(flag):
        """A failure flag (bool tensor), reduced (MAX) over the ranks so that EVERY rank takes the same branch even when only one
        device's eigensolve failed (a stalled chase is a property of one device, not of G)."""
        flag = flag.to(torch.int32).reshape(1)
        if grouped:
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)
        return bool(flag.item())

    eig = eigvals(reduced_gram())                                     # the eigensolver overwrites its input
    if ops is None and any_rank(torch.isnan(eig).any()):
        # fail soft: the policy of SpectrumPipeline._reap, every branch taken by all ranks together
        if rebuild is not None and any_rank(~torch.isfinite(S_local).all()):
            warn_non_finite_point()
            return row_sharded_spectrum(rebuild(), total_rows, ops=ops, block_rows=block_rows, rebuild=None)
        # no copy of G was kept for this rare path (1.2 GB of fp64 at D = 12288 otherwise sat beside G on every call): it is built
        # again, and once more for every further form, since the solver overwrites it
        G = reduced_gram()
        if not bool(torch.isfinite(G).all()):
            raise RuntimeError("the Gram matrix holds non-finite values (NaN / inf score vectors): no spectrum exists")
        fresh = [G]
        eig = _lib.solve_with_fallbacks(lambda: eigvals(fresh.pop() if fresh else reduced_gram()), any_rank=any_rank, log=_rank0_log())
    return eig.clamp_min(0.0).sqrt().flip(0).to(torch.float32)


def checked_spectra(spectra):
    """Host copy of gathered spectra.  The eigensolver poisons its output with NaN instead of returning a wrong spectrum
    (band-reduction residual above tolerance, a stalled chase: include/idiff_hip.h, idiff_symtridiag_f64); this is where
    the values first reach the host, so this is where that turns into an exception."""
    host = spectra.cpu()
    if bool(torch.isnan(host).any()):
        raise RuntimeError("NaN singular values reached the host: a spectrum that did not come through SpectrumPipeline / "
                           "row_sharded_spectrum (which re-solve a failed eigensolve in-process) reported a failure")
    return host


def tangent_width(singular_values, ambient_dim, cap=_lib.TANGENT_MAX):
    """``(d, k)`` for one point, on the host: d its ID by the rule every driver uses (``estimate_dim``; -1 with fewer than three
    singular values) and k the width of the tangent basis to ask for -- d itself, or None where no basis is served: d < 1,
    d above ``cap`` (the widest basis idiff_sym_lowvecs_f64 computes) or d not below the ambient dimension."""
    d = estimate_dim(list(singular_values)) if len(singular_values) >= 3 else -1
    return d, (d if 1 <= d <= cap and d < ambient_dim else None)


def _tangent_refused(config, world):
    """return_tangent is a one-rank mode: bases have a different width at every point, and their exchange is not built."""
    if world > 1 or str(config.get('dim_estimation.shard', 'points')) == 'rows':
        raise NotImplementedError("return_tangent / dim_estimation.save_tangent needs a single rank and dim_estimation.shard = "
                                  f"'points' (got world size {world}, shard = {config.get('dim_estimation.shard', 'points')!r}): "
                                  "the exchange of variable-width bases between ranks is not implemented")


METHODS = ('sampling', 'jacobian', 'flipd')


def estimation_method(config, method=None):
    """'sampling' (the default: the score matrix of a perturbed cloud), 'jacobian' (jacobian.py: the score Jacobian of an fcn network in
    closed form) or 'flipd' (one score divergence a point: a real-valued reading, no spectrum); the argument wins over the config key
    ``dim_estimation.method``.  Anything else is a ValueError."""
    if method is None:
        method = config.get('dim_estimation.method', None)
    method = 'sampling' if method is None else str(method)
    if method not in METHODS:
        raise ValueError(f"dim_estimation.method = {method!r}: one of {METHODS}")
    return method


def _jacobian_refused(config, world):
    """method = 'jacobian' is a one-rank mode: a hundred D x D Jacobians are a fraction of a second of one GPU."""
    if world > 1 or str(config.get('dim_estimation.shard', 'points')) == 'rows':
        raise NotImplementedError("dim_estimation.method = 'jacobian' needs a single rank and dim_estimation.shard = 'points' (got world "
                                  f"size {world}, shard = {config.get('dim_estimation.shard', 'points')!r}): the Jacobian method has no "
                                  "score rows to shard and its points are not distributed over ranks")


FLIPD_MODELS = ('fcn', 'empirical_exact')


def _flipd_refused(config, world, return_svd, want_tangent):
    """method = 'flipd', before the GPU is touched: the models that have a divergence here, one rank, and nothing that needs a spectrum."""
    name = config.model.get('name')
    if name not in FLIPD_MODELS:
        raise NotImplementedError(f"dim_estimation.method = 'flipd' serves model.name in {FLIPD_MODELS}, not {name!r}: the trace of the "
                                  "score Jacobian needs a JVP or VJP of the network, which the image networks do not have here (and "
                                  "finite differences are not a substitute)")
    if name == 'fcn':
        from . import jacobian
        try:
            jacobian.check_config(config)
        except NotImplementedError as e:
            raise NotImplementedError(str(e).replace("the Jacobian method", "the FLIPD method")) from None
    if world > 1 or str(config.get('dim_estimation.shard', 'points')) == 'rows':
        raise NotImplementedError("dim_estimation.method = 'flipd' needs a single rank and dim_estimation.shard = 'points' (got world "
                                  f"size {world}, shard = {config.get('dim_estimation.shard', 'points')!r}): it has no score rows to "
                                  "shard and its points are not distributed over ranks")
    if return_svd or want_tangent:
        raise NotImplementedError("dim_estimation.method = 'flipd' has no spectrum and no tangent basis: return_svd, return_tangent and "
                                  "dim_estimation.save_tangent are not served (return_dims=True returns the rounded readings)")


def _points_by_flipd(config, pl_module, points, device, seed):
    """(flipd float64 numpy [P], what it was read at) of ``points``: an fcn network through ``jacobian.flipd`` at t = sampling_eps (exact
    unless ``dim_estimation.flipd_probes`` > 0), the empirical score through the kernel at sigma = model.sigma_min with a point that is
    a row of the cloud left out of its own softmax."""
    xs = torch.stack([x.reshape(-1) for x, _ in points]).to(device=device, dtype=torch.float32).contiguous()
    if config.model.get('name') == 'fcn':
        from . import jacobian
        n_probes = int(config.get('dim_estimation.flipd_probes', 0) or 0)
        t = pl_module.sampling_eps
        f = jacobian.flipd(pl_module, pl_module.sde, xs, t, exact=n_probes <= 0, n_probes=max(n_probes, 1), seed=seed)
        return f.cpu().numpy(), {'t': float(t)}
    cloud = pl_module.score_model.cloud.detach()
    sigma = float(config.model.sigma_min)
    same = (xs[:, None, :] == cloud[None, :, :]).all(dim=2)              # [P, N]: the driver's points are a handful
    exclude = torch.where(same.any(dim=1), same.int().argmax(dim=1), torch.full((len(points),), -1, device=device)).cpu()
    f, _ = _lib.empirical_flipd(xs, pl_module.score_model.packed(), torch.full((1,), sigma, device=device, dtype=torch.float32),
                                exclude=exclude)
    return f[:, 0].cpu().numpy(), {'sigma': sigma}


def _deliver_flipd(flipd, where, return_dims, rank, save_path, name):
    """The exit of method 'flipd': the rounded readings (``return_dims``) or ``<name>_flipd.pkl`` on rank 0."""
    import numpy as np
    flipd = np.asarray(flipd, dtype=np.float64)
    if not np.isfinite(flipd).all():
        raise RuntimeError(f"method 'flipd': {int((~np.isfinite(flipd)).sum())} of {len(flipd)} readings are not finite")
    dims = np.rint(flipd).astype(np.int64)
    if return_dims:
        return dims.tolist()
    if rank == 0:
        Path(save_path).mkdir(parents=True, exist_ok=True)
        with open(os.path.join(save_path, f'{name}_flipd.pkl'), 'wb') as f:
            pickle.dump({'flipd': flipd, 'dims': dims, **where}, f)


def _points_by_jacobian(pl_module, points, device, want_tangent):
    """The spectra, IDs and (``want_tangent``) tangent bases of ``points`` from the score Jacobian of the module's fcn network:
    -> (info, dims, tangent or None) as ``deliver`` takes them."""
    from . import jacobian
    xs = torch.stack([x.reshape(-1) for x, _ in points]).to(device=device, dtype=torch.float32).contiguous()
    J = jacobian.network_jacobians(pl_module, pl_module.sde, xs, pl_module.sampling_eps)
    sv = checked_spectra(jacobian._spectra_from(J)).numpy()
    tangent = None
    if want_tangent:
        dims, tangent = jacobian._tangents(J, sv)
    else:
        dims = jacobian.dims_from_spectra(sv).tolist()
    return {'singular_values': sv.tolist()}, [int(d) for d in dims], tangent


def _sv_count(sample_shape, batchsize):
    """torch.linalg.svd returns min(M, D) values per point (dim_reduction.py:197): a short loader batch gives a shorter list."""
    return min(batching(tuple(sample_shape), batchsize)[2], math.prod(sample_shape))


def _safe_rebuild(builder, x, batchsize, **kw):
    """The ``rebuild`` of SpectrumPipeline.submit / row_sharded_spectrum for the point ``builder.build(x, batchsize, **kw)``: the
    same build on the safe route."""
    return lambda: builder.build(x.to(builder.device), batchsize, safe=True, **kw)


def _launch_groups(config, points, ids):
    """How the points ``ids`` share launches -> (batched, groups of ids).  Vector data (at most 4096 elements a point, one loader
    batch size): many points per launch set and the batched spectrum kernel (one workgroup per matrix for D <= 128), in groups
    of ``dim_estimation.points_per_launch`` (default: 131072 rows a launch).  Anything else: one point per group."""
    if not ids or points[ids[0]][0].numel() > 4096 or len({points[p][1] for p in ids}) != 1:
        return False, [[p] for p in ids]
    rows = batching(tuple(points[ids[0]][0].shape), points[ids[0]][1])[2]
    group = max(1, min(len(ids), int(config.get('dim_estimation.points_per_launch', max(1, 131072 // rows)))))
    return True, [ids[lo:lo + group] for lo in range(0, len(ids), group)]


def _group_scores(builder, points, ids, batched, point_seed):
    """(S, rebuild) of one launch group: S [P, M, D] of a batched group (``build_many``; no rebuild), or S [M, D] of the group's
    one point and its safe rebuild."""
    if batched:
        return build_many(builder, [points[p][0].to(builder.device) for p in ids], points[ids[0]][1],
                          [point_seed(p) for p in ids]), None
    x, batchsize = points[ids[0]]
    return (builder.build(x.to(builder.device), batchsize, seed=point_seed(ids[0])),
            _safe_rebuild(builder, x, batchsize, seed=point_seed(ids[0])))


def _group_stein_sums(builder, points, ids, S, point_seed):
    """[P, 6] fp64 on the device for the launch group ``ids`` whose score matrices are S [P, M, D]: the five sums of ``_lib.stein_rows``
    and |mean score|^2, from the noise ``build`` / ``build_many`` perturbed with -- the in-kernel Philox stream of ``point_seed(p)``,
    regenerated and never stored, or for D % 4 != 0 the seeded matrix of ``_seeded_noise``."""
    from . import stein
    P, M, D = S.shape
    seeds = [point_seed(p) for p in ids]
    Z = torch.stack([builder._seeded_noise(M, D, seed) for seed in seeds]) if D % 4 else None
    sums, norm2 = stein.sums_of(S.contiguous(), seeds=None if D % 4 else seeds, Z=Z)
    return torch.cat([sums, norm2[:, None]], dim=1)


def _points_with_tangent(builder, points, batched, groups, point_seed, want_tangent=True, stein_sums=None):
    """The loop of ``get_manifold_dimension(return_tangent=True)`` and of ``return_flipd=True``: every launch group is taken to
    completion -- score matrix, (``stein_sums``, a list: the group's ``_group_stein_sums`` appended to it) spectrum, ID on the host,
    (``want_tangent``) ``_lib.tangent_basis(S, d)``, S released -- on ONE stream: the width of the basis is known only
    once the spectrum has reached the host, so nothing of the next point is queued under it.  Score matrices and spectra come
    from the same launches as without the flags.  -> (spectra [P, D] on the device, dims, tangent)."""
    import warnings
    pipe = SpectrumPipeline(builder.device, overlap=False)
    spectra, dims, tangent, capped = [], [], [], 0
    for ids in groups:
        S, rebuild = _group_scores(builder, points, ids, batched, point_seed)
        # the possibly rebuilt S is needed for the basis afterwards, so the finite check is made here, not by the pipeline
        if rebuild is not None and not bool(torch.isfinite(S).all()):
            warn_non_finite_point()
            S = rebuild()
        if stein_sums is not None:                   # of the matrix the spectrum is taken of: a rebuilt point is read from the rebuilt one
            stein_sums.append(_group_stein_sums(builder, points, ids, S if batched else S[None], point_seed))
        pipe.submit(S)
        svs = pipe.results()[0] if batched else torch.stack(pipe.results())
        for S_p, sv, p in zip(S if batched else [S], checked_spectra(svs), ids):
            x, b = points[p]
            d, k = tangent_width(sv[:_sv_count(x.shape, b)].tolist(), x.numel())
            dims.append(d)
            if not want_tangent:
                continue
            capped += d > _lib.TANGENT_MAX
            if k is None:
                tangent.append(None)
                continue
            T, _, resid = _lib.tangent_basis(S_p, k)
            if not math.isfinite(float(resid)):
                raise RuntimeError(f"point {p}: the tangent basis of width {k} came back non-finite (the Gram matrix of the scores is "
                                   "not positive semi-definite to rounding, or holds non-finite values)")
            tangent.append(T.to(torch.float32).cpu().numpy())
        spectra.extend(svs)
        del S
    if capped:
        warnings.warn(f"id-diff_amd: {capped} point(s) have an intrinsic dimension above {_lib.TANGENT_MAX}, the widest tangent "
                      "basis that is computed: their entry of `tangent` is None")
    return torch.stack(spectra), dims, (tangent if want_tangent else None)


def _sampled_flipd_refused(config, world, method):
    """return_flipd / dim_estimation.save_flipd, before the GPU is touched: the reading is taken of the rows of the sampled path, every
    point to completion on one rank."""
    if method != 'sampling':
        raise NotImplementedError(f"return_flipd / dim_estimation.save_flipd reads the score rows of method 'sampling', and "
                                  f"dim_estimation.method = {method!r} has none (method 'flipd' is itself a FLIPD reading)")
    if world > 1 or str(config.get('dim_estimation.shard', 'points')) == 'rows':
        raise NotImplementedError("return_flipd / dim_estimation.save_flipd needs a single rank and dim_estimation.shard = 'points' (got "
                                  f"world size {world}, shard = {config.get('dim_estimation.shard', 'points')!r}): the exchange of the "
                                  "readings between ranks and the reduction of a point's row sums over ranks are not implemented")


def _sampled_flipd_readings(stein_sums, spectra, points, sde, t):
    """The dict ``return_flipd`` delivers, float64 arrays [P]: the readings of ``stein.reading_from_sums`` for every point from ONE
    read-back of the [P, 6] sums and from the points' spectra on the host (their squared singular values sum to the centred trace of
    the finite-M correction), 'dims' (rint of 'flipd') and where they were read ('t', 'sigma' = std(t))."""
    import numpy as np
    from . import stein
    host = torch.cat(stein_sums).cpu().numpy() if stein_sums else np.zeros((0, 6))
    sigma = stein.level_sigma(sde, t)
    out = {k: np.empty(len(points), dtype=np.float64) for k in stein.KEYS}
    for p, (x, b) in enumerate(points):              # (M and D are per point: loader batches may differ)
        one = stein.reading_from_sums(host[p, :5], batching(tuple(x.shape), b)[2], x.numel(), sigma, host[p, 5],
                                      centred_trace=stein.trace_of(spectra[p].numpy()))
        for k in stein.KEYS:
            out[k][p] = one[k][0]
    if not np.isfinite(out['flipd']).all():
        raise RuntimeError(f"return_flipd: {int((~np.isfinite(out['flipd'])).sum())} of {len(points)} readings are not finite")
    out['dims'] = np.rint(out['flipd'])
    out['t'] = np.full(len(points), float(t), dtype=np.float64)
    out['sigma'] = np.full(len(points), sigma, dtype=np.float64)
    return out


def build_many(builder, xs, batchsize, seeds):
    """S [P, M, D] for P small (vector) points with ONE score_fn call over all P*M rows: the k-sphere workload is
    launch-bound one point at a time (M = 1501 rows of a 7-layer MLP), so points are batched (BASELINE config 2)."""
    x0 = xs[0]
    _, _, rows = batching(tuple(x0.shape), batchsize)
    D, P = x0.numel(), len(xs)
    noise = [builder._seeded_noise(rows, D, seed) for seed in seeds] if D % 4 else None
    batch, _ = builder._perturbed([x.reshape(-1).contiguous() for x in xs], builder.eps, 0, rows, noise=noise, seeds=seeds)
    t_all = torch.full((P * rows,), float(builder.eps), device=builder.device, dtype=torch.float32)
    score = builder.score_fn(batch.view(P * rows, *x0.shape), t_all)
    return score.reshape(P, rows, D)


def setup_model(config):
    """Steps :123-141 of the reference: data module, module + checkpoint, SDE, device, score_fn."""
    DataModule = create_lightning_datamodule(config)
    DataModule.setup()
    pl_module = create_lightning_module(config)
    pl_module = pl_module.load_from_checkpoint(config.model.checkpoint_path)
    pl_module.configure_sde(config)
    device = torch.device(config.device)
    if device.type != "cuda":
        raise RuntimeError(f"config.device is {device}: id-diff_amd runs the manifold_dimension path on the "
                           "MI355X only (the CPU restatement lives in oracle/ and is test infrastructure)")
    pl_module = pl_module.to(device)
    pl_module.eval()
    score_fn = mutils.get_score_fn(pl_module.sde, pl_module.score_model, conditional=False, train=False, continuous=True)
    return DataModule, pl_module, score_fn, device


def collect_points(loader, num_datapoints):
    """The points the reference's double loop would visit, in order (dim_reduction.py:154-164)."""
    pts, idx = [], 0
    for orig_batch in loader:
        if isinstance(orig_batch, (list, tuple)):
            orig_batch = orig_batch[0]
        batchsize = orig_batch.size(0)
        if idx + 1 >= num_datapoints:
            break
        for x in orig_batch:
            if idx + 1 >= num_datapoints:
                break
            pts.append((x, batchsize))
            idx += 1
    return pts


def get_manifold_dimension(config, name=None, return_svd=False, return_dims=False, return_tangent=False, method=None,
                           return_flipd=False):
    """Drop-in for dim_reduction.py:116-215.  ``return_dims=True`` (not in the reference; needs ``return_svd``) also
    returns the integer ID of every point, computed by the reference's rule on the rank that owns the point and gathered
    as int32 in the same collective as the spectra.

    ``return_tangent=True`` (with ``return_svd``; the reference has the same information in the ``v`` it drops at :197) appends
    ``tangent`` to what is returned: one entry per point, a float32 numpy array [D, d] whose orthonormal columns span the
    estimated tangent space -- the right singular vectors of the d smallest singular values, d that point's ID -- or None where
    d < 1 or d > 128 (one warning names the cap).  In this mode every point is handled to completion on one stream (score
    matrix, spectrum, ID on the host, ``_lib.tangent_basis``): there is NO side-stream overlap of spectrum and score
    evaluations, and it needs a single rank with ``dim_estimation.shard = 'points'`` (NotImplementedError otherwise).  The
    singular values and dims are those of a call without the flag, bit for bit.  Without ``return_svd`` the config key
    ``dim_estimation.save_tangent`` (default False) selects the mode and writes ``<name>_tangent.pkl`` =
    ``{'tangent': [...], 'dims': [...]}`` beside the unchanged ``<name>.pkl``.

    The row-sharded mode (``dim_estimation.shard = 'rows'`` on more than one rank) does not serve ``return_dims``: it returns
    ``info`` alone.

    ``method`` (or the config key ``dim_estimation.method``; the argument wins): 'sampling', the default, is everything above.
    'jacobian' (``model.name == 'fcn'`` without dropout, one rank, ``shard = 'points'``; NotImplementedError otherwise, before the
    GPU is touched) takes the same points and returns or writes the same layout, but its singular values are those of the score
    Jacobian at mean(t) x in closed form (jacobian.py), which the spectrum of the sampled score matrix estimates up to the factor
    std(t) sqrt(M); dims and tangent bases are read off them by the same rules.
    'flipd' (``model.name`` 'fcn' or 'empirical_exact', one rank, ``shard = 'points'``; NotImplementedError otherwise, and for
    ``return_svd`` / ``return_tangent`` / ``save_tangent``: it has no spectrum) reads D + sigma^2 (tr grad s + |s|^2) at the same points:
    ``jacobian.flipd`` at t = sampling_eps (exact unless ``dim_estimation.flipd_probes`` > 0) or the empirical kernel at
    sigma = model.sigma_min.  It writes ``<name>_flipd.pkl`` = ``{'flipd': float64 [P], 'dims': rint of it, 't' or 'sigma'}``;
    ``return_dims=True`` returns the integers instead.

    ``return_flipd=True`` (with ``return_svd``; method 'sampling', one rank, ``shard = 'points'``: NotImplementedError otherwise, before
    the GPU is touched) serves EVERY model: FLIPD of the score smoothed over the sampling ball, read off the score rows the spectrum
    is taken of by Stein's identity (stein.py; ``_lib.stein_rows``) at zero extra network evaluations.  Every point is taken to
    completion on one stream, as with ``return_tangent``; a point rebuilt on the safe route is read from the rebuilt matrix.  It
    appends, after whatever ``return_dims`` / ``return_tangent`` append, one dict of float64 arrays [P]: ``{'flipd', 'stderr', 'plain',
    'beta', 'dims' (rint of flipd), 't', 'sigma'}``.  Singular values, dims and tangent bases are those of a call without the flag, bit
    for bit.  Without ``return_svd`` the config key ``dim_estimation.save_flipd`` (default False) selects the mode and writes that
    dict to ``<name>_flipd_sampled.pkl`` beside the unchanged ``<name>.pkl``."""
    method = estimation_method(config, method)
    log_path, log_name = config.logging.log_path, config.logging.log_name
    save_path = os.path.join(log_path, log_name, 'svd')
    rank, world = parallel.rank_world()
    if method == 'jacobian':
        from . import jacobian
        jacobian.check_config(config)
        _jacobian_refused(config, world)
    if method == 'flipd':
        _flipd_refused(config, world, return_svd, return_tangent or bool(config.get('dim_estimation.save_tangent', False)))
    if return_tangent and not return_svd:
        raise ValueError("return_tangent needs return_svd=True (set dim_estimation.save_tangent to have the bases written to disk)")
    save_tangent = not return_svd and bool(config.get('dim_estimation.save_tangent', False))
    if return_tangent or save_tangent:
        _tangent_refused(config, world)
    if return_flipd and not return_svd:
        raise ValueError("return_flipd needs return_svd=True (set dim_estimation.save_flipd to have the readings written to disk)")
    save_flipd = not return_svd and bool(config.get('dim_estimation.save_flipd', False))
    if return_flipd or save_flipd:
        _sampled_flipd_refused(config, world, method)
    if rank == 0 and not return_svd:
        Path(save_path).mkdir(parents=True, exist_ok=True)

    def deliver(info, dims=None, tangent=None, flipd=None):
        """The one exit of every mode: what the flags ask for (``dims=None``: a mode that serves no IDs), or the pickles on rank 0."""
        if return_svd:
            out = (info,) + ((dims,) if return_dims and dims is not None else ()) + ((tangent,) if return_tangent else ()) + \
                ((flipd,) if return_flipd else ())
            return out if len(out) > 1 else info
        if rank == 0:
            with open(os.path.join(save_path, f'{name}.pkl'), 'wb') as f:
                pickle.dump(info, f)
            if save_tangent:
                with open(os.path.join(save_path, f'{name}_tangent.pkl'), 'wb') as f:
                    pickle.dump({'tangent': tangent, 'dims': dims}, f)
            if save_flipd:
                with open(os.path.join(save_path, f'{name}_flipd_sampled.pkl'), 'wb') as f:
                    pickle.dump(flipd, f)

    seed = int(config.get('seed', 42))
    torch.manual_seed(seed)  # same data split / loader order on every rank
    DataModule, pl_module, score_fn, device = setup_model(config)
    num_datapoints = _num_datapoints(config)
    points = collect_points(DataModule.train_dataloader(), num_datapoints)
    if method == 'flipd':
        flipd, where = _points_by_flipd(config, pl_module, points, device, seed) if points else ([], {})
        return _deliver_flipd(flipd, where, return_dims, rank, save_path, name)
    if not points:                       # num_datapoints <= 1: the reference's loop body never runs (:159-164)
        return deliver({'singular_values': []}, [], [], _sampled_flipd_readings([], [], [], pl_module.sde, pl_module.sampling_eps)
                       if return_flipd or save_flipd else None)
    if method == 'jacobian':
        return deliver(*_points_by_jacobian(pl_module, points, device, return_tangent or save_tangent))
    builder = ScoreMatrixBuilder(score_fn, pl_module.sde, pl_module.sampling_eps, device,
                                 config.get('dim_estimation.inflight_rows', None))
    def point_seed(p):
        return seed + 1000003 * (p + 1)

    if str(config.get('dim_estimation.shard', 'points')) == 'rows' and world > 1:
        # one point at a time on ALL ranks, each computing a slice of its rows (latency of a single large point)
        spectra = []
        with torch.no_grad():
            for p, (x, batchsize) in enumerate(points):
                rows = batching(tuple(x.shape), batchsize)[2]
                kw = dict(seed=point_seed(p), row_range=parallel.my_rows(rows, rank, world))
                S_local = builder.build(x.to(device), batchsize, **kw)
                spectra.append(row_sharded_spectrum(S_local, rows, rebuild=_safe_rebuild(builder, x, batchsize, **kw)))
        return deliver({'singular_values': [s.tolist() for s in checked_spectra(torch.stack(spectra))]})

    mine = parallel.my_points(len(points), rank, world)
    batched, groups = _launch_groups(config, points, mine)
    keep = [_sv_count(x.shape, b) for x, b in points]
    flipd = None
    with torch.no_grad():
        if return_tangent or save_tangent or return_flipd or save_flipd:   # one rank: ``mine`` is every point, nothing to exchange
            stein_sums = [] if return_flipd or save_flipd else None
            spectra, dims, tangent = _points_with_tangent(builder, points, batched, groups, point_seed,
                                                          want_tangent=return_tangent or save_tangent, stein_sums=stein_sums)
            if stein_sums is not None:
                flipd = _sampled_flipd_readings(stein_sums, checked_spectra(spectra), points, pl_module.sde, pl_module.sampling_eps)
        else:
            pipe = SpectrumPipeline(device, overlap=bool(config.get('dim_estimation.overlap_spectrum', True)))
            for ids in groups:
                pipe.submit(*_group_scores(builder, points, ids, batched, point_seed))
            local = [sv for block in pipe.results() for sv in block] if batched else pipe.results()
            n_sv = points[0][0].numel()              # fixed-width rows for the exchange (a rank without points takes part too)
            local = torch.stack(local) if local else torch.empty(0, n_sv, device=device)
            # (the rule needs three singular values; -1 marks a point that has fewer)
            my_dims = [estimate_dim(sv[:keep[p]].tolist()) if keep[p] >= 3 else -1 for sv, p in zip(checked_spectra(local), mine)]
            spectra, dims = parallel.gather_spectra(local, len(points), n_sv, device, dims=my_dims)
            dims, tangent = dims.tolist(), None
    return deliver({'singular_values': [s[:k].tolist() for s, k in zip(checked_spectra(spectra), keep)]}, dims, tangent, flipd)


def collect_labelled_points(loader, num_datapoints, label=1):
    """The (x, y, loader batch size) triples the reference's conditional loop visits (dim_reduction.py:49-60): items
    whose label equals 1, ``num_datapoints - 1`` of them."""
    pts, idx = [], 0
    for orig_batch, orig_labels in loader:
        batchsize = orig_batch.size(0)
        if idx + 1 >= num_datapoints:
            break
        for x, y in zip(orig_batch, orig_labels):
            if y.item() != label:
                continue
            if idx + 1 >= num_datapoints:
                break
            pts.append((x, y.item(), batchsize))
            idx += 1
    return pts


def conditional_spectra(builder, loader, num_datapoints, seed=42, levels=None, noise=None, overlap=True):
    """Spectra of the label-1 validation points at the noise levels ``linspace(sampling_eps, 0.3, 12)``
    (dim_reduction.py:39-101).  Returns one dict per level: ``{'level', 't', 'images', 'singular_values', 'labels'}``.

    MI355X specifics: per level the points are sharded round-robin over the ranks and their spectra combined by one
    all-gather (parallel.py); the spectrum of point p runs on the side stream under the score evaluations of point
    p+1 (``SpectrumPipeline``); nothing is synchronised with the host until a level is complete.  The Philox stream
    of (level, point) is keyed by ``seed + 1000003 * (point + 1) + 7919 * level``: levels do not share draws.
    ``levels`` restricts the sweep to some of the 12 indices and ``noise(level, point) -> [rows, *x.shape]`` supplies
    explicit draws (parity tests); the drop-in entry point below uses neither."""
    rank, world = parallel.rank_world()
    device = builder.device
    times = torch.linspace(builder.eps, 0.3, 12)
    out = []
    for level, t_slice in enumerate(times):
        if levels is not None and level not in levels:
            continue
        points = collect_labelled_points(loader, num_datapoints)
        mine = parallel.my_points(len(points), rank, world)
        pipe = SpectrumPipeline(device, overlap=overlap)
        with torch.no_grad():
            for p in mine:
                x, _, batchsize = points[p]
                z = None if noise is None else noise(level, p).to(device)
                kw = dict(t=float(t_slice), noise=z, seed=seed + 1000003 * (p + 1) + 7919 * level)
                pipe.submit(builder.build(x.to(device), batchsize, **kw), rebuild=_safe_rebuild(builder, x, batchsize, **kw))
            local = pipe.results()
        if points:
            n_sv = points[0][0].numel()
            local = torch.stack(local) if local else torch.empty(0, n_sv, device=device)
            spectra = checked_spectra(parallel.gather_spectra(local, len(points), n_sv, device))
            spectra = [s[:_sv_count(x.shape, b)] for s, (x, _, b) in zip(spectra, points)]
        else:
            spectra = torch.empty(0, 0)
        out.append({'level': level, 't': float(t_slice),
                    'images': torch.stack([x.permute(1, 2, 0) for x, _, _ in points]).numpy() if points else [],
                    'singular_values': [s.tolist() for s in spectra], 'labels': [y for _, y, _ in points]})
    return out


def get_conditional_manifold_dimension(config, name=None):
    """dim_reduction.py:12-114: the same estimator at 12 noise levels linspace(sampling_eps, 0.3, 12) on the
    label==1 points of the validation loader; writes images.pkl / labels_svd.pkl / labels.pkl per level
    (rank 0 only when run under torch.distributed)."""
    log_path, log_name = config.logging.log_path, config.logging.log_name
    config.data.return_labels = True
    seed = int(config.get('seed', 42))
    torch.manual_seed(seed)
    DataModule, pl_module, score_fn, device = setup_model(config)
    num_datapoints = config.get('dim_estimation.num_datapoints', 26)
    builder = ScoreMatrixBuilder(score_fn, pl_module.sde, pl_module.sampling_eps, device,
                                 config.get('dim_estimation.inflight_rows', None))
    loader = DataModule.val_dataloader()
    results = conditional_spectra(builder, loader, num_datapoints, seed=seed,
                                  overlap=bool(config.get('dim_estimation.overlap_spectrum', True)))
    if parallel.rank_world()[0] != 0:
        return
    for lv in results:
        t_save_path = os.path.join(log_path, log_name, 'svd', '%.3f' % lv['t'])
        Path(t_save_path).mkdir(parents=True, exist_ok=True)
        for fname, payload in (('images.pkl', {'images': lv['images']}),
                               ('labels_svd.pkl', {'singular_values': lv['singular_values']}),
                               ('labels.pkl', {'labels': lv['labels']})):
            with open(os.path.join(t_save_path, fname), 'wb') as f:
                pickle.dump(payload, f)
