"""Adaptive Runge-Kutta 5(4) (Dormand-Prince) with the step-size control of ``scipy.integrate.solve_ivp(method='RK45')``.

The reference integrates the probability-flow ODE with scipy (likelihood.py, sampling/unconditional.py:66-131): the state goes to the
host as a flat numpy vector for every evaluation.  Here the state stays on the device and only the step controller runs on the host.

``rk45_host`` restates the solver in fp64 numpy, expression by expression (``select_initial_step``, the Dormand-Prince tableau with FSAL,
the RMS error norm against atol + rtol max(|y|, |y_new|), safety 0.9, step factors 0.2 .. 10 capped at 1 after a rejection, exponent
-1/5, the clip of the last step to t1, both directions of time): it gives scipy's bits and scipy's ``nfev``, and is what the device driver
is checked against without a GPU.

``rk45`` is the device driver.  The state y is [B, W] fp64, the stage derivatives K [7, B, W] fp64 as scipy keeps them;
``rhs(stage, t, K, v)`` fills K[stage] from the fp32 network-input rows that ``idiff_rk_stage_f64`` wrote (v: the same argument in
fp64).  Per attempted step the host reads back ONE double, the sum of squared scaled errors (``idiff_rk_error_f64``), and nothing
else: that read-back is what host step control costs.  The initial step reads three more, once.

Guards scipy does not have, each a RuntimeError naming t and h: a non-finite error norm (scipy would loop on a NaN step size), a step
below 10 ulp(t) (scipy returns a failure status), and more than ``max_steps`` attempted steps.  The loop ends for every input.
"""
import math

import numpy as np

# Dormand-Prince 5(4): Hairer, Norsett, Wanner, Solving ODEs I, table II.5.2
C = np.array([0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1])
A = np.array([
    [0, 0, 0, 0, 0],
    [1 / 5, 0, 0, 0, 0],
    [3 / 40, 9 / 40, 0, 0, 0],
    [44 / 45, -56 / 15, 32 / 9, 0, 0],
    [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729, 0],
    [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656]])
B = np.array([35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84])
E = np.array([-71 / 57600, 0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40])
ORDER, ERROR_ORDER, N_STAGES = 5, 4, 6
SAFETY, MIN_FACTOR, MAX_FACTOR = 0.9, 0.2, 10.0
ERROR_EXPONENT = -1 / (ERROR_ORDER + 1)
MAX_STEPS = 10000
_EPS = np.finfo(float).eps


def _rtol(rtol):
    """validate_tol: a relative tolerance below 100 eps is raised to it."""
    return max(float(rtol), 100 * _EPS)


def min_step(t, direction):
    return 10 * abs(np.nextafter(t, direction * np.inf) - t)


def initial_step_from_norms(d0, d1, interval):
    """h0 of select_initial_step from d0 = |y0 / scale|_rms and d1 = |f0 / scale|_rms."""
    h0 = 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1
    return min(h0, interval)


def initial_step_final(h0, d1, d2, interval):
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1, d2)) ** (1 / (ERROR_ORDER + 1))
    return min(100 * h0, h1, interval, np.inf)


def next_factor(error_norm, rejected):
    """(accepted, factor on |h|) of one attempted step."""
    if error_norm < 1:
        factor = MAX_FACTOR if error_norm == 0 else min(MAX_FACTOR, SAFETY * error_norm ** ERROR_EXPONENT)
        return True, min(1, factor) if rejected else factor
    return False, max(MIN_FACTOR, SAFETY * error_norm ** ERROR_EXPONENT)


class _Controller:
    """The host half of the loop, shared by ``rk45_host`` and ``rk45``: which step to attempt next, and when to stop."""

    def __init__(self, t0, t1, h_abs, max_steps):
        self.t, self.t1 = float(t0), float(t1)
        self.direction = float(np.sign(t1 - t0)) if t1 != t0 else 1.0
        self.h_abs = h_abs
        self.max_steps = int(max_steps)
        self.steps = self.rejected = self.attempted = 0
        self.error_norms = []
        self._rejected_here = False
        self._enter_step()

    def _enter_step(self):
        self._min = min_step(self.t, self.direction)
        self._rejected_here = False
        if self.h_abs < self._min:
            self.h_abs = self._min

    def done(self):
        return self.direction * (self.t - self.t1) >= 0

    def attempt(self):
        """(h, t_new) of the next attempted step."""
        if self.h_abs < self._min:
            raise RuntimeError(f"rk45: the step size fell below 10 ulp(t) at t = {self.t!r}, h = {self.h_abs * self.direction!r}")
        if self.attempted >= self.max_steps:
            raise RuntimeError(f"rk45: more than max_steps = {self.max_steps} attempted steps at t = {self.t!r}, "
                               f"h = {self.h_abs * self.direction!r}")
        self.attempted += 1
        t_new = self.t + self.h_abs * self.direction
        if self.direction * (t_new - self.t1) > 0:
            t_new = self.t1
        h = t_new - self.t
        self.h_abs = abs(h)
        return h, t_new

    def judge(self, error_norm, h, t_new):
        """True when the attempted step is accepted (the controller has then moved to t_new)."""
        error_norm = float(error_norm)
        if not math.isfinite(error_norm):
            raise RuntimeError(f"rk45: the error norm is {error_norm!r} at t = {self.t!r}, h = {h!r} (a non-finite right-hand side)")
        self.error_norms.append(error_norm)
        accepted, factor = next_factor(error_norm, self._rejected_here)
        self.h_abs *= factor
        if not accepted:
            self._rejected_here = True
            self.rejected += 1
            return False
        self.steps += 1
        self.t = t_new
        self._enter_step()
        return True


def _norm(x):
    return np.linalg.norm(x) / x.size ** 0.5


def rk45_host(f, t0, t1, y0, rtol=1e-3, atol=1e-6, max_steps=MAX_STEPS):
    """``solve_ivp(f, (t0, t1), y0, method='RK45', rtol=rtol, atol=atol)`` in fp64 numpy: ``(y, nfev, steps, rejected, error_norms)`` with
    y the solution at t1 (scipy's ``sol.y[:, -1]``, bit for bit), nfev scipy's, ``steps`` the accepted and ``rejected`` the rejected
    attempts, ``error_norms`` the error norm of every attempted step in order."""
    t0, t1 = float(t0), float(t1)
    y = np.array(y0, dtype=np.float64).reshape(-1)
    rtol, atol = _rtol(rtol), float(atol)
    nfev = [0]

    def fun(t, v):
        nfev[0] += 1
        return np.asarray(f(t, v), dtype=np.float64).reshape(-1)

    direction = float(np.sign(t1 - t0)) if t1 != t0 else 1.0
    f0 = fun(t0, y)
    interval = abs(t1 - t0)
    if y.size == 0:
        h_abs = np.inf
    elif interval == 0.0:
        h_abs = 0.0
    else:
        scale = atol + np.abs(y) * rtol
        d0, d1 = _norm(y / scale), _norm(f0 / scale)
        h0 = initial_step_from_norms(d0, d1, interval)
        f1 = fun(t0 + h0 * direction, y + h0 * direction * f0)
        h_abs = initial_step_final(h0, d1, _norm((f1 - f0) / scale) / h0, interval)
    K = np.empty((N_STAGES + 1, y.size), dtype=np.float64)
    ctl = _Controller(t0, t1, h_abs, max_steps)
    fcur = f0
    while not ctl.done():
        while True:
            h, t_new = ctl.attempt()
            K[0] = fcur
            for s, (a, c) in enumerate(zip(A[1:], C[1:]), start=1):
                dy = np.dot(K[:s].T, a[:s]) * h
                K[s] = fun(ctl.t + c * h, y + dy)
            y_new = y + h * np.dot(K[:-1].T, B)
            f_new = fun(ctl.t + h, y_new)
            K[-1] = f_new
            scale = atol + np.maximum(np.abs(y), np.abs(y_new)) * rtol
            if ctl.judge(_norm(np.dot(K.T, E) * h / scale), h, t_new):
                break
        y, fcur = y_new, f_new
    return y, nfev[0], ctl.steps, ctl.rejected, ctl.error_norms


def rk45(rhs, t0, t1, y, x32, D, label_of, rtol=1e-5, atol=1e-5, max_steps=MAX_STEPS, K=None):
    """The device driver.  ``y`` [B, W] fp64 on the device (W = D, or D + 1 with log p in the last column) is integrated in place from
    t0 to t1.  ``x32`` [B, > D] fp32 are the network's padded input rows, ``label_of(t)`` the time label written into their column D.
    ``rhs(stage, t, K, v)`` must fill ``K[stage]`` ([B, W] fp64) with the derivative at time t of the stage's argument, which it finds
    as fp32 rows in x32 and as fp64 in ``v`` [B, W].  Returns ``(nfev, steps, rejected, error_norms)`` with scipy's counting."""
    import torch
    from . import _lib
    t0, t1 = float(t0), float(t1)
    Bn, W = y.shape
    rtol, atol = _rtol(rtol), float(atol)
    if K is None:
        ldk = (W + 1) // 2 * 2                        # even pitch: 16-byte accesses
        K = torch.zeros(7, Bn, ldk, device=y.device, dtype=torch.float64)[:, :, :W]
    y_new, v = torch.zeros_like(K[0]), torch.zeros_like(K[0])
    ws, out = _lib.reduce_workspace(y.device), torch.zeros((), device=y.device, dtype=torch.float64)
    n = float(Bn * W)
    nfev = [0]

    def evaluate(stage, t, arg):
        nfev[0] += 1
        rhs(stage, t, K, arg)

    def rms(coef, a, b, at, rt):
        """sqrt(mean((sum_j coef_j K_j / (at + rt max(|a|, |b|)))^2)): the one read-back."""
        _lib.rk_error(K, coef, a, b, at, rt, out=out, workspace=ws)
        return math.sqrt(float(out) / n) if n else 0.0

    direction = float(np.sign(t1 - t0)) if t1 != t0 else 1.0
    interval = abs(t1 - t0)
    _lib.rk_stage(y, K, [], x32, D, label_of(t0))                         # the network input of (t0, y)
    evaluate(0, t0, y)
    if n == 0:
        h_abs = np.inf
    elif interval == 0.0:
        h_abs = 0.0
    else:
        K[6].copy_(y)                                                     # select_initial_step's three norms through the error kernel
        unit = lambda j: [1.0 if i == j else 0.0 for i in range(7)]
        d0, d1 = rms(unit(6), y, y, atol, rtol), rms(unit(0), y, y, atol, rtol)
        h0 = initial_step_from_norms(d0, d1, interval)
        t_probe = t0 + h0 * direction
        _lib.rk_stage(y, K, [h0 * direction], x32, D, label_of(t_probe), y_out=v)
        evaluate(1, t_probe, v)
        d2 = rms([-1.0, 1.0, 0, 0, 0, 0, 0], y, y, atol, rtol) / h0
        h_abs = initial_step_final(h0, d1, d2, interval)
    ctl = _Controller(t0, t1, h_abs, max_steps)
    while not ctl.done():
        while True:
            h, t_new = ctl.attempt()
            for s in range(1, N_STAGES):
                ts = ctl.t + float(C[s]) * h
                _lib.rk_stage(y, K, [float(a) * h for a in A[s][:s]], x32, D, label_of(ts), y_out=v)
                evaluate(s, ts, v)
            _lib.rk_stage(y, K, [float(b) * h for b in B], x32, D, label_of(ctl.t + h), y_out=y_new)
            evaluate(6, ctl.t + h, y_new)
            if ctl.judge(rms([float(e) * h for e in E], y, y_new, atol, rtol), h, t_new):
                break
        y.copy_(y_new)
        K[0].copy_(K[6])                                                  # FSAL
    return nfev[0], ctl.steps, ctl.rejected, ctl.error_norms
