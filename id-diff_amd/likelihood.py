"""Log-likelihood of a trained ``fcn`` score network through the probability-flow ODE (reference: likelihood.py).

The reverse SDE's ``probability_flow=True`` drift of a network whose score is -raw / std(t) is, with all rows at one time,

    dx/dt = a(t) x + b(t) raw(x, t),     a = d(t),   b = g(t)^2 / (2 std(t))          (sampling.flow_coefficients)

and log p changes along it by the divergence a D + b tr(d raw / dx).  The reference lets scipy's RK45 drive this through torch autograd,
the state crossing to the host at every evaluation; here the state [B, D + 1] stays on the device in fp64, ``ode.rk45`` restates scipy's
step control on the host, and one evaluation of the right-hand side is

    forward      the network's own launches (idiff_gemm_f32, bias + ELU in the epilogue) on the fp32 rows idiff_rk_stage_f64 wrote,
                 every ELU output kept
    Hutchinson   eps back through the layers with idiff_gemm_nn_f32 (ELU' from the ELU output, as train.py's backward), down to the
                 padded input: u = eps^T d raw / dx, and the estimate sum_c eps_c u_c inside idiff_flow_rhs_f64
    exact        the forward-mode tangent rows of jacobian.py up to the last hidden layer, then idiff_jvp_trace_f64 against the output
                 weights: the trace without the last tangent layer and without a [P, D, D] Jacobian; points in chunks under
                 jacobian.T_BYTES_PER_LAUNCH
    rhs          idiff_flow_rhs_f64: K_s = [a x + b raw, a D + b q]

Scope: ``models.fcn.FCN`` without dropout, one GPU, ``method='RK45'``.  Anything else is refused before the GPU is touched.
"""
import numpy as np
import torch

from . import ode, sampling

SALT_HUTCHINSON = 14              # train.stream_key salt of the probe vectors (sampling.py uses 11 .. 13)


class FcnFlow:
    """The right-hand side of the probability-flow ODE of an FCN for a batch of B rows: buffers allocated once, ``rhs(stage, t, K, v)`` as
    ``ode.rk45`` calls it.  ``aug``: carry log p in column D; ``exact``: the exact divergence instead of Hutchinson's estimate with the
    probe rows ``eps`` [B, D] fp32."""

    def __init__(self, net, sde, B, aug, exact=False, eps=None):
        from . import jacobian
        self.sde, self.B, self.D, self.aug, self.exact = sde, int(B), int(net.state_size), int(aug), bool(exact)
        self.ws, self.bs, self.kpad = jacobian._weights(net)
        dev = self.ws[0].device
        z = lambda r, c: torch.zeros(r, c, device=dev, dtype=torch.float32)
        p4 = jacobian.pad4
        self.x32 = z(B, self.kpad)                                        # the pads beyond the label stay zero
        self.acts = [z(B, p4(w.shape[0])) for w in self.ws[:-1]]
        self.raw = z(B, p4(self.D))
        self.q = self.eps = None
        if self.aug and self.exact:
            self.q = torch.zeros(B, device=dev, dtype=torch.float64)
            width = max(p4(w.shape[0]) for w in self.ws[:-1])
            self.chunk = max(1, jacobian.T_BYTES_PER_LAUNCH // (2 * 4 * self.D * width))
        elif self.aug:
            self.eps = z(B, p4(self.D))
            self.eps[:, :self.D] = eps
            self.dA = [z(B, p4(w.shape[0])) for w in self.ws[:-1]]
            self.u = z(B, self.kpad)

    def label_of(self, t):
        return sampling.label_of(self.sde, t)

    def forward(self):
        """raw = network(x32): every ELU output stays in self.acts.  The launches are held to fp32 arithmetic (IDIFF_NO_SPLIT on this
        thread): idiff_gemm_f32's default route cuts the operands into three bf16 pieces, whose error is as small as an fp32
        rounding but biased (measured on the fixture network: signed mean -1.5e-8 against -5e-10), and an integrator adds up a
        hundred evaluations: the bias arrives at the end point whole where rounding noise averages out."""
        from . import _lib, jacobian
        with _lib.thread_option("IDIFF_NO_SPLIT", 1):
            jacobian.forward_acts(self.ws, self.bs, self.x32, self.kpad, acts=self.acts)
            w, h = self.ws[-1], self.acts[-1]
            _lib.gemm(h, w, out=self.raw, epilogue=_lib.make_epilogue(bias=self.bs[-1], act=None), M=self.B, N=w.shape[0], K=h.shape[1],
                      lda=h.stride(0), ldb=w.stride(0), ldc=self.raw.stride(0))
        return self.raw

    def vjp(self):
        """u[:, :D] = eps^T d raw / d x, row by row."""
        from . import _lib
        dA = self.eps
        for i in range(len(self.ws) - 1, -1, -1):
            w = self.ws[i]
            if i > 0:
                nxt, act = self.dA[i - 1], self.acts[i - 1]
                _lib.gemm_nn(dA, w, out=nxt, elu_out=act, M=self.B, N=self.ws[i - 1].shape[0], K=w.shape[0], lda=dA.stride(0),
                             ldb=w.stride(0), ldc=nxt.stride(0), ldp=act.stride(0))
                dA = nxt
            else:
                _lib.gemm_nn(dA, w, out=self.u, M=self.B, N=self.D, K=w.shape[0], lda=dA.stride(0), ldb=w.stride(0),
                             ldc=self.u.stride(0))
        return self.u

    def trace(self):
        """q[r] = tr(d raw / d x) at row r."""
        from . import _lib, jacobian
        n, w_out = len(self.ws) - 1, self.ws[-1]
        for lo in range(0, self.B, self.chunk):
            acts = [a[lo:lo + self.chunk] for a in self.acts]
            P = acts[0].shape[0]
            T, ld = jacobian.tangent_rows(self.ws, acts, self.D, n)
            _lib.jvp_trace(T, w_out, out=self.q[lo:lo + P], P=P, D=self.D, N=self.ws[n - 1].shape[0], ldt=ld, stride_t=self.D * ld,
                           ldw=w_out.stride(0))
        return self.q

    def rhs(self, stage, t, K, v=None):
        from . import _lib
        if self.B == 0:
            return
        a, b, _, _ = sampling.flow_coefficients(self.sde, t)
        self.forward()
        if self.aug and self.exact:
            self.trace()
            _lib.flow_rhs(self.x32, self.raw, a, b, K[stage], self.D, 1, q=self.q)
        elif self.aug:
            self.vjp()
            _lib.flow_rhs(self.x32, self.raw, a, b, K[stage], self.D, 1, eps=self.eps, u=self.u)
        else:
            _lib.flow_rhs(self.x32, self.raw, a, b, K[stage], self.D, 0)


def fcn_of(model):
    """The FCN of ``model`` (or of a module that holds it as ``score_model``), refused without touching the GPU when it is another
    network or has dropout: no other network has a derivative path here."""
    from .jacobian import _network
    try:
        return _network(model)[0]
    except NotImplementedError as e:
        raise NotImplementedError(str(e).replace("the Jacobian method", "the likelihood")) from None


def check_config(config):
    """``jacobian.check_config`` for the likelihood: model.name == 'fcn' without dropout, before anything touches the GPU."""
    from . import jacobian
    try:
        jacobian.check_config(config)
    except NotImplementedError as e:
        raise NotImplementedError(str(e).replace("the Jacobian method", "the likelihood")) from None


def check_method(method):
    if str(method) != 'RK45':
        raise NotImplementedError(f"ODE solver method {method!r}: only 'RK45' is built (ode.py restates scipy's RK45 step control)")


def state_buffer(B, W, device):
    """[B, W] fp64 zeros with an even row pitch (16-byte accesses)."""
    return torch.zeros(B, (W + 1) // 2 * 2, device=device, dtype=torch.float64)[:, :W]


def probes(hutchinson_type, B, D, seed, device):
    """[B, D] fp32 probe vectors of the library's Philox stream (seed, salt 14): Gaussian draws, and their signs for Rademacher."""
    from . import _lib
    if hutchinson_type not in ('Gaussian', 'Rademacher'):
        raise NotImplementedError(f"Hutchinson type {hutchinson_type} unknown.")
    z = torch.zeros(B, D, device=device, dtype=torch.float32)
    _lib.sampler_step(z, z, 0.0, 0.0, 1.0, D=D, seed=sampling._stream_key(seed, 0, SALT_HUTCHINSON))
    if hutchinson_type == 'Rademacher':
        z = torch.where(z >= 0, torch.ones_like(z), -torch.ones_like(z))
    return z


def get_likelihood_fn(sde, inverse_scaler=None, exact=False, t=0.0, hutchinson_type='Rademacher', rtol=1e-5, atol=1e-5, method='RK45',
                      eps=1e-5):
    """likelihood.py:52-130 of the reference.  Returns ``likelihood_fn(model, data, *, seed=None, epsilon=None) -> (bpd, z, nfe)``:
    the flow is integrated from t + eps to sde.T; z [B, D] fp32 is the latent code, nfe the number of right-hand sides, and

        bpd = -(prior_logp(z) + delta_logp) + offset,    offset = 7 - inverse_scaler(-1) (0 without an inverse_scaler)

    as the reference returns it: NOT divided by D or by log 2 (the reference has those lines commented out), so "bpd" is the negative
    log-likelihood in nats plus the offset.  ``exact`` takes the exact divergence; otherwise Hutchinson's estimator with one probe vector
    per row: ``epsilon`` [B, D] replays explicit ones, else they are Gaussian draws of the library's Philox stream keyed by ``seed``
    (default 42), and their signs for ``hutchinson_type='Rademacher'``.  The same seed gives the same bits.

    ``model``: a ``models.fcn.FCN`` without dropout (or a module holding one as ``score_model``); any other network and any ``method``
    but 'RK45' raise NotImplementedError before the GPU is touched."""
    check_method(method)
    if hutchinson_type not in ('Gaussian', 'Rademacher'):
        raise NotImplementedError(f"Hutchinson type {hutchinson_type} unknown.")
    sampling._kind(sde)                                                  # VE, VP or subVP

    def likelihood_fn(model, data, *, seed=None, epsilon=None):
        net = fcn_of(model)
        D = int(net.state_size)
        if data.ndim != 2 or data.shape[1] != D:
            raise RuntimeError(f"likelihood_fn: data must be [B, {D}], got {tuple(data.shape)}")
        device = next(net.parameters()).device
        if device.type != 'cuda':
            raise RuntimeError(f"likelihood_fn: the model is on {device}; id-diff_amd integrates on the MI355X only (no CPU path)")
        B = data.shape[0]
        with torch.no_grad():
            data = torch.as_tensor(data, dtype=torch.float32).to(device)
            probe = None
            if not exact:
                if epsilon is not None:
                    probe = torch.as_tensor(epsilon, dtype=torch.float32).to(device).reshape(B, D)
                else:
                    probe = probes(hutchinson_type, B, D, 42 if seed is None else int(seed), device)
            flow = FcnFlow(net, sde, B, aug=1, exact=exact, eps=probe)
            y = state_buffer(B, D + 1, device)
            y[:, :D] = data.double()
            nfe, _, _, _ = ode.rk45(flow.rhs, float(t) + float(eps), float(sde.T), y, flow.x32, D, flow.label_of, rtol=rtol, atol=atol)
            z = y[:, :D].float()
            delta_logp = y[:, D].float()
            bpd = -(sde.prior_logp(z) + delta_logp)
            offset = 7. - inverse_scaler(-1.) if inverse_scaler is not None else 0
            return bpd + offset, z, nfe

    return likelihood_fn


def evaluate(config, checkpoint_path=None, num_samples=None, exact=False, seed=None, log_path=None, log_name=None, log=print):
    """``--mode likelihood``: the likelihood of the first ``num_samples`` (default 1000) points of the config's test split on one GPU;
    writes ``<log_path>/<log_name>/likelihood/likelihood.pkl`` = {bpd, z, nfe, exact} and logs the mean, minimum and maximum."""
    import os
    import pickle
    from .lightning_modules.utils import create_lightning_module
    from .train import data_split
    check_config(config)
    device = torch.device(config.get('device', 'cuda:0'))
    module = create_lightning_module(config)
    module = module.load_from_checkpoint(checkpoint_path if checkpoint_path is not None else config.model.get('checkpoint_path'))
    module.configure_sde(config)
    module.to(device).eval()
    n = 1000 if num_samples is None else int(num_samples)
    data = data_split(config, 'test')[:n].to(device)
    fn = get_likelihood_fn(module.sde, exact=exact, eps=module.sampling_eps)
    bpd, z, nfe = fn(module.score_model, data, seed=int(config.get('seed', 42)) if seed is None else int(seed))
    log_path = log_path if log_path is not None else (config.logging.get('log_path') or './')
    log_name = log_name if log_name is not None else (config.logging.get('log_name') or 'likelihood')
    path = os.path.join(log_path, log_name, 'likelihood', 'likelihood.pkl')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    bpd_np = bpd.cpu().numpy().astype(np.float32)
    with open(path, 'wb') as f:
        pickle.dump(dict(bpd=bpd_np, z=z.cpu().numpy().astype(np.float32), nfe=int(nfe), exact=bool(exact)), f)
    if log is not None:
        log(f"{len(bpd_np)} points, nfe {int(nfe)}: mean {bpd_np.mean():.6g} min {bpd_np.min():.6g} max {bpd_np.max():.6g}; wrote {path}")
    return bpd, z, nfe, path
