"""Sampling-free diffusion ID for a trained ``fcn`` score network: the Jacobian of the score in closed form.

The estimator reads the dimension off the spectrum of a point's score matrix S [M, D], whose rows are score_fn(mean(t) x + std(t) z_i, t).
To first order a row is J std z_i with J = d score_fn / dx at the centre mean(t) x of the cloud, so the spectrum of the centred S is a
Monte-Carlo estimate of the singular values of J times std sqrt(M), every value blurred by about sqrt(D / M) (25 % at the paper's
M = 1501, D = 100).  This module computes the thing that is estimated.  The network is Linear + ELU layers, so the D input directions of
a point go through it in forward mode as D tangent rows:

    forward      the P centres through the network's own launches (idiff_gemm_f32, bias + ELU in the epilogue), every ELU output kept
    seed         T_1[p][i, n] = W_1[n, i] g(a_1[p, n])                              idiff_jvp_seed_f32
    layers       T_l[p] = (T_(l-1)[p] W_l^T) (*) g(a_l[p]),  then T_out = T_L W_out^T    idiff_jvp_layer_f32 (csrc/fcn_jacobian.hip)
    scale        J[p] = -T_out[p] / std(t)                                           get_score_fn's factor

with g(a) = a > 0 ? 1 : a + 1, ELU' written in the ELU output.  D tangent rows a point instead of M sample rows, and a D x D spectrum
problem instead of an M x D one.  ``J[p][i, j] = d score_j / d x_i``: the rows of J[p] play the part of the score rows, and its uncentred
fp64 Gram sum_i J[i, :]^T J[i, :] is the matrix whose eigenvectors are the right singular vectors the sampled path estimates.

Limits.  ``model.name == 'fcn'`` without dropout only: no other network has a derivative path here, and finite differences are not a
substitute.  One GPU.  The Jacobian at a single point sees the roughness of the network at that point, which the sampled cloud averages
over a ball of radius std(t) sqrt(D): where the two disagree, that is what they disagree about.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib, dim_reduction, sde_lib
from .models.fcn import FCN
from .plot_utils import estimate_dim

T_BYTES_PER_LAUNCH = 256 << 20          # the two ping-pong tangent buffers of one chunk of points


def pad4(n):
    return (n + 3) // 4 * 4


def check_config(config):
    """Refuse, before anything touches the GPU, a config whose network has no derivative path here."""
    name = config.model.get('name')
    if name != 'fcn':
        raise NotImplementedError(f"the Jacobian method serves model.name == 'fcn' only, not {name!r}: no other network has a "
                                  "forward-mode derivative path here (and finite differences are not a substitute)")
    if float(config.model.get('dropout', 0.0) or 0.0) > 0:
        raise NotImplementedError(f"the Jacobian method of model 'fcn' needs model.dropout == 0 (got {config.model.dropout})")


def _network(model):
    """(the FCN, the sampling_eps of the module around it or None) of an FCN or of a module that holds one as ``score_model``."""
    eps = getattr(model, 'sampling_eps', None)
    net = getattr(model, 'score_model', model)
    if not isinstance(net, FCN):
        name = getattr(net, 'name', None) or type(net).__name__
        raise NotImplementedError(f"the Jacobian method serves the 'fcn' network only, not {name}: no other network has a "
                                  "forward-mode derivative path here (and finite differences are not a substitute)")
    for layer in net.mlp:
        if isinstance(layer, nn.Dropout) and layer.p > 0:
            raise NotImplementedError(f"the Jacobian method of model 'fcn' needs dropout == 0 (got {layer.p})")
    return net, eps


def default_eps(sde):
    """The sampling_eps ``sde_lib.configure_sde`` pairs with this SDE."""
    return 1e-5 if isinstance(sde, sde_lib.VESDE) else 1e-3


def _weights(net):
    """The Linear weights [out, pad4(in)] (zero pad columns) and biases: the network's own pack where its rows are 16-byte already."""
    pk = net.packed()
    ws = []
    for w in pk["w"]:
        if w.shape[1] % 4:
            wp = torch.zeros(w.shape[0], pad4(w.shape[1]), device=w.device, dtype=torch.float32)
            wp[:, :w.shape[1]] = w
            w = wp
        ws.append(w)
    return ws, pk["b"], pk["kpad"]


def forward_acts(ws, bs, h, kpad, acts=None):
    """The ELU output [P, pad4(N)] of every hidden layer for the padded input rows ``h`` [P, kpad]: FCN.forward's launches with every
    activation kept (rows padded to 16 bytes, pads zero).  ``acts``: buffers to reuse (their pads must be zero)."""
    P = h.shape[0]
    out, K = [], kpad
    for i, (w, b) in enumerate(zip(ws[:-1], bs[:-1])):
        N = w.shape[0]
        a = torch.zeros(P, pad4(N), device=h.device, dtype=torch.float32) if acts is None else acts[i]
        _lib.gemm(h, w, out=a, epilogue=_lib.make_epilogue(bias=b, act="elu"), M=P, N=N, K=K, lda=h.stride(0), ldb=w.stride(0),
                  ldc=a.stride(0))
        out.append(a)
        h, K = a, pad4(N)                      # the pad columns of the activations and of the weights are zero
    return out


def tangent_rows(ws, acts, D, n_layers):
    """(flat buffer, ld): the tangent rows [P][D, ld] of the D input directions behind the first ``n_layers`` Linear layers (the seed and
    ws[1:n_layers]; a layer without an activation behind it, the output layer, gets no ELU' factor), in one of two ping-pong buffers."""
    P = acts[0].shape[0]
    width = max(pad4(w.shape[0]) for w in ws[:n_layers])
    bufs = [torch.empty(P * D * width, device=acts[0].device, dtype=torch.float32) for _ in range(2)]
    N = ws[0].shape[0]
    ld = pad4(N)
    _lib.jvp_seed(ws[0], acts[0], out=bufs[0], P=P, D=D, N=N, ldw=ws[0].stride(0), ld_act=acts[0].stride(0), ldt=ld, stride_t=D * ld)
    cur = 0
    for i, w in enumerate(ws[1:n_layers], start=1):
        act = acts[i] if i < len(acts) else None
        N, K = w.shape[0], ws[i - 1].shape[0]
        ldc = pad4(N)
        _lib.jvp_layer(bufs[cur], w, act=act, out=bufs[1 - cur], P=P, R=D, N=N, K=K, lda=ld, stride_a=D * ld, ldw=w.stride(0),
                       ld_act=None if act is None else act.stride(0), ldc=ldc, stride_c=D * ldc)
        cur, ld = 1 - cur, ldc
    return bufs[cur], ld


def _chunk_jacobians(net, sde, xs, t):
    """J [P, D, D] of one chunk of points (see ``network_jacobians``)."""
    P, D = xs.shape
    dev = xs.device
    ws, bs, kpad = _weights(net)
    # the SDE's scalars in fp64, rounded once: in fp32 the VP std = sqrt(1 - exp(2 log_mean_coeff)) cancels to 1e-4 relative at t = 1e-3
    vec_t = torch.full((P,), float(t), device=dev, dtype=torch.float64)
    centre, std = sde.marginal_prob(xs.double(), vec_t)
    centre, labels = centre.float(), (vec_t * (sde.N - 1)).float()
    # 1. the forward of the centres: FCN.forward's launches, every ELU output kept (rows padded to 16 bytes)
    tpad = torch.zeros(P, kpad - D, device=dev, dtype=torch.float32)
    tpad[:, 0] = labels
    h = torch.empty(P, kpad, device=dev, dtype=torch.float32)
    _lib.concat_cols(centre.contiguous(), D, tpad, kpad - D, h, P)
    acts = forward_acts(ws, bs, h, kpad)
    # 2.-4. seed, hidden layers, output layer: two ping-pong buffers of tangent rows
    buf, ld = tangent_rows(ws, acts, D, len(ws))
    out = buf[:P * D * ld].view(P, D, ld)[:, :, :D]
    # 5. get_score_fn's factor: -1 / std, rounded to fp32 once
    return out * (-1.0 / std).float().view(P, 1, 1)


def network_jacobians(model, sde, xs, t=None):
    """J [P, D, D] fp32 on the device, ``J[p][i, j] = d score_j / d x_i`` of the score ``models.utils.get_score_fn`` makes of the network
    (its -1 / std(t) included), evaluated at mean(t) x_p, the centre of the cloud the driver draws around x_p.  ``model``: the FCN, or a
    module that holds it as ``score_model``; ``t`` defaults to that module's ``sampling_eps`` (for a bare FCN: the one
    ``sde_lib.configure_sde`` pairs with the SDE).  xs [P, D] fp32 on the device.  mean(t), std(t) and the time label are evaluated in fp64
    and rounded once (``get_score_fn``'s fp32 std of the VP SDE cancels to 1e-4 relative at t = 1e-3).  Points go in chunks whose two
    tangent buffers stay under ``T_BYTES_PER_LAUNCH``.  Nothing inside reads the device back."""
    net, eps = _network(model)
    _lib._dev(xs, "xs")
    D = net.state_size
    if xs.ndim != 2 or xs.shape[1] != D:
        raise RuntimeError(f"network_jacobians: xs must be [P, {D}], got {tuple(xs.shape)}")
    if t is None:
        t = default_eps(sde) if eps is None else eps
    P = xs.shape[0]
    J = torch.empty(P, D, D, device=xs.device, dtype=torch.float32)
    width = max(pad4(l.out_features) for l in net.mlp if isinstance(l, nn.Linear))
    step = max(1, T_BYTES_PER_LAUNCH // (2 * 4 * D * width))
    with torch.no_grad():
        for lo in range(0, P, step):
            J[lo:lo + step] = _chunk_jacobians(net, sde, xs[lo:lo + step], t)
    return J


def _grams(J):
    """The uncentred fp64 Gram [P, D, D] of the rows of every J[p]: idiff_centered_gram_f64 with a zero mean and batch P."""
    P, D, _ = J.shape
    G = torch.empty(P, D, D, dtype=torch.float64, device=J.device)
    zero = torch.zeros(min(P, 65535), D, dtype=torch.float64, device=J.device)
    for lo in range(0, P, 65535):
        n = min(65535, P - lo)
        _lib._check(_lib.lib().idiff_centered_gram_f64(J[lo:lo + n].data_ptr(), zero.data_ptr(), n, D, D, G[lo:lo + n].data_ptr(),
                                                       _lib._stream()), "idiff_centered_gram_f64")
    return G


def _spectra_from(J):
    """Singular values [P, D] fp64, descending, on the device, of every J[p] (through the Gram and ``_lib.sym_eigvals_batched``)."""
    if J.shape[0] == 0:
        return torch.empty(0, J.shape[1], dtype=torch.float64, device=J.device)
    return _lib.sym_eigvals_batched(_grams(J)).clamp_min(0.0).sqrt().flip(1)


def jacobian_spectra(model, sde, xs, t=None):
    """Singular values [P, D] (fp64 numpy, descending) of the score Jacobian at every point of xs: what the spectrum of the driver's
    centred score matrix estimates, up to the factor std(t) sqrt(M) and its sampling noise."""
    return dim_reduction.checked_spectra(_spectra_from(network_jacobians(model, sde, xs, t))).numpy()


def dims_from_spectra(sv):
    """``estimate_dim`` per row of sv [P, D] (the rule is scale-invariant); -1 with fewer than three singular values."""
    return np.asarray([estimate_dim(list(s)) if len(s) >= 3 else -1 for s in np.asarray(sv).tolist()], dtype=np.int64)


def local_dims(model, sde, xs, t=None):
    """int64 numpy [P]: the intrinsic dimension at every point of xs, by the driver's rule from the spectrum of the score Jacobian."""
    return dims_from_spectra(jacobian_spectra(model, sde, xs, t))


def _tangents(J, sv, dtype=np.float32):
    """(dims, bases) from the Jacobians and their spectra (host): per point ``_lib.sym_lowvecs`` of its Gram at the width
    ``dim_reduction.tangent_width`` gives."""
    D = J.shape[1]
    dims, out = [], []
    for p, s in enumerate(sv.tolist()):
        d, k = dim_reduction.tangent_width(s, D)
        dims.append(d)
        if k is None:
            out.append(None)
            continue
        # sym_lowvecs takes four steps of inverse iteration, each contracting by lambda_k / lambda_(k+1).  A trained network's tangent
        # singular values are about a tenth of its normal ones, so the ratio is 1e-2 and four steps would leave 1e-7 of the start
        # block (measured: DESIGN.md 4.9).  G^2 has the same invariant subspaces and the squared ratio; sum_k G[i, k] G[j, k] is
        # symmetric to the bit.
        G = _grams(J[p:p + 1])[0]
        T, _, resid = _lib.sym_lowvecs((G[:, None, :] * G[None, :, :]).sum(-1), k)
        if not np.isfinite(float(resid)):
            raise RuntimeError(f"point {p}: the tangent basis of width {k} came back non-finite (the Jacobian holds non-finite values)")
        out.append(T.cpu().numpy().astype(dtype))
    return dims, out


def local_tangent(model, sde, xs, t=None, dtype=np.float32):
    """One float32 numpy array [D, d] per point, in the layout of ``get_manifold_dimension(return_tangent=True)``: orthonormal columns
    spanning the right singular vectors of the d smallest singular values of the score Jacobian, d the point's ID; None where no basis
    is served (``dim_reduction.tangent_width``: d < 1, d above ``_lib.TANGENT_MAX`` or d not below D).  ``dtype=np.float64`` keeps the
    vectors as ``_lib.sym_lowvecs`` computed them: rounding an exact basis to float32 alone turns it by about 3e-8."""
    J = network_jacobians(model, sde, xs, t)
    return _tangents(J, dim_reduction.checked_spectra(_spectra_from(J)).numpy(), dtype=dtype)[1]


def flipd(model, sde, xs, t=None, exact=True, n_probes=1, hutchinson_type='Rademacher', seed=0):
    """FLIPD [P] fp64 on the device (Kamkari et al. 2024; LIDL of Tempczyk et al. 2022 through the Fokker-Planck equation): the REAL-valued
    local dimension

        D + std(t)^2 [ tr grad_y s(y, t) + |s(y, t)|^2 ],     y = mean(t) x,   s = -raw / std(t) the score ``get_score_fn`` makes

    of a trained fcn network at every point of xs [P, D]: one forward and one trace, no Jacobian, no Gram, no eigensolve.  With
    raw the network's output it is D - std tr(d raw / dy) + |raw|^2.  ``exact``: the trace from the forward-mode tangent rows up to the
    last hidden layer and ``_lib.jvp_trace`` against the output weights, as the exact divergence of the likelihood (``FcnFlow.trace``);
    otherwise Hutchinson's estimate, the mean over ``n_probes`` probe rows eps of eps^T (d raw / dy) eps through the backward
    launches of ``FcnFlow.vjp`` (probe k is ``likelihood.probes(hutchinson_type, P, D, seed + k, device)``).  mean(t), std(t) and the
    time label are evaluated in fp64 and rounded once, as in ``network_jacobians``; the [P]-sized combination is torch fp64 on the device.
    ``t`` defaults as in ``network_jacobians``.  Same refusals (``_network``); nothing reads the device back."""
    from . import likelihood
    net, eps = _network(model)
    _lib._dev(xs, "xs")
    D = net.state_size
    if xs.ndim != 2 or xs.shape[1] != D:
        raise RuntimeError(f"flipd: xs must be [P, {D}], got {tuple(xs.shape)}")
    if not exact and int(n_probes) < 1:
        raise ValueError(f"flipd: n_probes must be at least 1 for Hutchinson's estimate, got {n_probes}")
    if t is None:
        t = default_eps(sde) if eps is None else eps
    P, dev = xs.shape[0], xs.device
    if P == 0:
        return torch.empty(0, device=dev, dtype=torch.float64)
    with torch.no_grad():
        vec_t = torch.full((P,), float(t), device=dev, dtype=torch.float64)
        centre, std = sde.marginal_prob(xs.double(), vec_t)
        probe = None if exact else likelihood.probes(hutchinson_type, P, D, int(seed), dev)
        flow = likelihood.FcnFlow(net, sde, P, aug=1, exact=exact, eps=probe)
        flow.x32[:, :D] = centre.float()
        flow.x32[:, D] = (vec_t * (sde.N - 1)).float()
        raw = flow.forward()[:, :D].double()
        if exact:
            tr = flow.trace()
        else:
            tr = torch.zeros(P, device=dev, dtype=torch.float64)
            for k in range(int(n_probes)):
                if k:
                    flow.eps[:, :D] = likelihood.probes(hutchinson_type, P, D, int(seed) + k, dev)
                u = flow.vjp()
                tr += (flow.eps[:, :D].double() * u[:, :D].double()).sum(dim=1)
            tr /= int(n_probes)
        return D - std * tr + (raw * raw).sum(dim=1)
