"""GPU tests of csrc/ode.hip and of the device driver: each of the four kernels element-wise against numpy longdouble with a bound
counted from the kernel's own roundings ((terms + 1) 2^-53 sum |terms| for the fp64 outputs, 2^-24 |ref| more for the fp32 rows), outputs
NaN-filled between guard regions that must stay untouched, on both access paths (even pitches: 16-byte accesses; odd: scalar); the
driver with a linear right-hand side against scipy in both directions of time."""
import numpy as np
import pytest
import torch
from scipy import integrate

import ode_cases as oc
from id_diff_amd import _lib, ode

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 16
SENTINEL = -777.25
ids = lambda s: "x".join(map(str, s))


def guarded(rows, cols, pitch, dtype, lead=1, fill=np.nan):
    """(whole, view): a ``fill``-filled flat device buffer with GUARD elements before and after, and its [lead, rows, cols] view with row
    pitch ``pitch`` (lead = 1: [rows, cols])."""
    whole = torch.full((2 * GUARD + lead * rows * pitch,), fill, dtype=dtype, device=DEV)
    view = whole[GUARD:GUARD + lead * rows * pitch].view(lead, rows, pitch)[:, :, :cols]
    return whole, (view[0] if lead == 1 else view)


def put(view, a):
    view.copy_(torch.as_tensor(np.ascontiguousarray(a).reshape(tuple(view.shape))).to(view.dtype).to(DEV))
    return view


def untouched(whole, view, fill=np.nan):
    """Everything of ``whole`` outside ``view`` still holds the fill."""
    probe = torch.zeros_like(whole)
    lead = view.unsqueeze(0) if view.ndim == 2 else view
    inner = probe[GUARD:whole.numel() - GUARD].view(lead.shape[0], lead.shape[1], -1)
    inner[:, :, :lead.shape[2]] = 1
    mask = probe == 0
    rest = whole[mask]
    return bool(torch.isnan(rest).all()) if np.isnan(fill) else bool((rest == fill).all())


def pitches(W, even):
    p = (W + 1) // 2 * 2
    return p if even else p + 1


def problem(B, D, aug, even, seed=0):
    rng = np.random.default_rng([seed, B, D, aug])
    W = D + aug
    ld = pitches(W, even)
    y_w, y = guarded(B, W, ld, torch.float64)
    k_w, K = guarded(B, W, ld, torch.float64, lead=7)
    yn_w, y_new = guarded(B, W, ld, torch.float64)
    h = dict(y=rng.standard_normal((B, W)) * 2, K=rng.standard_normal((7, B, W)), y_new=rng.standard_normal((B, W)) * 2)
    put(y, h['y']); put(K, h['K']); put(y_new, h['y_new'])
    return h, dict(y=y, K=K, y_new=y_new, y_w=y_w, k_w=k_w, yn_w=yn_w, ld=ld)


# ---------------------------------------------------------------------------------------------- 1. rk_stage
@pytest.mark.parametrize("even", [True, False], ids=["vec", "scalar"])
@pytest.mark.parametrize("shape", oc.SHAPES, ids=ids)
def test_rk_stage_against_longdouble(shape, even):
    B, D, aug = shape
    h, d = problem(B, D, aug, even)
    W, kpad = D + aug, (D + 1 + 3) // 4 * 4 + 4
    worst = 0.0
    for ns in range(1, 7):
        c = [0.37 * a for a in (ode.A[ns][:ns] if ns < 6 else ode.B)]
        ref, bound = oc.stage_ref(h['y'], h['K'], c)
        for with_state in (False, True):
            x_w, x32 = guarded(B, kpad, kpad, torch.float32, fill=SENTINEL)
            o_w, out = guarded(B, W, d['ld'], torch.float64)
            _lib.rk_stage(d['y'], d['K'], c, x32, D, 38.5, y_out=out if with_state else None)
            got32 = x32.cpu().numpy()
            b32 = np.asarray(bound + oc.U32 * np.abs(ref), dtype=np.float64)[:, :D] + 2.0 ** -149
            worst = max(worst, float((np.abs(got32[:, :D].astype(np.longdouble) - ref[:, :D]) / b32).max()))
            assert np.all(got32[:, D] == np.float32(38.5))
            assert np.all(got32[:, D + 1:] == np.float32(SENTINEL))          # the pad columns beyond the label are never written
            assert untouched(x_w, x32, SENTINEL)
            if with_state:
                worst = max(worst, float((np.abs(out.cpu().numpy().astype(np.longdouble) - ref) / (bound + 2.0 ** -1074)).max()))
                assert untouched(o_w, out)
            else:
                assert bool(torch.isnan(o_w).all())
    # the inputs are read only
    assert np.array_equal(d['y'].cpu().numpy(), h['y']) and np.array_equal(d['K'].cpu().numpy(), h['K'])
    assert untouched(d['y_w'], d['y']) and untouched(d['k_w'], d['K'])
    print(f"rk_stage {shape} {'vec' if even else 'scalar'}: {worst:.3f} of the bound")
    assert worst <= 1.0


def test_rk_stage_in_place_and_without_stages():
    h, d = problem(5, 6, 1, True)
    x_w, x32 = guarded(5, 8, 8, torch.float32, fill=SENTINEL)
    _lib.rk_stage(d['y'], d['K'], [], x32, 6, 2.0)                          # ns = 0: the rows of y itself
    assert np.array_equal(x32.cpu().numpy()[:, :6], h['y'][:, :6].astype(np.float32))
    c = [0.1, -0.2, 0.3]
    ref, bound = oc.stage_ref(h['y'], h['K'], c)
    _lib.rk_stage(d['y'], d['K'], c, x32, 6, 2.0, y_out=d['y'])
    assert (np.abs(d['y'].cpu().numpy().astype(np.longdouble) - ref) <= bound).all() and untouched(d['y_w'], d['y'])


# ---------------------------------------------------------------------------------------------- 2. rk_error
@pytest.mark.parametrize("even", [True, False], ids=["even", "odd"])
@pytest.mark.parametrize("shape", [(s[0], s[1] + s[2]) for s in oc.SHAPES] + oc.REDUCE_SHAPES, ids=ids)
def test_rk_error_against_longdouble(shape, even):
    B, W = shape
    h, d = problem(B, W, 0, even, seed=1)
    e = [0.37 * v for v in ode.E]
    ws_w, ws = guarded(1, _lib.REDUCE_WS_DOUBLES, _lib.REDUCE_WS_DOUBLES, torch.float64)
    o_w, out = guarded(1, 1, 1, torch.float64)
    _lib.rk_error(d['K'], e, d['y'], d['y_new'], 1e-5, 1e-3, out=out.view(()), workspace=ws.view(-1))
    ref, bound = oc.error_ref(h['K'], e, h['y'], h['y_new'], 1e-5, 1e-3)
    got = float(out.cpu().view(-1)[0])
    print(f"rk_error {shape}: {abs(got - float(ref)) / bound:.3f} of the bound ({got:.6e})")
    assert abs(np.longdouble(got) - ref) <= bound
    assert untouched(ws_w, ws) and untouched(o_w, out)
    again = torch.zeros((), dtype=torch.float64, device=DEV)
    _lib.rk_error(d['K'], e, d['y'], d['y_new'], 1e-5, 1e-3, out=again)
    assert float(again) == got                                                # the same bits twice


# ---------------------------------------------------------------------------------------------- 3. flow_rhs
@pytest.mark.parametrize("even", [True, False], ids=["vec", "scalar"])
@pytest.mark.parametrize("shape", oc.SHAPES, ids=ids)
def test_flow_rhs_against_longdouble(shape, even):
    B, D, aug = shape
    rng = np.random.default_rng([2, B, D, aug])
    pitch = (D + 3) // 4 * 4 + (0 if even else 1)
    hx, hv, hu = (rng.standard_normal((B, D)).astype(np.float32) for _ in range(3))
    he = (rng.integers(0, 2, (B, D)) * 2 - 1).astype(np.float32)
    hq = rng.standard_normal(B)
    x32, v, u, eps = (put(guarded(B, D, pitch, torch.float32)[1], a) for a in (hx, hv, hu, he))
    q = torch.as_tensor(hq).to(DEV)
    a, b = -0.7134, 1.2971
    for kw, hkw in ((dict(eps=eps, u=u), dict(eps=he, u=hu)), (dict(q=q), dict(q=hq))) if aug else ((dict(), dict()),):
        k_w, Ks = guarded(B, D + aug, pitches(D + aug, even), torch.float64)
        _lib.flow_rhs(x32, v, a, b, Ks, D, aug, **kw)
        ref, bound = oc.rhs_ref(hx, hv, a, b, D, aug, **hkw)
        share = float((np.abs(Ks.cpu().numpy().astype(np.longdouble) - ref) / (bound + 2.0 ** -1074)).max())
        print(f"flow_rhs {shape} {'vec' if even else 'scalar'} {sorted(kw)}: {share:.3f} of the bound")
        assert share <= 1.0 and untouched(k_w, Ks)
        if aug:                                                               # the bound tells a missing a D term from a rounding
            assert (np.abs(oc.rhs_ref(hx, hv, a, b, D, aug, a_term=False, **hkw)[0] - ref) > bound)[:, D].all()


# ---------------------------------------------------------------------------------------------- 4. jvp_trace
@pytest.mark.parametrize("shape", oc.TRACE_SHAPES + [(2, 3, 6)], ids=ids)
def test_jvp_trace_against_longdouble(shape):
    P, D, H = shape
    rng = np.random.default_rng([3, P, D, H])
    ld = (H + 3) // 4 * 4
    hT, hW = rng.standard_normal((P, D, H)).astype(np.float32), rng.standard_normal((D, H)).astype(np.float32)
    t_w, T = guarded(D, H, ld, torch.float32, lead=P)                         # the pads of the tangent rows are NaN, as jvp_layer leaves them
    w_w, Wo = guarded(D, H, ld, torch.float32)
    put(T, hT); put(Wo, hW)
    o_w, out = guarded(1, P, P, torch.float64)
    _lib.jvp_trace(T, Wo, out=out.view(-1), P=P, D=D, N=H, ldt=ld, stride_t=D * ld, ldw=ld)
    ref, bound = oc.trace_ref(hT, hW)
    share = float((np.abs(out.cpu().numpy().reshape(-1).astype(np.longdouble) - ref) / bound).max())
    print(f"jvp_trace {shape}: {share:.3f} of the bound")
    assert share <= 1.0 and untouched(o_w, out) and untouched(t_w, T) and untouched(w_w, Wo)


# ---------------------------------------------------------------------------------------------- 5. nothing to do, and the refusals
def test_empty_batches_do_nothing():
    """B = 0 (P = 0): through the wrappers, and at the C entry points with valid pointers, nothing is launched or written."""
    y = torch.zeros(0, 7, dtype=torch.float64, device=DEV)
    K = torch.zeros(7, 0, 7, dtype=torch.float64, device=DEV)
    x32 = torch.zeros(0, 8, device=DEV)
    out = torch.full((), 3.0, dtype=torch.float64, device=DEV)
    _lib.rk_stage(y, K, [0.5], x32, 6, 1.0, y_out=y)
    _lib.rk_error(K, [1.0] * 7, y, y, 1e-5, 1e-5, out=out)
    _lib.flow_rhs(x32, x32, 1.0, 1.0, K[0], 6, 1, q=torch.zeros(0, dtype=torch.float64, device=DEV))
    _lib.jvp_trace(torch.zeros(0, 6, 16, device=DEV), torch.zeros(6, 16, device=DEV))
    d64 = torch.full((64,), np.nan, dtype=torch.float64, device=DEV)
    f32 = torch.full((64,), np.nan, dtype=torch.float32, device=DEV)
    lib, st, coef = _lib.lib(), _lib._stream(), (_lib.c_d * 7)(*([1.0] * 7))
    p64, p32 = d64.data_ptr(), f32.data_ptr()
    assert lib.idiff_rk_stage_f64(p64, 8, p64, 8, 0, coef, 6, p64, 8, p32, 8, 0, 6, 1, 1.0, st) == 0
    assert lib.idiff_rk_error_f64(p64, 8, 0, coef, p64, 8, p64, 8, 0, 7, 1e-5, 1e-5, p64, out.data_ptr(), st) == 0
    assert lib.idiff_flow_rhs_f64(p32, 8, p32, 8, 1.0, 1.0, p64, 8, 0, 6, 1, 0, 0, 0, 0, p64, st) == 0
    assert lib.idiff_jvp_trace_f64(p32, 16, 96, p32, 16, p64, 0, 6, 16, st) == 0
    assert float(out) == 3.0 and bool(torch.isnan(d64).all()) and bool(torch.isnan(f32).all())


# ---------------------------------------------------------------------------------------------- 6. the driver
@pytest.mark.parametrize("span", [(0.0, 2.0), (1.5, 0.25)], ids=["forward", "backward"])
@pytest.mark.parametrize("shape", [(5, 6, 1), (33, 7, 0)], ids=ids)
def test_driver_with_a_linear_right_hand_side_against_scipy(shape, span):
    B, D, aug = shape
    W = D + aug
    rng = np.random.default_rng([4, B, W])
    M = rng.standard_normal((W, W)) / np.sqrt(W) - 0.5 * np.eye(W)
    y0 = rng.standard_normal((B, W))
    Mt = torch.as_tensor(M.T.copy()).to(DEV)

    def rhs(stage, t, K, v):
        K[stage].copy_(v @ Mt * (1.0 + 0.5 * t))

    sol = integrate.solve_ivp(lambda t, v: ((v.reshape(B, W) @ M.T) * (1.0 + 0.5 * t)).reshape(-1), span, y0.reshape(-1), method='RK45',
                              rtol=1e-6, atol=1e-8)
    y = torch.zeros(B, pitches(W, True), dtype=torch.float64, device=DEV)[:, :W]
    y.copy_(torch.as_tensor(y0))
    x32 = torch.zeros(B, (D + 1 + 3) // 4 * 4, device=DEV)
    nfev, steps, rejected, norms = ode.rk45(rhs, span[0], span[1], y, x32, D, lambda t: 7.0 * t, rtol=1e-6, atol=1e-8)
    want = sol.y[:, -1].reshape(B, W)
    rel = float(np.abs(y.cpu().numpy() - want).max() / np.abs(want).max())
    print(f"driver {shape} {span}: nfev {nfev} (scipy {sol.nfev}), steps {steps} + {rejected} rejected, relative deviation {rel:.2e}")
    assert nfev == sol.nfev and steps == len(sol.t) - 1
    assert rel <= 1e-12
    assert np.array_equal(x32.cpu().numpy()[:, :D], want[:, :D].astype(np.float32)) or \
        np.abs(x32.cpu().numpy()[:, :D] - want[:, :D]).max() <= 2.0 ** -23 * np.abs(want).max()
    assert np.abs(x32.cpu().numpy()[:, D] - 7.0 * span[1]).max() <= 1e-5 and np.all(x32.cpu().numpy()[:, D + 1:] == 0)


def test_driver_guards_on_the_device():
    y = torch.ones(3, 2, dtype=torch.float64, device=DEV)
    x32 = torch.zeros(3, 4, device=DEV)

    def nan_rhs(stage, t, K, v):
        K[stage].copy_(v * float('nan') if t > 0.5 else v)
    with pytest.raises(RuntimeError, match=r"error norm is nan at t = .*h = "):
        ode.rk45(nan_rhs, 0.0, 1.0, y, x32, 2, float)
    with pytest.raises(RuntimeError, match=r"more than max_steps = 3 attempted steps at t = .*h = "):
        ode.rk45(lambda s, t, K, v: K[s].copy_(-30.0 * v), 0.0, 10.0, y.fill_(1.0), x32, 2, float, max_steps=3)
