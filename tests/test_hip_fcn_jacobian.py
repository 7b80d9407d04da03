"""The fcn Jacobian feature on the MI355X: both kernels of csrc/fcn_jacobian.hip element-wise against fp64 under the bounds of
tests/fcn_jacobian_cases.py (derived there, not fitted), the whole Jacobian against fp64 autograd under a bar measured in the test,
the tangent basis, the dimension a trained network reads, and that the sampled path has not moved."""
import os
import pickle

import numpy as np
import pytest
import torch

import fcn_jacobian_cases as cases
from id_diff_amd import _lib, dim_reduction, jacobian, main, sde_lib, train
from id_diff_amd.configs.utils import read_config
from id_diff_amd.lightning_modules import checkpoint_io
from id_diff_amd.models.fcn import FCN
from id_diff_amd.plot_utils import estimate_dim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_CONFIG = 'configs/dimension_estimation/paper/euclidean_data/ksphere/train_small.py'
GUARD = 64              # floats of NaN in front of and behind every output buffer
LAYER_CASES = [(s, 0, 0) for s in cases.LAYER_SHAPES] + [(cases.LAYER_PADDED, 12, 3)]
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"pad{v}"


def nan_blocks(data, ld, rows):
    """[P, r, c] -> device tensor [P, rows, ld] (rows >= r, ld >= c) that is NaN outside the data."""
    P, r, c = data.shape
    buf = np.full((P, rows, ld), np.nan, dtype=np.float32)
    buf[:, :r, :c] = data
    return torch.from_numpy(buf).to(DEV)


def guarded(P, rows, ld):
    """(flat NaN buffer with GUARD floats on either side, its [P, rows, ld] view behind the front guard)."""
    flat = torch.full((2 * GUARD + P * rows * ld,), float("nan"), device=DEV)
    return flat, flat[GUARD:GUARD + P * rows * ld].view(P, rows, ld)


def written_only_inside(flat, view, r, c):
    """The block [:, :r, :c] of the view is finite and every other float of the flat buffer is still NaN."""
    host = flat.cpu().numpy()
    P, rows, ld = view.shape
    body = host[GUARD:GUARD + P * rows * ld].reshape(P, rows, ld)
    mask = np.zeros_like(body, dtype=bool)
    mask[:, :r, :c] = True
    return (np.isfinite(body[mask]).all() and np.isnan(body[~mask]).all() and np.isnan(host[:GUARD]).all()
            and np.isnan(host[GUARD + P * rows * ld:]).all())


# ---------------------------------------------------------------------------------------------- 1. the layer kernel
@pytest.mark.parametrize("shape,extra,gap", LAYER_CASES, ids=_ids)
def test_jvp_layer_against_fp64(shape, extra, gap):
    P, R, N, K = shape
    A, W, act = cases.layer_case(P, R, N, K)
    lda, ldw, ld_act, ldc = (cases.tc.pad4(n) + extra for n in (K, K, N, N))
    a = nan_blocks(A, lda, R + gap)
    w = nan_blocks(W[None], ldw, N)[0]
    g = nan_blocks(act[None], ld_act, P)[0]
    geometry = dict(R=R, N=N, K=K, lda=lda, stride_a=(R + gap) * lda, ldw=ldw, ldc=ldc, stride_c=(R + gap) * ldc)
    for mask in (g, None):
        ref, bound = cases.layer_reference(A, W, None if mask is None else act)
        runs = []
        for _ in range(2):
            flat, c = guarded(P, R + gap, ldc)
            _lib.jvp_layer(a, w, act=mask, out=c, P=P, ld_act=None if mask is None else ld_act, **geometry)
            assert written_only_inside(flat, c, R, N)
            runs.append(c[:, :R, :N].cpu().numpy())
        s = cases.share(runs[0], ref, bound)
        print(f"jvp_layer {shape} pad {extra} act {mask is not None}: {s:.3f} of the bound")
        assert s <= 1.0
        assert np.array_equal(runs[0], runs[1])
        # a point alone is the point inside the batch, bit for bit
        p = min(1, P - 1)
        flat, c1 = guarded(1, R + gap, ldc)
        _lib.jvp_layer(a[p], w, act=None if mask is None else mask[p:p + 1], out=c1, P=1, ld_act=None if mask is None else ld_act, **geometry)
        assert written_only_inside(flat, c1, R, N)
        assert np.array_equal(c1[0, :R, :N].cpu().numpy(), runs[0][p])


def test_jvp_wrappers_take_tensors():
    """The 3-D / 2-D tensor form of both wrappers gives the bits of the explicit geometry."""
    P, R, N, K = 3, 8, 128, 128
    A, W, act = cases.layer_case(P, R, N, K)
    a, w, g = (torch.from_numpy(v).to(DEV) for v in (A, W, act))
    got = _lib.jvp_layer(a, w, act=g)
    want = torch.empty(P, R, N, device=DEV)
    _lib.jvp_layer(a, w, act=g, out=want, P=P, R=R, N=N, K=K, lda=K, stride_a=R * K, ldw=K, ld_act=N, ldc=N, stride_c=R * N)
    assert got.shape == (P, R, N) and torch.equal(got, want)
    s = cases.share(got.cpu().numpy(), *cases.layer_reference(A, W, act))
    assert s <= 1.0
    W1, act1 = cases.seed_case(3, 8, 128, 12)
    t = _lib.jvp_seed(torch.from_numpy(W1).to(DEV), torch.from_numpy(act1).to(DEV), D=8)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), cases.seed_reference(W1, act1, 8).view(np.uint32))
    with pytest.raises(RuntimeError, match="jvp_layer"):
        _lib.jvp_layer(a, w[:, :64].contiguous(), act=g)


# ---------------------------------------------------------------------------------------------- 2. the seed kernel
@pytest.mark.parametrize("shape", cases.SEED_SHAPES, ids=_ids)
def test_jvp_seed_is_bit_equal(shape):
    P, D, N, ldw = shape
    W1, act = cases.seed_case(P, D, N, ldw)                       # NaN from column D on: the time column and the pads
    ref = cases.seed_reference(W1, act, D)
    w = torch.from_numpy(W1).to(DEV)
    for extra, gap in ((0, 0), (8, 2)):
        ld_act = ldt = cases.tc.pad4(N) + extra
        g = nan_blocks(act[None], ld_act, P)[0]
        runs = []
        for _ in range(2):
            flat, t = guarded(P, D + gap, ldt)
            _lib.jvp_seed(w, g, out=t, P=P, D=D, N=N, ldw=ldw, ld_act=ld_act, ldt=ldt, stride_t=(D + gap) * ldt)
            assert written_only_inside(flat, t, D, N)
            runs.append(t[:, :D, :N].cpu().numpy())
        assert np.array_equal(runs[0].view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))


# ---------------------------------------------------------------------------------------------- 3. the whole Jacobian
def _network(D, H, L, kind):
    config = cases.net_config(D, H, L, 4, sde=kind)
    torch.manual_seed(0)
    model = FCN(config).to(DEV).eval()
    sde, eps = sde_lib.configure_sde(config)
    return model, sde, eps


@pytest.mark.parametrize("kind", cases.NET_SDES)
@pytest.mark.parametrize("shape", cases.NET_SHAPES, ids=_ids)
def test_network_jacobian_against_fp64_autograd(shape, kind):
    """Measured on an MI355X (shares of the bar, 8 x the fp32 CPU autograd error, over the 5 matrices): 0.07-0.15 at (8, 128, 2) and
    0.08-0.15 at (100, 256, 3), VE and VP alike; singular values within 2.4e-7 sigma_max of the fp64 SVD.  DESIGN.md 4.9."""
    D, H, L = shape
    model, sde, eps = _network(D, H, L, kind)
    xs = cases.net_points(D)
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    J64 = cases.autograd_jacobians(state, sde, xs, eps, torch.float64)
    bars = cases.measured_bars(cases.autograd_jacobians(state, sde, xs, eps, torch.float32), J64)
    J = jacobian.network_jacobians(model, sde, xs.to(DEV))
    assert J.shape == (cases.NET_POINTS, D, D) and J.dtype == torch.float32 and J.is_contiguous()
    err = cases.relative_errors(J.cpu().numpy(), J64)
    print(f"jacobian {shape} {kind}: error / max|J| {err.tolist()}, bars {bars.tolist()}, shares {np.round(err / bars, 3).tolist()}")
    assert (err <= bars).all()
    assert torch.equal(J, jacobian.network_jacobians(model, sde, xs.to(DEV), eps))          # the default t, and the same bits again
    sv = jacobian.jacobian_spectra(model, sde, xs.to(DEV))
    assert sv.shape == (cases.NET_POINTS, D) and sv.dtype == np.float64
    for s, j in zip(sv, J64):
        want = np.linalg.svd(j, compute_uv=False)
        print(f"  singular values: worst |dev - svd| / sigma_max = {np.abs(s - want).max() / want[0]:.3g}")
        assert np.abs(s - want).max() <= cases.SV_RTOL * want[0]
        assert (np.diff(s) <= 0).all()
    dims = jacobian.local_dims(model, sde, xs.to(DEV))
    assert dims.tolist() == [estimate_dim(list(s)) for s in sv]


def test_widths_that_are_no_multiple_of_four():
    """D = 6 and 30 hidden nodes: the rows of every buffer are padded to 16 bytes and the weights get zero pad columns."""
    D, H, L = 6, 30, 2
    model, sde, eps = _network(D, H, L, 'vesde')
    xs = cases.net_points(D)
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    J64 = cases.autograd_jacobians(state, sde, xs, eps, torch.float64)
    bars = cases.measured_bars(cases.autograd_jacobians(state, sde, xs, eps, torch.float32), J64)
    err = cases.relative_errors(jacobian.network_jacobians(model, sde, xs.to(DEV)).cpu().numpy(), J64)
    print(f"jacobian {(D, H, L)}: shares {np.round(err / bars, 3).tolist()}")
    assert (err <= bars).all()
    sv = jacobian.jacobian_spectra(model, sde, xs.to(DEV))
    for s, j in zip(sv, J64):
        want = np.linalg.svd(j, compute_uv=False)
        assert np.abs(s - want).max() <= cases.SV_RTOL * want[0]


def test_points_go_in_chunks(monkeypatch):
    D, H, L = cases.NET_SHAPES[0]
    model, sde, _ = _network(D, H, L, 'vesde')
    xs = cases.net_points(D, P=7).to(DEV)
    whole = jacobian.network_jacobians(model, sde, xs)
    monkeypatch.setattr(jacobian, "T_BYTES_PER_LAUNCH", 3 * 2 * 4 * D * H)      # three points a chunk
    assert torch.equal(jacobian.network_jacobians(model, sde, xs), whole)
    assert jacobian.network_jacobians(model, sde, xs[:0]).shape == (0, D, D)


# ---------------------------------------------------------------------------------------------- 5. a trained network
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """train_small after 8000 steps (2 s on an MI355X), as test_trained_network_reads_the_sphere_dimension trains it: (config, checkpoint)."""
    root = str(tmp_path_factory.mktemp("jacobian"))
    config = read_config(SMALL_CONFIG)
    config.device = DEV
    config.logging.log_path = root
    trainer, _ = train.train(config, log_path=root, n_iters=8000, log=None)
    assert trainer.global_step == 8000
    config.model.checkpoint_path = train.last_checkpoint_path(config, root)
    return config, root


def _driver_points(config):
    """The points get_manifold_dimension visits, and the module it evaluates (the same seeding, the same calls)."""
    torch.manual_seed(int(config.get('seed', 42)))
    DataModule, pl_module, _, _ = dim_reduction.setup_model(config)
    points = dim_reduction.collect_points(DataModule.train_dataloader(), dim_reduction._num_datapoints(config))
    return pl_module, torch.stack([x for x, _ in points]).float()


def test_trained_network_jacobian_reads_the_dimension(trained):
    config, root = trained
    info, dims = dim_reduction.get_manifold_dimension(config, return_svd=True, return_dims=True, method='jacobian')
    pl_module, xs = _driver_points(config)
    state = checkpoint_io.score_model_state_dict(checkpoint_io.load_checkpoint(config.model.checkpoint_path))
    J64 = cases.autograd_jacobians(state, pl_module.sde, xs, pl_module.sampling_eps, torch.float64)
    want_sv = [np.linalg.svd(j, compute_uv=False) for j in J64]
    want_dims = [estimate_dim(list(s)) for s in want_sv]
    for s, w in zip(info['singular_values'], want_sv):
        print("singular values:", " ".join(f"{v:.3f}" for v in s), "| fp64 autograd:", " ".join(f"{v:.3f}" for v in w))
    print("dims:", list(dims), "fp64 autograd:", want_dims)
    assert len(dims) == len(xs) >= 7 and [int(d) for d in dims] == want_dims
    for s, w in zip(info['singular_values'], want_sv):
        assert len(s) == len(w) and np.abs(np.asarray(s) - w).max() <= cases.SV_RTOL * w[0]
    assert all(int(d) == 2 for d, w in zip(dims, want_dims) if w == 2)
    # with tangent bases, and through the config key instead of the argument
    config['dim_estimation.method'] = 'jacobian'
    info2, dims2, tangent = dim_reduction.get_manifold_dimension(config, return_svd=True, return_dims=True, return_tangent=True)
    del config['dim_estimation']
    assert info2 == info and list(dims2) == list(dims) and len(tangent) == len(dims)
    for d, T in zip(dims, tangent):
        assert T is None or (T.dtype == np.float32 and T.shape == (xs.shape[1], d))


def test_main_writes_the_usual_pickle(trained):
    """The same config, as a pickle with dim_estimation.method = 'jacobian', through main.py --mode manifold_dimension; and the flag."""
    config, root = trained
    as_dict = train.plain(config)
    as_dict['dim_estimation'] = {'method': 'jacobian'}
    cfg_pkl = os.path.join(root, 'config.pkl')
    with open(cfg_pkl, 'wb') as f:
        pickle.dump(as_dict, f)
    main.main(["--config", cfg_pkl, "--mode", "manifold_dimension", "--log_name", "by_key"])
    with open(os.path.join(root, config.logging.log_name, 'svd', 'by_key.pkl'), 'rb') as f:
        info = pickle.load(f)
    want = dim_reduction.get_manifold_dimension(config, return_svd=True, method='jacobian')
    del as_dict['dim_estimation']
    with open(cfg_pkl, 'wb') as f:
        pickle.dump(as_dict, f)
    main.main(["--config", cfg_pkl, "--mode", "manifold_dimension", "--log_name", "by_flag", "--dim_method", "jacobian"])
    with open(os.path.join(root, config.logging.log_name, 'svd', 'by_flag.pkl'), 'rb') as f:
        assert pickle.load(f) == want
    assert list(info) == ['singular_values'] and info == want
    assert len(info['singular_values']) >= 7 and all(len(s) == 8 for s in info['singular_values'])


# ---------------------------------------------------------------------------------------------- 4. the tangent basis
def test_local_tangent_against_numpy(trained):
    config, _ = trained
    pl_module, xs = _driver_points(config)
    xs = xs.to(DEV)
    J = jacobian.network_jacobians(pl_module, pl_module.sde, xs).cpu().numpy().astype(np.float64)
    dims = jacobian.local_dims(pl_module, pl_module.sde, xs)
    exact = jacobian.local_tangent(pl_module, pl_module.sde, xs, dtype=np.float64)
    rounded = jacobian.local_tangent(pl_module, pl_module.sde, xs)
    served = 0
    for j, d, T, T32 in zip(J, dims, exact, rounded):
        _, k = dim_reduction.tangent_width(np.linalg.svd(j, compute_uv=False).tolist(), j.shape[0])
        if k is None:
            assert T is None and T32 is None
            continue
        served += 1
        _, vec = np.linalg.eigh(j.T @ j)                          # the Gram of the rows of J, ascending
        Q = vec[:, :k]
        sine = float(np.linalg.norm(T - Q @ (Q.T @ T), 2))
        print(f"d = {d}: sine(device, numpy) = {sine:.3e}; |T^T T - I| fp32 = {np.abs(T32.T @ T32 - np.eye(k)).max():.3e}")
        assert T.shape == T32.shape == (j.shape[0], k) and k == d and T32.dtype == np.float32
        assert sine <= 1e-9
        assert np.abs(T32.astype(np.float64).T @ T32.astype(np.float64) - np.eye(k)).max() <= 1e-6
    assert served >= 1


# ---------------------------------------------------------------------------------------------- 6. nothing else moved
def test_default_method_is_the_sampled_path_bit_for_bit(trained):
    config, _ = trained
    default = dim_reduction.get_manifold_dimension(config, return_svd=True, return_dims=True)
    named = dim_reduction.get_manifold_dimension(config, return_svd=True, return_dims=True, method='sampling')
    assert default[0] == named[0] and list(default[1]) == list(named[1])
    by_jacobian = dim_reduction.get_manifold_dimension(config, return_svd=True, method='jacobian')
    assert by_jacobian != default[0] and len(by_jacobian['singular_values']) == len(default[0]['singular_values'])


def test_jacobian_method_refusals_by_message(trained):
    config, _ = trained
    with pytest.raises(NotImplementedError, match="world size 2"):
        dim_reduction._jacobian_refused(config, 2)
    config['dim_estimation.shard'] = 'rows'
    try:
        with pytest.raises(NotImplementedError, match="shard = 'rows'"):
            dim_reduction.get_manifold_dimension(config, return_svd=True, method='jacobian')
    finally:
        del config['dim_estimation']
    other = read_config('configs/dimension_estimation/paper/image_data/MNIST/config.py')
    with pytest.raises(NotImplementedError, match="ddpm"):
        dim_reduction.get_manifold_dimension(other, return_svd=True, method='jacobian')


def test_no_host_synchronisation_inside_network_jacobians():
    """After one call (the network's pack and the SDE's cached scalars are in place) torch's synchronisation check stays silent."""
    D, H, L = cases.NET_SHAPES[0]
    for kind in cases.NET_SDES:
        model, sde, _ = _network(D, H, L, kind)
        xs = cases.net_points(D).to(DEV)
        first = jacobian.network_jacobians(model, sde, xs)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            again = jacobian.network_jacobians(model, sde, xs)
            G = jacobian._spectra_from(again)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(first, again) and bool(torch.isfinite(G).all())
