"""Host side of the fcn Jacobian feature (no GPU): the bounds of tests/fcn_jacobian_cases.py hold for a numpy fp32 restatement of both
kernels' order of operations on the GPU tests' shapes and a handful of wrong kernels leave them; the new entry points refuse bad
arguments before any device call; jacobian.py and the driver's method switch refuse what they do not serve before the GPU is touched."""
import os

import numpy as np
import pytest
import torch

import fcn_jacobian_cases as cases
from id_diff_amd import _lib, dim_reduction, jacobian, main, sde_lib
from id_diff_amd.configs.utils import read_config

SMALL_CONFIG = 'configs/dimension_estimation/paper/euclidean_data/ksphere/train_small.py'
MNIST_CONFIG = 'configs/dimension_estimation/paper/image_data/MNIST/config.py'


# ---------------------------------------------------------------------------------------------- bounds against the restated arithmetic
@pytest.mark.parametrize("shape", cases.LAYER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layer_bound_holds_for_the_restated_order(shape):
    A, W, act = cases.layer_case(*shape)
    for a in (act, None):
        ref, bound = cases.layer_reference(A, W, a)
        s = cases.share(cases.layer_restated(A, W, a), ref, bound)
        print(f"jvp_layer {shape} act {a is not None}: {s:.3f} of the bound")
        assert s <= 1.0


@pytest.mark.parametrize("shape", cases.SEED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seed_restatement_is_the_rounded_exact_product(shape):
    P, D, N, ldw = shape
    W1, act = cases.seed_case(P, D, N, ldw)
    got, ref = cases.seed_restated(W1, act, D), cases.seed_reference(W1, act, D)
    assert got.shape == (P, D, N) and np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_the_slope_at_zero_is_one_either_way():
    """a >= 0 instead of a > 0 is NOT a mutation: at a = 0 and a = -0.0 both branches give exactly 1."""
    a = np.array([0.0, -0.0, 1e-30, -1e-10], dtype=np.float32)
    other = np.where(a >= 0, np.float32(1.0), (a + np.float32(1.0)).astype(np.float32))
    assert np.array_equal(cases.slope32(a), other) and (cases.slope32(a) == 1.0).all()


def test_layer_mutations_leave_the_bound():
    P, R, N, K = cases.LAYER_PADDED
    A, W, act = cases.layer_case(P, R, N, K)
    ref, bound = cases.layer_reference(A, W, act)
    plain = cases.layer_restated(A, W, None)
    assert cases.share(plain * cases.slope32(act)[:, None, :], ref, bound) <= 1.0
    wrong_point = plain * cases.slope32(np.roll(act, 1, axis=0))[:, None, :]
    on_rows = plain * cases.slope32(act)[:, :R, None]
    no_factor = plain
    for name, got in (("g of another point", wrong_point), ("g on the rows", on_rows), ("no g", no_factor)):
        s = cases.share(got, ref, bound)
        print(f"{name}: {s:.3g} of the bound")
        assert s > 1.0, name


def test_seed_mutations_are_not_bit_equal():
    P, D, N, ldw = 3, 8, 8, 12
    W1, act = cases.seed_case(P, D, N, ldw)
    W1[:, D] = 0.25                                                    # a finite time column, so that reading it shows as a wrong number
    ref = cases.seed_reference(W1, act, D)
    assert np.array_equal(cases.seed_restated(W1, act, D), ref)
    transposed = np.ascontiguousarray(cases.seed_restated(W1, act, D).transpose(0, 2, 1))       # T[p][n, i] in the [i, n] buffer
    with_time = cases.seed_restated(W1[:, 1:], act, D)                 # columns 1 .. D: the time column is read
    wrong_point = cases.seed_restated(W1, np.roll(act, 1, axis=0), D)
    for name, got in (("transposed", transposed), ("time column", with_time), ("g of another point", wrong_point)):
        assert not np.array_equal(got, ref), name


@pytest.mark.parametrize("kind", cases.NET_SDES)
def test_whole_jacobian_restated_against_fp64_autograd(kind):
    """The pipeline of jacobian.network_jacobians, kernel by kernel in numpy fp32, meets the GPU test's measured bar on the small network;
    without the -1 / std, or with the time column in the seed, it does not."""
    D, H, L = cases.NET_SHAPES[0]
    config = cases.net_config(D, H, L, 4, sde=kind)
    from id_diff_amd.models.fcn import FCN
    torch.manual_seed(0)
    state = FCN(config).state_dict()
    sde, eps = sde_lib.configure_sde(config)
    xs = cases.net_points(D)
    J64 = cases.autograd_jacobians(state, sde, xs, eps, torch.float64)
    bars = cases.measured_bars(cases.autograd_jacobians(state, sde, xs, eps, torch.float32), J64)
    err = cases.relative_errors(cases.network_restated(state, sde, xs, eps), J64)
    print(f"{kind}: shares of the measured bar {np.round(err / bars, 3).tolist()} (bars {bars.tolist()})")
    assert (err <= bars).all()
    for mutate in ('no_scale', 'time_column'):
        bad = cases.relative_errors(cases.network_restated(state, sde, xs, eps, mutate=mutate), J64)
        assert (bad > bars).all(), mutate


# ---------------------------------------------------------------------------------------------- refusals of the C entry points
A16 = 0x10000            # fabricated, 16-byte aligned: never dereferenced, the launchers refuse first


def _seed(W1=A16, ldw=12, act=A16, ld_act=8, T=A16, ldt=8, strideT=64, P=2, D=8, N=8):
    return _lib.lib().idiff_jvp_seed_f32(W1, ldw, act, ld_act, T, ldt, strideT, P, D, N, None)


def _layer(A=A16, lda=8, strideA=64, W=A16, ldw=8, act=A16, ld_act=8, C=A16, ldc=8, strideC=64, P=2, R=8, N=8, K=8):
    return _lib.lib().idiff_jvp_layer_f32(A, lda, strideA, W, ldw, act, ld_act, C, ldc, strideC, P, R, N, K, None)


REFUSALS = [
    ("jvp_seed: ", lambda: _seed(W1=0)), ("jvp_seed: ", lambda: _seed(act=0)), ("jvp_seed: ", lambda: _seed(T=0)),
    ("jvp_seed: ", lambda: _seed(W1=A16 + 4)), ("jvp_seed: ", lambda: _seed(act=A16 + 8)), ("jvp_seed: ", lambda: _seed(T=A16 + 4)),
    ("jvp_seed: ", lambda: _seed(ldw=10)), ("jvp_seed: ", lambda: _seed(ldw=4)), ("jvp_seed: ", lambda: _seed(ld_act=4)),
    ("jvp_seed: ", lambda: _seed(ld_act=9)), ("jvp_seed: ", lambda: _seed(ldt=4)), ("jvp_seed: ", lambda: _seed(ldt=10)),
    ("jvp_seed: ", lambda: _seed(strideT=66)), ("jvp_seed: ", lambda: _seed(strideT=32)),
    ("jvp_seed: ", lambda: _seed(P=-1)), ("jvp_seed: ", lambda: _seed(D=0)), ("jvp_seed: ", lambda: _seed(N=-2)),
    ("jvp_layer: ", lambda: _layer(A=0)), ("jvp_layer: ", lambda: _layer(W=0)), ("jvp_layer: ", lambda: _layer(C=0)),
    ("jvp_layer: ", lambda: _layer(A=A16 + 4)), ("jvp_layer: ", lambda: _layer(W=A16 + 8)), ("jvp_layer: ", lambda: _layer(C=A16 + 4)),
    ("jvp_layer: ", lambda: _layer(act=A16 + 4)),
    ("jvp_layer: ", lambda: _layer(lda=4)), ("jvp_layer: ", lambda: _layer(lda=9)), ("jvp_layer: ", lambda: _layer(ldw=4)),
    ("jvp_layer: ", lambda: _layer(ldw=10)), ("jvp_layer: ", lambda: _layer(ldc=4)), ("jvp_layer: ", lambda: _layer(ldc=11)),
    ("jvp_layer: ", lambda: _layer(ld_act=4)), ("jvp_layer: ", lambda: _layer(ld_act=9)),
    ("jvp_layer: ", lambda: _layer(strideA=66)), ("jvp_layer: ", lambda: _layer(strideC=62)), ("jvp_layer: ", lambda: _layer(strideC=32)),
    ("jvp_layer: ", lambda: _layer(P=-1)), ("jvp_layer: ", lambda: _layer(R=0)), ("jvp_layer: ", lambda: _layer(N=0)),
    ("jvp_layer: ", lambda: _layer(K=-1)),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_jacobian_entry_points_refuse_before_any_device_call(case):
    prefix, call = REFUSALS[case]
    assert call() == 1001
    msg = _lib.lib().idiff_last_error().decode()
    assert msg.startswith(prefix), msg


def test_no_points_is_a_no_op_and_the_ok_query():
    assert _seed(P=0) == 0 and _layer(P=0) == 0                       # fabricated addresses: a launch would fault
    lib = _lib.lib()
    assert lib.idiff_jvp_layer_ok(1, 1, 1) == 1 and lib.idiff_jvp_layer_ok(100, 2048, 104) == 1
    assert lib.idiff_jvp_layer_ok(0, 1, 1) == 0 and lib.idiff_jvp_layer_ok(1, -1, 1) == 0 and lib.idiff_jvp_layer_ok(1, 1, 0) == 0
    assert _lib.jvp_layer_ok(100, 100, 2048) and not _lib.jvp_layer_ok(0, 1, 1)


def test_the_new_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "idiff_hip.h")).read()
    for name in ("idiff_jvp_seed_f32", "idiff_jvp_layer_f32", "idiff_jvp_layer_ok"):
        assert name in _lib.EXPORTED_SYMBOLS and name + "(" in header


# ---------------------------------------------------------------------------------------------- host logic
def test_jacobian_refuses_other_networks_and_dropout_before_any_device_call():
    config = read_config(SMALL_CONFIG)
    jacobian.check_config(config)
    config.model.dropout = 0.1
    with pytest.raises(NotImplementedError, match="dropout"):
        jacobian.check_config(config)
    with pytest.raises(NotImplementedError, match="dropout"):
        dim_reduction.get_manifold_dimension(config, return_svd=True, method='jacobian')
    with pytest.raises(NotImplementedError, match="ddpm"):
        jacobian.check_config(read_config(MNIST_CONFIG))
    # the same on model objects, on the CPU: nothing here has a device to touch
    from id_diff_amd.models.fcn import FCN
    sde, _ = sde_lib.configure_sde(config)
    xs = torch.zeros(2, 8)
    with pytest.raises(NotImplementedError, match="dropout"):
        jacobian.network_jacobians(FCN(config), sde, xs)
    with pytest.raises(NotImplementedError, match="Linear"):
        jacobian.local_dims(torch.nn.Linear(8, 8), sde, xs)


def test_method_switch():
    config = read_config(SMALL_CONFIG)
    assert dim_reduction.estimation_method(config) == 'sampling'
    config['dim_estimation.method'] = 'jacobian'
    assert dim_reduction.estimation_method(config) == 'jacobian'
    assert dim_reduction.estimation_method(config, 'sampling') == 'sampling'          # the argument wins
    with pytest.raises(ValueError, match="bogus"):
        dim_reduction.estimation_method(config, 'bogus')
    with pytest.raises(ValueError, match="bogus"):
        dim_reduction.get_manifold_dimension(config, return_svd=True, method='bogus')
    config['dim_estimation.method'] = 'nonsense'
    with pytest.raises(ValueError, match="nonsense"):
        dim_reduction.get_manifold_dimension(config, return_svd=True)


def test_jacobian_method_is_a_one_rank_mode():
    config = read_config(SMALL_CONFIG)
    dim_reduction._jacobian_refused(config, 1)
    with pytest.raises(NotImplementedError, match="world size 2"):
        dim_reduction._jacobian_refused(config, 2)
    config['dim_estimation.shard'] = 'rows'
    with pytest.raises(NotImplementedError, match="shard = 'rows'"):
        dim_reduction._jacobian_refused(config, 1)
    with pytest.raises(NotImplementedError, match="shard = 'rows'"):
        dim_reduction.get_manifold_dimension(config, return_svd=True, method='jacobian')


def test_dim_method_flag_sets_the_config_key():
    flags = main.parse(["--config", SMALL_CONFIG, "--mode", "manifold_dimension", "--dim_method", "jacobian"])
    assert flags.dim_method == "jacobian"
    assert main.parse(["--config", SMALL_CONFIG, "--mode", "manifold_dimension"]).dim_method is None
    with pytest.raises(SystemExit):
        main.parse(["--config", SMALL_CONFIG, "--mode", "manifold_dimension", "--dim_method", "bogus"])


def test_dims_from_spectra_uses_the_drivers_rule():
    from id_diff_amd.plot_utils import estimate_dim
    sv = np.array([[10.0, 9.0, 8.5, 0.5, 0.2, 0.1], [5.0, 4.0, 0.3, 0.2, 0.1, 0.05]])
    assert jacobian.dims_from_spectra(sv).tolist() == [estimate_dim(list(s)) for s in sv]
    assert jacobian.dims_from_spectra(np.ones((2, 2))).tolist() == [-1, -1]
