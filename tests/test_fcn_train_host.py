"""Host side of the fcn training feature (no GPU): the bounds of tests/fcn_train_cases.py hold for a numpy fp32 restatement of each
kernel's order of operations on the GPU tests' shapes; the new entry points refuse bad arguments before any device call; the warm-up
schedule, the checkpoint layout and the argument handling of ``--mode train``."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fcn_train_cases as cases
from id_diff_amd import _lib, main, train
from id_diff_amd.configs.utils import read_config
from id_diff_amd.lightning_modules import checkpoint_io

SMALL_CONFIG = 'configs/dimension_estimation/paper/euclidean_data/ksphere/train_small.py'


# ---------------------------------------------------------------------------------------------- bounds against the restated arithmetic
@pytest.mark.parametrize("kind", ["nn", "tn"])
@pytest.mark.parametrize("shape", cases.GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_contraction_bound_holds_for_the_restated_order(kind, shape):
    A, Bm, P = cases.gemm_case(kind, *shape)
    if kind == "nn":
        ref, bound = cases.gemm_reference(kind, A, Bm, P)
        got = cases.gemm_restated(kind, A, Bm, P)
        plain_ref, plain_bound = cases.gemm_reference(kind, A, Bm)
        share = max(float((np.abs(got - ref) / bound).max()),
                    float((np.abs(cases.gemm_restated(kind, A, Bm) - plain_ref) / plain_bound).max()))
    else:
        ref, bound, cref, cbound = cases.gemm_reference(kind, A, Bm)
        got, cs = cases.gemm_restated(kind, A, Bm)
        share = float((np.abs(got - ref) / bound).max())
        cshare = float((np.abs(cs - cref) / cbound).max())
        print(f"colsum {shape}: {cshare:.3f} of the bound")
        assert cshare <= 1.0
    print(f"gemm_{kind} {shape}: {share:.3f} of the bound")
    assert share <= 1.0


@pytest.mark.parametrize("reduce_mean", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B", cases.LOSS_B)
@pytest.mark.parametrize("D", cases.LOSS_D)
def test_loss_bounds_hold_for_the_restated_order(B, D, weighted, reduce_mean):
    out, z, w = cases.loss_case(B, D, weighted)
    loss, G = cases.loss_reference(out, z, w, reduce_mean)
    got_loss, got_G = cases.loss_restated(out, z, w, reduce_mean)
    gshare = float((np.abs(got_G - G) / np.maximum(4 * cases.U * np.abs(G), 1e-300)).max())
    lshare = abs(float(got_loss) - loss) / (2.0 ** -23 * abs(loss))
    print(f"loss B={B} D={D}: G {gshare:.3f}, loss {lshare:.3f} of the bound")
    assert gshare <= 1.0 and lshare <= 1.0


@pytest.mark.parametrize("name", sorted(cases.ADAM_CASES))
@pytest.mark.parametrize("n", cases.ADAM_N)
def test_adam_bounds_hold_for_the_restated_order(n, name):
    """The kernel's arithmetic IS the fp64 update rounded once; what is checked is that the rounding of the outputs fits the bounds."""
    _, max_norm, wd, warmup = cases.ADAM_CASES[name]
    theta, grad = cases.adam_case(n, name)
    st = (theta.astype(np.float64), np.zeros(n), np.zeros(n))
    worst = 0.0
    for k in range(cases.ADAM_STEPS):
        lr = cases.warmup_lr(cases.ADAM_LR, k, warmup)
        inp = tuple(a.astype(np.float32) for a in st)
        target = cases.adam_update(*inp, grad, k + 1, lr, max_norm, wd)
        got = tuple(a.astype(np.float32) for a in target)
        for g, t, b in zip(got, target, cases.adam_bounds(inp[0], *target)):
            worst = max(worst, float((np.abs(g.astype(np.float64) - t) / b).max()))
        if k == 0 and warmup > 0:
            assert np.array_equal(got[0], inp[0])                  # lr 0: theta does not move
        st = cases.adam_update(*st, grad, k + 1, lr, max_norm, wd)
    print(f"adam n={n} {name}: {worst:.3f} of the bound")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------- refusals
A16 = 0x10000            # fabricated, 16-byte aligned: never dereferenced, the launchers refuse first


def _nn(A=A16, lda=8, Bm=A16, ldb=8, C=A16, ldc=8, P=0, ldp=0, M=4, N=8, K=8):
    return _lib.lib().idiff_gemm_nn_f32(A, lda, Bm, ldb, C, ldc, P, ldp, M, N, K, None)


def _tn(At=A16, lda=8, Bm=A16, ldb=8, C=A16, ldc=8, cs=0, M=8, N=8, K=4):
    return _lib.lib().idiff_gemm_tn_f32(At, lda, Bm, ldb, C, ldc, cs, M, N, K, None)


def _loss(out=A16, z=A16, w=0, G=A16, ldg=8, loss=A16, ws=A16, B=4, D=8):
    return _lib.lib().idiff_dsm_loss_grad_f32(out, z, w, G, ldg, loss, ws, B, D, 1, None)


def _adam(theta=A16, grad=A16, m=A16, v=A16, n=8, sumsq=0, max_norm=1.0, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, step=1):
    return _lib.lib().idiff_adam_step_f32(theta, grad, m, v, n, sumsq, max_norm, lr, b1, b2, eps, wd, step, None)


REFUSALS = [
    ("gemm_nn: ", lambda: _nn(A=0)), ("gemm_nn: ", lambda: _nn(Bm=0)), ("gemm_nn: ", lambda: _nn(C=0)),
    ("gemm_nn: ", lambda: _nn(A=A16 + 4)), ("gemm_nn: ", lambda: _nn(C=A16 + 8)), ("gemm_nn: ", lambda: _nn(P=A16 + 4, ldp=8)),
    ("gemm_nn: ", lambda: _nn(M=0)), ("gemm_nn: ", lambda: _nn(N=-1)), ("gemm_nn: ", lambda: _nn(K=0)),
    ("gemm_nn: ", lambda: _nn(lda=4)), ("gemm_nn: ", lambda: _nn(ldb=6)), ("gemm_nn: ", lambda: _nn(ldc=9)),
    ("gemm_nn: ", lambda: _nn(P=A16, ldp=4)),
    ("gemm_tn: ", lambda: _tn(At=0)), ("gemm_tn: ", lambda: _tn(Bm=0)), ("gemm_tn: ", lambda: _tn(C=0)),
    ("gemm_tn: ", lambda: _tn(Bm=A16 + 4)), ("gemm_tn: ", lambda: _tn(cs=A16 + 2)),
    ("gemm_tn: ", lambda: _tn(M=0)), ("gemm_tn: ", lambda: _tn(N=0)), ("gemm_tn: ", lambda: _tn(K=-3)),
    ("gemm_tn: ", lambda: _tn(lda=4)), ("gemm_tn: ", lambda: _tn(ldb=10)), ("gemm_tn: ", lambda: _tn(ldc=4)),
    ("dsm_loss_grad: ", lambda: _loss(out=0)), ("dsm_loss_grad: ", lambda: _loss(z=0)), ("dsm_loss_grad: ", lambda: _loss(loss=0)),
    ("dsm_loss_grad: ", lambda: _loss(ws=0)), ("dsm_loss_grad: ", lambda: _loss(ws=A16 + 4)), ("dsm_loss_grad: ", lambda: _loss(B=0)),
    ("dsm_loss_grad: ", lambda: _loss(D=0)), ("dsm_loss_grad: ", lambda: _loss(ldg=4)), ("dsm_loss_grad: ", lambda: _loss(G=A16 + 1)),
    ("grad_sumsq: ", lambda: _lib.lib().idiff_grad_sumsq_f32(0, 8, A16, A16, None)),
    ("grad_sumsq: ", lambda: _lib.lib().idiff_grad_sumsq_f32(A16, 0, A16, A16, None)),
    ("grad_sumsq: ", lambda: _lib.lib().idiff_grad_sumsq_f32(A16, 8, A16, A16 + 4, None)),
    ("adam_step: ", lambda: _adam(theta=0)), ("adam_step: ", lambda: _adam(grad=0)), ("adam_step: ", lambda: _adam(m=0)),
    ("adam_step: ", lambda: _adam(v=0)), ("adam_step: ", lambda: _adam(n=0)), ("adam_step: ", lambda: _adam(step=0)),
    ("adam_step: ", lambda: _adam(b1=1.0)), ("adam_step: ", lambda: _adam(lr=-1.0)), ("adam_step: ", lambda: _adam(sumsq=A16, max_norm=0.0)),
    ("adam_step: ", lambda: _adam(sumsq=A16 + 4)),
    ("fcn_train_input: ", lambda: _lib.lib().idiff_fcn_train_input_f32(0, A16, A16, 0, A16, A16, 4, 5, 8, None)),
    ("fcn_train_input: ", lambda: _lib.lib().idiff_fcn_train_input_f32(A16, A16, A16, 0, A16, A16, 4, 8, 8, None)),
    ("fcn_train_input: ", lambda: _lib.lib().idiff_fcn_train_input_f32(A16, A16, A16, 0, A16, A16, 0, 5, 8, None)),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_training_entry_points_refuse_before_any_device_call(case):
    prefix, call = REFUSALS[case]
    assert call() == 1001
    msg = _lib.lib().idiff_last_error().decode()
    assert msg.startswith(prefix), msg


def test_ok_queries():
    lib = _lib.lib()
    assert lib.idiff_gemm_nn_ok(1, 1, 1) == 1 and lib.idiff_gemm_tn_ok(500, 2048, 100) == 1
    assert lib.idiff_gemm_nn_ok(0, 1, 1) == 0 and lib.idiff_gemm_tn_ok(1, 1, -1) == 0


# ---------------------------------------------------------------------------------------------- host logic
def test_warmup_schedule():
    assert train.warmup_lr(1e-3, 0, 5) == 0.0                       # the first step has lr 0, as LambdaLR(lambda s: min(s / w, 1))
    assert train.warmup_lr(1e-3, 2, 5) == pytest.approx(4e-4, rel=1e-15)
    assert train.warmup_lr(1e-3, 5, 5) == 1e-3 and train.warmup_lr(1e-3, 10 ** 9, 5) == 1e-3
    assert train.warmup_lr(1e-3, 0, 0) == 1e-3
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: min(s / 5, 1.0))
    for s in range(8):
        assert opt.param_groups[0]['lr'] == pytest.approx(train.warmup_lr(1e-3, s, 5), rel=1e-15, abs=0)
        opt.step(); sched.step()


def test_stream_keys_differ_and_repeat():
    keys = {train.stream_key(42, i, s) for i in range(100) for s in range(4)}
    assert len(keys) == 400 and all(0 <= k < 2 ** 63 for k in keys)
    assert train.stream_key(42, 7, 1) == train.stream_key(42, 7, 1) != train.stream_key(43, 7, 1)


def test_checkpoint_round_trips_with_weights_only(tmp_path):
    config = read_config(SMALL_CONFIG)
    from id_diff_amd.models.fcn import FCN
    model = FCN(config)
    n = sum(p.numel() for p in model.parameters())
    m, v = torch.arange(n, dtype=torch.float32), torch.ones(n)
    path = str(tmp_path / "checkpoints" / "last.ckpt")
    train.write_checkpoint(path, train.checkpoint_dict(model.state_dict(), config, 17, 2, m, v))
    raw = torch.load(path, map_location="cpu", weights_only=True)        # no foreign class anywhere in the file
    assert raw['global_step'] == 17 and raw['epoch'] == 2
    ckpt = checkpoint_io.load_checkpoint(path)
    state = checkpoint_io.score_model_state_dict(ckpt)
    assert list(state) == list(model.state_dict()) == [f"mlp.{i}.{p}" for i in (0, 3, 6, 9) for p in ("weight", "bias")]
    for k, t in model.state_dict().items():
        assert torch.equal(state[k], t)
    assert torch.equal(ckpt['optimizer_states'][0]['m'], m) and torch.equal(ckpt['optimizer_states'][0]['v'], v)
    cfg = ckpt['hyper_parameters']['config']
    assert type(cfg) is dict and cfg['model']['hidden_nodes'] == 128 and cfg['optim']['warmup'] == 100
    again = FCN(config)
    again.load_state_dict(state, strict=True)


def test_scope_checks():
    config = read_config(SMALL_CONFIG)
    train.check_scope(config)
    config.model.dropout = 0.1
    with pytest.raises(NotImplementedError, match="model.dropout"):
        train.check_scope(config)
    config.model.dropout = 0.0
    config.model.name = 'ddpm'
    with pytest.raises(SystemExit, match="fcn"):
        train.check_scope(config)


def test_mode_train_argument_handling():
    flags = main.parse(["--config", SMALL_CONFIG, "--mode", "train", "--n_iters", "1e20", "--log_every=50", "--checkpoint_every", "1000"])
    assert flags.n_iters == 1e20 and flags.log_every == 50 and flags.checkpoint_every == 1000
    with pytest.raises(SystemExit, match="one GPU"):
        main.main(["--config", SMALL_CONFIG, "--mode", "train", "--n_iters", "5", "--gpus", "2"])
    with pytest.raises(SystemExit, match="--n_iters"):
        main.main(["--config", SMALL_CONFIG, "--mode", "train"])
    with pytest.raises(SystemExit, match="fcn"):
        main.main(["--config", "configs/dimension_estimation/paper/image_data/MNIST/config.py", "--mode", "train", "--n_iters", "5"])
    with pytest.raises(SystemExit, match="outside the scope"):
        main.main(["--config", SMALL_CONFIG, "--mode", "sample"])


def test_last_checkpoint_path():
    config = read_config(SMALL_CONFIG)
    assert train.last_checkpoint_path(config, "/x", None) == os.path.join("/x", "2-sphere-small", "checkpoints", "last.ckpt")
    assert train.last_checkpoint_path(config, "/x", "run") == os.path.join("/x", "run", "checkpoints", "last.ckpt")
