"""Training the fcn score network on the MI355X: every new kernel element by element against fp64 under the bounds of
tests/fcn_train_cases.py, the whole network's gradients and a 20-step trajectory against fp64 torch on the CPU (bars measured from
fp32 torch on the CPU), bit-exact determinism and resume, the entry points, and the one test that ties training to the estimator:
a network trained here on a 2-sphere in R^8 makes ``get_manifold_dimension`` read 2 at every point.

Measured on an MI355X (share of each bound / bar used, worst case over the parametrisation): DESIGN.md 4.7.
"""
import os

import numpy as np
import pytest
import torch

import fcn_train_cases as cases
from id_diff_amd import _lib, dim_reduction, main, train
from id_diff_amd.configs.utils import read_config
from id_diff_amd.lightning_modules import checkpoint_io

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_CONFIG = 'configs/dimension_estimation/paper/euclidean_data/ksphere/train_small.py'
GEMM_CASES = [(s, 0) for s in cases.GEMM_SHAPES] + [(cases.GEMM_PADDED, 12)]


def dev_padded(a, extra=0):
    """The device copy of ``a`` with rows padded to 16 bytes (+ ``extra`` floats), NaN in the pad; returns (the [rows, cols] view, ld)."""
    buf, ld = cases.padded(a, extra)
    t = torch.from_numpy(buf).to(DEV)
    return t[:, :a.shape[1]], ld


def share(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref) / bound).max())


# ---------------------------------------------------------------------------------------------- 1. contractions
@pytest.mark.parametrize("shape,extra", GEMM_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"pad{v}")
def test_gemm_nn_against_fp64(shape, extra):
    M, N, K = shape
    A, Bm, P = cases.gemm_case("nn", M, N, K)
    a, lda = dev_padded(A, extra)
    b, ldb = dev_padded(Bm, extra)
    p, ldp = dev_padded(P, extra)
    for mask in (None, p):
        ref, bound = cases.gemm_reference("nn", A, Bm, None if mask is None else P)
        runs = []
        for _ in range(2):
            c, ldc = dev_padded(np.zeros((M, N), dtype=np.float32), extra)
            _lib.gemm_nn(a, b, out=c, elu_out=mask, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, ldp=ldp)
            full = c.cpu().numpy()
            runs.append(full)
        s = share(runs[0], ref, bound)
        print(f"gemm_nn {shape} pad {extra} mask {mask is not None}: {s:.3f} of the bound")
        assert s <= 1.0
        assert np.array_equal(runs[0], runs[1])


@pytest.mark.parametrize("shape,extra", GEMM_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"pad{v}")
def test_gemm_tn_against_fp64(shape, extra):
    M, N, K = shape
    At, Bm, _ = cases.gemm_case("tn", M, N, K)
    a, lda = dev_padded(At, extra)
    b, ldb = dev_padded(Bm, extra)
    ref, bound, cref, cbound = cases.gemm_reference("tn", At, Bm)
    runs = []
    for with_colsum in (True, True, False):
        c, ldc = dev_padded(np.zeros((M, N), dtype=np.float32), extra)
        cs = torch.full((M,), float("nan"), device=DEV) if with_colsum else None
        _lib.gemm_tn(a, b, out=c, colsum=cs, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc)
        runs.append((c.cpu().numpy(), None if cs is None else cs.cpu().numpy()))
    s, sc = share(runs[0][0], ref, bound), share(runs[0][1], cref, cbound)
    print(f"gemm_tn {shape} pad {extra}: {s:.3f} of the bound, colsum {sc:.3f}")
    assert s <= 1.0 and sc <= 1.0
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][0], runs[2][0])            # the column sums do not touch the product


def test_gemm_outputs_stay_inside_their_rows():
    """The pad of C (columns N .. ldc) and the rows after M are not written."""
    M, N, K = cases.GEMM_PADDED
    A, Bm, P = cases.gemm_case("nn", M, N, K)
    a, lda = dev_padded(A); b, ldb = dev_padded(Bm)
    ldc = cases.pad4(N) + 8
    buf = torch.full((M + 3, ldc), 7.0, device=DEV)
    _lib.gemm_nn(a, b, out=buf[:M, :N], M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc)
    got = buf.cpu().numpy()
    assert (got[:M, N:] == 7.0).all() and (got[M:] == 7.0).all() and not (got[:M, :N] == 7.0).any()
    At, Bm2, _ = cases.gemm_case("tn", M, N, K)
    a2, lda2 = dev_padded(At); b2, ldb2 = dev_padded(Bm2)
    buf.fill_(7.0)
    cs = torch.full((M + 5,), 7.0, device=DEV)
    _lib.gemm_tn(a2, b2, out=buf[:M, :N], colsum=cs[:M], M=M, N=N, K=K, lda=lda2, ldb=ldb2, ldc=ldc)
    got = buf.cpu().numpy()
    assert (got[:M, N:] == 7.0).all() and (got[M:] == 7.0).all() and (cs[M:] == 7.0).all().item()


# ---------------------------------------------------------------------------------------------- 2. loss
@pytest.mark.parametrize("reduce_mean", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B", cases.LOSS_B)
@pytest.mark.parametrize("D", cases.LOSS_D)
def test_dsm_loss_grad_against_fp64(B, D, weighted, reduce_mean):
    out, z, w = cases.loss_case(B, D, weighted)
    ref_loss, ref_G = cases.loss_reference(out, z, w, reduce_mean)
    o, zz = torch.from_numpy(out).to(DEV), torch.from_numpy(z).to(DEV)
    ww = None if w is None else torch.from_numpy(w).to(DEV)
    loss, G = _lib.dsm_loss_grad(o, zz, weight=ww, reduce_mean=reduce_mean)
    loss2, G2 = _lib.dsm_loss_grad(o, zz, weight=ww, reduce_mean=reduce_mean)
    eval_loss, none = _lib.dsm_loss_grad(o, zz, weight=ww, reduce_mean=reduce_mean, want_grad=False)      # null G
    gs = float((np.abs(G.cpu().numpy().astype(np.float64) - ref_G) / np.maximum(4 * cases.U * np.abs(ref_G), 1e-300)).max())
    ls = abs(float(loss) - ref_loss) / (2.0 ** -23 * abs(ref_loss))
    print(f"dsm_loss_grad B={B} D={D} weighted={weighted} reduce_mean={reduce_mean}: G {gs:.3f}, loss {ls:.3f} of the bound")
    assert gs <= 1.0 and ls <= 1.0
    assert none is None and float(eval_loss) == float(loss) == float(loss2) and torch.equal(G, G2)


# ---------------------------------------------------------------------------------------------- 3. Adam
@pytest.mark.parametrize("name", sorted(cases.ADAM_CASES))
@pytest.mark.parametrize("n", cases.ADAM_N)
def test_adam_step_against_fp64(n, name):
    _, max_norm, wd, warmup = cases.ADAM_CASES[name]
    theta0, grad = cases.adam_case(n, name)
    g = torch.from_numpy(grad).to(DEV)
    st = (theta0.astype(np.float64), np.zeros(n), np.zeros(n))
    worst = 0.0
    for k in range(cases.ADAM_STEPS):
        lr = cases.warmup_lr(cases.ADAM_LR, k, warmup)
        inp = tuple(a.astype(np.float32) for a in st)
        target = cases.adam_update(*inp, grad, k + 1, lr, max_norm, wd)
        th, m, v = (torch.from_numpy(a.copy()).to(DEV) for a in inp)
        sumsq = _lib.grad_sumsq(g) if max_norm is not None else None
        _lib.adam_step(th, g, m, v, k + 1, train.warmup_lr(cases.ADAM_LR, k, warmup), betas=cases.ADAM_BETAS, eps=cases.ADAM_EPS,
                       weight_decay=wd, sumsq=sumsq, max_norm=max_norm or 0.0)
        got = (th.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy())
        for a, t, b in zip(got, target, cases.adam_bounds(inp[0], *target)):
            worst = max(worst, share(a, t, b))
        if lr == 0.0:
            assert np.array_equal(got[0], inp[0])
        assert torch.equal(g, torch.from_numpy(grad).to(DEV))          # the gradient is read, not clipped in place
        st = cases.adam_update(*st, grad, k + 1, lr, max_norm, wd)
    print(f"adam n={n} {name}: {worst:.3f} of the bound")
    assert worst <= 1.0


def test_grad_sumsq_is_fixed_order_fp64():
    x = torch.randn(2 ** 20 + 3, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    a, b = _lib.grad_sumsq(x), _lib.grad_sumsq(x)
    ref = float((x.cpu().double() ** 2).sum())
    assert float(a) == float(b) and abs(float(a) - ref) <= 1e-12 * ref


# ---------------------------------------------------------------------------------------------- 4. whole-network gradients
@pytest.mark.parametrize("mode", sorted(cases.NET_MODES))
@pytest.mark.parametrize("shape", cases.NET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_network_gradients_against_fp64_autograd(shape, mode):
    D, H, L, B = shape
    sde, lw = cases.NET_MODES[mode]
    config = cases.net_config(D, H, L, B, sde=sde, likelihood_weighting=lw)
    trainer = train.FcnTrainer(config, DEV)
    x, t, z = cases.batch(D, B, seed=11)
    xd, td, zd = x.to(DEV), t.to(DEV), z.to(DEV)
    loss = float(trainer.loss_and_grad(xd, td, zd))
    state = {k: v.detach().cpu().clone() for k, v in trainer.state_dict().items()}
    terms = cases.sde_terms_for_reference(trainer, td)
    loss64, g64 = cases.torch_grads(state, x, t, z, terms, lw, False, torch.float64)
    _, g32 = cases.torch_grads(state, x, t, z, terms, lw, False, torch.float32)
    got = {}
    for i, idx in enumerate(sorted({int(k.split('.')[1]) for k in state})):
        got[f'mlp.{idx}.weight'] = trainer.gW[i][:, :trainer.layers[i]['k']].cpu().double()
        got[f'mlp.{idx}.bias'] = trainer.gb[i].cpu().double()
        assert not trainer.gW[i][:, trainer.layers[i]['k']:].any().item()          # pad columns: zero gradient
    worst = 0.0
    for k in state:
        bar = max(cases.NET_FACTOR * float((g32[k] - g64[k]).abs().max()), cases.NET_FLOOR * float(g64[k].abs().max()))
        err = float((got[k] - g64[k]).abs().max())
        ratio = err / max(float((g32[k] - g64[k]).abs().max()), 1e-300)
        worst = max(worst, err / bar)
        print(f"{shape} {mode} {k}: err {err:.3e} = {ratio:.2f} x torch fp32 CPU, {err / bar:.3f} of the bar")
        assert err <= bar, k
    lrel = abs(loss - loss64) / abs(loss64)
    print(f"{shape} {mode}: loss rel err {lrel:.3e}, worst gradient share {worst:.3f}")
    assert lrel <= cases.LOSS_RTOL


# ---------------------------------------------------------------------------------------------- 5. trajectory
def _explicit_batches(D, B, steps):
    return [cases.batch(D, B, seed=100 + i) for i in range(steps)]


def test_trajectory_against_fp64_torch():
    D, H, L, B = cases.TRAJ_SHAPE
    steps = 20
    config = cases.net_config(D, H, L, B, lr=1e-3, warmup=5, grad_clip=1.0)
    trainer = train.FcnTrainer(config, DEV)
    state = {k: v.detach().cpu().clone() for k, v in trainer.state_dict().items()}
    batches = _explicit_batches(D, B, steps)
    terms = [cases.sde_terms_for_reference(trainer, t.to(DEV)) for _, t, _ in batches]
    losses = []
    for x, t, z in batches:
        losses.append(trainer.step(x.to(DEV), t.to(DEV), z.to(DEV)).clone())
    got = [float(v) for v in losses]
    ref64 = cases.torch_trajectory(state, batches, terms, config, torch.float64, steps)
    ref32 = cases.torch_trajectory(state, batches, terms, config, torch.float32, steps)
    worst = 0.0
    for i in range(steps):
        bar = max(cases.NET_FACTOR * abs(ref32[i] - ref64[i]), cases.LOSS_RTOL * abs(ref64[i]))
        err = abs(got[i] - ref64[i])
        worst = max(worst, err / bar)
        print(f"step {i}: loss {got[i]:.6f} fp64 {ref64[i]:.6f} err {err:.2e} torch fp32 {abs(ref32[i] - ref64[i]):.2e} ({err / bar:.3f} of the bar)")
        assert err <= bar, i
    assert got[-1] < got[0]
    print(f"trajectory: worst {worst:.3f} of the bar")


# ---------------------------------------------------------------------------------------------- 6. determinism and resume
def _run(config, batches, lo, hi, trainer=None):
    trainer = trainer or train.FcnTrainer(config, DEV)
    for x, t, z in batches[lo:hi]:
        trainer.step(x.to(DEV), t.to(DEV), z.to(DEV))
    return trainer


def test_determinism_and_resume(tmp_path):
    D, H, L, B = cases.TRAJ_SHAPE
    config = cases.net_config(D, H, L, B)
    batches = _explicit_batches(D, B, 20)
    a = _run(config, batches, 0, 20)
    b = _run(config, batches, 0, 20)
    half = _run(config, batches, 0, 10)
    path = half.save_checkpoint(str(tmp_path / "ckpt" / "last.ckpt"))
    c = train.FcnTrainer(config, DEV).load_checkpoint(path)
    assert c.global_step == 10
    c = _run(config, batches, 10, 20, trainer=c)
    for other in (b, c):
        assert other.global_step == 20
        assert torch.equal(a.theta, other.theta) and torch.equal(a.m, other.m) and torch.equal(a.v, other.v)
    assert not torch.equal(a.theta, half.theta)


def test_drawn_streams_repeat_and_resume(tmp_path):
    """step() without (t, z): the draws are keyed by (seed, step), so a resumed run continues the stream of the straight one."""
    config = read_config(SMALL_CONFIG)
    config.device = DEV
    a = train.FcnTrainer(config, DEV)
    a.fit(12, log=None)
    b = train.FcnTrainer(config, DEV)
    b.fit(6, log=None)
    path = b.save_checkpoint(str(tmp_path / "last.ckpt"))
    c = train.FcnTrainer(config, DEV).load_checkpoint(path)
    c.fit(12, log=None)
    assert torch.equal(a.theta, c.theta) and torch.equal(a.m, c.m) and torch.equal(a.v, c.v)
    t1, z1 = a.draw(256, 3)
    t1, z1 = t1.clone(), z1.clone()
    t2, z2 = a.draw(256, 4)
    assert not torch.equal(t1, t2) and not torch.equal(z1, z2)
    t3, z3 = a.draw(256, 3)
    assert torch.equal(t1, t3) and torch.equal(z1, z3)
    assert abs(float(z1.mean())) < 0.1 and abs(float(z1.std()) - 1) < 0.1 and 1e-5 <= float(t1.min()) and float(t1.max()) <= 1.0


def test_eval_loss_is_repeatable_and_matches_the_training_loss():
    """eval_loss: the gradient-free kernel path (null G) on the validation split with its own keyed draws; eval_batch gives the bits
    of loss_and_grad on the same (x, t, z)."""
    config = read_config(SMALL_CONFIG)
    config.device = DEV
    trainer = train.FcnTrainer(config, DEV)
    a, b = trainer.eval_loss('val', max_batches=2), trainer.eval_loss('val', max_batches=2)
    assert a == b and np.isfinite(a) and a > 0
    x = trainer.next_batch()
    t, z = trainer.draw(x.shape[0], 0)
    theta = trainer.theta.clone()
    assert float(trainer.eval_batch(x, t, z)) == float(trainer.loss_and_grad(x, t, z))
    assert torch.equal(theta, trainer.theta)                       # neither moves the weights
    trainer.fit(300, log=None)
    assert trainer.eval_loss('val', max_batches=2) < 0.5 * a


def test_no_host_synchronisation_inside_a_step():
    """A step with drawn (t, z) and the next batch of the epoch permutation: torch's synchronisation check stays silent."""
    config = read_config(SMALL_CONFIG)
    config.device = DEV
    trainer = train.FcnTrainer(config, DEV)
    trainer.fit(2, log=None)                                   # buffers, data and the permutation are in place
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            loss = trainer.step(trainer.next_batch())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.isfinite(float(loss)) and trainer.global_step == 5


def test_model_view_follows_the_flat_buffer():
    """The trainer's FCN reads the trained weights, never a stale pack: its forward equals the trainer's own forward after steps."""
    D, H, L, B = cases.NET_SHAPES[0]
    config = cases.net_config(D, H, L, B, warmup=0)
    trainer = train.FcnTrainer(config, DEV)
    x, t, z = (a.to(DEV) for a in cases.batch(D, B, seed=3))
    before = trainer.model(x, t * 999).clone()
    for _ in range(3):
        trainer.step(x, t, z)
    after = trainer.model(x, t * 999)
    assert not torch.equal(before, after)
    ref = cases.sequential({k: v.detach().cpu() for k, v in trainer.state_dict().items()}, torch.float64)
    with torch.no_grad():
        want = ref(torch.cat([x.cpu().double(), (t * 999).cpu().double()[:, None]], dim=1))
    assert float((after.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


# ---------------------------------------------------------------------------------------------- 7. it learns
def test_trained_network_reads_the_sphere_dimension(tmp_path):
    """8000 steps on the unit 2-sphere in R^8 (not padding: the plain-torch check behind this recipe read 3 everywhere at 2000 steps, the
    radial normal is learned late), then the estimator on the written checkpoint: every point must report 2.  Measured: 2.0 s of
    training on an MI355X (247 us a step), 7 of 7 points read 2."""
    config = read_config(SMALL_CONFIG)
    config.device = DEV
    config.logging.log_path = str(tmp_path)
    torch.cuda.synchronize()
    import time
    t0 = time.perf_counter()
    trainer, history = train.train(config, log_path=str(tmp_path), n_iters=8000, log_every=2000, log=None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    first, last = history[0][1], history[-1][1]
    print(f"8000 steps in {dt:.2f} s ({dt / 8000 * 1e6:.0f} us per step); loss {first:.4f} -> {last:.4f}")
    ckpt = train.last_checkpoint_path(config, str(tmp_path))
    assert os.path.exists(ckpt) and trainer.global_step == 8000
    assert last < 0.1 * first
    config.model.checkpoint_path = ckpt
    info, dims = dim_reduction.get_manifold_dimension(config, return_svd=True, return_dims=True)
    for sv in info['singular_values']:
        print("singular values:", " ".join(f"{s:.1f}" for s in sv))
    print("dims:", list(dims))
    assert len(dims) >= 7 and all(int(d) == 2 for d in dims)


# ---------------------------------------------------------------------------------------------- 8. entry points
def test_main_mode_train_writes_and_resumes(tmp_path):
    args = ["--config", SMALL_CONFIG, "--mode", "train", "--log_path", str(tmp_path), "--log_name", "run"]
    main.main(args + ["--n_iters", "20"])
    path = os.path.join(str(tmp_path), "run", "checkpoints", "last.ckpt")
    ckpt = checkpoint_io.load_checkpoint(path)
    assert ckpt['global_step'] == 20
    first = {k: v.clone() for k, v in checkpoint_io.score_model_state_dict(ckpt).items()}
    main.main(args + ["--n_iters", "30", "--checkpoint_path", path, "--checkpoint_every", "5"])
    again = checkpoint_io.load_checkpoint(path)
    assert again['global_step'] == 30
    assert any(not torch.equal(first[k], v) for k, v in checkpoint_io.score_model_state_dict(again).items())
    straight = train.FcnTrainer(read_config(SMALL_CONFIG), DEV)
    straight.fit(30, log=None)
    for k, v in checkpoint_io.score_model_state_dict(again).items():
        assert torch.equal(v, straight.state_dict()[k].cpu()), k            # resumed at step 20 of the same streams
    # the written file restores into the estimator's module unchanged
    from id_diff_amd.lightning_modules.BaseSdeGenerativeModel import BaseSdeGenerativeModel
    module = BaseSdeGenerativeModel(read_config(SMALL_CONFIG)).load_from_checkpoint(path)
    assert torch.equal(module.score_model.mlp[0].weight.detach().cpu(), checkpoint_io.score_model_state_dict(again)['mlp.0.weight'])


def test_refused_configurations():
    with pytest.raises(SystemExit, match="fcn"):
        main.main(["--config", "configs/dimension_estimation/paper/image_data/MNIST/config.py", "--mode", "train", "--n_iters", "5"])
    config = read_config(SMALL_CONFIG)
    config.model.dropout = 0.1
    with pytest.raises(NotImplementedError, match="model.dropout"):
        train.FcnTrainer(config, DEV)
    with pytest.raises(SystemExit, match="one GPU"):
        main.main(["--config", SMALL_CONFIG, "--mode", "train", "--n_iters", "5", "--gpus", "2"])
