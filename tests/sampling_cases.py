"""What tests/golden/make_sampling.py, tests/test_sampling_host.py and tests/test_hip_sampling.py share: the cases of the sampling
fixture, how its arrays are read back, the fp64 numpy restatement of the fixture's network, and the shapes and bounds of the kernel tests.

The fixture (tests/golden/sampling.npz) holds, per case, the N(0, 1) draws in the order the reference consumed them, the reference's
fp32 trajectory (x and x_mean after every update) and the same trajectory re-run with model and state in fp64 on the same draws.  The
fp64 arrays are stored as fp32 differences to the fp32 ones (``d64 = fl32(x64 - x32)``): read back as x32 + d64 they are the fp64
trajectory to 2^-24 of the fp32-fp64 gap, i.e. to about 1e-13 of the state, seven orders below the bars that use them.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling.npz")

# ---------------------------------------------------------------------------------------------- the fixture's set-up
D, HIDDEN, HIDDEN_LAYERS, N_STEPS, B = 6, 16, 1, 40, 5
LAST_LAYER_SCALE = 0.05
SNR = 0.15
SDE_PARAMS = {'ve': dict(sigma_min=0.01, sigma_max=4.0), 'vp': dict(beta_min=0.1, beta_max=20.0), 'subvp': dict(beta_min=0.1, beta_max=20.0)}
EPS = {'ve': 1e-5, 'vp': 1e-3, 'subvp': 1e-3}

_PRED = ('reverse_diffusion', 'euler_maruyama', 'ancestral_sampling')
CASES = ([('ve', p, c, False) for p in _PRED for c in ('none', 'langevin', 'ald')] +
         [('vp', p, c, False) for p in _PRED for c in ('none', 'langevin')] +
         [('subvp', p, 'none', False) for p in _PRED[:2]] +
         [(k, 'reverse_diffusion', 'none', True) for k in ('ve', 'vp', 'subvp')])


def case_id(case):
    kind, pred, corr, pf = case
    return f"{kind}-{pred}-{corr}" + ("-pf" if pf else "")


def make_sde(kind, N=N_STEPS):
    from id_diff_amd import sde_lib
    p = SDE_PARAMS[kind]
    if kind == 've':
        return sde_lib.VESDE(sigma_min=p['sigma_min'], sigma_max=p['sigma_max'], N=N)
    return (sde_lib.VPSDE if kind == 'vp' else sde_lib.subVPSDE)(beta_min=p['beta_min'], beta_max=p['beta_max'], N=N)


def fcn_config(kind='ve'):
    from id_diff_amd.configs.config_dict import ConfigDict
    c = ConfigDict()
    c.model = ConfigDict(name="fcn", state_size=D, hidden_layers=HIDDEN_LAYERS, hidden_nodes=HIDDEN, dropout=0.0, sigma_min=0.01,
                         sigma_max=4.0, beta_min=0.1, beta_max=20.0, num_scales=N_STEPS)
    c.training = ConfigDict(sde={'ve': 'vesde', 'vp': 'vpsde', 'subvp': 'subvpsde'}[kind], continuous=True)
    return c


def load():
    return np.load(GOLDEN, allow_pickle=False)


def weights(fx):
    return {k[4:]: fx[k] for k in fx.files if k.startswith("sd::")}


def updates(case):
    """The updates of a case in order: [(time index, 'corrector' | 'predictor')]."""
    out = []
    for i in range(N_STEPS):
        if case[2] != 'none':
            out.append((i, 'corrector'))
        out.append((i, 'predictor'))
    return out


def trajectory(fx, case):
    """dict(draws [n, B, D] fp32, x32, xm32 fp32, x64, xm64 fp64) of a case; entry k is the state after update k."""
    cid = case_id(case)
    x32, xm32 = fx[f"{cid}::x32"], fx[f"{cid}::xm32"]
    return dict(draws=fx[f"{cid}::draws"], x32=x32, xm32=xm32, x64=x32.astype(np.float64) + fx[f"{cid}::dx64"].astype(np.float64),
                xm64=xm32.astype(np.float64) + fx[f"{cid}::dxm64"].astype(np.float64))


def prior_state(fx, kind, dtype=np.float64):
    """The state before the first update: the prior draw times the prior's standard deviation."""
    scale = SDE_PARAMS['ve']['sigma_max'] if kind == 've' else 1.0
    return (fx["prior_z"].astype(dtype) * dtype(scale)).astype(dtype)


def elu(v):
    return np.where(v > 0, v, np.expm1(np.minimum(v, 0)))


def network(w, x, label):
    """The fixture's fcn in fp64 numpy: rows x [B, D], one time feature ``label`` for all rows."""
    h = np.concatenate([np.asarray(x, dtype=np.float64), np.full((len(x), 1), float(label))], axis=1)
    keys = sorted({int(k.split('.')[1]) for k in w})
    for j, i in enumerate(keys):
        h = h @ w[f"mlp.{i}.weight"].astype(np.float64).T + w[f"mlp.{i}.bias"].astype(np.float64)
        if j < len(keys) - 1:
            h = elu(h)
    return h


def score64(w, sde, x, t):
    """get_score_fn in fp64: -network(x, t (N - 1)) / std(t) with t the fp32 grid value widened to fp64."""
    from id_diff_amd import sampling
    return -network(w, x, float(t) * (sde.N - 1)) / sampling.marginal_std(sde, t)


# ---------------------------------------------------------------------------------------------- kernel tests
STEP_SHAPES = [(1, 1, 1), (5, 6, 6), (5, 6, 8), (33, 100, 104), (3, 7, 7)]          # (B, D, pitch)
NORM_SHAPES = [(5, 6), (33, 100)]
SENTINEL = -777.25
U = 2.0 ** -24


def step_bound(ref, ax, bs, cz):
    """One rounding to fp32 of a value evaluated in fp64."""
    return U * np.abs(ref) + 2.0 ** -50 * (np.abs(ax) + np.abs(bs) + np.abs(cz)) + 2.0 ** -149


def norm_rtol(B_, D_):
    return (D_ + B_ + 8) * 2.0 ** -53 + 2.0 ** -52


TRAJ_FACTOR, TRAJ_FLOOR = 16.0, 2.0 ** -20

# ---------------------------------------------------------------------------------------------- acceptance without a checkpoint
EMP = dict(points=256, ambient=8, sigma_min=4e-4, sigma_max=2.0, N=200, samples=128, seed=7)


def empirical_cloud():
    """256 equally spaced points of a unit circle in a random plane of R^8 (fp32, as the model stores them)."""
    rng = np.random.default_rng(EMP['seed'])
    q, _ = np.linalg.qr(rng.standard_normal((EMP['ambient'], 2)))
    ang = 2 * np.pi * np.arange(EMP['points']) / EMP['points']
    return (np.stack([np.cos(ang), np.sin(ang)], axis=1) @ q.T).astype(np.float32)


def nearest_distance(samples, cloud):
    d = np.asarray(samples, dtype=np.float64)[:, None, :] - np.asarray(cloud, dtype=np.float64)[None]
    return np.sqrt((d * d).sum(-1)).min(axis=1)
