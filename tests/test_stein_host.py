"""Host side of the Stein-divergence FLIPD (no GPU): ``stein.reading_from_sums`` against the whole estimator ``stein.reading_host`` in long
double, the reading and its error bar on a synthetic linear field, the bound the kernel is held to (tests/stein_cases.py) validated on
the kernel's order of operations restated in numpy and shown to catch ten planted bugs, the driver's new refusals, the CLI flag and
what the C entry point refuses before any device call."""
import os

import numpy as np
import pytest
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd import _lib, dim_reduction, main, parallel, sde_lib, stein
from id_diff_amd.configs.utils import read_config

import stein_cases as sc

LD = np.longdouble


# ------------------------------------------------------------------------------------------- sums -> reading
def _from_sums_of(S, Z, sigma):
    ref = stein.reading_host(S, Z, sigma, LD)
    got = stein.reading_from_sums(np.asarray(ref['sums'], dtype=np.float64)[None], S.shape[0], S.shape[1], sigma, float(ref['mean_norm2']))
    return ref, {k: v[0] for k, v in got.items()}


def _tolerance(ref, M, D, sigma):
    """What forming the centred moments from raw fp64 sums may cost: each raw sum is exact to 2^-53 (rounded from long double), the
    centred moment c = raw - s1 s2 / M loses the factor kappa = raw / c, and beta = sigma c_aq / c_qq carries both; the readings are
    linear in beta with weight |mean q - D|.  8 roundings of slack; scale: the magnitudes the reading is assembled from."""
    a1, q = ref['rows'][:, 0].astype(np.float64), ref['rows'][:, 1].astype(np.float64)
    kq = (q * q).sum() / max(((q - q.mean()) ** 2).sum(), 1e-300)
    ka = max((np.abs(a1 * q)).sum(), abs(a1.sum() * q.sum()) / M) / max(abs(((a1 - a1.mean()) * (q - q.mean())).sum()), 1e-300)
    kappa = max(kq, ka, 1.0)
    beta = abs(float(ref['beta']))
    return 8 * 2.0 ** -53 * kappa * (1.0 + beta) * (abs(float(ref['plain'])) + D + abs(q.mean() - D) * max(beta, 1.0))


@pytest.mark.parametrize("M,D", [(1, 4), (2, 8), (3, 8), (17, 5), (65, 100), (1501, 64)])
def test_reading_from_sums_equals_the_host_estimator(M, D):
    for seed in range(3):
        S, Z = sc.inputs(1, M, D, seed=seed)
        sigma = 0.05
        ref, got = _from_sums_of(S[0], Z[0], sigma)
        if M < 3:
            assert got['beta'] == 0.0 and ref['beta'] == 0 and got['flipd'] == got['plain']
        if M < 2:
            assert np.isnan(got['stderr']) and np.isnan(ref['stderr'])
        tol = _tolerance(ref, M, D, sigma)
        for k in ('flipd', 'plain', 'beta') + (('stderr',) if M >= 2 else ()):
            assert abs(got[k] - float(ref[k])) <= tol, (k, got[k], float(ref[k]), tol)
        if M == 2:                                        # two rows, no fit: the error bar is that of the plain mean
            a = sigma * ref['rows'][:, 0]
            assert abs(got['stderr'] - float(abs(a[0] - a[1]) / 2)) <= tol


def test_a_constant_q_gets_no_control_variate():
    """Rows of +-1 entries: q = D exactly for every row, var(q) = 0; the raw sums give a centred moment of rounding size, which must
    read as 0 (beta = 0, flipd = plain), not as a ratio of two rounding errors."""
    rng = np.random.default_rng(5)
    M, D = 301, 24
    Z = rng.choice([-1.0, 1.0], size=(M, D)).astype(np.float32)
    S = (-Z / 0.1 + rng.standard_normal((M, D))).astype(np.float32)
    ref, got = _from_sums_of(S, Z, 0.1)
    assert ref['beta'] == 0 and got['beta'] == 0.0 and got['flipd'] == got['plain']
    assert abs(got['plain'] - float(ref['plain'])) <= 1e-12 * D and abs(got['stderr'] - float(ref['stderr'])) <= 1e-10
    # and with the q of a kernel that rounds: sums off by a few units in the last place must read the same
    sums = np.asarray(ref['sums'], dtype=np.float64)
    sums[3] *= 1 + 3 * 2.0 ** -52
    assert stein.reading_from_sums(sums[None], M, D, 0.1, float(ref['mean_norm2']))['beta'][0] == 0.0


def test_vp_and_subvp_go_through_the_same_scalars():
    """sigma is std(t) of the SDE, evaluated in fp64 on the host as jacobian.flipd evaluates it; the reading is that of reading_host at
    that sigma."""
    S, Z = sc.inputs(1, 400, 16, seed=2)
    for sde, t in ((sde_lib.VPSDE(0.1, 20.0), 1e-3), (sde_lib.subVPSDE(0.1, 20.0), 1e-3), (sde_lib.VESDE(0.01, 50.0), 1e-5)):
        sigma = stein.level_sigma(sde, t)
        want = float(sde.marginal_prob(torch.ones((), dtype=torch.float64), torch.tensor([t], dtype=torch.float64))[1])
        assert sigma == want and 0 < sigma < 0.05
        ref, got = _from_sums_of(S[0], Z[0], sigma)
        tol = _tolerance(ref, 400, 16, sigma)
        assert abs(got['flipd'] - float(ref['flipd'])) <= tol and abs(got['stderr'] - float(ref['stderr'])) <= tol


def test_poisoned_sums_stay_poisoned_and_only_there():
    S, Z = sc.inputs(2, 50, 8)
    sums = np.stack([np.asarray(stein.reading_host(S[p], Z[p], 0.05)['sums'], dtype=np.float64) for p in range(2)])
    sums[1] = np.nan
    out = stein.reading_from_sums(sums, 50, 8, 0.05, np.array([1.0, 1.0]))
    assert all(np.isfinite(out[k][0]) and np.isnan(out[k][1]) for k in stein.KEYS)


def test_linear_field_reads_its_dimension_with_the_predicted_error_bar():
    """s = -P_N z / sigma, D = 64, d = 5, M = 1501, seed 0: in long double the reading is 5.1249 with stderr 0.07707 (prediction
    sqrt(2 5 59 / (64 1501)) = 0.07837); the plain reading 5.0912 has the wider bar sqrt(2 59 / 1501) = 0.28.  Asserted: within 4 reported
    stderr of 5, stderr within 20 % of the formula."""
    S, Z = sc.linear_field(seed=0)
    M, D, d = 1501, 64, 5
    predicted = np.sqrt(2 * d * (D - d) / (D * M))
    for ref in (stein.reading_host(S, Z, 0.05, LD), stein.reading_host(S, Z, 0.05)):
        print(f"linear field: flipd {float(ref['flipd']):.4f} +- {float(ref['stderr']):.5f} (predicted {predicted:.5f}), plain "
              f"{float(ref['plain']):.4f}, beta {float(ref['beta']):.4f}")
        assert abs(float(ref['flipd']) - d) <= 4 * float(ref['stderr'])
        assert abs(float(ref['stderr']) / predicted - 1) <= 0.2
        assert -1.0 < float(ref['beta']) < -0.8                       # a_i ~ -|P_N z_i|^2: almost all of q's fluctuation
    _, got = _from_sums_of(S, Z, 0.05)
    assert abs(got['flipd'] - d) <= 4 * got['stderr'] and abs(got['stderr'] / predicted - 1) <= 0.2


def test_finite_m_correction_removes_two_times_d_minus_d_over_m():
    """D = 256, d = 4, M = 1030 (the M ~ 4 D of an image config): the plain formulas read d + 2 (D - d) / M = 4.49 in the mean, the
    corrected ones d.  Deterministic part: the two readings differ by exactly sigma mean(a') / (M - 1) - sigma^2 T / (M (M - 1)), from the
    sums as in the host estimator, and the correction uses the trace it is handed.  Statistical part, seed 0 checked in long double
    first: corrected within 4 stderr of 4, uncorrected more than 4 stderr above it."""
    M, D, d, sigma = 1030, 256, 4, 0.01
    S, Z = sc.linear_field(seed=0, D=D, d=d, M=M, sigma=sigma)
    plain, fixed = stein.reading_host(S, Z, sigma, LD), stein.reading_host(S, Z, sigma, LD, debias=True)
    T, sa = plain['centred_trace'], plain['sums'][0]
    shift = sigma * sa / LD(M) / LD(M - 1) - sigma * sigma * T / (LD(M) * LD(M - 1))
    assert abs(float(fixed['flipd'] - plain['flipd'] - shift)) <= 1e-12 and abs(float(shift) + 2 * (D - d) / M) <= 0.05
    got = stein.reading_from_sums(np.asarray(plain['sums'], dtype=np.float64)[None], M, D, sigma, float(plain['mean_norm2']),
                                  centred_trace=float(T))
    assert abs(got['flipd'][0] - float(fixed['flipd'])) <= _tolerance(fixed, M, D, sigma)
    assert abs(got['plain'][0] - float(fixed['plain'])) <= _tolerance(fixed, M, D, sigma)
    other = stein.reading_host(S, Z, sigma, LD, debias=True, centred_trace=float(T) * 2)
    assert abs(float(other['flipd'] - fixed['flipd']) + sigma * sigma * float(T) / (M * (M - 1.0))) <= 1e-9
    print(f"finite M: plain formulas {float(plain['flipd']):.4f}, corrected {float(fixed['flipd']):.4f} +- {float(fixed['stderr']):.4f}")
    assert abs(float(fixed['flipd']) - d) <= 4 * float(fixed['stderr']) < float(plain['flipd']) - d
    one = stein.reading_from_sums(np.array([[1.0, 1.0, 4.0, 16.0, 4.0]]), 1, 4, 0.5, 2.0, centred_trace=0.0)     # M = 1: ignored
    assert one['plain'][0] == 4 + 0.5 + 0.5 and np.isnan(one['stderr'][0])


def test_reading_host_refuses_mismatched_shapes():
    with pytest.raises(ValueError, match="same"):
        stein.reading_host(np.zeros((3, 4)), np.zeros((3, 5)), 1.0)


# ------------------------------------------------------------------------------------------- the bound, on the kernel's arithmetic
def _worst(S, Z, mutate=None):
    rows_ref, sums_ref, mean, A = sc.oracle(S, Z)
    P, M, D = S.shape
    b_rows, b_sums = sc.bounds(M, D, rows_ref, A)
    worst = 0.0
    for p in range(P):
        rows, sums = sc.restated(S[p], Z[p], mean[p].astype(np.float64), mutate=mutate)
        worst = max(worst, sc.worst_ratio(np.abs(rows - rows_ref[p]), b_rows[p]), sc.worst_ratio(np.abs(sums - sums_ref[p]), b_sums[p]))
    return worst


@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.shape_id)
def test_restated_arithmetic_stays_under_half_the_bound(shape):
    """(A tenth at D >= 100; at D = 8 the handful of roundings of a row is a larger share of a bound of D + 4 units.)"""
    P, M, D, _ = shape
    worst = _worst(*sc.inputs(P, M, D))
    print(f"{sc.shape_id(shape)}: worst error / bound of the float replay {worst:.2e}")
    assert worst <= 0.5


# the shapes on which each planted bug can show: a tail (D % 4 != 0), more lanes than 32 groups, two rows, more rows than one pass
_WHERE = {"drop_tail": [(2, 17, 5), (1, 130, 193)], "lost_lanes": [(1, 130, 193), (1, 40, 1024)], "sums_drop_last_pass": [(1, 257, 12), (3, 65, 100)]}


@pytest.mark.parametrize("mutate", sc.MUTATIONS)
def test_a_planted_bug_leaves_the_bound(mutate):
    worst = np.inf
    for P, M, D in _WHERE.get(mutate, [(3, 65, 100), (1, 257, 12)]):
        S, Z = sc.inputs(P, M, D)
        assert _worst(S, Z) <= 0.5
        worst = min(worst, _worst(S, Z, mutate=mutate))
    print(f"{mutate}: smallest worst error / bound {worst:.2e}")
    assert worst >= 1e3


# ------------------------------------------------------------------------------------------- the driver's refusals and the CLI
def _ksphere_config(tmp_path):
    cfg = read_config('configs/dimension_estimation/paper/euclidean_data/ksphere/10dim.py')
    cfg.model.name = 'ksphere_exact'
    cfg.logging.log_path = str(tmp_path)
    cfg.dim_estimation.num_datapoints = 3
    return cfg


def _no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the driver went on to set up the model")
    monkeypatch.setattr(dim_reduction, "setup_model", touched)
    monkeypatch.setattr(dim_reduction, "create_lightning_datamodule", touched)


@pytest.mark.parametrize("method", ["jacobian", "flipd"])
def test_sampled_flipd_needs_the_sampling_method(tmp_path, monkeypatch, method):
    _no_device(monkeypatch)
    cfg = _ksphere_config(tmp_path)
    cfg.model.name = 'fcn'
    with pytest.raises(NotImplementedError, match="method 'sampling'" if method == 'jacobian' else "flipd"):
        dim_reduction.get_manifold_dimension(cfg, return_svd=True, return_flipd=True, method=method)
    cfg2 = _ksphere_config(tmp_path)
    cfg2['dim_estimation.method'] = 'jacobian'
    cfg2.model.name = 'fcn'
    cfg2.dim_estimation.save_flipd = True
    with pytest.raises(NotImplementedError, match="method 'sampling'"):
        dim_reduction.get_manifold_dimension(cfg2, name="x")
    assert not os.listdir(tmp_path)


def test_sampled_flipd_refuses_two_ranks_before_any_device_work(tmp_path, monkeypatch):
    _no_device(monkeypatch)
    monkeypatch.setattr(parallel, "rank_world", lambda: (1, 2))
    cfg = _ksphere_config(tmp_path)
    with pytest.raises(NotImplementedError, match="world size 2"):
        dim_reduction.get_manifold_dimension(cfg, return_svd=True, return_flipd=True)
    cfg.dim_estimation.save_flipd = True
    with pytest.raises(NotImplementedError, match="save_flipd"):
        dim_reduction.get_manifold_dimension(cfg, name="x")
    assert not os.listdir(tmp_path)                    # refused before the output directory was made


def test_sampled_flipd_refuses_row_sharding_on_one_rank_too(tmp_path, monkeypatch):
    _no_device(monkeypatch)
    cfg = _ksphere_config(tmp_path)
    cfg.dim_estimation.shard = 'rows'
    with pytest.raises(NotImplementedError, match="shard = 'rows'"):
        dim_reduction.get_manifold_dimension(cfg, return_svd=True, return_flipd=True)


def test_return_flipd_without_svd_is_a_usage_error(tmp_path, monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="return_flipd needs return_svd"):
        dim_reduction.get_manifold_dimension(_ksphere_config(tmp_path), return_flipd=True)


def test_method_flipd_goes_on_refusing_the_image_networks(tmp_path, monkeypatch):
    _no_device(monkeypatch)
    cfg = _ksphere_config(tmp_path)
    cfg.model.name = 'ncsnpp'
    with pytest.raises(NotImplementedError, match="JVP or VJP"):
        dim_reduction.get_manifold_dimension(cfg, return_dims=True, method='flipd')
    assert dim_reduction.METHODS == ('sampling', 'jacobian', 'flipd') and dim_reduction.FLIPD_MODELS == ('fcn', 'empirical_exact')


def test_main_parse_takes_sampled_flipd():
    base = ["--config", "c.py", "--mode", "manifold_dimension"]
    assert main.parse(base).sampled_flipd is False
    assert main.parse(base + ["--sampled_flipd"]).sampled_flipd is True
    with pytest.raises(SystemExit):
        main.parse(base + ["--dim_method", "stein"])             # the methods' choices are what they were


# ------------------------------------------------------------------------------------------- the C ABI
def test_ok_truth_table():
    ok = _lib.stein_rows_ok
    assert ok(1, 1) and ok(1501, 100) and ok(4480, 3072) and ok((1 << 31) - 1, 1 << 30) and ok(1, 5)
    assert not ok(0, 4) and not ok(4, 0) and not ok(-1, 4) and not ok(1 << 31, 4) and not ok(4, (1 << 30) + 1)
    assert _lib.STEIN_P_MAX == 65535


_A, _B, _C, _D, _E, _F = (0x10000 * i for i in range(1, 7))              # fabricated addresses: a call let through would fault
_CALL = lambda S=_A, lds=8, stride_s=24, mean=_B, Z=0, ldz=0, stride_z=0, seeds=_C, row0=0, rows=_D, sums=_E, P=2, M=3, D=8: \
    [S, lds, stride_s, mean, Z, ldz, stride_z, seeds, row0, rows, sums, P, M, D]
_REFUSED = {
    "null_S": _CALL(S=0), "null_mean": _CALL(mean=0), "null_rows": _CALL(rows=0), "null_sums": _CALL(sums=0),
    "neither_Z_nor_seeds": _CALL(seeds=0), "philox_needs_D_mod_4": _CALL(D=6, lds=6, stride_s=18), "M0": _CALL(M=0), "D0": _CALL(D=0),
    "negative_M": _CALL(M=-3), "negative_P": _CALL(P=-1), "P_above_grid": _CALL(P=65536), "M_above_limit": _CALL(M=1 << 31),
    "D_above_limit": _CALL(D=(1 << 30) + 4, lds=(1 << 30) + 4, stride_s=1 << 40), "negative_row0": _CALL(row0=-1),
    "row0_overflow": _CALL(row0=1 << 60), "pitch_below_D": _CALL(lds=7), "point_stride_below_rows": _CALL(stride_s=23),
    "Z_pitch_below_D": _CALL(Z=_F, ldz=7, stride_z=24), "Z_point_stride_below_rows": _CALL(Z=_F, ldz=8, stride_z=23),
    "misaligned_S": _CALL(S=_A + 2), "misaligned_Z": _CALL(Z=_F + 1, ldz=8, stride_z=24), "misaligned_mean": _CALL(mean=_B + 4),
    "misaligned_seeds": _CALL(seeds=_C + 4), "misaligned_rows": _CALL(rows=_D + 4), "misaligned_sums": _CALL(sums=_E + 4),
    "null_S_at_P0": _CALL(S=0, P=0),
}


@pytest.mark.parametrize("case", sorted(_REFUSED))
def test_entry_point_refuses_before_any_device_call(case):
    handle = _lib.lib()
    assert handle.idiff_stein_rows_f64(*_REFUSED[case], None) == 1001            # IDIFF_EINVAL
    assert handle.idiff_last_error().decode().startswith("stein_rows: ")


def test_p0_with_good_pointers_is_a_no_op():
    assert _lib.lib().idiff_stein_rows_f64(*_CALL(P=0), None) == 0
    assert _lib.lib().idiff_stein_rows_f64(*_CALL(P=0, Z=_F, ldz=8, stride_z=24, seeds=0, D=7, lds=7, stride_s=21), None) == 0


def test_wrappers_have_no_cpu_path():
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.stein_rows(torch.zeros(3, 8), torch.zeros(8, dtype=torch.float64), seeds=[1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.column_means(torch.zeros(1, 3, 8))
