"""Host side of the Isomap embedding (no GPU): the schedule of the eigenvector routine, the numpy restatements of the embedding and
of the out-of-sample transform against scikit-learn's stored results (tests/golden/isomap_embed.npz), what the new C entry points
refuse before any device call, and the classifier step of ``run(embed=True)``."""
import math
import os
import re

import numpy as np
import pytest

import id_diff_amd
from id_diff_amd import _lib, isomap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ("roll257", "roll1000", "sphere193")


@pytest.fixture(scope="module")
def gold(golden):
    return golden("isomap.npz"), golden("isomap_embed.npz")


# ------------------------------------------------------------------------------------------- topvecs_plan
def test_plan_raises_on_a_flat_spectrum_and_names_the_eigenvalues():
    lam = np.concatenate([[3.0], np.full(40, 1.0), [-0.5]])
    with pytest.raises(ValueError, match=r"lambda_2 = 1\.0 and lambda_19 = 1\.0 .*matrix products"):
        _lib.topvecs_plan(lam, 2)
    with pytest.raises(ValueError, match="matrix products"):
        _lib.topvecs_plan(np.concatenate([[3.0], 1.0 + 1e-9 * np.arange(40, 0, -1), [-0.5]]), 2)      # nearly flat: too many products
    with pytest.raises(ValueError, match="matrix products"):
        _lib.topvecs_plan(np.ones(30), 2)


def test_plan_raises_when_lambda_k_is_not_positive():
    lam = np.array([4.0, 2.0, 1e-13, -1.0, -2.0, -3.0])
    assert isomap.n_positive(lam) == 2
    assert _lib.topvecs_plan(lam, 2)["p"] == 5
    with pytest.raises(ValueError, match=r"lambda_3 = 1e-13 is not positive .* 2 positive eigenvalues"):
        _lib.topvecs_plan(lam, 3)
    with pytest.raises(ValueError, match="not positive"):
        _lib.topvecs_plan(-np.arange(1.0, 9.0), 1)
    for k in (0, 65, 6):
        with pytest.raises(ValueError, match="outside"):
            _lib.topvecs_plan(lam if k != 65 else np.arange(100.0, 0.0, -1.0), k)


def _kernel_eigenvalues(D):
    S = -0.5 * D ** 2
    K = S - S.mean(axis=0, keepdims=True) - S.mean(axis=1, keepdims=True) + S.mean()
    return np.linalg.eigvalsh(K)[::-1]


def test_plan_bounds_the_amplification_on_the_fixture_spectra(gold):
    """lambda_1 over lambda_k per sweep never exceeds 1e6; recomputed here from the plan's interval, not read from it.  The full
    spectrum of sphere193 comes from its stored geodesic matrix.  Of the two rolls the fixture stores the top 64 eigenvalues and
    the smallest one; the plan reads lambda_1, lambda_k, lambda_p, lambda_(p+1) and lambda_min only, so for p + 1 <= 64 it is the plan
    of the true spectrum whatever lies between (a linear ramp here)."""
    pts, emb = gold
    spectra = {"sphere193": _kernel_eigenvalues(pts["sphere193_dist"])}
    for name, n in (("roll257", 257), ("roll1000", 1000)):
        top, low = emb[f"{name}_eig64"], float(emb[f"{name}_eigmin"])
        spectra[name] = np.concatenate([top, np.linspace(top[-1], low, n - 64 + 1)[1:]])
    assert abs(spectra["sphere193"][-1] - float(emb["sphere193_eigmin"])) <= 1e-12 * spectra["sphere193"][0]
    assert _lib.TOPVECS_AMPLIFICATION == 1e6
    for name, lam in spectra.items():
        for k in (1, 2, 3, 5, 10, 30):
            plan = _lib.topvecs_plan(lam, k)
            c, e = 0.5 * (plan["hi"] + plan["lo"]), 0.5 * (plan["hi"] - plan["lo"])
            cheb = lambda x: math.cosh(plan["degree"] * math.acosh(x))
            amp = cheb((lam[0] - c) / e) / cheb((lam[k - 1] - c) / e)
            print(f"{name}, k = {k}: {plan}, recomputed amplification {amp:.4g}")
            assert plan["lo"] == lam[-1] < 0 and plan["hi"] == lam[plan["p"]] and plan["top"] == lam[0]
            assert plan["p"] == k + max(16, k) <= 63
            assert 1 <= plan["degree"] <= 32 and plan["products"] == plan["degree"] * plan["sweeps"] <= 1000
            assert abs(amp - plan["amplification"]) <= 1e-9 * amp
            assert amp <= 1e6
            assert cheb((lam[k - 1] - c) / e) ** (plan["sweeps"] - 1) >= 1e13      # enough sweeps, with the one to spare


def test_plan_serves_every_k_of_the_reference_list_on_a_slowly_decaying_spectrum():
    """lambda_i = 1 / i above a negative tail, N = 1000: the block grows with k (p = min(2 k, 128) beyond k = 16), which keeps
    lambda_(p+1) at about half of lambda_k, and every k <= 64 of the reference's list gets a plan."""
    lam = np.concatenate([1.0 / np.arange(1, 501), -0.01 * np.arange(1, 501) / 500])
    for k in [k for k in isomap.DEFAULT_KS if k <= 64] + [64]:
        plan = _lib.topvecs_plan(lam, k)
        assert plan["p"] == min(k + max(16, k), 128) and plan["products"] <= 1000


def test_plan_does_not_overflow_on_a_narrow_interval():
    """[lambda_min, lambda_(p+1)] 1e-11 wide under well separated wanted eigenvalues: T_m there is beyond a double, its logarithm
    is not, and a cheap plan exists."""
    plan = _lib.topvecs_plan(np.concatenate([np.linspace(10, 5, 18), [-1, -1 - 1e-11]]), 2)
    assert plan["products"] <= 10 and np.isfinite(plan["amplification"])
    lam = np.concatenate([np.linspace(10, 5, 18), [-1], [-1 - 1e-11] * 3])
    plan = _lib.topvecs_plan(lam, 2)                                # p = 18 < N - 1: the narrow interval itself
    assert plan["hi"] - plan["lo"] < 1e-10 and plan["products"] <= 10 and np.isfinite(plan["amplification"])


def test_first_rows_collects_points_and_labels():
    import torch
    x, y = torch.arange(40.0).reshape(10, 2, 2), torch.arange(10)
    X, lab = isomap._first_rows([[x[:4], y[:4]], [x[4:8], y[4:8]], [x[8:], y[8:]]], 6)
    assert X.shape == (6, 4) and torch.equal(X, x.reshape(10, 4)[:6]) and lab.tolist() == [0, 1, 2, 3, 4, 5]
    X, lab = isomap._first_rows([x[:4], x[4:]], 100)
    assert X.shape == (10, 4) and lab is None
    X, lab = isomap._first_rows([[x[:4], y[:4]], x[4:]], 100)      # a loader that stops yielding labels has none
    assert X.shape == (10, 4) and lab is None


# ------------------------------------------------------------------------------------------- host oracles
def test_host_oracles_reproduce_sklearn(gold):
    """Same LAPACK on both sides: 1e-9 max|Z| is far above the rounding-level match (measured 5e-15)."""
    pts, emb = gold
    D, want, want_tr = pts["sphere193_dist"], emb["sphere193_k5_emb"], emb["sphere193_k5_tr"]
    err, lam, (V, lam_k) = isomap.errors_from_geodesics(D, [5], return_eigenvalues=True, return_embedding=True)
    Z = V * np.sqrt(lam_k)
    T = isomap.transform_from_geodesics(D, V, lam_k, emb["sphere193_k10_qdist"], emb["sphere193_k10_qidx"])
    scale = np.abs(want).max()
    print(f"|Z - scikit-learn| / max|Z| = {np.abs(Z - want).max() / scale:.3g}, transform {np.abs(T - want_tr).max() / scale:.3g}")
    assert np.abs(Z - want).max() <= 1e-9 * scale
    assert np.abs(T - want_tr).max() <= 1e-9 * scale
    assert np.array_equal(lam_k, lam[:5])
    assert abs(err[0] - isomap.errors_from_geodesics(D, [5])[0]) <= 1e-12 * err[0]      # eigh here, eigvalsh there
    _, (V2, _) = isomap.errors_from_geodesics(D, [5], return_embedding=True)
    assert np.array_equal(V, V2)
    flipped = isomap.svd_flip_columns(-V)
    assert np.array_equal(flipped, V)


def test_fixture_holds_what_the_tests_read(gold):
    pts, emb = gold
    for name, k, n in (("roll257", 3, 257), ("roll1000", 2, 1000), ("sphere193", 5, 193), ("sphere193", 10, 193)):
        assert emb[f"{name}_k{k}_emb"].shape == (n, k) and emb[f"{name}_k{k}_tr"].shape == (40, k)
        assert emb[f"{name}_Xq"].shape == (40, pts[f"{name}_X"].shape[1]) and emb[f"{name}_Xq"].dtype == np.float32
        assert emb[f"{name}_eig64"].shape == (64,) and 0 < float(emb[f"{name}_k{k}_gmin"]) < 1
        np.testing.assert_allclose(emb[f"{name}_eig64"][:32], pts[f"{name}_eig"], rtol=0, atol=1e-12 * pts[f"{name}_eig"][0])
    assert emb["sphere193_k10_qidx"].shape == emb["sphere193_k10_qdist"].shape == (40, 6)
    size = lambda f: os.path.getsize(os.path.join(ROOT, "tests", "golden", f))
    assert size("isomap_embed.npz") < size("isomap.npz")


# ------------------------------------------------------------------------------------------- refusals of the C entry points
_A, _B, _C, _D, _E, _F, _G, _H = (0x10000 * i for i in range(1, 9))       # fabricated addresses: a call let through would fault
_TOP = lambda K=_A, N=100, k=3, p=19, lo=-1.0, hi=0.5, top=2.0, deg=4, sw=3, V=_B, ritz=_C, resid=_D, scr=_E: (
    "idiff_sym_topvecs_f64", [K, N, k, p, lo, hi, top, deg, sw, V, ritz, resid, scr])
_CROSS = lambda Xq=_A, M=4, X=_B, N=100, D=3, k=5, ws=_C, nbytes=1 << 20, dist=_D, idx=_E: (
    "idiff_knn_cross_f64", [Xq, M, X, N, D, k, ws, nbytes, dist, idx])
_PROJ = lambda dist=_A, idx=_B, M=4, k=5, D=_C, N=100, A=_D, c=2, colmean=_E, grand=_F, Z=_G, scr=_H: (
    "idiff_isomap_project_f64", [dist, idx, M, k, D, N, A, c, colmean, grand, Z, scr])
_REFUSED = {
    "topvecs-k0": _TOP(k=0), "topvecs-k65": _TOP(k=65, p=80), "topvecs-k_is_N": _TOP(N=3, k=3, p=3), "topvecs-N_above_limit": _TOP(N=(1 << 20) + 1),
    "topvecs-p_below_k": _TOP(p=2), "topvecs-p_above_128": _TOP(N=300, p=129), "topvecs-p_is_N": _TOP(N=19),
    "topvecs-null_K": _TOP(K=0), "topvecs-null_V": _TOP(V=0), "topvecs-null_ritz": _TOP(ritz=0), "topvecs-null_resid": _TOP(resid=0),
    "topvecs-null_scratch": _TOP(scr=0), "topvecs-empty_interval": _TOP(lo=0.5), "topvecs-top_inside": _TOP(top=0.4),
    "topvecs-nan_interval": _TOP(lo=float("nan")), "topvecs-degree0": _TOP(deg=0), "topvecs-too_many_products": _TOP(deg=64, sw=65),
    "cross-k0": _CROSS(k=0), "cross-k65": _CROSS(k=65), "cross-k_above_N": _CROSS(N=4, k=5), "cross-N_above_limit": _CROSS(N=(1 << 20) + 1),
    "cross-M0": _CROSS(M=0), "cross-D0": _CROSS(D=0), "cross-null_Xq": _CROSS(Xq=0), "cross-null_X": _CROSS(X=0),
    "cross-null_workspace": _CROSS(ws=0), "cross-null_dist": _CROSS(dist=0), "cross-null_idx": _CROSS(idx=0), "cross-small_workspace": _CROSS(nbytes=8),
    "project-k0": _PROJ(k=0), "project-k65": _PROJ(k=65), "project-c0": _PROJ(c=0), "project-c65": _PROJ(c=65),
    "project-N_above_limit": _PROJ(N=(1 << 20) + 1), "project-M0": _PROJ(M=0), "project-null_dist": _PROJ(dist=0), "project-null_idx": _PROJ(idx=0),
    "project-null_D": _PROJ(D=0), "project-null_A": _PROJ(A=0), "project-null_colmean": _PROJ(colmean=0), "project-null_grand": _PROJ(grand=0),
    "project-null_Z": _PROJ(Z=0), "project-null_scratch": _PROJ(scr=0),
}


@pytest.mark.parametrize("case", sorted(_REFUSED))
def test_new_entries_refuse_bad_arguments(case):
    symbol, args = _REFUSED[case]
    handle = _lib.lib()
    rc = getattr(handle, symbol)(*args, None)
    assert rc == 1001                                            # IDIFF_EINVAL
    assert handle.idiff_last_error().decode().startswith(symbol[len("idiff_"):].rsplit("_f64", 1)[0] + ": ")


def test_scratch_queries_and_limits():
    handle = _lib.lib()
    assert _lib.TOPVECS_MAX == 64 and _lib.TOPVECS_BLOCK_MAX == 128
    assert handle.idiff_sym_topvecs_scratch_doubles(100, 3, 19) >= 2 * 100 * 19 + 2 * 19 * 19
    for bad in ((100, 0, 19), (100, 65, 80), (3, 3, 3), (100, 3, 2), (300, 3, 129)):
        assert handle.idiff_sym_topvecs_scratch_doubles(*bad) == 0
    assert handle.idiff_knn_cross_workspace_bytes(4, 100) == 4 * 100 * 8 and handle.idiff_knn_cross_workspace_bytes(1000, 100) == 256 * 100 * 8
    assert handle.idiff_knn_cross_workspace_bytes(0, 100) == 0
    assert handle.idiff_isomap_project_scratch_doubles(2) == 4 and handle.idiff_isomap_project_scratch_doubles(65) == 0


def test_readme_counts_the_entry_points_of_the_header():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "idiff_hip.h")).read(), flags=re.S)
    n = len(set(re.findall(r"\b(idiff_[a-z0-9_]+)\s*\(", header)))
    counts = [int(c) for c in re.findall(r"(\d+) entry points now", open(os.path.join(ROOT, "README.md")).read())]
    assert n == len(_lib.EXPORTED_SYMBOLS) == max(counts)


def test_isomap_class_refuses_before_any_device_call():
    with pytest.raises(ValueError, match="n_components"):
        isomap.Isomap(5, 65)
    with pytest.raises(ValueError, match="n_components"):
        isomap.Isomap(5, 0)
    with pytest.raises(ValueError, match="12288"):
        isomap.Isomap(5, 2).fit(np.zeros((12289, 3), dtype=np.float32))


# ------------------------------------------------------------------------------------------- the classifier step
def test_classifier_step_on_two_classes(tmp_path):
    pytest.importorskip("sklearn")
    rng = np.random.default_rng(0)
    def blobs(n):
        y = np.arange(n) % 2
        return rng.standard_normal((n, 2)) * 0.1 + np.where(y[:, None] == 1, 5.0, -5.0), y
    (train, y_train), (test, y_test) = blobs(60), blobs(30)
    assert isomap.classifier_scores(train, y_train, test, y_test) == 1.0
    assert isomap.classifier_scores(train, y_train, test, 1 - y_test) == 0.0
