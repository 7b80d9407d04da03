"""Host side of ``connect="closest"`` (no GPU): the three numpy restatements of the repair of a disconnected neighbourhood graph
(isomap.component_labels, bridges_from_points, repair_geodesics) against scikit-learn's stored results
(tests/golden/isomap_connect.npz, written by tests/golden/make_isomap_connect.py), the argument checks, the CLI switch, and what
the new C entry points refuse before any device call.

The neighbourhood graph is built here in numpy from direct fp64 differences of the fp32 points (the generator asserts that no
neighbour set and no closest pair hangs on a rounding) and closed by a vectorised Floyd-Warshall; the bound of the shortest
paths is the one of tests/test_hip_geodesic.py, |got - ref| <= 4 N 2^-53 ref: both sides sum the same edges in another order.
"""
import ctypes
import os

import numpy as np
import pytest

import id_diff_amd
from id_diff_amd import _lib, isomap

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "isomap_connect.npz")
U = 2.0 ** -53
SETS = ("arc193", "blobs257", "blobs600", "two130", "lattice")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def host_paths(X, nn):
    """Shortest paths of the nn-nearest-neighbour graph of X in numpy fp64 (+inf between components)."""
    X = X.astype(np.float64)
    d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    N = len(X)
    np.fill_diagonal(d, np.inf)
    idx = np.argsort(d, axis=1, kind="stable")[:, :nn]
    G = np.full((N, N), np.inf)
    G[np.repeat(np.arange(N), nn), idx.reshape(-1)] = np.take_along_axis(d, idx, axis=1).reshape(-1)
    G = np.minimum(G, G.T)
    np.fill_diagonal(G, 0.0)
    for k in range(N):
        np.minimum(G, G[:, k:k + 1] + G[k:k + 1, :], out=G)
    return G


@pytest.fixture(scope="module")
def paths(gold):
    return {name: host_paths(gold[f"{name}_X"], int(gold[f"{name}_nn"])) for name in SETS}


@pytest.mark.parametrize("name", SETS)
def test_labels_are_scipys(gold, paths, name):
    labels = isomap.component_labels(np.isfinite(paths[name]))
    assert labels.dtype == np.int64 and np.array_equal(labels, gold[f"{name}_labels"])
    assert isomap.count_components(np.isfinite(paths[name])) == labels.max() + 1


def test_labels_of_interleaved_blocks():
    finite = np.zeros((7, 7), dtype=bool)
    for block in ([1, 3, 4], [0, 6], [2], [5]):
        finite[np.ix_(block, block)] = True
    assert isomap.component_labels(finite).tolist() == [0, 1, 2, 1, 1, 3, 0]
    assert isomap.component_labels(np.ones((1, 1), dtype=bool)).tolist() == [0]


@pytest.mark.parametrize("name", SETS)
def test_bridges_are_sklearns(gold, name):
    """The pairs exactly (lattice: the one of five exactly tied pairs that scikit-learn's argmin takes); the weights against the
    generator's direct fp64 differences, (D + 2) 2^-53 relative for two orders of one sum of D squares and a square root."""
    X = gold[f"{name}_X"]
    bi, bj, bw = isomap.bridges_from_points(X, gold[f"{name}_labels"])
    C = int(gold[f"{name}_labels"].max()) + 1
    assert bi.dtype == bj.dtype == np.int64 and bw.dtype == np.float64 and len(bi) == C * (C - 1) // 2
    assert np.array_equal(bi, gold[f"{name}_bi"]) and np.array_equal(bj, gold[f"{name}_bj"])
    want = gold[f"{name}_bw_exact"]
    assert (np.abs(bw - want) <= (X.shape[1] + 2) * U * want).all()
    assert (gold[f"{name}_labels"][bi] > gold[f"{name}_labels"][bj]).all()


def _check_rows(got, ref, N, slack=0.0):
    assert np.isfinite(got).all()
    excess = (np.abs(got - ref) - slack) / (4 * N * U * np.maximum(ref, np.finfo(float).tiny))
    print(f"N = {N}: largest (|got - ref| - slack) / (4 N 2^-53 ref) = {excess.max():.3g}")
    assert excess.max() <= 1.0


@pytest.mark.parametrize("name", [s for s in SETS if s != "lattice"])
def test_repair_reproduces_sklearns_rows(gold, paths, name):
    """scikit-learn's own (rounded) edge weights go in, so the only difference is the order of the sums."""
    D0 = paths[name]
    N = len(D0)
    D = isomap.repair_geodesics(D0, (gold[f"{name}_bi"], gold[f"{name}_bj"], gold[f"{name}_bw"]))
    assert np.array_equal(D, D.T) and (np.diagonal(D) == 0).all()
    rows = gold[f"{name}_rows"]
    _check_rows(D[rows], gold[f"{name}_dist_rows"], N)
    if name == "two130":
        _check_rows(D, gold["two130_dist"], N)
    assert (D <= D0).all() and np.isinf(D0).any()


def test_repair_shortens_paths_inside_a_component(gold, paths):
    """arc193: the edges across the gap of the arc are short cuts for pairs of points that were connected all along.  A repair that
    only fills the infinite blocks leaves those geodesics up to 5 times too long."""
    D0, labels = paths["arc193"], gold["arc193_labels"]
    D = isomap.repair_geodesics(D0, (gold["arc193_bi"], gold["arc193_bj"], gold["arc193_bw"]))
    same = labels[:, None] == labels[None, :]
    assert np.isfinite(D0[same]).all() and np.isinf(D0[~same]).all()
    shorter = same & (D < D0 * (1 - 1e-9))
    assert shorter.sum() // 2 == int(gold["arc193_n_shortened"]) >= 100
    assert (D0[shorter] / D[shorter]).max() > 4.0


def test_errors_from_the_repaired_matrix_reproduce_sklearn(gold):
    """Both sides are fp64 LAPACK on the same matrix.  Two clusters put nearly all of ||K||_F^2 into lambda_1, so the error is a
    difference of nearly equal numbers: the bound is the propagation bound of tests/test_hip_geodesic.py (eigenvalues to
    delta = 5e-14 max|lambda|, ||K||_F^2 to N^2 2^-53 relative, doubled for scikit-learn's own rounding)."""
    ks, want = gold["two130_ks"].tolist(), gold["two130_err"]
    got, lam = isomap.errors_from_geodesics(gold["two130_dist"], ks, return_eigenvalues=True)
    N, delta = 130, 5e-14 * np.abs(lam).max()
    for k, g, w in zip(ks, got, want):
        head = np.abs(lam[:k])
        bound = 2 * (N * N * U * ((N * w) ** 2 + (head ** 2).sum()) + 2 * delta * head.sum()) / (2 * N * N * w)
        assert abs(g - w) <= bound, (k, g, w, bound)
    np.testing.assert_allclose(lam[:32], gold["two130_eig"], rtol=0, atol=delta)


# ---- arguments
def test_an_unknown_connect_raises_before_any_device_call(monkeypatch):
    X = np.zeros((8, 3), dtype=np.float32)
    monkeypatch.setattr(isomap, "_points", lambda X: pytest.fail("reached the device path"))
    for call in (lambda: isomap.geodesics(X, connect="nearest"), lambda: isomap.reconstruction_errors(X, [1], connect="nearest"),
                 lambda: isomap.Isomap(5, 2, connect="nearest"), lambda: isomap.run(None, connect=None)):
        with pytest.raises(ValueError, match="connect = "):
            call()
    assert isomap.Isomap(5, 2).connect == "raise" and isomap.Isomap(5, 2, connect="closest").connect == "closest"
    with pytest.raises(ValueError, match="route"):
        _lib.repair_geodesics(None, None, None, None, route="partial")


def test_more_than_1024_components_are_refused():
    assert isomap.C_MAX == 1024
    with pytest.raises(ValueError, match="1025 connected components"):
        isomap.bridges_from_points(np.zeros((1025, 2), dtype=np.float32), np.arange(1025))
    bi, bj, bw = isomap.bridges_from_points(np.arange(6, dtype=np.float32).reshape(3, 2), np.arange(3))
    assert (bi.tolist(), bj.tolist()) == ([1, 2, 2], [0, 0, 1]) and np.allclose(bw, np.sqrt(8) * np.array([1, 2, 1]))


def test_cli_connect_reaches_run(monkeypatch):
    from id_diff_amd.configs import utils as config_utils
    seen = []
    monkeypatch.setattr(config_utils, "read_config", lambda path: "the config")
    monkeypatch.setattr(isomap, "run", lambda config, **kw: seen.append((config, kw)) or ([], []))
    isomap.main(["--config", "unused.py", "--connect", "closest"])
    isomap.main(["--config", "unused.py"])
    assert [c for c, _ in seen] == ["the config"] * 2
    assert seen[0][1]["connect"] == "closest" and seen[1][1]["connect"] == "raise"
    with pytest.raises(SystemExit):
        isomap.main(["--config", "unused.py", "--connect", "nearest"])


# ---- the C ABI refuses bad arguments before touching the device (fabricated addresses: a call let through would fault)
_A, _B, _C, _D, _E, _F = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
_LABELS = lambda D=_A, N=8, labels=_B, count=_C, scratch=_D: ("idiff_component_labels_f64", [D, N, labels, count, scratch])
_BRIDGES = lambda X=_A, N=8, D=3, labels=_B, C=3, ws=_C, ws_bytes=48, bi=_D, bj=_E, bw=_F: (
    "idiff_component_bridges_f64", [X, N, D, labels, C, ws, ws_bytes, bi, bj, bw])
_MINPLUS = lambda A=_A, lda=5, B=_B, ldb=7, C=_C, ldc=7, m=4, n=7, p=5: ("idiff_minplus_f64", [A, lda, B, ldb, C, ldc, m, n, p])
_SYM = lambda G=_A, N=8: ("idiff_symmetrize_min_f64", [G, N])
_REFUSED = {
    "labels-N0": _LABELS(N=0), "labels-null_D": _LABELS(D=0), "labels-null_labels": _LABELS(labels=0), "labels-null_count": _LABELS(count=0),
    "labels-null_scratch": _LABELS(scratch=0),
    "bridges-N0": _BRIDGES(N=0), "bridges-D0": _BRIDGES(D=0), "bridges-one_component": _BRIDGES(C=1), "bridges-C_above_1024": _BRIDGES(N=2000, C=1025, ws_bytes=1 << 24),
    "bridges-C_above_N": _BRIDGES(N=2), "bridges-null_X": _BRIDGES(X=0), "bridges-null_labels": _BRIDGES(labels=0), "bridges-null_ws": _BRIDGES(ws=0),
    "bridges-null_bi": _BRIDGES(bi=0), "bridges-null_bj": _BRIDGES(bj=0), "bridges-null_bw": _BRIDGES(bw=0), "bridges-small_ws": _BRIDGES(ws_bytes=40),
    "bridges-misaligned_ws": _BRIDGES(ws=_C + 4),
    "minplus-m0": _MINPLUS(m=0), "minplus-n0": _MINPLUS(n=0), "minplus-p0": _MINPLUS(p=0), "minplus-null_A": _MINPLUS(A=0), "minplus-null_B": _MINPLUS(B=0),
    "minplus-null_C": _MINPLUS(C=0), "minplus-lda_below_p": _MINPLUS(lda=4), "minplus-ldb_below_n": _MINPLUS(ldb=6), "minplus-ldc_below_n": _MINPLUS(ldc=6),
    "minplus-C_is_A": _MINPLUS(C=_A), "minplus-C_inside_B": _MINPLUS(C=_B + 8 * 20),
    "symmetrize_min-N0": _SYM(N=0), "symmetrize_min-null_G": _SYM(G=0),
}


@pytest.fixture(scope="module")
def library():
    if not os.path.exists(_lib.library_path()):
        _lib.build()
    return ctypes.CDLL(_lib.library_path())


@pytest.mark.parametrize("case", sorted(_REFUSED))
def test_connect_entries_refuse_bad_arguments(library, case):
    symbol, args = _REFUSED[case]
    handle = _lib.lib()
    rc = getattr(handle, symbol)(*args, None)
    assert rc == 1001                                        # IDIFF_EINVAL
    assert handle.idiff_last_error().decode().startswith(symbol[len("idiff_"):].rsplit("_f64", 1)[0] + ": ")


def test_bridge_workspace_query(library):
    handle = _lib.lib()
    assert [handle.idiff_component_bridges_workspace_bytes(C) for C in (0, 1, 2, 3, 1024, 1025)] == [0, 0, 16, 48, 16 * 523776, 0]
    assert 0 < _lib.UPDATE_MAX_ENDPOINT_FRACTION <= 1
