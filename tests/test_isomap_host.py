"""Host side of the Isomap reconstruction-error curve (no GPU): the arithmetic after the eigenvalues against scikit-learn's
stored results (tests/golden/isomap.npz, written by tests/golden/make_isomap.py), the component counter, and what the three
C entry points of csrc/geodesic.hip refuse before any device call."""
import ctypes
import os

import numpy as np
import pytest

import id_diff_amd
from id_diff_amd import _lib, isomap

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "isomap.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def test_errors_from_geodesics_reproduce_sklearn(gold):
    """Both sides are fp64 LAPACK on the same matrix: 1e-12 relative (measured 2e-15)."""
    ks, want = gold["sphere193_ks"].tolist(), gold["sphere193_err"]
    got, lam = isomap.errors_from_geodesics(gold["sphere193_dist"], ks, return_eigenvalues=True)
    rel = np.abs(np.array(got) - want) / want
    print("relative differences:", rel)
    assert {1, 2, 3, 5, 10} <= set(ks)
    assert rel.max() <= 1e-12
    np.testing.assert_allclose(lam[:32], gold["sphere193_eig"], rtol=0, atol=1e-12 * lam[0])
    assert np.all(np.diff(lam) <= 0)


def test_rows_of_the_stored_matrix_are_its_rows(gold):
    np.testing.assert_array_equal(gold["sphere193_dist"][gold["sphere193_rows"]], gold["sphere193_dist_rows"])
    for name, n in (("roll257", 257), ("roll1000", 1000), ("sphere193", 193)):
        assert gold[f"{name}_X"].shape[0] == n and gold[f"{name}_X"].dtype == np.float32
        assert gold[f"{name}_dist_rows"].shape == (16, n) and gold[f"{name}_eig"].shape == (32,)


def test_k_beyond_the_positive_eigenvalues_raises(gold):
    D = gold["sphere193_dist"]
    _, lam = isomap.errors_from_geodesics(D, [1], return_eigenvalues=True)
    pos = isomap.n_positive(lam)
    assert 10 < pos < 193                       # a geodesic kernel is not positive semi-definite
    assert len(isomap.errors_from_geodesics(D, [pos])) == 1
    with pytest.raises(ValueError, match=f"{pos} positive eigenvalues"):
        isomap.errors_from_geodesics(D, [1, pos + 1])
    with pytest.raises(ValueError):
        isomap.errors_from_geodesics(D, [0])
    assert isomap.n_positive([3.0, 1.0, 1e-13, -2.0]) == 2 and isomap.n_positive([-1.0]) == 0 and isomap.n_positive([]) == 0


def test_error_formula_on_a_hand_made_spectrum():
    lam = np.array([4.0, 2.0, 1.0, -1.0])
    fro2 = float((lam ** 2).sum())
    got = isomap.errors_from_eigenvalues(fro2, lam, 4, [1, 2, 3])
    assert got == [np.sqrt(6.0) / 4, np.sqrt(2.0) / 4, 1.0 / 4]


def test_component_counter_on_two_blocks():
    finite = np.zeros((7, 7), dtype=bool)
    a, b = [0, 2, 5], [1, 3, 4, 6]              # interleaved: the blocks are not contiguous index ranges
    finite[np.ix_(a, a)] = True
    finite[np.ix_(b, b)] = True
    assert isomap.count_components(finite) == 2
    assert isomap.count_components(np.ones((5, 5), dtype=bool)) == 1
    assert isomap.count_components(np.eye(4, dtype=bool)) == 4
    D = np.where(finite, 1.0, np.inf)
    np.fill_diagonal(D, 0.0)
    with pytest.raises(ValueError, match="2 connected components"):
        isomap.errors_from_geodesics(D, [1])


def test_more_points_than_the_eigensolver_is_exercised_at_raise_before_any_device_call():
    with pytest.raises(ValueError, match="12288"):
        isomap.reconstruction_errors(np.zeros((12289, 3), dtype=np.float32), [1])


def test_default_ks_are_the_reference_list():
    assert isomap.DEFAULT_KS == list(range(1, 11)) + list(range(11, 200, 10)) and len(isomap.DEFAULT_KS) == 29
    assert isomap.N_MAX == 12288


# ---- the C ABI refuses bad arguments before touching the device (fabricated addresses: a call let through would fault)
_A, _B, _C, _D = 0x10000, 0x20000, 0x30000, 0x40000
_GRAPH = lambda dist=_A, idx=_B, N=8, k=3, G=_C: ("idiff_knn_graph_f64", [dist, idx, N, k, G])
_APSP = lambda G=_A, N=8: ("idiff_apsp_f64", [G, N])
_CENTER = lambda D=_A, N=8, K=_B, fro2=_C, scratch=_D: ("idiff_double_center_f64", [D, N, K, fro2, scratch])
_REFUSED = {
    "graph-N0": _GRAPH(N=0, k=0), "graph-N_negative": _GRAPH(N=-1), "graph-k_negative": _GRAPH(k=-1), "graph-k_above_N_minus_1": _GRAPH(k=8),
    "graph-null_dist": _GRAPH(dist=0), "graph-null_idx": _GRAPH(idx=0), "graph-null_G": _GRAPH(G=0),
    "apsp-N0": _APSP(N=0), "apsp-null_G": _APSP(G=0),
    "center-N0": _CENTER(N=0), "center-null_D": _CENTER(D=0), "center-null_K": _CENTER(K=0), "center-null_fro2": _CENTER(fro2=0),
    "center-null_scratch": _CENTER(scratch=0),
}


@pytest.fixture(scope="module")
def library():
    if not os.path.exists(_lib.library_path()):
        _lib.build()
    return ctypes.CDLL(_lib.library_path())


@pytest.mark.parametrize("case", sorted(_REFUSED))
def test_geodesic_entries_refuse_bad_arguments(library, case):
    symbol, args = _REFUSED[case]
    handle = _lib.lib()
    rc = getattr(handle, symbol)(*args, None)
    assert rc == 1001                                        # IDIFF_EINVAL
    assert handle.idiff_last_error().decode().startswith(symbol[len("idiff_"):].rsplit("_f64", 1)[0] + ": ")


def test_tile_and_scratch_queries(library):
    handle = _lib.lib()
    assert handle.idiff_apsp_tile() == _lib.APSP_TILE == 64
    assert handle.idiff_double_center_scratch_doubles(0) == 0
    assert handle.idiff_double_center_scratch_doubles(193) >= 193
