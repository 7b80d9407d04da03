"""GPU: ``connect="closest"``, scikit-learn's repair of a disconnected neighbourhood graph, stage by stage and end to end
(csrc/graph_connect.hip, idiff_minplus_f64 of csrc/geodesic.hip, _lib.repair_geodesics, isomap.*), against scikit-learn's stored
results (tests/golden/isomap_connect.npz, written by tests/golden/make_isomap_connect.py) and the numpy restatements of isomap.py.

Bounds.  Labels and the pairs of points are integers: exact.  An edge weight is one sum of D squares and a square root on either
side, in another order: (D + 2) 2^-53 relative.  The (min, +) product rounds each sum once, as numpy does: 2 * 2^-53 relative is
asked, equality is what one expects.  Shortest paths: |got - ref| <= 4 N 2^-53 ref as in tests/test_hip_geodesic.py (either side
sums the same non-negative edges in another order); against scikit-learn's rows the bound is widened by B max|w_sklearn - w_exact|,
since a shortest path uses each of the B added edges at most once and scikit-learn's expanded distance formula rounds its
weights.  The curve and the embedding: the bounds of tests/test_hip_geodesic.py and tests/test_hip_isomap_embed.py, restated below.
"""
import warnings

import numpy as np
import pytest
import torch

import id_diff_amd
from id_diff_amd import _lib, isomap

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -53
SETS = ("arc193", "blobs257", "blobs600", "two130", "lattice")
KERNEL_SETS = SETS[:-1]                 # lattice stores only its labels and its edge


@pytest.fixture(scope="module")
def gold(golden):
    return golden("isomap_connect.npz")


@pytest.fixture(scope="module")
def stages(gold):
    """name -> the device stages of one set, each computed once: the first shortest paths D0 (numpy), labels, C, the edges (numpy),
    and the matrices of both routes (numpy)."""
    out = {}
    for name in SETS:
        X = torch.from_numpy(gold[f"{name}_X"]).to(DEV)
        dist, idx, _ = _lib.knn(X, int(gold[f"{name}_nn"]))
        D0 = _lib.geodesic_distances(_lib.knn_graph(dist, idx))
        d0 = D0.cpu().numpy()
        labels, count = _lib.component_labels(D0)
        assert np.array_equal(D0.cpu().numpy(), d0)                           # only read
        C = int(count)
        bridges = _lib.component_bridges(X, labels, C)
        full = _lib.repair_geodesics(D0.clone(), *bridges, route="full", knn=(dist, idx)).cpu().numpy()
        update = _lib.repair_geodesics(D0, *bridges, route="update").cpu().numpy()
        out[name] = dict(D0=d0, labels=labels.cpu().numpy(), C=C, bridges=tuple(b.cpu().numpy() for b in bridges), full=full, update=update)
    return out


def check_paths(got, ref, slack=0.0):
    N = got.shape[1]
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    excess = (np.abs(got - ref) - slack) / (4 * N * U * np.maximum(ref, np.finfo(float).tiny))
    print(f"N = {N}: largest (|got - ref| - {slack:.3g}) / (4 N 2^-53 ref) = {excess.max():.3g}")
    assert excess.max() <= 1.0


# ------------------------------------------------------------------------------------------- labels
@pytest.mark.parametrize("name", SETS)
def test_labels_are_scipys(gold, stages, name):
    s = stages[name]
    assert s["labels"].dtype == np.int32 and np.array_equal(s["labels"], gold[f"{name}_labels"])
    assert s["C"] == int(gold[f"{name}_labels"].max()) + 1
    assert np.array_equal(s["labels"], isomap.component_labels(np.isfinite(s["D0"])))


@pytest.mark.parametrize("N,C", [(1, 1), (65, 1), (65, 4), (300, 7), (300, 300)])
def test_labels_of_a_made_up_pattern(N, C):
    """Interleaved components, a matrix that is no multiple of the wave or of the scan's 256, every vertex its own component."""
    rng = np.random.default_rng(N + C)
    member = np.arange(N) if C == N else rng.integers(0, C, N)
    member[:min(C, N)] = rng.permutation(min(C, N))                           # every component has a vertex
    D = np.where(member[:, None] == member[None, :], rng.random((N, N)) + 1.0, np.inf)
    np.fill_diagonal(D, 0.0)
    labels, count = _lib.component_labels(torch.from_numpy(D).to(DEV))
    assert int(count) == C
    assert np.array_equal(labels.cpu().numpy(), isomap.component_labels(np.isfinite(D)))


# ------------------------------------------------------------------------------------------- the edges
@pytest.mark.parametrize("name", SETS)
def test_bridges_are_sklearns(gold, stages, name):
    """lattice: five pairs tie exactly; scikit-learn's argmin takes the first in row-major order over the ranks."""
    bi, bj, bw = stages[name]["bridges"]
    D = gold[f"{name}_X"].shape[1]
    assert bi.dtype == bj.dtype == np.int64 and bw.dtype == np.float64
    assert np.array_equal(bi, gold[f"{name}_bi"]) and np.array_equal(bj, gold[f"{name}_bj"])
    want = gold[f"{name}_bw_exact"]
    rel = np.abs(bw - want) / want
    print(f"{name}: largest |w - numpy| / ((D + 2) 2^-53 w) = {(rel / ((D + 2) * U)).max():.3g}")
    assert (rel <= (D + 2) * U).all()
    hi, hj, hw = isomap.bridges_from_points(gold[f"{name}_X"], stages[name]["labels"])
    assert np.array_equal(bi, hi) and np.array_equal(bj, hj)


def test_bridge_ties_do_not_depend_on_the_tile():
    """Two columns of 40 points on integer coordinates, 7 apart, rows permuted over three 32-point tiles: every point is exactly 7 from its
    partner and further from everything else of the other column, so 40 pairs tie across all the tile pairs.  The smallest a of
    component 1 wins, with its partner."""
    rng = np.random.default_rng(5)
    left = np.stack([np.zeros(40), 10.0 * np.arange(40)], axis=1)
    order = rng.permutation(80)
    X = np.concatenate([left, left + np.array([7.0, 0.0])]).astype(np.float32)[order]
    side = (order >= 40)
    member = (side != side[0]).astype(np.int64)                               # vertex 0 names component 0
    labels = torch.from_numpy(member.astype(np.int32)).to(DEV)
    bi, bj, bw = (t.cpu().numpy() for t in _lib.component_bridges(torch.from_numpy(X).to(DEV), labels, 2))
    a = int(np.flatnonzero(member == 1)[0])
    b = int(np.flatnonzero((X[:, 1] == X[a, 1]) & (member == 0))[0])
    assert (bi.tolist(), bj.tolist(), bw.tolist()) == ([a], [b], [7.0])
    hi, hj, hw = isomap.bridges_from_points(X, member)
    assert (hi.tolist(), hj.tolist(), hw.tolist()) == ([a], [b], [7.0])


# ------------------------------------------------------------------------------------------- the (min, +) product
@pytest.mark.parametrize("p", [1, 2, 63, 64, 65, 130])
def test_minplus_against_numpy(p):
    rng = np.random.default_rng(p)
    worst = 0.0
    for m in (1, 63, 64, 65, 193):
        for n in (1, 63, 64, 65, 193):
            A, B, C = rng.random((m, p)) * 3, rng.random((p, n)) * 3, rng.random((m, n)) * 4 + 1
            A[rng.random((m, p)) < 0.2] = np.inf
            B[rng.random((p, n)) < 0.2] = np.inf
            C[rng.random((m, n)) < 0.5] = np.inf
            A[rng.integers(m)] = np.inf                                       # a whole +inf row of A: that row of C stays
            if p > 1:
                B[rng.integers(p)] = np.inf
            ref = np.minimum(C, (A[:, :, None] + B[None, :, :]).min(axis=1))
            Cd = torch.from_numpy(C).to(DEV)
            out = _lib.minplus(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV), Cd)
            assert out is Cd
            got = Cd.cpu().numpy()
            fin = np.isfinite(ref)
            assert not np.isnan(got).any() and np.array_equal(np.isfinite(got), fin) and (got[~fin] == np.inf).all()
            if fin.any():
                worst = max(worst, (np.abs(got[fin] - ref[fin]) / ref[fin]).max())
    print(f"p = {p}: largest relative difference {worst:.3g} (bound {2 * U:.3g})")
    assert worst <= 2 * U


def test_minplus_on_views_with_a_pitch():
    rng = np.random.default_rng(3)
    big = [torch.from_numpy(rng.random(s) + 0.5).to(DEV) for s in ((70, 90), (80, 100), (70, 110))]
    A, B, C = big[0][:65, 3:3 + 66], big[1][2:2 + 66, :67], big[2][1:66, 5:5 + 67]
    keep = big[2].clone()
    ref = np.minimum(C.cpu().numpy(), (A.cpu().numpy()[:, :, None] + B.cpu().numpy()[None, :, :]).min(axis=1))
    _lib.minplus(A, B, C)
    assert np.array_equal(C.cpu().numpy(), ref)
    keep[1:66, 5:5 + 67] = C
    assert torch.equal(big[2], keep)                                          # nothing outside the view is written
    with pytest.raises(RuntimeError, match="overlaps"):
        _lib.minplus(big[0][:, :70], big[0], big[0][:, :90])


# ------------------------------------------------------------------------------------------- both routes of the repair
@pytest.mark.parametrize("route", ["update", "full"])
@pytest.mark.parametrize("name", SETS)
def test_routes_against_the_host_repair(stages, name, route):
    s = stages[name]
    got = s[route]
    assert np.array_equal(got, got.T) and (np.diagonal(got) == 0).all()       # bit-symmetric, zero diagonal: double_center assumes both
    check_paths(got, isomap.repair_geodesics(s["D0"], s["bridges"]))
    assert np.isinf(s["D0"]).any()


@pytest.mark.parametrize("route", ["update", "full"])
@pytest.mark.parametrize("name", KERNEL_SETS)
def test_routes_against_sklearns_rows(gold, stages, name, route):
    rows = gold[f"{name}_rows"]
    slack = len(gold[f"{name}_bw"]) * np.abs(gold[f"{name}_bw"] - gold[f"{name}_bw_exact"]).max()
    check_paths(stages[name][route][rows], gold[f"{name}_dist_rows"], slack=slack)
    if name == "two130":
        check_paths(stages[name][route], gold["two130_dist"], slack=slack)


def test_the_repair_shortens_paths_inside_a_component(gold, stages):
    s, labels = stages["arc193"], gold["arc193_labels"]
    same = labels[:, None] == labels[None, :]
    for route in ("update", "full"):
        shorter = same & (s[route] < s["D0"] * (1 - 1e-9))
        assert shorter.sum() // 2 == int(gold["arc193_n_shortened"])


def test_default_route_and_its_threshold(gold, stages):
    """route=None updates up to UPDATE_MAX_ENDPOINT_FRACTION (two130: 2 endpoints of 130 points) and solves again above it."""
    X = torch.from_numpy(gold["two130_X"]).to(DEV)
    dist, idx, _ = _lib.knn(X, 5)
    D0 = torch.from_numpy(stages["two130"]["D0"]).to(DEV)
    b = tuple(torch.from_numpy(v).to(DEV) for v in stages["two130"]["bridges"])
    assert np.array_equal(_lib.repair_geodesics(D0.clone(), *b, knn=(dist, idx)).cpu().numpy(), stages["two130"]["update"])
    keep = _lib.UPDATE_MAX_ENDPOINT_FRACTION
    try:
        _lib.UPDATE_MAX_ENDPOINT_FRACTION = 1.0 / 130
        assert np.array_equal(_lib.repair_geodesics(D0.clone(), *b, knn=(dist, idx)).cpu().numpy(), stages["two130"]["full"])
    finally:
        _lib.UPDATE_MAX_ENDPOINT_FRACTION = keep
    with pytest.raises(ValueError, match="knn"):
        _lib.repair_geodesics(D0, *b, route="full")


# ------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", KERNEL_SETS)
def test_geodesics_warn_once_and_return_the_update(gold, stages, name):
    X, nn = gold[f"{name}_X"], int(gold[f"{name}_nn"])
    with pytest.warns(UserWarning, match=f"{stages[name]['C']} connected components") as seen:
        D = isomap.geodesics(X, nn, connect="closest")
    assert len(seen) == 1
    assert np.array_equal(D.cpu().numpy(), stages[name]["update"])


@pytest.mark.parametrize("name", KERNEL_SETS)
def test_reconstruction_errors_against_sklearn(gold, name):
    """The bound of tests/test_hip_geodesic.py::test_reconstruction_errors_against_sklearn: sym_eigvals is held to
    delta = 5e-14 max|lambda|, double_center's ||K||_F^2 to dF = N^2 2^-53 ||K||_F^2; with R(k) = ||K||_F^2 - sum_{i<k} lambda_i^2 and
    err = sqrt(R) / N, |d err(k)| <= (dF + 2 delta sum_{i<k} |lambda_i|) / (2 N^2 err(k)), doubled for scikit-learn's own rounding."""
    X, nn = gold[f"{name}_X"], int(gold[f"{name}_nn"])
    ks, want, eig32 = gold[f"{name}_ks"].tolist(), gold[f"{name}_err"], gold[f"{name}_eig"]
    N = X.shape[0]
    with pytest.warns(UserWarning, match="connected components"):
        got, lam = isomap.reconstruction_errors(X, ks, n_neighbors=nn, return_eigenvalues=True, connect="closest")
    assert lam.shape == (N,) and np.all(np.diff(lam) <= 0)
    delta = 5e-14 * np.abs(lam).max()
    print(f"{name}: max |lambda - stored| / delta = {np.abs(lam[:32] - eig32).max() / delta:.3g}")
    assert np.abs(lam[:32] - eig32).max() <= delta
    worst = 0.0
    for k, g, w in zip(ks, got, want):
        head = np.abs(lam[:k])
        fro2 = (N * w) ** 2 + (head ** 2).sum()
        bound = 2 * (N * N * U * fro2 + 2 * delta * head.sum()) / (2 * N * N * w)
        worst = max(worst, abs(g - w) / bound)
        print(f"{name}: k = {k}: got {g!r}, scikit-learn {w!r}, |difference| / bound = {abs(g - w) / bound:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", KERNEL_SETS)
def test_isomap_fit_and_transform_against_sklearn(gold, stages, name):
    """The criterion of tests/test_hip_isomap_embed.py: fit() accepts a basis with a residual within 1e-9 lambda_1 sqrt(k), so
    |embedding_ - scikit-learn|_max <= 10 (1e-9 / g_min) max|Z| with g_min the smallest relative gap the 3 columns depend on (stored),
    and 100 (1e-9 / g_min) max|Z| for transform() of the 24 held-out points.  Column signs are compared as returned."""
    X, nn, gmin = gold[f"{name}_X"], int(gold[f"{name}_nn"]), float(gold[f"{name}_k3_gmin"])
    want, want_tr = gold[f"{name}_k3_emb"], gold[f"{name}_k3_tr"]
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        iso = isomap.Isomap(nn, 3, connect="closest")
        Z = iso.fit_transform(X)
    assert len(seen) == 1 and issubclass(seen[0].category, UserWarning) and f"{stages[name]['C']} connected components" in str(seen[0].message)
    assert Z is iso.embedding_ and Z.dtype == torch.float64 and tuple(Z.shape) == want.shape
    assert isinstance(iso.n_connected_components_, int) and iso.n_connected_components_ == stages[name]["C"]
    for mine, stored, dtype in zip(iso.bridges_, (gold[f"{name}_bi"], gold[f"{name}_bj"], gold[f"{name}_bw_exact"]), (np.int64, np.int64, np.float64)):
        assert isinstance(mine, np.ndarray) and mine.dtype == dtype and mine.shape == stored.shape
    assert np.array_equal(iso.bridges_[0], gold[f"{name}_bi"]) and np.array_equal(iso.bridges_[1], gold[f"{name}_bj"])
    assert np.array_equal(iso.bridges_[2], stages[name]["bridges"][2])
    assert np.array_equal(iso.dist_matrix_.cpu().numpy(), stages[name]["update"])
    Z, scale = Z.cpu().numpy(), np.abs(want).max()
    d_emb = np.abs(Z - want).max()
    d_tr = np.abs(iso.transform(gold[f"{name}_Xq"]).cpu().numpy() - want_tr).max()
    print(f"{name}: g_min = {gmin:.3g}; |embedding_ - scikit-learn| / max|Z| = {d_emb / scale:.3g} (bound {10 * 1e-9 / gmin:.3g}); "
          f"|transform - scikit-learn| / max|Z| = {d_tr / scale:.3g} (bound {100 * 1e-9 / gmin:.3g}); plan {iso.plan_}")
    assert d_emb <= 10 * (1e-9 / gmin) * scale
    assert d_tr <= 100 * (1e-9 / gmin) * scale
    np.testing.assert_allclose(iso.eigenvalues_, gold[f"{name}_eig"][:3], rtol=0, atol=1e-10 * gold[f"{name}_eig"][0])
    assert iso.reconstruction_error() == isomap.errors_from_eigenvalues(*_spectrum(iso, X, nn), [3])[0]


def _spectrum(iso, X, nn):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return isomap._kernel_spectrum(X, nn, connect="closest")


# ------------------------------------------------------------------------------------------- what does not change
def test_a_connected_graph_is_left_alone(golden):
    pts = golden("isomap.npz")
    X, nn = pts["sphere193_X"], int(pts["sphere193_nn"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        D = isomap.geodesics(X, nn, connect="closest")
        iso = isomap.Isomap(nn, 2, connect="closest").fit(X)
    assert torch.equal(D, isomap.geodesics(X, nn)) and torch.equal(D, isomap.geodesics(X, nn, connect="raise"))
    assert iso.n_connected_components_ == 1 and [len(b) for b in iso.bridges_] == [0, 0, 0]
    assert [b.dtype for b in iso.bridges_] == [np.int64, np.int64, np.float64]
    plain = isomap.Isomap(nn, 2).fit(X)
    assert torch.equal(iso.embedding_, plain.embedding_) and plain.n_connected_components_ == 1


def test_the_default_still_raises(gold):
    X = gold["two130_X"]
    for kw in ({}, {"connect": "raise"}):
        with pytest.raises(ValueError, match="2 connected components"):
            isomap.geodesics(X, 5, **kw)
        with pytest.raises(ValueError, match="2 connected components"):
            isomap.reconstruction_errors(X, [1, 2], n_neighbors=5, **kw)
        with pytest.raises(ValueError, match="2 connected components"):
            isomap.Isomap(5, 2, **kw).fit(X)
