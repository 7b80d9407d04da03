"""GPU: the geodesic stages of the Isomap curve (csrc/geodesic.hip) and isomap.reconstruction_errors end to end.

Oracles: a numpy construction of the neighbourhood graph (bit-equal), a numpy fp64 Floyd-Warshall of N vectorised steps
(local to this file), numpy fp64 centring, and scikit-learn's stored results (tests/golden/isomap.npz).

Bound of the shortest paths.  A path has at most N - 1 additions of non-negative terms on either side and only their order
differs: each side is within (N - 1) 2^-53 (1 + o(1)) of the exact length of the path it found, and min() and the rounded
addition are monotone, so neither side's result exceeds the rounded length of the other side's best path by more than that:
|got - ref| <= 4 N 2^-53 ref on the finite entries, +inf in exactly the same places, the diagonal exactly 0.
"""
import numpy as np
import pytest
import torch

import id_diff_amd
from id_diff_amd import _lib, isomap

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = _lib.APSP_TILE
U = 2.0 ** -53
SETS = ("roll257", "roll1000", "sphere193")


# ------------------------------------------------------------------------------------------- oracles
def np_graph(dist, idx):
    N, k = dist.shape
    G = np.full((N, N), np.inf)
    np.fill_diagonal(G, 0.0)
    G[np.repeat(np.arange(N), k), idx.reshape(-1)] = dist.reshape(-1)
    return np.minimum(G, G.T)


def np_floyd_warshall(G):
    D = G.copy()
    for k in range(D.shape[0]):
        np.minimum(D, D[:, k:k + 1] + D[k:k + 1, :], out=D)
    return D


def check_paths(got, ref, rows=None):
    N = got.shape[1]
    if rows is None:
        assert (np.diagonal(got) == 0).all()
    else:
        assert (got[np.arange(len(rows)), rows] == 0).all()
    assert not np.isnan(got).any()
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    assert (got[~fin] == np.inf).all()
    excess = np.abs(got[fin] - ref[fin]) / (4 * N * U * np.maximum(ref[fin], np.finfo(float).tiny))
    print(f"N = {N}: largest |got - ref| / (4 N 2^-53 ref) = {excess.max():.3g}")
    assert excess.max() <= 1.0


# ------------------------------------------------------------------------------------------- inputs, each made once
@pytest.fixture(scope="module")
def gold(golden):
    return golden("isomap.npz")


def device_graph(X, k):
    """(dist, idx) of the exact kNN as numpy and the device graph built from them."""
    dist, idx, _ = _lib.knn(torch.as_tensor(X).to(DEV).contiguous(), k)
    return dist.cpu().numpy(), idx.cpu().numpy(), _lib.knn_graph(dist, idx)


@pytest.fixture(scope="module")
def fixture_paths(gold):
    """name -> (graph as numpy, device geodesics as numpy) of the three fixture sets, computed once."""
    out = {}
    for name in SETS:
        _, _, G = device_graph(gold[f"{name}_X"], int(gold[f"{name}_nn"]))
        g = G.cpu().numpy()
        out[name] = (g, _lib.geodesic_distances(G).cpu().numpy())
    return out


def shuffled_chain():
    """3 T + 5 points on a line, spacings in [1, 1.5) (so the two nearest points of an inner point are its two neighbours on
    the line and the graph is the chain), vertex order permuted: the path between the ends has about 3 T + 4 edges (an end vertex's second neighbour
    is two steps along the line) and hops between tiles in both directions."""
    rng = np.random.default_rng(11)
    n = 3 * T + 5
    pos = np.cumsum(1.0 + 0.5 * rng.random(n))
    return pos[rng.permutation(n)].astype(np.float32)[:, None]


def two_clusters():
    """40 + 45 points on two circles 100 apart (angles jittered by a tenth of the spacing: with k = 4 each circle is connected
    through its +-1, +-2 neighbours), vertex order permuted."""
    rng = np.random.default_rng(12)
    pts = []
    for n, off in ((40, 0.0), (45, 100.0)):
        a = (np.arange(n) + 0.1 * rng.uniform(-1, 1, n)) * 2 * np.pi / n
        pts.append(np.stack([np.cos(a) + off, np.sin(a), np.zeros(n)], axis=1))
    X = np.concatenate(pts)
    perm = rng.permutation(len(X))
    return X[perm].astype(np.float32), perm < 40              # and which points are of the first circle


# ------------------------------------------------------------------------------------------- knn_graph
@pytest.mark.parametrize("N", [2, 40, 65, 257])
def test_knn_graph_is_bit_equal_to_numpy(gold, N):
    dist, idx, G = device_graph(gold["roll257_X"][:N], min(8, N - 1))
    got = G.cpu().numpy()
    assert got.shape == (N, N) and got.dtype == np.float64
    assert np.array_equal(got, np_graph(dist, idx))
    assert np.array_equal(got, got.T) and (np.diagonal(got) == 0).all()


# ------------------------------------------------------------------------------------------- shortest paths
@pytest.mark.parametrize("N", [1, 2, T - 1, T, T + 1, 193, 257, 4 * T])
def test_apsp_sizes_around_the_tile(gold, N):
    """The first N points of the N = 1000 roll with 8 neighbours (any graph serves: a disconnected one checks the +inf pattern)."""
    if N == 1:
        G = torch.zeros(1, 1, dtype=torch.float64, device=DEV)
    else:
        _, _, G = device_graph(gold["roll1000_X"][:N], min(8, N - 1))
    ref = np_floyd_warshall(G.cpu().numpy())
    out = _lib.geodesic_distances(G)
    assert out is G
    check_paths(G.cpu().numpy(), ref)


@pytest.mark.parametrize("name", SETS)
def test_apsp_fixture_sets(fixture_paths, name):
    g, got = fixture_paths[name]
    check_paths(got, np_floyd_warshall(g))
    assert np.isfinite(got).all()


def test_apsp_shuffled_chain():
    X = shuffled_chain()
    dist, idx, G = device_graph(X, 2)
    g = G.cpu().numpy()
    assert (np.isfinite(g).sum(axis=1) <= 4).all()                         # the chain (an end vertex also reaches one further)
    got = _lib.geodesic_distances(G).cpu().numpy()
    check_paths(got, np_floyd_warshall(g))
    lo, hi = int(X.argmin()), int(X.argmax())
    assert abs(got[lo, hi] - (float(X.max()) - float(X.min()))) <= 1e-12 * got[lo, hi]  # the whole line (differences of fp32 positions are exact)


def test_apsp_two_clusters_keep_their_inf_block():
    X, first = two_clusters()
    _, _, G = device_graph(X, 4)
    g = G.cpu().numpy()
    got = _lib.geodesic_distances(G).cpu().numpy()
    check_paths(got, np_floyd_warshall(g))
    same = first[:, None] == first[None, :]
    assert np.isfinite(got[same]).all() and (got[~same] == np.inf).all()


def test_apsp_rows_against_sklearn_dijkstra(gold, fixture_paths):
    """16 stored rows of scikit-learn's dist_matrix_ per set, N = 1000 among them: Floyd-Warshall against Dijkstra."""
    for name in SETS:
        rows = gold[f"{name}_rows"]
        check_paths(fixture_paths[name][1][rows], gold[f"{name}_dist_rows"], rows=rows)


# ------------------------------------------------------------------------------------------- centring
@pytest.mark.parametrize("name", ["sphere193", "roll257"])
def test_double_center(fixture_paths, name):
    D = fixture_paths[name][1]
    N = D.shape[0]
    Dd = torch.from_numpy(D).to(DEV)
    K, fro2 = _lib.double_center(Dd)
    assert np.array_equal(Dd.cpu().numpy(), D)                             # D is only read
    S = D ** 2
    ref = -0.5 * (S - S.mean(axis=1, keepdims=True) - S.mean(axis=0, keepdims=True) + S.mean())
    diff = np.abs(K.cpu().numpy() - ref).max()
    bound = (N + 8) * U * S.max()
    rel = abs(float(fro2) - (ref ** 2).sum()) / (ref ** 2).sum()
    print(f"{name}: max |K - ref| = {diff:.3g} (bound {bound:.3g}), fro2 relative difference {rel:.3g} (bound {N * N * U:.3g})")
    assert diff <= bound
    assert rel <= N * N * U


# ------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", SETS)
def test_reconstruction_errors_against_sklearn(gold, name):
    """Bound from the project's own eigenvalue accuracy: tests/test_hip_spectrum.py holds sym_eigvals to delta = 5e-14 max|lambda|,
    double_center's ||K||_F^2 to dF = N^2 2^-53 ||K||_F^2; with R(k) = ||K||_F^2 - sum_{i<k} lambda_i^2 and err = sqrt(R) / N,
    |d err(k)| <= (dF + 2 delta sum_{i<k} |lambda_i|) / (2 N^2 err(k)), doubled for scikit-learn's own rounding."""
    X, nn = gold[f"{name}_X"], int(gold[f"{name}_nn"])
    ks, want, eig32 = gold[f"{name}_ks"].tolist(), gold[f"{name}_err"], gold[f"{name}_eig"]
    N = X.shape[0]
    got, lam = isomap.reconstruction_errors(X, ks, n_neighbors=nn, return_eigenvalues=True)
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


# ------------------------------------------------------------------------------------------- error paths
def test_geodesics_names_the_components():
    X, _ = two_clusters()
    with pytest.raises(ValueError, match="2 connected components"):
        isomap.geodesics(X, n_neighbors=4)
    with pytest.raises(ValueError, match="2 connected components"):
        isomap.reconstruction_errors(X, [1, 2], n_neighbors=4)


def test_more_points_than_the_eigensolver_is_exercised_at():
    with pytest.raises(ValueError, match="12288"):
        isomap.reconstruction_errors(np.zeros((12289, 3), dtype=np.float32), [1])


def test_k_beyond_the_positive_eigenvalues_raises(gold):
    X = gold["sphere193_X"]
    with pytest.raises(ValueError, match="positive eigenvalues"):
        isomap.reconstruction_errors(X, [1, 193], n_neighbors=6)
