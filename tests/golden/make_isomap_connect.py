"""Generator of tests/golden/isomap_connect.npz: scikit-learn's Isomap on point sets whose neighbourhood graph is NOT connected,
so that scikit-learn joins the components (sklearn.utils.graph._fix_connected_components, mode="distance") before it goes on
(CPU only).

    python tests/golden/make_isomap_connect.py

Needs scikit-learn >= 1.7, scipy and numpy; eigen_solver="dense" and fp64 copies of the fp32 points as in make_isomap.py.
neighbors_algorithm="kd_tree": the tree measures neighbour distances by direct differences.  "auto" sends 16 and 24 dimensions to
brute force, whose expanded formula |x|^2 + |y|^2 - 2 x.y rounds every edge of the neighbourhood graph by about |x|^2 / d^2 ulps
(thousands, for clusters far from the origin): scikit-learn's rounding, not Isomap's, and far outside the bound of a shortest
path.  The edges that JOIN the components do come from that formula (pairwise_distances), which is why both weights are stored.
Per set `s` the file holds

    s_X, s_nn           the points [N, D] float32, n_neighbors
    s_labels            scipy's connected_components labels of the neighbourhood graph [N] int64
    s_bi, s_bj, s_bw    the edges scikit-learn adds, in its order (component i = 1 .. C - 1, j < i): the point of component i, the
                        point of component j, and ITS weight (pairwise_distances: the expanded formula, rounded)
    s_bw_exact          the same edges' weights by direct differences in numpy fp64: sqrt(sum_d (a_d - b_d)^2)
    s_rows, s_dist_rows 16 fixed row indices and dist_matrix_[rows];  two130_dist the full matrix of two130
    arc193_n_shortened  the number of pairs of points of ONE component whose geodesic the added edges shorten
    s_ks, s_err         reconstruction_error() for the k of make_isomap.py that scikit-learn accepts, up to the number of positive
                        eigenvalues (beyond it isomap.reconstruction_errors raises by contract)
    s_eig               the top 32 eigenvalues of the centred kernel (LAPACK, descending)
    s_k3_emb, s_k3_tr   embedding_ for 3 components and transform of the 24 held-out points s_Xq
    s_k3_gmin           min_{i <= 3} (lambda_i - lambda_{i+1}) / lambda_1

(`lattice` holds only X, nn, labels and the edges: its kernel is of no interest.)  The edges are found here by the loop of
_fix_connected_components with scikit-learn's own pairwise_distances, and the generator asserts that the shortest paths of the
neighbourhood graph plus these edges ARE scikit-learn's dist_matrix_, bit for bit.  It also asserts, for every set but `lattice`,
that the runner-up of every edge is more than 1e-9 relative away (a more exact distance cannot pick another pair), and that the
24 queries' neighbour sets do not hang on a rounding.

The sets:  arc193: 150 points on a 300-degree arc of radius 10 and blobs of 20 and 23 points in its gap, a 2-D figure embedded
isometrically in 9-D, rows permuted, k = 5: 3 components, and the edges across the gap shorten geodesics INSIDE the arc;
blobs257, blobs600: 5 clusters in 16-D, 9 clusters in 24-D (3-dimensional blobs), k = 5; two130: two clusters of 65 points;
lattice: two 5 x 3 integer grids 3 apart, so that five pairs tie exactly for the closest (integer coordinates keep scikit-learn's
expanded formula exact), rows permuted.
"""
import os
import warnings

import numpy as np
from scipy.sparse.csgraph import connected_components, shortest_path
from sklearn.manifold import Isomap
from sklearn.metrics import pairwise_distances
from sklearn.neighbors import NearestNeighbors, kneighbors_graph
from sklearn.preprocessing import KernelCenterer

from make_isomap import KS, isometry

HERE = os.path.dirname(os.path.abspath(__file__))
N_QUERIES = 24


def arc(n_arc, n1, n2, seed):
    """(X [n_arc + n1 + n2, 9], Xq [24, 9]): the queries are further points of the same figure (12 on the arc, 6 + 6 in the blobs)."""
    rng = np.random.default_rng(seed)
    theta = np.deg2rad(30.0) + np.deg2rad(300.0) * np.arange(n_arc) / (n_arc - 1) + 0.002 * rng.standard_normal(n_arc)
    theta_q = np.deg2rad(30.0) + np.deg2rad(300.0) * rng.random(12)
    circle = lambda t: 10.0 * np.stack([np.cos(t), np.sin(t)], axis=1) + 0.05 * rng.standard_normal((len(t), 2))
    blob = lambda y, n: np.array([9.4, y]) + 0.2 * rng.standard_normal((n, 2))
    P = np.concatenate([circle(theta), blob(2.3, n1), blob(-2.3, n2)])
    Q = np.concatenate([circle(theta_q), blob(2.3, 6), blob(-2.3, 6)])
    iso = isometry(rng, 9, 2)
    return (P[rng.permutation(len(P))] @ iso.T).astype(np.float32), (Q @ iso.T).astype(np.float32)


def blobs(sizes, d_ambient, seed, d_blob=3, spread=12.0):
    """(X, Xq): clusters of the given sizes, standard normal in d_blob dimensions, each with its own isometry into d_ambient and its
    own centre; the 24 queries are further points of the same clusters."""
    rng = np.random.default_rng(seed)
    P, Q = [], []
    for c, n in enumerate(sizes):
        iso, centre = isometry(rng, d_ambient, d_blob), spread * rng.standard_normal(d_ambient)
        nq = N_QUERIES // len(sizes) + (c < N_QUERIES % len(sizes))
        pts = rng.standard_normal((n + nq, d_blob)) @ iso.T + centre
        P.append(pts[:n]); Q.append(pts[n:])
    P = np.concatenate(P)
    return P[rng.permutation(len(P))].astype(np.float32), np.concatenate(Q).astype(np.float32)


def lattice(seed):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(5), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 2)      # 5 x 3 grid
    P = np.concatenate([g, g + np.array([0, 5])])                       # the second grid starts 3 beyond the first one's last column
    P = np.concatenate([P, np.zeros((len(P), 1))], axis=1)
    return P[rng.permutation(len(P))].astype(np.float32)


def direct_distances(A, B):
    d = A.astype(np.float64)[:, None, :] - B.astype(np.float64)[None, :, :]
    return np.sqrt((d * d).sum(axis=2))


def sklearn_bridges(X64, labels, C, want_gap):
    """The loop of _fix_connected_components (mode="distance") with scikit-learn's pairwise_distances."""
    bi, bj, bw, n_ties = [], [], [], 0
    for i in range(C):
        idx_i = np.flatnonzero(labels == i)
        for j in range(i):
            idx_j = np.flatnonzero(labels == j)
            D = pairwise_distances(X64[idx_i], X64[idx_j], metric="euclidean")
            ii, jj = np.unravel_index(D.argmin(axis=None), D.shape)
            bi.append(idx_i[ii]); bj.append(idx_j[jj]); bw.append(D[ii, jj])
            exact = np.sort(direct_distances(X64[idx_i], X64[idx_j]).reshape(-1))
            if want_gap:
                assert exact.size > 1 and (exact[1] - exact[0]) > 1e-9 * exact[0], (i, j, exact[:2])
            else:
                n_ties += int((exact == exact[0]).sum())
    return np.array(bi, dtype=np.int64), np.array(bj, dtype=np.int64), np.array(bw, dtype=np.float64), n_ties


def record(out, name, X, Xq, nn, C_want, kernel=True):
    X64 = X.astype(np.float64)
    N = X.shape[0]
    nbg = kneighbors_graph(NearestNeighbors(n_neighbors=nn, algorithm="kd_tree").fit(X64), nn, mode="distance")
    C, labels = connected_components(nbg)
    assert C == C_want, (name, C)
    first = np.array([np.flatnonzero(labels == c)[0] for c in range(C)])
    assert np.all(np.diff(first) > 0)                                   # numbered in the order of the smallest vertex
    bi, bj, bw, n_ties = sklearn_bridges(X64, labels, C, want_gap=kernel)
    bw_exact = np.sqrt(((X64[bi] - X64[bj]) ** 2).sum(axis=1))
    G = nbg.toarray()
    G[G == 0] = np.inf
    G[bi, bj] = bw
    G[bj, bi] = bw
    np.fill_diagonal(G, 0.0)
    mine = shortest_path(G, method="auto", directed=False)
    out[f"{name}_X"], out[f"{name}_nn"], out[f"{name}_labels"] = X, np.int64(nn), labels.astype(np.int64)
    out[f"{name}_bi"], out[f"{name}_bj"], out[f"{name}_bw"], out[f"{name}_bw_exact"] = bi, bj, bw, bw_exact
    print(f"{name}: N = {N}, C = {C}, B = {len(bi)}, endpoints = {np.unique(np.concatenate([bi, bj])).size}, "
          f"max |w_sklearn - w_exact| / w = {np.abs(bw - bw_exact).max() / bw_exact.min():.3g}")
    if not kernel:
        assert n_ties >= 3, n_ties                                      # several exactly tied closest pairs
        assert np.array_equal(bw, bw_exact)                             # integer coordinates: the expanded formula is exact
        print(f"{name}: {n_ties} exactly tied closest pairs; scikit-learn picks ({bi[0]}, {bj[0]})")
        return None
    ks, errs, dist = [], [], None
    for k in KS:
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                warnings.filterwarnings("ignore", message="The number of connected components")
                warnings.filterwarnings("ignore", message="Changing the sparsity structure")     # scikit-learn's own insertion
                iso = Isomap(n_neighbors=nn, n_components=k, eigen_solver="dense", neighbors_algorithm="kd_tree").fit(X64)
            err = float(iso.reconstruction_error())
        except Exception as e:                                          # scikit-learn refuses this k
            print(f"{name}: k = {k} refused by scikit-learn: {type(e).__name__}: {e}")
            continue
        if not np.isfinite(err):
            print(f"{name}: k = {k}: scikit-learn returns {err}")
            continue
        ks.append(k); errs.append(err)
        if dist is None:
            dist = np.array(iso.dist_matrix_, dtype=np.float64)
            assert np.array_equal(dist, mine), name                     # these edges are the ones scikit-learn added
        if k == 3:
            emb, tr = iso.embedding_.copy(), iso.transform(Xq.astype(np.float64))
    assert {1, 2, 3} <= set(ks), ks
    assert np.isfinite(dist).all()
    full = np.sort(direct_distances(Xq, X), axis=1)
    assert ((full[:, nn] - full[:, nn - 1]) / full[:, nn]).min() > 1e-9
    rows = np.sort(np.random.default_rng(N).choice(N, size=16, replace=False))
    lam = np.linalg.eigvalsh(KernelCenterer().fit_transform(-0.5 * dist ** 2))[::-1]
    pos = int(np.count_nonzero(lam > 1e-12 * lam[0]))
    beyond = [k for k in ks if k > pos]
    if beyond:                                                          # the top k then include negative eigenvalues: no curve of ours
        print(f"{name}: k = {beyond} left out: the centred kernel has {pos} positive eigenvalues")
        ks, errs = ks[:len(ks) - len(beyond)], errs[:len(ks) - len(beyond)]
    out[f"{name}_Xq"] = Xq
    out[f"{name}_ks"], out[f"{name}_err"] = np.array(ks, dtype=np.int64), np.array(errs, dtype=np.float64)
    out[f"{name}_rows"], out[f"{name}_dist_rows"] = rows.astype(np.int64), dist[rows]
    out[f"{name}_eig"] = lam[:32].copy()
    out[f"{name}_k3_emb"], out[f"{name}_k3_tr"] = emb, tr
    out[f"{name}_k3_gmin"] = np.float64(np.min((lam[:3] - lam[1:4]) / lam[0]))
    print(f"{name}: ks = {ks}, err[0] = {errs[0]:.6g}, eig[0] = {lam[0]:.6g}, g_min(3) = {out[f'{name}_k3_gmin']:.4g}")
    return dist, labels, G


def main():
    out = {}
    dist, labels, G = record(out, "arc193", *arc(150, 20, 23, 7), 5, 3)
    # the case that catches a repair which only fills the infinite blocks: the new edges shorten paths INSIDE a component
    G0 = G.copy()
    G0[out["arc193_bi"], out["arc193_bj"]] = np.inf
    G0[out["arc193_bj"], out["arc193_bi"]] = np.inf
    before = shortest_path(G0, method="auto", directed=False)
    same = labels[:, None] == labels[None, :]
    shorter = same & (dist < before * (1 - 1e-9))
    assert shorter.sum() >= 100, shorter.sum()
    print(f"arc193: {shorter.sum() // 2} same-component pairs shortened by the repair, by up to {(before[shorter] / dist[shorter]).max():.3g} x")
    out["arc193_n_shortened"] = np.int64(shorter.sum() // 2)
    record(out, "blobs257", *blobs([60, 50, 47, 55, 45], 16, 21), 5, 5)
    record(out, "blobs600", *blobs([70, 66, 64, 72, 60, 68, 62, 71, 67], 24, 22), 5, 9)
    out["two130_dist"] = record(out, "two130", *blobs([65, 65], 8, 23), 5, 2)[0]
    record(out, "lattice", lattice(24), None, 4, 2, kernel=False)
    path = os.path.join(HERE, "isomap_connect.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes (isomap.npz:", os.path.getsize(os.path.join(HERE, "isomap.npz")), "bytes)")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "isomap.npz"))


if __name__ == "__main__":
    main()
