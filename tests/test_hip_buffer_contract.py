"""The workspace and output contract ("Buffers"; tests/buffer_contract.py) of the fp64 linear-algebra, neighbour-search
and graph launchers, called through the C ABI with every buffer of exactly the documented size between guard regions and run over
zero-filled, stale and 0xFF-filled outputs and scratch.  Every assertion is bit equality or "untouched"; the values themselves are
vouched for by comparing each case bit for bit with the ``_lib`` wrapper, whose fp64-oracle tests live beside this file.

Before a case was first run its launcher's host function was read: every word of scratch that a kernel uses as an index, a count, a
flag or a spin target is written earlier in the same call --
  knn                 amax and n_exact_rows by hipMemsetAsync; Xc, nrm, arow (pad rows and columns too) by knn_center_kernel; the
                      candidate lists cd / ci for every (split, row, entry) by knn_tiles_kernel (-1 / +inf where a list is short);
                      flag_rows, rk_d, rk_i by knn_refine_kernel for exactly the rows knn_exact_kernel then reads; sd / si by the
                      exact kernel itself below its own counter
  symtridiag          the mailboxes of chase_systolic_kernel ([nodes][2][2][128] granules) and the abort word by hipMemsetAsync in
                      sbr_chase; residual^2 and ||G||_F^2 by hipMemsetAsync in sbr_to_band; the carried reflectors vs[s] of
                      chase_kernel by task (s, t) exactly when task (s, t + 1) exists; the band, its bulge room and the two pad
                      columns by extract_band_kernel.  Everything else in that scratch is fp64 data of the panel kernels
  component_bridges   best / key by bridges_init_kernel
  component_labels    first[i] for every i < N by first_reachable_kernel, 0 <= first[i] <= i, checked again where it indexes
  knn_cross, isomap_project, double_center, colmean, sym_lowvecs, sym_topvecs, empirical_flipd
                      fp64 data only, each word written by the launch before the one that reads it (ctl[0..1] of the two
                      eigenvector routines by prepare_kernel / clear_ctl_kernel)
-- so the stale and 0xFF runs are kept for every launcher below.
"""
import ctypes

import numpy as np
import pytest
import torch

import buffer_contract as bc
import simplex_cases
from buffer_contract import Buf
from id_diff_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = np.inf


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    """A fault is a finding, not something to run into again: once the device reports an error the session ends."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:          # noqa: BLE001 -- whatever the runtime raises
        pytest.exit(f"the GPU reported an error ({e}); no further case is started on it", returncode=3)


class Problem:
    """One call: read-only ``inputs`` {name: host array}, ``outputs`` / ``scratch`` {name: Buf}, ``launch(bufs)`` and the
    keyword arguments of ``run_contract`` that belong to it."""

    def __init__(self, what, inputs, outputs, scratch, launch, **kw):
        self.what, self.inputs, self.outputs, self.scratch, self.launch, self.kw = what, inputs, outputs, scratch, launch, kw


def run(main, other):
    """``main`` under the three fills, ``other`` (the same launcher on another problem that fits the same buffers) in between."""
    for group in ("outputs", "scratch"):
        for name, b in getattr(other, group).items():
            assert b.nbytes <= getattr(main, group)[name].nbytes, f"{name}: the other problem needs a larger buffer"
    inits = {n: b.init for g in (other.outputs, other.scratch) for n, b in g.items() if b.init is not None}
    return bc.run_contract(main.launch, main.inputs, main.outputs, main.scratch, other.inputs, other_launch=other.launch,
                           other_init=inits, device=DEV, what=main.what, **main.kw)


def call(name, *args):
    """The C ABI directly: the entry point, the current stream appended, the return code checked."""
    _lib._check(getattr(_lib.lib(), name)(*args, _lib._stream()), name)
    return 0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want, what):
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.size == want.size, f"{what}: {got.dtype}[{got.size}] against {want.dtype}[{want.size}]"
    i, n = bc._first_diff(got, want)
    assert i is None, f"{what}: element {i} is {got[i]!r}, the _lib wrapper gives {want[i]!r} ({n} differ)"


def rng(*seed):
    return np.random.default_rng([7, *seed])


def scores(P, M, D, seed):
    """Score-like rows: a few strong directions over a weak floor, offset from the origin."""
    r = rng(P, M, D, seed)
    S = r.standard_normal((P, M, D)) * np.where(np.arange(D) < 6, 1.0, 0.05) + 0.3
    return S.astype(np.float32)


def gram(P, D, seed, M=None):
    """P symmetric positive semi-definite matrices [D, D] fp64 (exactly symmetric)."""
    S = scores(P, M or D + 20, D, seed).astype(np.float64)
    S -= S.mean(axis=1, keepdims=True)
    return np.einsum("pmi,pmj->pij", S, S)


# ------------------------------------------------------------------------------------------------ the checker, on the device
def _device_standin(bufs, defect=None):
    """total = sum of x through 8 partial sums in the scratch, y = 2 x: torch ops on the arenas' device views."""
    x, y, total, part = bufs["x"].f64(), bufs["y"].f64(), bufs["total"].f64(), bufs["part"].f64()
    n = 8 if defect != "scratch_read_first" else 7
    part[:n] = x.reshape(8, -1).sum(dim=1)[:n]
    if defect == "accumulates":
        total += part.sum()
    else:
        total[0] = part.sum()
    y[:] = 2.0 * x
    if defect == "past_scratch":
        a = bufs["part"]
        a.raw[a.offset + 64:a.offset + 72] = 0
    if defect == "modifies_input":
        x[3] += 1.0
    return 0


@pytest.mark.parametrize("defect, pattern", [
    (None, None), ("scratch_read_first", "output 'total' element 0 differs"), ("accumulates", "output 'total' element 0 differs"),
    ("past_scratch", "scratch 'part' was written outside its 64 bytes"), ("modifies_input", "read-only input 'x' was modified: element 3")])
def test_the_checker_sees_planted_defects_in_device_buffers(defect, pattern):
    """tests/test_buffer_contract_host.py checks the checker on host arenas; this is the same on the torch path the cases below use
    (fills, typed views, guards compared on the device, copies back)."""
    x = {"x": rng(1).standard_normal(40)}
    args = (lambda b: _device_standin(b, defect), x, {"y": Buf("f64", 40), "total": Buf("f64", 1, align=8)},
            {"part": Buf("f64", 8, align=8)}, {"x": rng(2).standard_normal(40)})
    if pattern is None:
        res = bc.run_contract(*args, device=DEV, what="stand-in")
        assert (res.outputs["y"] == 2.0 * x["x"]).all()
    else:
        with pytest.raises(bc.ContractError, match=pattern):
            bc.run_contract(*args, device=DEV, what="stand-in")


# ------------------------------------------------------------------------------------------------ spectrum and its stages
def colmean_problem(P, M, D, seed=0):
    S = scores(P, M, D, seed)
    return Problem(f"idiff_colmean_f64 {P, M, D}", {"S": S}, {"mean": Buf("f64", P * D)}, {"part": Buf("f64", P * 32 * D)},
                   lambda b: call("idiff_colmean_f64", b["S"].ptr, P, M, D, b["mean"].ptr, b["part"].ptr))


def test_colmean():
    P, M, D = 2, 257, 70                                 # 32 chunks of 9 rows: the 29th is short, three are empty
    res = run(colmean_problem(P, M, D), colmean_problem(1, 100, 50, 1))
    S = dev(colmean_problem(P, M, D).inputs["S"])
    same_bits(res.outputs["mean"], _lib.column_means(S), "mean")


def gram_problem(P, M, D, seed=0):
    S = scores(P, M, D, seed)
    mean = S.astype(np.float64).mean(axis=1)
    return Problem(f"idiff_centered_gram_f64 {P, M, D}", {"S": S, "mean": mean}, {"G": Buf("f64", P * D * D)}, {},
                   lambda b: call("idiff_centered_gram_f64", b["S"].ptr, b["mean"].ptr, P, M, D, b["G"].ptr))


@pytest.mark.parametrize("P, M, D", [(2, 257, 70), (1, 40, 129)])
def test_centered_gram(P, M, D):
    main = gram_problem(P, M, D)
    res = run(main, gram_problem(1, 33, 65, 1))
    G = res.outputs["G"].reshape(P, D, D)
    for p in range(P):
        same_bits(G[p], _lib.centered_gram(dev(main.inputs["S"][p]), dev(main.inputs["mean"][p])), f"G[{p}]")


def spectrum_problem(P, M, D, with_eig, seed=0):
    S = scores(P, M, D, seed)
    nbytes = _lib.lib().idiff_spectrum_workspace_bytes(P, M, D)
    outputs = {"sv": Buf("f32", P * D)}
    if with_eig:
        outputs["eig"] = Buf("f64", P * D)
    return Problem(f"idiff_spectrum_f32 {P, M, D}, eig_out {'given' if with_eig else 'null'}", {"S": S}, outputs,
                   {"ws": Buf("u8", nbytes, align=8)},
                   lambda b: call("idiff_spectrum_f32", b["S"].ptr, P, M, D, b["ws"].ptr, nbytes, b["sv"].ptr,
                                  b["eig"].ptr if with_eig else 0))


@pytest.mark.parametrize("with_eig", [False, True], ids=["eig_null", "eig_given"])
@pytest.mark.parametrize("P, M, D", [(3, 70, 40), (2, 150, 129), (2, 40, 100)])
def test_spectrum(P, M, D, with_eig):
    """(3, 70, 40): the LDS path with P > 1; (2, 150, 129): two-stage, the scratch shared by the matrices in turn; (2, 40, 100): M < D."""
    main = spectrum_problem(P, M, D, with_eig)
    res = run(main, spectrum_problem(P, M + 3, D, with_eig, 1))
    sv, eig = _lib.spectrum(dev(main.inputs["S"]), return_eig=True, full=True)
    same_bits(res.outputs["sv"], sv, "sv")
    if with_eig:
        same_bits(res.outputs["eig"], eig, "eig")


def symtridiag_problem(P, D, seed=0):
    G = gram(P, D, seed)
    n = _lib.lib().idiff_symtridiag_scratch_doubles(D)
    return Problem(f"idiff_symtridiag_f64 P = {P}, D = {D}", {}, {"G": Buf("f64", P * D * D, init=G), "diag": Buf("f64", P * D),
                                                                  "offdiag": Buf("f64", P * D)}, {"scratch": Buf("f64", n)},
                   lambda b: call("idiff_symtridiag_f64", b["G"].ptr, P, D, b["diag"].ptr, b["offdiag"].ptr, b["scratch"].ptr),
                   unspecified=("G",))              # "overwritten": what G holds on return is nobody's to read


@pytest.mark.parametrize("D, option, plan", [(64, None, 0), (128, None, 0), (129, None, 1), (160, None, 1), (257, None, 1),
                                             (129, "IDIFF_CHASE_WAVEFRONT", 2), (257, "IDIFF_CHASE_WAVEFRONT", 2),
                                             (160, "IDIFF_TRIDIAG_ONESTAGE", 3)])
def test_symtridiag(D, option, plan):
    P = 2
    main, other = symtridiag_problem(P, D), symtridiag_problem(P, D, 1)

    def body():
        assert _lib.symtridiag_plan(D) == plan
        res = run(main, other)
        d, e = dev(res.outputs["diag"]), dev(res.outputs["offdiag"])
        assert (res.outputs["offdiag"].reshape(P, D)[:, D - 1] == 0.0).all()      # the unused entry: 0 on every path
        eig = torch.empty(P, D, dtype=torch.float64, device=DEV)
        call("idiff_tridiag_eigvals_f64", d.data_ptr(), e.data_ptr(), P, D, eig.data_ptr())
        for p in range(P):
            same_bits(eig[p].cpu().numpy(), _lib.sym_eigvals(dev(main.outputs["G"].init.reshape(P, D, D)[p])), f"eigenvalues of G[{p}]")

    if option is None:
        body()
    else:
        with _lib.thread_option(option, 1):
            body()


def symband_problem(D, seed=0):
    G = gram(1, D, seed)[0]
    n = _lib.lib().idiff_symtridiag_scratch_doubles(D)
    ld = _lib.lib().idiff_symband_ld()
    return Problem(f"idiff_symband_f64 D = {D}", {}, {"G": Buf("f64", D * D, init=G)}, {"scratch": Buf("f64", n)},
                   lambda b: call("idiff_symband_f64", b["G"].ptr, D, b["scratch"].ptr),
                   unspecified=("G",), documented={"scratch": np.arange(D * ld)})


@pytest.mark.parametrize("D", [129, 257])
def test_symband(D):
    """The first D * ld doubles of the scratch are the band and its bulge room, zero, whatever the scratch held."""
    main = symband_problem(D)
    res = run(main, symband_problem(D, 1))
    ld = _lib.lib().idiff_symband_ld()
    band = res.scratch["scratch"][:D * ld].reshape(D, ld)
    assert not band[:, 33:].any(), "bulge room"
    j, k = np.meshgrid(np.arange(D), np.arange(33), indexing="ij")
    assert not band[:, :33][j + k >= D].any(), "band entries below the last row"
    same_bits(band, _lib.sym_band(dev(main.outputs["G"].init.reshape(D, D)), dense=False), "band")


def eigvals_problem(P, D, seed=0):
    r = rng(P, D, seed)
    diag, offd = r.standard_normal((P, D)), r.standard_normal((P, D))
    offd[:, D - 1] = np.nan                              # the unused entry (include/idiff_hip.h)
    return Problem(f"idiff_tridiag_eigvals_f64 P = {P}, D = {D}", {"diag": diag, "offdiag": offd}, {"eig": Buf("f64", P * D)}, {},
                   lambda b: call("idiff_tridiag_eigvals_f64", b["diag"].ptr, b["offdiag"].ptr, P, D, b["eig"].ptr))


@pytest.mark.parametrize("D", [1, 2, 70, 129])
def test_tridiag_eigvals(D):
    P = 3
    main = eigvals_problem(P, D)
    res = run(main, eigvals_problem(P, D, 1))
    d, e = dev(main.inputs["diag"]), dev(main.inputs["offdiag"])
    e[:, D - 1] = 0.0
    eig = torch.empty(P, D, dtype=torch.float64, device=DEV)
    call("idiff_tridiag_eigvals_f64", d.data_ptr(), e.data_ptr(), P, D, eig.data_ptr())
    got = res.outputs["eig"].reshape(P, D)
    assert np.isfinite(got).all() and (np.diff(got, axis=1) >= 0).all()
    same_bits(got, eig, "eig with offdiag[:, D - 1] = 0 instead of NaN")


# ------------------------------------------------------------------------------------------------ eigenvectors
def lowvecs_problem(D, k, seed=0):
    G = gram(1, D, seed)[0]
    n = _lib.lib().idiff_sym_lowvecs_scratch_doubles(D, k)
    return Problem(f"idiff_sym_lowvecs_f64 D = {D}, k = {k}", {"G": G}, {"T": Buf("f64", D * k), "ritz": Buf("f64", k, align=8),
                                                                           "resid": Buf("f64", 1, align=8)}, {"scratch": Buf("f64", n)},
                   lambda b: call("idiff_sym_lowvecs_f64", b["G"].ptr, D, k, b["T"].ptr, b["ritz"].ptr, b["resid"].ptr, b["scratch"].ptr))


@pytest.mark.parametrize("D, k", [(33, 1), (100, 7), (130, 32), (257, 64)])
def test_sym_lowvecs(D, k):
    main = lowvecs_problem(D, k)
    res = run(main, lowvecs_problem(D, k, 1))
    T, ritz, resid = _lib.sym_lowvecs(dev(main.inputs["G"]), k)
    assert np.isfinite(res.outputs["T"]).all()
    same_bits(res.outputs["T"], T, "T"); same_bits(res.outputs["ritz"], ritz, "ritz"); same_bits(res.outputs["resid"], resid, "resid")


def topvecs_problem(N, k, p, seed=0):
    r = rng(N, k, p, seed)
    Q, _ = np.linalg.qr(r.standard_normal((N, N)))
    lam = np.concatenate([np.linspace(2.0, 1.0, p + 4), 0.2 * r.random(N - p - 4) - 0.1])   # a separated top, an indefinite tail
    K = (Q * lam) @ Q.T
    K = 0.5 * (K + K.T)
    eigvals = np.linalg.eigvalsh(K)
    plan = dict(_lib.topvecs_plan(eigvals, k))
    plan["p"], plan["hi"] = p, float(np.sort(eigvals)[::-1][p])                         # this block width: hi = lambda_(p + 1)
    n = _lib.lib().idiff_sym_topvecs_scratch_doubles(N, k, p)
    prob = Problem(f"idiff_sym_topvecs_f64 N = {N}, k = {k}, p = {p}", {"K": K},
                   {"V": Buf("f64", N * k), "ritz": Buf("f64", k, align=8), "resid": Buf("f64", 1, align=8)}, {"scratch": Buf("f64", n)},
                   lambda b: call("idiff_sym_topvecs_f64", b["K"].ptr, N, k, p, plan["lo"], plan["hi"], plan["top"], plan["degree"],
                                  plan["sweeps"], b["V"].ptr, b["ritz"].ptr, b["resid"].ptr, b["scratch"].ptr))
    prob.plan, prob.eigvals = plan, eigvals
    return prob


@pytest.mark.parametrize("N, k, p", [(130, 3, 11), (257, 16, 48)])
def test_sym_topvecs(N, k, p):
    main = topvecs_problem(N, k, p)
    res = run(main, topvecs_problem(N, k, p, 1))
    V, ritz, resid = _lib.sym_topvecs(dev(main.inputs["K"]), k, main.eigvals, plan=main.plan)
    assert np.isfinite(res.outputs["V"]).all()
    same_bits(res.outputs["V"], V, "V"); same_bits(res.outputs["ritz"], ritz, "ritz"); same_bits(res.outputs["resid"], resid, "resid")


# ------------------------------------------------------------------------------------------------ neighbours
def points(N, D, seed=0):
    r = rng(N, D, seed)
    return (r.standard_normal((N, D)) * np.where(np.arange(D) < 20, 1.0, 0.05)).astype(np.float32)


def tight_clusters(N, D, seed=0):
    """Clusters of radius 1e-4 at distance 10 from the mean (test_knn_tight_clusters_take_the_exact_pass): the fp32 pass cannot
    order the neighbours, every row goes through the brute-force buffers."""
    r = rng(N, D, seed)
    centres = r.standard_normal((4, D))
    centres = 10.0 * centres / np.linalg.norm(centres, axis=1, keepdims=True)
    return (np.repeat(centres, N // 4, axis=0) + 1e-4 * r.random((N, D)) / D ** 0.5).astype(np.float32)


def knn_problem(X, k):
    N, D = X.shape
    nbytes = _lib.lib().idiff_knn_workspace_bytes(N, D, k)
    return Problem(f"idiff_knn_f32 N = {N}, D = {D}, k = {k}", {"X": X},
                   {"dist": Buf("f64", N * k), "idx": Buf("i64", N * k), "n_exact_rows": Buf("i32", 1, align=4)},
                   {"ws": Buf("u8", nbytes, align=256)},
                   lambda b: call("idiff_knn_f32", b["X"].ptr, N, D, k, b["ws"].ptr, nbytes, b["dist"].ptr, b["idx"].ptr,
                                  b["n_exact_rows"].ptr))


@pytest.mark.parametrize("N, D, k, tight", [(2, 1, 1, False), (33, 3, 5, False), (300, 70, 21, False), (257, 129, 64, False),
                                            (240, 129, 21, True)])
def test_knn(N, D, k, tight):
    """The order in which the brute-force rows are visited is free; it does not reach dist, idx or n_exact_rows."""
    make = tight_clusters if tight else points
    main = knn_problem(make(N, D), k)
    res = run(main, knn_problem(make(N, D, 1), k))
    dist, idx, n_exact = _lib.knn(dev(main.inputs["X"]), k)
    same_bits(res.outputs["dist"], dist, "dist"); same_bits(res.outputs["idx"], idx, "idx")
    same_bits(res.outputs["n_exact_rows"], n_exact, "n_exact_rows")
    if tight:
        assert res.outputs["n_exact_rows"][0] > 0


def brute_knn(X, k, Xq=None):
    """(dist [M, k] fp64, idx [M, k] int64) by numpy; the rows of X themselves (self excluded) when Xq is None."""
    X64 = X.astype(np.float64)
    Q = X64 if Xq is None else Xq.astype(np.float64)
    d2 = ((Q[:, None, :] - X64[None, :, :]) ** 2).sum(axis=2)
    if Xq is None:
        np.fill_diagonal(d2, np.inf)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int64)
    return np.sqrt(np.take_along_axis(d2, idx, axis=1)), idx


def knn_cross_problem(M, N, D, k, seed=0):
    Xq, X = points(M, D, seed + 100), points(N, D, seed)
    nbytes = _lib.lib().idiff_knn_cross_workspace_bytes(M, N)
    return Problem(f"idiff_knn_cross_f64 {M, N, D, k}", {"Xq": Xq, "X": X}, {"dist": Buf("f64", M * k), "idx": Buf("i64", M * k)},
                   {"ws": Buf("u8", nbytes, align=8)},
                   lambda b: call("idiff_knn_cross_f64", b["Xq"].ptr, M, b["X"].ptr, N, D, k, b["ws"].ptr, nbytes, b["dist"].ptr,
                                  b["idx"].ptr))


@pytest.mark.parametrize("M, N, D, k", [(5, 70, 3, 4), (130, 257, 20, 64)])
def test_knn_cross(M, N, D, k):
    main = knn_cross_problem(M, N, D, k)
    res = run(main, knn_cross_problem(M, N - 7, D, k, 1))
    dist, idx = _lib.knn_cross(dev(main.inputs["Xq"]), dev(main.inputs["X"]), k)
    same_bits(res.outputs["dist"], dist, "dist"); same_bits(res.outputs["idx"], idx, "idx")


# ------------------------------------------------------------------------------------------------ graph and geodesics
def graph_of(N, seed=0, k=5, components=1):
    """A symmetric neighbourhood graph [N, N] fp64 (0 diagonal, +inf = no edge) of points in R^3, in ``components`` far-apart
    groups, and the points."""
    X = points(N, 3, seed)
    X[:, 0] += 1000.0 * (np.arange(N) % components)
    dist, idx = brute_knn(X, k)
    G = np.full((N, N), INF)
    np.fill_diagonal(G, 0.0)
    G[np.arange(N)[:, None], idx] = dist
    i = np.arange(N - components)                      # a chain through every group, so that a group is one component
    G[i, i + components] = np.sqrt(((X[i].astype(np.float64) - X[i + components]) ** 2).sum(axis=1))
    return np.minimum(G, G.T), X, dist, idx


def closure(G):
    D = G.copy()
    for m in range(G.shape[0]):
        D = np.minimum(D, D[:, m:m + 1] + D[m:m + 1, :])
    return D


SIZES = [63, 64, 65, 130]          # around the Floyd-Warshall tile (64) and the symmetrisation tile (32), more than one block


def knn_graph_problem(N, seed=0, k=5):
    _, _, dist, idx = graph_of(N, seed, k)
    return Problem(f"idiff_knn_graph_f64 N = {N}", {"dist": dist, "idx": idx}, {"G": Buf("f64", N * N)}, {},
                   lambda b: call("idiff_knn_graph_f64", b["dist"].ptr, b["idx"].ptr, N, k, b["G"].ptr))


@pytest.mark.parametrize("N", SIZES)
def test_knn_graph(N):
    main = knn_graph_problem(N)
    res = run(main, knn_graph_problem(N - 3, 1))
    same_bits(res.outputs["G"], _lib.knn_graph(dev(main.inputs["dist"]), dev(main.inputs["idx"])), "G")


def symmetrize_problem(N, seed=0):
    G = rng(N, seed).random((N, N))
    return Problem(f"idiff_symmetrize_min_f64 N = {N}", {}, {"G": Buf("f64", N * N, init=G)}, {},
                   lambda b: call("idiff_symmetrize_min_f64", b["G"].ptr, N))


@pytest.mark.parametrize("N", SIZES)
def test_symmetrize_min(N):
    main = symmetrize_problem(N)
    res = run(main, symmetrize_problem(N - 3, 1))
    same_bits(res.outputs["G"], _lib.symmetrize_min(dev(main.outputs["G"].init.reshape(N, N))), "G")


def apsp_problem(N, seed=0):
    G = graph_of(N, seed)[0]
    return Problem(f"idiff_apsp_f64 N = {N}", {}, {"G": Buf("f64", N * N, init=G)}, {}, lambda b: call("idiff_apsp_f64", b["G"].ptr, N))


@pytest.mark.parametrize("N", SIZES)
def test_apsp(N):
    main = apsp_problem(N)
    res = run(main, apsp_problem(N - 3, 1))
    same_bits(res.outputs["G"], _lib.geodesic_distances(dev(main.outputs["G"].init.reshape(N, N))), "G")


def test_minplus_pitched():
    """Row pitches wider than the rows: the pad columns of C keep what they held, those of A and B are never part of the result."""
    m, n, p, lda, ldb, ldc = 70, 65, 33, 36, 70, 67
    r = rng(m, n, p)

    def pitched(rows, cols, ld, seed):
        flat = rng(seed).random((rows - 1) * ld + cols)          # exactly the extent the header's pitches describe
        mask = (np.arange(flat.size) % ld) < cols
        return flat, mask

    def problem(seed):
        A, _ = pitched(m, p, lda, seed)
        B, _ = pitched(p, n, ldb, seed + 1)
        C, cmask = pitched(m, n, ldc, seed + 2)
        C[r.random(C.size) < 0.3] = INF
        return Problem("idiff_minplus_f64 (70, 65, 33), pitched", {"A": A, "B": B}, {"C": Buf("f64", C.size, init=C, init_mask=cmask)}, {},
                       lambda b: call("idiff_minplus_f64", b["A"].ptr, lda, b["B"].ptr, ldb, b["C"].ptr, ldc, m, n, p),
                       unwritten={"C": ~cmask})

    main = problem(0)
    res = run(main, problem(10))
    view = lambda flat, rows, cols, ld: torch.as_strided(dev(flat), (rows, cols), (ld, 1))
    want = _lib.minplus(view(main.inputs["A"], m, p, lda), view(main.inputs["B"], p, n, ldb), view(main.outputs["C"].init, m, n, ldc))
    cmask = main.outputs["C"].init_mask
    same_bits(res.outputs["C"][cmask], want.contiguous(), "C")


def double_center_problem(N, seed=0):
    D = closure(graph_of(N, seed, k=6)[0])
    assert np.isfinite(D).all() and (D == D.T).all()
    n = _lib.lib().idiff_double_center_scratch_doubles(N)
    assert n == 2 * N + 1
    return Problem(f"idiff_double_center_f64 N = {N}", {"D": D}, {"K": Buf("f64", N * N), "fro2": Buf("f64", 1, align=8)},
                   {"scratch": Buf("f64", n, align=8)},
                   lambda b: call("idiff_double_center_f64", b["D"].ptr, N, b["K"].ptr, b["fro2"].ptr, b["scratch"].ptr),
                   documented={"scratch": np.concatenate([np.arange(N), [2 * N]])})


@pytest.mark.parametrize("N", [65, 130])
def test_double_center(N):
    main = double_center_problem(N)
    res = run(main, double_center_problem(N - 2, 1))
    K, fro2, (colmean, grand) = _lib.double_center(dev(main.inputs["D"]), return_means=True)
    same_bits(res.outputs["K"], K, "K"); same_bits(res.outputs["fro2"], fro2, "fro2")
    same_bits(-0.5 * res.scratch["scratch"][:N], colmean, "scratch[:N]")
    same_bits(-0.5 * res.scratch["scratch"][2 * N:], grand, "scratch[2 N]")


def project_problem(c, M=5, N=70, k=4, seed=0):
    G, X, _, _ = graph_of(N, seed, k=6)
    D = closure(G)
    dist, idx = brute_knn(X, k, points(M, 3, seed + 50))
    r = rng(c, seed)
    A, colmean, grand = r.standard_normal((N, c)), -0.5 * (D * D).mean(axis=0), np.array([-0.5 * (D * D).mean()])
    n = _lib.lib().idiff_isomap_project_scratch_doubles(c)
    return Problem(f"idiff_isomap_project_f64 c = {c}", {"dist": dist, "idx": idx, "D": D, "A": A, "colmean": colmean, "grand": grand},
                   {"Z": Buf("f64", M * c)}, {"scratch": Buf("f64", n, align=8)},
                   lambda b: call("idiff_isomap_project_f64", b["dist"].ptr, b["idx"].ptr, M, k, b["D"].ptr, N, b["A"].ptr, c,
                                  b["colmean"].ptr, b["grand"].ptr, b["Z"].ptr, b["scratch"].ptr))


@pytest.mark.parametrize("c", [2, 8, 9])
def test_isomap_project(c):
    """c <= 8: one pass over the columns; c = 9: two."""
    main = project_problem(c)
    res = run(main, project_problem(c, seed=1))
    i = main.inputs
    Z = _lib.isomap_project(dev(i["dist"]), dev(i["idx"]), dev(i["D"]), dev(i["A"]), dev(i["colmean"]), dev(i["grand"]).reshape(()))
    same_bits(res.outputs["Z"], Z, "Z")


def labels_problem(N, components, seed=0):
    D = closure(graph_of(N, seed, k=4, components=components)[0])
    return Problem(f"idiff_component_labels_f64 N = {N}, {components} component(s)", {"D": D},
                   {"labels": Buf("i32", N, align=4), "count": Buf("i32", 1, align=4)}, {"first": Buf("i32", N, align=4)},
                   lambda b: call("idiff_component_labels_f64", b["D"].ptr, N, b["labels"].ptr, b["count"].ptr, b["first"].ptr))


@pytest.mark.parametrize("components", [1, 3])
def test_component_labels(components):
    N = 130
    main = labels_problem(N, components)
    res = run(main, labels_problem(N, 4 - components, 1))
    assert res.outputs["count"][0] == components
    labels, count = _lib.component_labels(dev(main.inputs["D"]))
    same_bits(res.outputs["labels"], labels, "labels"); same_bits(res.outputs["count"], count, "count")


def bridges_problem(C, N=130, D=3, seed=0):
    X = points(N, D, seed)
    labels = (np.arange(N) % C).astype(np.int32)
    X[:, 0] += 50.0 * labels
    B, nbytes = C * (C - 1) // 2, _lib.lib().idiff_component_bridges_workspace_bytes(C)
    assert nbytes == 16 * B
    return Problem(f"idiff_component_bridges_f64 C = {C}", {"X": X, "labels": labels},
                   {"bi": Buf("i64", B, align=8), "bj": Buf("i64", B, align=8), "bw": Buf("f64", B, align=8)},
                   {"ws": Buf("u8", nbytes, align=8)},
                   lambda b: call("idiff_component_bridges_f64", b["X"].ptr, N, D, b["labels"].ptr, C, b["ws"].ptr, nbytes, b["bi"].ptr,
                                  b["bj"].ptr, b["bw"].ptr))


@pytest.mark.parametrize("C", [2, 3, 5])
def test_component_bridges(C):
    main = bridges_problem(C)
    res = run(main, bridges_problem(C, seed=1))
    bi, bj, bw = _lib.component_bridges(dev(main.inputs["X"]), dev(main.inputs["labels"]), C)
    same_bits(res.outputs["bi"], bi, "bi"); same_bits(res.outputs["bj"], bj, "bj"); same_bits(res.outputs["bw"], bw, "bw")


# ------------------------------------------------------------------------------------------------ per-point estimators
def neighbourhoods(N, D, k, seed=0):
    """X and five queries: 0 and 4 served, 1 with an index outside [0, N) (status 2), 2 with a NaN among its rows (status 3),
    3 on identical points (local PCA: zeros and NaN vectors, status 0; simplex skewness: status 4)."""
    X = simplex_cases.data(N, D, k).numpy().copy()
    X[20:20 + k + 1] = X[20]
    X[N - 1, D // 2] = np.nan
    idx = simplex_cases.brute_knn(np.nan_to_num(X), k)
    centre = np.array([0, 1, 2, 20, 5], dtype=np.int64)
    rows = idx[centre].copy()
    rows[1, k // 2] = N
    rows[2, 1] = N - 1
    rows[3] = np.arange(21, 21 + k)
    for q in (0, 4):
        rows[q][rows[q] == N - 1] = 6 if q == 0 else 7      # keep the NaN row out of the served queries
    return X, centre, rows


def lpca_problem(N, D, k, n_vec, seed=0):
    X, centre, idx = neighbourhoods(N, D, k, seed)
    Q, r = centre.size, min(k, D)
    return Problem(f"idiff_local_pca_f64 {N, D, k}, {n_vec} vectors", {"X": X, "centre": centre, "idx": idx},
                   {"eig": Buf("f64", Q * r), "basis": Buf("f64", Q * n_vec * D), "status": Buf("i32", Q, align=4)}, {},
                   lambda b: call("idiff_local_pca_f64", b["X"].ptr, N, D, b["centre"].ptr, b["idx"].ptr, Q, k, n_vec, b["eig"].ptr,
                                  b["basis"].ptr, b["status"].ptr))


def test_local_pca_writes_every_query():
    """The smallest shape of tests/test_hip_lpca.py that has room for a refused and a degenerate query beside served ones: eig,
    basis and status are written for all five."""
    N, D, k, n_vec = 40, 3, 15, 2
    main = lpca_problem(N, D, k, n_vec)
    other = lpca_problem(N, D, k, n_vec)
    other.inputs["X"] = other.inputs["X"][::-1].copy()
    res = run(main, other)
    assert res.outputs["status"].tolist() == [0, 2, 3, 0, 0]
    eig, basis = res.outputs["eig"].reshape(5, -1), res.outputs["basis"].reshape(5, n_vec, D)
    assert np.isnan(eig[1]).all() and np.isnan(basis[1]).all() and not eig[3].any() and np.isnan(basis[3]).all()
    served = [0, 3, 4]
    i = main.inputs
    e, b = _lib.local_pca(dev(i["X"]), dev(i["centre"][served]), dev(i["idx"][served]), n_vectors=n_vec)
    same_bits(eig[served], e, "eig of the served queries"); same_bits(basis[served], b, "basis of the served queries")


def simplex_problem(N, D, k, scales, seed=0):
    X, centre, idx = neighbourhoods(N, D, k, seed)
    Q, S = centre.size, len(scales)
    host_scales = (ctypes.c_int * S)(*scales)
    return Problem(f"idiff_simplex_skewness_f64 {N, D, k}, scales {scales}", {"X": X, "centre": centre, "idx": idx},
                   {"ess": Buf("f64", Q * S * 3), "status": Buf("i32", Q, align=4)}, {},
                   lambda b: call("idiff_simplex_skewness_f64", b["X"].ptr, N, D, b["centre"].ptr, b["idx"].ptr, Q, k,
                                  ctypes.cast(host_scales, ctypes.c_void_p), S, b["ess"].ptr, b["status"].ptr))


def test_simplex_skewness_writes_every_query():
    N, D, k, scales = 40, 3, 15, (2, 7, 15)              # simplex_cases.cases: the smallest with room for the five queries
    assert (N, D, k, scales) in simplex_cases.cases(_lib.LOCAL_PCA_CHUNK)
    main = simplex_problem(N, D, k, scales)
    other = simplex_problem(N, D, k, scales)
    other.inputs["X"] = other.inputs["X"][::-1].copy()
    res = run(main, other)
    assert res.outputs["status"].tolist() == [0, 2, 3, 4, 0]
    ess = res.outputs["ess"].reshape(5, len(scales), 3)
    assert np.isnan(ess[1]).all() and np.isnan(ess[2]).all() and np.isnan(ess[3, :, :2]).all() and not ess[3, :, 2].any()
    served = [0, 3, 4]
    i = main.inputs
    same_bits(ess[served], _lib.simplex_skewness(dev(i["X"]), dev(i["centre"][served]), dev(i["idx"][served]), scales), "ess of the served queries")


def flipd_problem(splits, P=4, S=3, N=70, D=5, seed=0):
    cloud = points(N, D, seed)
    x = np.concatenate([cloud[:2], points(P - 2, D, seed + 9)])
    sigmas = np.array([0.05, 0.4, 3.0], dtype=np.float32)[:S]
    exclude = np.array([0, 1] + [-1] * (P - 2), dtype=np.int32)
    c = cloud.astype(np.float64).mean(axis=0)
    Y = np.zeros((N, (D + 3) // 4 * 4))
    Y[:, :D] = cloud.astype(np.float64) - c
    h = 0.5 * (Y * Y).sum(axis=1)
    n = _lib.lib().idiff_empirical_flipd_workspace_doubles(P, S, splits)
    assert n == 4 * P * S * splits
    prob = Problem(f"idiff_empirical_flipd_f64 splits = {splits}", {"x": x, "Y": Y, "h": h, "c": c, "sigmas": sigmas, "exclude": exclude},
                   {"flipd": Buf("f64", P * S, align=8), "ess": Buf("f32", P * S, align=4)}, {"ws": Buf("f64", n, align=8)},
                   lambda b: call("idiff_empirical_flipd_f64", b["x"].ptr, b["Y"].ptr, b["h"].ptr, b["c"].ptr, b["sigmas"].ptr,
                                  b["exclude"].ptr, b["flipd"].ptr, b["ess"].ptr, b["ws"].ptr, n, P, N, D, S, splits),
                   align={"x": 4, "sigmas": 4, "exclude": 4, "h": 8, "c": 8})
    return prob


@pytest.mark.parametrize("splits", [1, 2, 3])
def test_empirical_flipd(splits):
    main = flipd_problem(splits)
    res = run(main, flipd_problem(splits, seed=1))
    i = main.inputs
    pack = {"Y": dev(i["Y"]), "h": dev(i["h"]), "c": dev(i["c"]), "N": i["Y"].shape[0], "D": i["x"].shape[1]}
    flipd, ess = _lib.empirical_flipd(dev(i["x"]), pack, dev(i["sigmas"]), exclude=i["exclude"], splits=splits)
    assert np.isfinite(res.outputs["flipd"]).all()
    same_bits(res.outputs["flipd"], flipd, "flipd"); same_bits(res.outputs["ess"], ess, "ess")
