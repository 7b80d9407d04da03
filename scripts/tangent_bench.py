"""Time the tangent-space basis (_lib.tangent_basis, csrc/lowvecs.hip) beside the eigensolver of the spectrum path.

    python scripts/tangent_bench.py [--reps 5] [--warmup 2] [--timeout 300]

Per shape (D, k): a score matrix S [D + 8, D] fp32 with k small singular directions; median of --reps timed calls after
--warmup (CUDA events around each call) of
    gram      column means + centred fp64 Gram matrix (what both paths start from),
    lowvecs   _lib.sym_lowvecs(G, k): Cholesky, four inverse iterations, Rayleigh-Ritz, residual,
    eigvals   _lib.sym_eigvals(G): the eigensolver behind every spectrum (the yardstick of DESIGN 4.3).
Every shape runs in a fresh child process under its own time limit; the first child that fails or runs out of time ends the run
(nothing more is started on the device).
"""
import argparse
import json
import os
import subprocess
import sys

SHAPES = [(100, 10), (1024, 10), (3072, 64), (12288, 64)]


def timed(fn, reps, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return round(float(np.median(ms)), 3)


def one(D, k, reps, warmup):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import id_diff_amd  # noqa: F401
    from id_diff_amd import _lib
    assert torch.cuda.is_available(), "tangent_bench needs the MI355X"
    g = torch.Generator(device="cuda").manual_seed(D + k)
    M = D + 8
    S = torch.randn(M, D, device="cuda", generator=g)
    scale = torch.ones(D, device="cuda")
    scale[D - k:] = 1e-3                                   # k directions with small singular values: the gap the ID rule finds
    Qm, _ = torch.linalg.qr(torch.randn(D, D, device="cuda", generator=g)) if D <= 3072 else (None, None)
    S = S * scale
    if Qm is not None:
        S = (S @ Qm).contiguous()                          # (at D = 12288 the small directions stay axis-aligned: same work for the kernels)
    del Qm

    def gram():
        return _lib.centered_gram(S, _lib.column_sums(S) / float(M))
    G = gram()
    T, ritz, resid = _lib.sym_lowvecs(G, k)
    row = dict(D=D, k=k, M=M, resid=float(resid), ritz_max=float(ritz[-1]), orth=float((T.T @ T - torch.eye(k, device="cuda", dtype=torch.float64)).abs().max()))
    row["gram_ms"] = timed(gram, reps, warmup)
    row["lowvecs_ms"] = timed(lambda: _lib.sym_lowvecs(G, k), reps, warmup)
    row["tangent_basis_ms"] = timed(lambda: _lib.tangent_basis(S, k), reps, warmup)
    row["eigvals_ms"] = timed(lambda: _lib.sym_eigvals(G.clone()), reps, warmup)      # (the eigensolver overwrites its input; the copy is timed with it)
    row["cholesky_gflop"] = round(D ** 3 / 3 / 1e9, 2)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300, help="seconds granted to each shape's child process")
    ap.add_argument("--one", type=int, nargs=2, metavar=("D", "K"), help="(internal) time this shape in this process")
    args = ap.parse_args()
    if args.one:
        return one(args.one[0], args.one[1], args.reps, args.warmup)
    for D, k in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(D), str(k), "--reps", str(args.reps), "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"tangent_bench: shape ({D}, {k}) ran out of its {args.timeout} s; nothing more is started")
        if rc != 0:
            raise SystemExit(f"tangent_bench: shape ({D}, {k}) ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
