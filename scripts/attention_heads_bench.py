"""Streaming multi-head attention (csrc/attention.hip, attention_heads_kernel) at the bench's launch-set size, B = 2240 samples:
    (a) the one-launch kernel
    (b) the three-launch form once per head on the library's gemm / softmax_rows (what the executor falls back to: the baseline)
    (c) at 256 tokens, attention256_kernel at C = H D (one head over all channels: the same flops and the same compulsory bytes)
One process; every form warmed up; the forms interleaved within each repeat; median of the repeats; device events around REPS
back-to-back launches.  Rates: fp32-equivalent flops 4 B T^2 C (two contractions), compulsory bytes 16 B T C (q, k, v, out once).
    python scripts/attention_heads_bench.py > profiles/attention_heads_bench.txt      (ROWS=<B> for another batch)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import id_diff_amd  # noqa: F401
from id_diff_amd import _lib

dev = torch.device("cuda:0")
B = int(os.environ.get("ROWS", 2240))
SHAPES = [(256, 4, 64), (256, 2, 128), (256, 8, 32), (64, 4, 64), (1024, 2, 64), (1024, 4, 64)]
REPEATS = 7


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3                 # us per call


def main():
    print(f"{torch.cuda.get_device_name(0)}, B = {B}, library stamp {_lib.source_stamp()}; us per attention (QK^T -> softmax -> PV of all heads), "
          f"median of {REPEATS} interleaved repeats [min .. max]")
    for T, H, D in SHAPES:
        C = H * D
        g = torch.Generator(device=dev).manual_seed(T + H + D)
        qk = torch.randn(B * T, 2 * C, device=dev, generator=g)
        vt = torch.randn(B, C, T, device=dev, generator=g)
        bv = torch.randn(C, device=dev, generator=g)
        out = torch.empty(B * T, C, device=dev)
        one = torch.tensor([1.0, 1.0], device=dev)
        lg = torch.empty(B, T, T, device=dev)
        mixed = torch.empty(B, T, C, device=dev)
        eps = [_lib.make_epilogue(bias=bv[h * D:(h + 1) * D]) for h in range(H)]
        assert _lib.attention_heads_ok(B, T, H, D)

        def fused():
            _lib.attention_heads(qk, vt, out, B, T, H, D, one, one, D ** -0.5, bias_v=bv)

        def per_head():
            for h in range(H):
                _lib.gemm(qk[:, h * D:], qk[:, C + h * D:], out=lg, M=T, N=T, K=D, lda=2 * C, ldb=2 * C, ldc=T, batch=B,
                          stride_a=T * 2 * C, stride_b=T * 2 * C, stride_c=T * T)
                _lib.softmax_rows(lg, lg, B * T, T, D ** -0.5)
                _lib.gemm(lg, vt[:, h * D:(h + 1) * D], out=mixed[..., h * D:], M=T, N=D, K=T, lda=T, ldb=T, ldc=C, batch=B,
                          stride_a=T * T, stride_b=C * T, stride_c=T * C, epilogue=eps[h])

        forms = [("a fused", fused), ("b per-head x3", per_head)]
        if T == 256 and _lib.attention256_ok(B, T, C):
            forms.append(("c attention256", lambda: _lib.attention256(qk, vt, out, B, C, one, one, C ** -0.5, bias_v=bv)))
        reps = 8 if T <= 256 else 2
        for _, fn in forms:                                 # warm-up: code objects, attributes, clocks
            fn(); fn()
        torch.cuda.synchronize()
        # the two forms on the same operands compute the same function (the timing compares like with like)
        fused(); per_head(); torch.cuda.synchronize()
        diff = float((out.view(B, T, C)[:4] - mixed[:4]).abs().max())
        assert diff < 1e-4, diff
        times = {name: [] for name, _ in forms}
        for _ in range(REPEATS):
            for name, fn in forms:
                times[name].append(timed(fn, reps))
        med = {name: statistics.median(v) for name, v in times.items()}
        flops, byt = 4.0 * B * T * T * C, 16.0 * B * T * C
        line = f"T = {T:4d}, H = {H}, D = {D:3d} (C = {C:3d}):"
        for name, _ in forms:
            v = times[name]
            line += f"  {name} {med[name]:8.0f} [{min(v):.0f} .. {max(v):.0f}]"
        a = med["a fused"]
        line += f"   b / a = {med['b per-head x3'] / a:.2f}x"
        if "c attention256" in med:
            line += f", a / c = {a / med['c attention256']:.2f}"
        line += f"   fused: {flops / a / 1e6:.0f} TFLOP/s fp32-equivalent, {byt / a / 1e3:.0f} GB/s of compulsory bytes"
        print(line, flush=True)
        del qk, vt, out, lg, mixed
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
