"""Both fused attention kernels of csrc/attention.hip, every output element against fp64 (python -m pytest -m gpu).

Cases, reference and bound come from tests/attention_cases.py (its docstring derives the bound term by term from the kernels'
roundings; tests/test_attention_cases_host.py checks it on the CPU: a float32 replay of each kernel stays inside, ten mutations leave).
Every launch here
  * asserts the instantiation `_lib.attention_heads_route` / `_lib.attention256_route` report for its arguments (the chooser the
    launcher itself calls); the case lists are asserted to reach all six streaming forms and both attention256 forms,
  * writes into a NaN-filled output over-allocated by 8 rows: the rows past B T stay NaN, every element before them is finite,
  * is held element by element to |got - ref| <= tol_ic, with bias_v and without.

Streaming kernel: 12 shapes (T in {64, 128, 192, 256}, D in {32, 64, 128}, H in {1, 2, 3}; grids 1, 3, 4, 6, 9, 10, 12, 13, 15: every
non-zero residue mod 8 for the XCD remap, seven of the grids below 8), all with the random recipe at gain 1, and each of the
profiles random (gains 0.05, 6), uniform, one-hot, ascending, descending, jump, small-channel v and q|k on one shape per (D, NW)
form; band cases at T = 2048 and 4096 (at 1024 keys the band's mass is 6.4 times the tolerance, under the 10 the host test asks for).  attention256: C in {128, 256} x B in {1, 3} x random, uniform, one-hot, small-channel; its band
case (narrowed to [-17.5, -17]) runs under the bound like any other, but 255 keys carry only 2.4 times the tolerance: the small-channel
cases are that kernel's subnormal tests.

Scales (test_power_of_two_scales_are_exact): s_qk, s_v at 2^-12, 1, 2^12 with the operands scaled inversely.  A softmax is not
invariant under a scaling of q and k, so the softmax scale goes with them (scale 4^e, exact): then every scaled operand, the exponent's
factor and every probability are the same numbers; V's scale leaves the outputs multiplied by 2^-e (bias_v scaled alike).  The outputs
are bit-identical across the three.

Pitched q|k (ld_qk = 2 C + 4, 2 C + 32, pad columns NaN) and the refusals go through the raw C entry points.

Measured on the MI355X (largest err / tol over the launches with and without bias_v; a ratio above 0.5 is called out):
    kernel      profile                  cases  forms   max err / tol   at
    streaming   random, gain 1             12     6       0.037         5x64x3x32    heads<32,4>
    streaming   random, gain 0.05           6     6       0.127         5x256x1x64   heads<64,8>
    streaming   random, gain 6              6     6       0.865         5x64x3x32    heads<32,4>
    streaming   uniform                     6     6       0.084         1x256x2x128  heads<128,8>
    streaming   one-hot                     6     6       0.913         13x64x1x64   heads<64,4>
    streaming   ascending                   6     6       0.113         3x192x1x128  heads<128,4>
    streaming   descending                  6     6       0.128         13x64x1x64   heads<64,4>
    streaming   jump                        6     6       0.635         3x192x1x128  heads<128,4>
    streaming   small channel of v          6     6       0.691         5x64x3x32    heads<32,4>
    streaming   small channel of q|k        6     6       0.033         1x64x1x32    heads<32,4>
    streaming   band, 2048 / 4096 keys    1 / 1   1    0.281 / 0.339    1xTx1x32     heads<32,8>
    attention256  random, gain 1 / 0.05 / 6  2 / 1 / 1   0.017 / 0.103 / 0.590         attention256<128>, <256>
    attention256  uniform                     2     2       0.056         3x256        attention256<256>
    attention256  one-hot                     2     2       0.656         1x128        attention256<128>
    attention256  small channel of v / q|k  2 / 2   2    0.440 / 0.033    1x128        attention256<128>
    attention256  band [-17.5, -17]           1     1       0.600         1x128        attention256<128>
81 cases, 162 launches, every element inside its bound; with bias_v the one-hot cases give the ratios of the CPU replay to three digits
(0.809, 0.788, 0.740).  Above 0.5, all by ONE term: where a single key carries a row (one-hot, jump,
gain 6) and where v is small (its small channel; the band of attention256, whose row sum loses 63 additions), the bound shrinks to V's
quantum 2^-25 / s_v or the counted rounding of l, and both are exact worst cases of what the kernel does, reached in the replay too.
The largest, 0.913, is an output of 13x64x1x64 one-hot without bias.  The scale and pitch comparisons are bit-identical, every refusal
left its output untouched.  No case failed: no kernel bug was found.
"""
import pytest
import torch

import attention_cases as ac
import id_diff_amd  # noqa: F401
from id_diff_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD_ROWS = 8


def scale_pair(s):
    return torch.tensor([s, 1.0 / s], dtype=torch.float32, device=DEV)


class Device:
    """A case's operands on the device.  ld: the q|k row pitch (pad columns NaN); the NaN-filled output has PAD_ROWS rows to spare."""

    def __init__(self, case, ld=None):
        C = case.C
        self.case, self.ld = case, ld or 2 * C
        buf = torch.full((case.B * case.T, self.ld), float("nan"), device=DEV)
        buf[:, :2 * C] = case.qk.to(DEV)
        self.qk, self.vt, self.bias = buf, case.vt.to(DEV), case.bias.to(DEV)
        self.s_qk, self.s_v = scale_pair(case.s_qk), scale_pair(case.s_v)
        self.big = torch.empty(case.B * case.T + PAD_ROWS, C, device=DEV)

    def launch(self, bias=True, scale=None):
        """One launch through the raw entry point; returns the [B, T, C] outputs on the host after the checks every launch gets."""
        c = self.case
        bv = self.bias if bias else None
        scale = c.scale if scale is None else scale
        self.big.fill_(float("nan"))
        args = (self.qk.data_ptr(), self.ld, self.vt.data_ptr(), _lib._ptr(bv), self.s_qk.data_ptr(), self.s_v.data_ptr(), self.big.data_ptr())
        if c.kernel == "heads":
            assert _lib.attention_heads_route(*args, c.B, c.T, c.H, c.D) == c.route
            rc = _lib.lib().idiff_attention_heads_f32(*args, c.B, c.T, c.H, c.D, scale, _lib._stream())
        else:
            assert _lib.attention256_route(*args, c.B, 256, c.C) == c.route
            rc = _lib.lib().idiff_attention256_f32(*args, c.B, 256, c.C, scale, _lib._stream())
        assert rc == 0, _lib.lib().idiff_last_error().decode()
        got = self.big.cpu()
        assert bool(torch.isnan(got[c.B * c.T:]).all()), "rows past B * tokens were written"
        got = got[:c.B * c.T].reshape(c.B, c.T, c.C)
        assert bool(torch.isfinite(got).all()), "non-finite outputs"
        return got


def check(case, ld=None):
    """Both launches of a case against the bound; returns the outputs with bias (for the bit comparisons)."""
    out, tol = ac.reference(case)
    dev = Device(case, ld)
    ratios, keep = [], None
    for bias in (True, False):
        got = dev.launch(bias=bias)
        ref, t = ac.with_bias(case, out, tol, bias)
        ratio = (got.double() - ref).abs() / t
        ratios.append(float(ratio.max()))
        keep = got if bias else keep
    print(f"ATTN_EW {case.name:34s} {case.route:18s} grid {case.grid:3d}  max err/tol {ratios[0]:.3f} (bias) {ratios[1]:.3f} (no bias)")
    assert max(ratios) <= 1.0, (case.name, ratios)
    return keep


HEADS_KEYS = ac.grid_cases()


@pytest.mark.parametrize("idx,profile", HEADS_KEYS, ids=[f"{'x'.join(map(str, ac.HEADS_SHAPES[i]))}-{p}" for i, p in HEADS_KEYS])
def test_streaming_kernel_elementwise(idx, profile):
    case = ac.heads_case(ac.HEADS_SHAPES[idx], profile)
    got = check(case)
    if profile == "onehot":                         # the key-slot order of V, pinned element by element: out_i = v_pi(i) + bias
        v = case.vt.reshape(case.B, case.C, case.T).permute(0, 2, 1)[:, ac.onehot_permutation(case.T)]
        assert float((got - (v + case.bias)).abs().max()) < 1e-5


@pytest.mark.parametrize("B,C,profile", ac.A256_CASES, ids=[f"{B}x{C}-{p}" for B, C, p in ac.A256_CASES])
def test_attention256_elementwise(B, C, profile):
    case = ac.a256_case(B, C, profile)
    got = check(case)
    if profile == "onehot":
        v = case.vt.permute(0, 2, 1)[:, ac.onehot_permutation(256)]
        assert float((got - (v + case.bias)).abs().max()) < 1e-5


@pytest.mark.parametrize("T", ac.BAND_T)
def test_streaming_kernel_band_of_subnormal_probabilities(T):
    """Key 0 at logit 0 in chunk 0, every other key in [-19, -17]: p 2^10 is an fp16 subnormal in hi AND lo, relative to a running
    maximum that never moves.  A flushed half loses the band's mass (3.7e-5 / 7.4e-5 of the row), a doubled one adds it again: 23 and 30
    times the tolerance (tests/test_attention_cases_host.py)."""
    check(ac.band_case(T))


def test_attention256_band_of_subnormal_probabilities():
    check(ac.a256_band_case(128))


def test_the_cases_reach_every_instantiation():
    F = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000)      # fabricated aligned addresses: the queries dereference nothing
    seen = set()
    for idx, _ in HEADS_KEYS:
        B, T, H, D = ac.HEADS_SHAPES[idx]
        seen.add(_lib.attention_heads_route(F[0], 2 * H * D, F[1], F[2], F[3], F[4], F[5], B, T, H, D))
    assert seen == {f"heads<{D},{NW}>" for D in (32, 64, 128) for NW in (4, 8)}
    seen = {_lib.attention256_route(F[0], 2 * C, F[1], F[2], F[3], F[4], F[5], B, 256, C) for B, C, _ in ac.A256_CASES}
    assert seen == {"attention256<128>", "attention256<256>"}


SCALE_CASES = [("heads", (2, 192, 2, 64), "random1"), ("heads", (1, 256, 3, 32), "small_qk"), ("heads", (1, 64, 1, 128), "small_v"),
               ("a256", (1, 128), "random1"), ("a256", (1, 256), "small_v")]


@pytest.mark.parametrize("kernel,shape,profile", SCALE_CASES, ids=[f"{k}-{'x'.join(map(str, s))}-{p}" for k, s, p in SCALE_CASES])
def test_power_of_two_scales_are_exact(kernel, shape, profile):
    base = ac.heads_case(shape, profile) if kernel == "heads" else ac.a256_case(shape[0], shape[1], profile)
    want = Device(base).launch(bias=True)
    for e in (-12, 12):
        # s 2^e with the operands 2^-e: the same scaled operands.  The logits are q . k scale, so scale takes 4^e; out and bias_v scale with v.
        c = ac.scaled(base, e, e)
        c.bias = base.bias * 2.0 ** -e
        got = Device(c).launch(bias=True, scale=base.scale * 4.0 ** e)
        assert torch.equal(got * 2.0 ** e, want), (e, float((got * 2.0 ** e - want).abs().max()))


PITCH_CASES = [("heads", (2, 192, 2, 64), "random1"), ("heads", (1, 256, 3, 32), "random1"), ("heads", (1, 64, 1, 128), "random1"),
               ("a256", (3, 128), "random6"), ("a256", (1, 256), "random0.05")]


@pytest.mark.parametrize("pad", [4, 32])
@pytest.mark.parametrize("kernel,shape,profile", PITCH_CASES, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s, p in PITCH_CASES])
def test_pitched_qk_is_bit_equal_to_the_contiguous_launch(kernel, shape, profile, pad):
    case = ac.heads_case(shape, profile) if kernel == "heads" else ac.a256_case(shape[0], shape[1], profile)
    want = Device(case).launch(bias=True)
    dev = Device(case, ld=2 * case.C + pad)
    assert bool(torch.isnan(dev.qk[:, 2 * case.C:]).all())
    assert torch.equal(dev.launch(bias=True), want)
    assert torch.equal(dev.launch(bias=False), Device(case).launch(bias=False))


def test_refusals_of_the_raw_entry_points():
    """Each refused call returns non-zero, names its entry point in idiff_last_error and leaves a NaN-filled output untouched; B == 0
    returns 0 and writes nothing.  (tests/test_hip_ops.py::test_attention256_limits only reaches the binding's shape error.)"""
    L = _lib.lib()
    for kernel in ("heads", "a256"):
        B, T, H, D = (2, 128, 2, 32) if kernel == "heads" else (2, 256, 1, 128)
        C = H * D
        qk = torch.zeros(B * T * (2 * C + 8) + 4, device=DEV)
        vt, bias = torch.zeros(B * C * T + 4, device=DEV), torch.zeros(C + 4, device=DEV)
        out = torch.full((B * T * C + 4,), float("nan"), device=DEV)
        one = scale_pair(1.0)
        ok = dict(qk=qk.data_ptr(), ld=2 * C, vt=vt.data_ptr(), bias=bias.data_ptr(), s_qk=one.data_ptr(), s_v=one.data_ptr(),
                  out=out.data_ptr(), B=B, T=T, H=H, D=D)
        bad = [dict(ld=2 * C + 2), dict(ld=2 * C + 1), dict(ld=2 * C - 4), dict(qk=ok["qk"] + 4), dict(vt=ok["vt"] + 4), dict(out=ok["out"] + 4),
               dict(bias=ok["bias"] + 4), dict(qk=0), dict(vt=0), dict(out=0), dict(s_qk=0), dict(s_v=0), dict(B=-1)]
        bad += [dict(T=96), dict(D=48), dict(H=64)] if kernel == "heads" else [dict(T=192), dict(D=96), dict(T=128)]

        def call(a):
            head = (a["qk"], a["ld"], a["vt"], a["bias"], a["s_qk"], a["s_v"], a["out"])
            if kernel == "heads":
                return (L.idiff_attention_heads_f32(*head, a["B"], a["T"], a["H"], a["D"], 0.125, _lib._stream()),
                        _lib.attention_heads_route(*head, a["B"], a["T"], a["H"], a["D"]))
            return (L.idiff_attention256_f32(*head, a["B"], a["T"], a["H"] * a["D"], 0.125, _lib._stream()),
                    _lib.attention256_route(*head, a["B"], a["T"], a["H"] * a["D"]))
        for change in bad:
            rc, route = call(dict(ok, **change))
            assert rc != 0 and route is None, (kernel, change)
            assert L.idiff_last_error().decode().startswith("attention_heads: " if kernel == "heads" else "attention256: "), (kernel, change)
        rc, route = call(dict(ok, B=0))
        assert rc == 0 and route == "none"
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), kernel
        rc, route = call(ok)                        # the same arguments unchanged are served
        assert rc == 0 and route == (f"heads<{D},8>" if kernel == "heads" else f"attention256<{C}>")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out[:B * T * C]).all()) and bool(torch.isnan(out[B * T * C:]).all())
