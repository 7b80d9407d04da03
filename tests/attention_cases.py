"""Shared, CPU-only ground of the element-wise attention tests (tests/test_attention_cases_host.py, tests/test_hip_attention_elementwise.py):
case builders with planted logits, the fp64 reference with a per-element bound, and a float32 replay of the arithmetic of both kernels of
csrc/attention.hip (``attention256_kernel<C>`` and the streaming ``attention_heads_kernel<D, NW>``).

Reference (``reference``).  Per sample and head, on the fp32 operands promoted to fp64: x_ij = scale q_i . k_j, p = softmax_j x,
out_ic = sum_j p_ij v_jc (+ bias_c); `scale` is the fp32 value the kernel is given.

Bound (``reference`` returns it beside the outputs; u = 2^-24, s_qk / s_v the operands' power-of-two scales, E below):

    tol_ic = 2 sum_j p_ij eps_ij |v_jc - out_ic|                the probabilities' relative errors, first order, times 2
           + E sum_j p_ij |v_jc|                                 the P V contraction
           + lambda_i |out_ic|                                   the row sum l, counted addition by addition (``lane_sum_bound``)
           + T 2^-35 max_j |v_jc|  +  2^-25 / s_v                q_p, q_v: the absolute quanta of subnormal pair halves
           + 4 u (|out_ic + bias_c| + |bias_c|)                  descale product, division, bias add, final store
    eps_ij = E scale A_ij                                        A_ij = sum_c |q_ic| |k_jc|: the Q K^T contraction
           + scale 2^-25 / s_qk (sum_c |q_ic| + sum_c |k_jc|)    an operand half below 2^-14 carries an ABSOLUTE error of 2^-25
           + 4 u |x_ij - m_i| + 4 u                              the exponent's argument and v_exp_f32
           + 3 u (n_ij + 1)                                      streaming kernel only: the rescalings by alpha

Where each term comes from, read from the kernel, and where it departs from the first sketch of this bound (|v_jc| + |out_ic| in the
first line, E |out_ic| or nothing for the row sum):
  * A factor common to a row's probabilities cancels between the numerator and l (both kernels use the SAME e_ij for the sum and for
    P V), so the error of the maximum m itself does not enter; only each logit's own error does: eps_ij.  For relative errors d_ij of
    the probabilities out moves by sum_j p_ij d_ij (v_jc - out_ic) / (1 + sum_j p_ij d_ij).  The sketch bounds |v_jc - out_ic| by
    |v_jc| + |out_ic|; the difference itself is used here (never larger, and much smaller on a row one key dominates, which is what
    lets the band cases see their band).  The factor 2 covers the denominator and exp(eps) - 1 > eps.
  * cut2 writes s x as hi = fp16(s x), lo = fp16(s x - hi): 22 bits where both halves are normal (inside E), an absolute 2^-25 (half
    the subnormal spacing 2^-24) where lo, or hi too, is below 2^-14.  For q and k that is 2^-25 / s_qk per element, times the other
    operand's magnitude, times scale: the second line of eps.  For v it is 2^-25 / s_v times sum_j p_ij = 1: q_v.  For the
    probabilities (cut at scale 2^10, relative to the row's maximum in attention256 and to the running maximum in the streaming
    kernel, later multiplied by alpha <= 1 and divided by l >= 1) it is 2^-35 per key times |v_jc|: q_p with T keys.
    q_v is the exact worst case of ONE cut and is reached: where one key carries a row and |s_v v| of that key is below 2^-14, the
    other terms vanish and err / tol comes to 0.9 (one-hot, jump and gain-6 cases), in the replay and on the device alike.
  * exp: sc = fl(scale s^-2 log2 e) (s^-2 exact; one rounding, and 0.22 u in the fp32 constant), fl(S - m) and the product with sc,
    one rounding each: below 3.3 u |x - m| in the exponent, taken as 4 u |x - m|; v_exp_f32 is a 1-ulp instruction (2 u), the
    product e * (2^10 / sum) of attention256 one more rounding, 1 u spare: 4 u.
  * streaming kernel: a chunk in which the running maximum moves multiplies every accumulator and l_run by alpha = v_exp_f32(...)
    (2 u) with one rounding (1 u); where it does not move alpha is exactly 1.  The arguments of successive alphas telescope into
    |x_ij - m_i| (the running maximum is monotone), so only 3 u per move remain: n_ij = the number of chunks AFTER key j's in which
    query i's fp64 running maximum moves, + 1 for a move the fp32 logits see and fp64 does not (a tie within the logits' error).
  * l is missing from the sketch.  Each lane adds its 16 e of a chunk (its 64 of the row in attention256) one after the other, adds
    the chunk's sum to l_run, and the four lanes meet in two shuffles, all in fp32 and each addition rounding by u times its result.
    With a leading key first in its lane every later addition of that lane rounds at the size of the whole sum (the band cases: 63
    additions of 3e-8 to 1.0 in attention256 are all lost, 2e-6 of l, more than E), so the term is not statistical: lambda_i is u
    times the sum of the partial sums in the kernel's order, computed from the fp64 probabilities.
  * 1 / (l 2^10) s_v^-1, its product with the accumulator, the bias add: 4 u on the magnitudes involved.

E: the relative error |err| / A of a three-product fp16-pair contraction (hi hi + hi lo + lo hi, fp32 accumulation over 32-wide steps),
NOT measured on the kernels.  ``measure_pair_contraction_error`` runs the replay's own contraction on O(1) Gaussian operands at the
contraction lengths of the cases (K = 32, 64, 128, 256 for Q K^T; K = 64, 256, 1024, 4096 with a non-negative operand for P V; 65,536
outputs each) against fp64: max |err| / A = 3.39e-7 at K = 32, 1.4e-7 at K = 64 and 0.8 - 1.6e-7 beyond.  Times 4
(tests/test_hip_epilogue_matrix.py: the kernels' accumulation order differs, and the tail over ~1e5 elements) = 1.36e-6:
    E = 1.4e-6.
The project's pair-GEMM class uses 1e-6, measured at K >= 64 where the same replay gives 1.4e-7 x 4 = 0.6e-6; a head of 32 channels
sums too few products for the operands' 2^-22 cuts to average out (the worst case of ONE product is 3 x 2^-22 = 7.2e-7 A).
tests/test_attention_cases_host.py asserts 4 x measured <= E <= 8 x measured.

Replay (``replay``): torch float32 on the CPU, the kernels' arithmetic with round-to-nearest fp16 cuts that PRESERVE subnormals, the
three products accumulated per 32-wide step, the lane-wise sums of e in the kernels' order, exp2 on fl((S - m) sc).  Streaming form:
chunks of 64 keys with m_run, l_run (four lanes per query), alpha, probabilities x 2^10 cut to pairs, one division at the end;
attention256: e * (2^10 / sum) before the cut.  ``mut`` names one deliberate error (MUTATIONS) for the host tests.

Largest err / tol of the replays over the 81 cases (tests/test_attention_cases_host.py prints every one): 0.81 streaming
(heads-onehot-64x3x32), 0.60 attention256 (a256-onehot-256x1x256).  Above 0.5: the one-hot cases (0.56 - 0.81) and the gain-6 cases
(0.52 - 0.66; attention256 0.58), by q_v as said above; next the band of attention256 (0.49) and the jump cases (up to 0.47); the
streaming band cases 0.17 and 0.23; every other case below 0.3.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
E_PAIR = 1.4e-6
PSCALE = 1024.0
KC = 64                                             # keys per chunk of the streaming kernel
LOG2E_F32 = np.float32(1.44269504088896340736)
MUTATIONS = ("drop_lo_hi", "drop_hi_lo", "flush_hi", "lo_eq_hi", "no_alpha_l", "no_alpha_o", "v_slot_order", "scale_C", "bias_head0",
             "no_lane_sum")


class Case:
    """One launch: kernel "heads" or "a256"; qk [B * T, 2 C] fp32 (q | k, head h in columns [h D, (h + 1) D)), vt [B, C, T] fp32,
    bias [C] fp32, s_qk / s_v powers of two (python floats), scale = fl32(D^-1/2)."""

    def __init__(self, name, kernel, B, T, H, D, qk, vt, bias, s_qk, s_v):
        self.name, self.kernel, self.B, self.T, self.H, self.D, self.C = name, kernel, B, T, H, D, H * D
        self.qk, self.vt, self.bias, self.s_qk, self.s_v = qk.contiguous(), vt.contiguous(), bias.contiguous(), float(s_qk), float(s_v)
        self.scale = float(np.float32(D ** -0.5))
        assert kernel in ("heads", "a256") and (kernel == "heads" or (H == 1 and T == 256))
        assert qk.shape == (B * T, 2 * self.C) and vt.shape == (B, self.C, T) and bias.shape == (self.C,)
        for s, t in ((self.s_qk, qk), (self.s_v, vt)):                       # the kernels' documented range
            assert math.log2(s) == round(math.log2(s)) and float(t.abs().max()) * s < 65504

    @property
    def route(self):
        return f"attention256<{self.C}>" if self.kernel == "a256" else f"heads<{self.D},{8 if self.T % 128 == 0 else 4}>"

    @property
    def grid(self):
        return self.B * 2 if self.kernel == "a256" else self.B * self.H * (self.T // (128 if self.T % 128 == 0 else 64))

    def __repr__(self):
        return self.name


def pow2_scale(t):
    """The power of two that brings the tensor's root mean square nearest to one (what _lib.pairs_scale_from_rows estimates from weights)."""
    ms = float((t.double() ** 2).mean())
    return 2.0 ** max(-24, min(24, round(-0.5 * math.log2(max(ms, 1e-300)))))


# ------------------------------------------------------------------------------------------------------------------ case builders
def random_case(kernel, B, T, H, D, gain, seed, name=None):
    """The existing recipe (tests/test_hip_attention_heads.py make_operands): projections of a GroupNorm's output; gain 6: peaked rows,
    logits up to +-60, 0.05: nearly uniform rows."""
    C = H * D
    g = torch.Generator().manual_seed(seed)
    n = F.group_norm(torch.randn(B, C, T, generator=g) * 3 + 1, 32, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2)
    n = n.permute(0, 2, 1).contiguous()
    wqk = torch.randn(2 * C, C, generator=g) * (gain / C ** 0.5)
    bqk = torch.randn(2 * C, generator=g) * 0.1
    wv, bv = torch.randn(C, C, generator=g) * (0.7 / C ** 0.5), torch.randn(C, generator=g) * 0.1
    qk = (n.reshape(-1, C) @ wqk.T + bqk).contiguous()
    vt = torch.einsum("oc,bpc->bop", wv, n).contiguous()
    return Case(name or f"{kernel}-random{gain:g}-{T}x{H}x{D}", kernel, B, T, H, D, qk, vt, bv, pow2_scale(qk), pow2_scale(vt))


def _noise_operands(B, T, H, D, g, sigma=0.05):
    C = H * D
    q = torch.randn(B, T, H, D, generator=g) * sigma
    k = torch.randn(B, T, H, D, generator=g) * sigma
    vt = torch.randn(B, C, T, generator=g) * 0.7 + torch.randn(C, generator=g)[None, :, None] * 0.3
    bias = torch.randn(C, generator=g) * 0.1
    return q, k, vt, bias


def _finish(name, kernel, B, T, H, D, q, k, vt, bias, s_qk=None, s_v=None):
    qk = torch.cat([q.reshape(B * T, H * D), k.reshape(B * T, H * D)], dim=1).float().contiguous()
    return Case(name, kernel, B, T, H, D, qk, vt.float(), bias.float(), s_qk or pow2_scale(qk), s_v or pow2_scale(vt))


def profile_logits(profile, T, g, band=(-19.0, -17.0)):
    """L_j, the logit planted on channel 0 (the same for every query)."""
    j = torch.arange(T, dtype=torch.float64)
    if profile == "ascending":                      # + 8 per chunk of 64: the running maximum moves in every chunk
        return j * 0.125
    if profile == "descending":                     # the maximum is key 0: it never moves after chunk 0
        return -j * 0.125
    if profile == "jump":                           # a key of the last chunk leads by 220: alpha = exp(-220) underflows to 0
        L = torch.zeros(T, dtype=torch.float64)
        L[T - 3] = 220.0
        return L
    if profile == "band":                           # key 0 at 0, the others in the band: p 2^10 in [5.7e-6, 4.2e-5], fp16 subnormal
        L = band[0] + (band[1] - band[0]) * torch.rand(T, generator=g, dtype=torch.float64)
        L[0] = 0.0
        return L
    raise ValueError(profile)


def planted_case(kernel, B, T, H, D, profile, seed, band=(-19.0, -17.0), name=None):
    """Channel 0 of each head carries the profile: q[:, 0] = 4 and k[j, 0] = L_j / (4 scale); the other channels hold noise of 0.05
    so that the lo halves are exercised.  The reference uses the fp32 operands as they are: nothing here needs to be exact."""
    g = torch.Generator().manual_seed(seed)
    q, k, vt, bias = _noise_operands(B, T, H, D, g)
    name = name or f"{kernel}-{profile}-{T}x{H}x{D}"
    if profile == "uniform":                        # q = 0: every logit is exactly 0, out = mean(v)
        q.zero_()
    elif profile == "onehot":
        nbits = max(1, (T - 1).bit_length())
        rep = D // nbits
        assert rep >= 1
        code = ((torch.arange(T)[:, None] >> torch.arange(nbits)[None, :]) & 1).float() * 2 - 1        # [T, nbits] of +-1
        code = code.repeat_interleave(rep, dim=1)                                                     # [T, nbits rep]
        amp = (140.0 / (2 * rep * D ** -0.5)) ** 0.5                 # two codes differ in >= rep places: a gap of 2 rep amp^2 scale = 140
        perm = onehot_permutation(T)
        assert sorted(perm.tolist()) == list(range(T))
        k[..., :nbits * rep] += amp * code[None, :, None, :]
        q[..., :nbits * rep] += amp * code[perm][None, :, None, :]
    else:
        L = profile_logits(profile, T, g, band)
        q[..., 0] = 4.0
        k[..., 0] = (L / (4.0 * D ** -0.5)).float()[None, :, None]
    return _finish(name, kernel, B, T, H, D, q, k, vt, bias)


def onehot_permutation(T):
    """pi: key pi(i) leads query i (37 is coprime to every T = 64 m in use)."""
    return (torch.arange(T) * 37 + 11) % T


def small_channel_case(kernel, B, T, H, D, which, seed, name=None):
    """One channel (index 1 of each head) 2^-16 of the tensor's rms, the scale still derived from the whole tensor, so the channel's
    scaled entries lie in the fp16 subnormal band.  which = "v": that channel of V (its outputs are small: only an element-wise bound
    sees them).  which = "qk": that channel of K, against a channel of Q 32 times the rms, so that the subnormal halves move the logits."""
    base = random_case(kernel, B, T, H, D, 1.0, seed)
    C = H * D
    g = torch.Generator().manual_seed(seed + 1)
    qk, vt = base.qk.clone().reshape(B, T, 2, H, D), base.vt.clone().reshape(B, H, D, T)
    if which == "v":
        rms = float(vt.double().pow(2).mean().sqrt())
        vt[:, :, 1, :] = torch.randn(B, H, T, generator=g) * rms * 2.0 ** -16
    else:
        rms = float(qk.double().pow(2).mean().sqrt())
        qk[:, :, 0, :, 1] = (torch.randint(0, 2, (B, T, H), generator=g).float() * 2 - 1) * rms * 32
        rms = float(qk.double().pow(2).mean().sqrt())
        qk[:, :, 1, :, 1] = torch.randn(B, T, H, generator=g) * rms * 2.0 ** -16
    qk, vt = qk.reshape(B * T, 2 * C), vt.reshape(B, C, T)
    c = Case(name or f"{kernel}-small_{which}-{T}x{H}x{D}", kernel, B, T, H, D, qk, vt, base.bias, pow2_scale(qk), pow2_scale(vt))
    small = (vt.reshape(B, H, D, T)[:, :, 1] * c.s_v) if which == "v" else (qk.reshape(B, T, 2, H, D)[:, :, 1, :, 1] * c.s_qk)
    assert 2.0 ** -24 < float(small.abs().median()) < 2.0 ** -14              # both halves of the pair subnormal
    return c


def scaled(case, e_qk, e_v):
    """The same case with s_qk, s_v multiplied by 2^e and the operands by 2^-e: the kernel sees the same scaled values."""
    return Case(f"{case.name}-s{e_qk:+d}", case.kernel, case.B, case.T, case.H, case.D, case.qk * 2.0 ** -e_qk, case.vt * 2.0 ** -e_v,
                case.bias, case.s_qk * 2.0 ** e_qk, case.s_v * 2.0 ** e_v)


# ------------------------------------------------------------------------------------------------------------------ fp64 reference
def lane_sum_bound(p, nkeys):
    """The rounding of the row sum l relative to l, counted from the kernel's order of additions on the fp64 probabilities p [Q, T]
    (p is e / l, so partial sums of p are the kernel's partial sums relative to the final l; alpha only rescales them).  Lane g of a
    query adds the keys 16 kb + 4 g + i of each group of `nkeys` (64: a chunk of the streaming kernel; 256: attention256's row) one
    after the other starting from zero (the first addition is exact), then adds the group's sum to its running sum (exact for the
    first group); the four lanes meet in two shuffles.  Each addition rounds by at most u times its result."""
    Q, T = p.shape
    per = p.reshape(Q, T // nkeys, nkeys // 16, 4, 4).permute(0, 1, 3, 2, 4).reshape(Q, T // nkeys, 4, nkeys // 4)
    within = torch.cumsum(per, dim=3)
    running = torch.cumsum(within[..., -1], dim=1)                            # [Q, groups, 4]
    return U * (within[..., 1:].sum(dim=(1, 2, 3)) + running[:, 1:].sum(dim=(1, 2)) + 2.0)


def reference_head(q, k, v, scale, streaming, s_qk, E=E_PAIR):
    """One head in fp64, a block of queries against all keys.  q [Q, D], k, v [T, D] (fp64).  Returns out [Q, D] (no bias) and the
    pieces the bound needs -- logits x, probabilities p, A_ij = sum_c |q_ic| |k_jc|, pv = sum_j p_ij |v_jc| -- with eps [Q, T] and the
    relative rounding of the row sum, l_err [Q]."""
    Q, T = q.shape[0], k.shape[0]
    x = (q @ k.T) * scale
    m = x.max(dim=1, keepdim=True).values
    p = torch.softmax(x, dim=1)
    A = q.abs() @ k.abs().T
    eps = E * scale * A + scale * 2.0 ** -25 / s_qk * (q.abs().sum(1)[:, None] + k.abs().sum(1)[None, :]) + 4 * U * (x - m).abs() + 4 * U
    if streaming:
        nch = T // KC
        cmax = x.reshape(Q, nch, KC).max(dim=2).values
        run = torch.cummax(cmax, dim=1).values
        moved = torch.zeros(Q, nch, dtype=torch.float64)
        moved[:, 1:] = (cmax[:, 1:] > run[:, :-1]).double()
        n_after = moved.sum(1, keepdim=True) - torch.cumsum(moved, dim=1)      # moves in the chunks after c
        eps = eps + 3 * U * (n_after.repeat_interleave(KC, dim=1) + 1)
    return dict(out=p @ v, x=x, p=p, A=A, pv=p @ v.abs(), eps=eps, l_err=lane_sum_bound(p, KC if streaming else T))


def reference(case, E=E_PAIR):
    """fp64 outputs without the bias [B, T, C] and the bound without its bias term [B, T, C]; ``with_bias`` turns the pair into what a
    launch with or without bias_v is held to."""
    B, T, H, D, C = case.B, case.T, case.H, case.D, case.C
    qk = case.qk.double().reshape(B, T, 2, H, D)
    vt = case.vt.double().reshape(B, H, D, T)
    out = torch.empty(B, T, C, dtype=torch.float64)
    tol = torch.empty(B, T, C, dtype=torch.float64)
    qblock = max(16, min(T, (1 << 23) // (T * D)))                           # the [Q, T, D] term below stays at 64 MB
    for b in range(B):
        for h in range(H):
            k, v = qk[b, :, 1, h], vt[b, h].T.contiguous()
            vmax = v.abs().max(dim=0).values
            for i0 in range(0, T, qblock):
                r = reference_head(qk[b, i0:i0 + qblock, 0, h], k, v, case.scale, case.kernel == "heads", case.s_qk, E)
                o, pe = r["out"], r["p"] * r["eps"]
                # sum_j p_ij eps_ij |v_jc - out_ic|: a sum of non-negative terms, in fp32 (1e-4 relative) for the time it takes at T = 4096
                spread = torch.einsum("ij,ijc->ic", pe.float(), (v.float()[None, :, :] - o.float()[:, None, :]).abs()).double() * 1.001
                t = 2 * spread + E * r["pv"] + r["l_err"][:, None] * o.abs() + T * 2.0 ** -35 * vmax[None, :] + 2.0 ** -25 / case.s_v
                out[b, i0:i0 + qblock, h * D:(h + 1) * D] = o
                tol[b, i0:i0 + qblock, h * D:(h + 1) * D] = t
    return out, tol


def with_bias(case, out, tol, bias=True):
    """(reference, bound) of a launch with bias_v (or without): the last term of the bound."""
    b = case.bias.double() if bias else torch.zeros(case.C, dtype=torch.float64)
    ref = out + b
    return ref, tol + 4 * U * (ref.abs() + b.abs())


def band_visibility(case, out, tol):
    """For a band case: (mass of the keys other than key 0, the largest tol / max|v| over the outputs of sample 0 head 0).  The band's
    keys all lie more than 16 below the leading key, so their mass is what a flushed or doubled subnormal probability moves."""
    D, T = case.D, case.T
    qk = case.qk.double().reshape(case.B, T, 2, case.H, D)
    x = (qk[0, :, 0, 0] @ qk[0, :, 1, 0].T) * case.scale
    p = torch.softmax(x, dim=1)
    mass = float((1 - p[:, 0]).min())
    vmax = float(case.vt[0, :D].abs().max())
    return mass, float(tol[0, :, :D].max()) / vmax


# ------------------------------------------------------------------------------------------------------------------ float32 replay
def cut_pairs(x, mut=None):
    """x fp32 (already multiplied by its scale) -> (hi, lo) as fp32 tensors holding fp16 values; round to nearest, subnormals kept."""
    hi = x.half()
    seen = hi.float()                               # what the residual instruction reads as hi
    if mut == "lo_eq_hi":                           # the residual instruction flushes a subnormal fp16 input: lo = fp16(x - 0) = hi
        seen = torch.where(seen.abs() < 2.0 ** -14, torch.zeros_like(seen), seen)
    lo = (x - seen).half().float()
    hi = hi.float()
    if mut == "flush_hi":                           # the matrix instruction flushes a subnormal hi: its mass is dropped
        hi = torch.where(hi.abs() < 2.0 ** -14, torch.zeros_like(hi), hi)
    return hi, lo


def pair_dot(ah, al, bh, bl, mut=None):
    """out[n, m] = sum_k B[n, k] A[m, k]: per 32-wide step acc += Ah Bh, Ah Bl, Al Bh in fp32 (A: the operand read from LDS -- K or
    V^T --, B: the one in registers -- Q or P)."""
    acc = torch.zeros(bh.shape[0], ah.shape[0])
    for k0 in range(0, ah.shape[1], 32):
        a_h, a_l, b_h, b_l = ah[:, k0:k0 + 32], al[:, k0:k0 + 32], bh[:, k0:k0 + 32], bl[:, k0:k0 + 32]
        acc = acc + b_h @ a_h.T
        if mut != "drop_hi_lo":
            acc = acc + b_l @ a_h.T                 # A hi x B lo
        if mut != "drop_lo_hi":
            acc = acc + b_h @ a_l.T                 # A lo x B hi
    return acc


def _lane_sums(e):
    """e [Q, n keys] -> [Q, 4]: lane g of a query adds, in order, the keys 16 kb + 4 g + i (kb outer, i inner)."""
    Q, n = e.shape
    per = e.reshape(Q, n // 16, 4, 4).permute(0, 2, 1, 3).reshape(Q, 4, n // 4)
    s = torch.zeros(Q, 4)
    for t in range(n // 4):
        s = s + per[:, :, t]
    return s


def _shuffle_sum(l, mut=None):
    """Two xor shuffles over the four lanes of a query, as lane 0 sees them; the mutation omits them."""
    return l[:, 0] if mut == "no_lane_sum" else (l[:, 0] + l[:, 1]) + (l[:, 2] + l[:, 3])


_SLOT = torch.tensor([16 * ((kk % 8) // 4) + 4 * (kk // 8) + kk % 4 for kk in range(32)])   # k index 8 g + j of a step -> key of the 32


def _sc(case, mut=None):
    scale = np.float32(case.C ** -0.5) if mut == "scale_C" else np.float32(case.scale)
    inv = np.float32(1.0 / case.s_qk)
    return float(np.float32(np.float32(np.float32(scale * inv) * inv) * LOG2E_F32))


def replay(case, mut=None):
    """The kernel's arithmetic in float32 on the CPU -> [B, T, C] fp32 (with bias)."""
    B, T, H, D, C = case.B, case.T, case.H, case.D, case.C
    sq, sv = np.float32(case.s_qk), np.float32(case.s_v)
    inv_v = float(np.float32(1.0 / case.s_v))
    qk = (case.qk * float(sq)).reshape(B, T, 2, H, D)
    vt = (case.vt * float(sv)).reshape(B, H, D, T)
    sc = _sc(case, mut)
    out = torch.empty(B, T, C)
    for b in range(B):
        for h in range(H):
            qh, ql = cut_pairs(qk[b, :, 0, h], mut)
            kh, kl = cut_pairs(qk[b, :, 1, h], mut)
            vh, vl = cut_pairs(vt[b, h], mut)       # [D, T]
            if case.kernel == "a256":
                S = pair_dot(kh, kl, qh, ql, mut)                                  # [queries, keys]
                m = S.max(dim=1, keepdim=True).values
                e = torch.exp2((S - m) * sc)
                inv = PSCALE / _shuffle_sum(_lane_sums(e), mut)
                ph, pl = cut_pairs(e * inv[:, None], mut)
                if mut == "v_slot_order":
                    idx = (torch.arange(0, T, 32)[:, None] + _SLOT[None, :]).reshape(-1)
                    ph, pl = ph[:, idx], pl[:, idx]
                y = pair_dot(vh, vl, ph, pl, mut) * float(np.float32(np.float32(inv_v) * np.float32(1.0 / PSCALE)))
            else:
                m_run = torch.full((T,), -float("inf"))
                l_run = torch.zeros(T, 4)
                o = torch.zeros(T, D)
                for c0 in range(0, T, KC):
                    S = pair_dot(kh[c0:c0 + KC], kl[c0:c0 + KC], qh, ql, mut)      # [queries, 64]
                    m = torch.maximum(m_run, S.max(dim=1).values)
                    alpha = torch.exp2((m_run - m) * sc)
                    m_run = m
                    e = torch.exp2((S - m[:, None]) * sc)
                    l_run = (l_run if mut == "no_alpha_l" else l_run * alpha[:, None]) + _lane_sums(e)
                    if mut != "no_alpha_o":
                        o = o * alpha[:, None]
                    ph, pl = cut_pairs(e * PSCALE, mut)
                    if mut == "v_slot_order":
                        idx = (torch.arange(0, KC, 32)[:, None] + _SLOT[None, :]).reshape(-1)
                        ph, pl = ph[:, idx], pl[:, idx]
                    o = o + pair_dot(vh[:, c0:c0 + KC], vl[:, c0:c0 + KC], ph, pl, mut)
                l = _shuffle_sum(l_run, mut)
                y = o * (inv_v / (l * PSCALE))[:, None]
            bias = case.bias[:D] if mut == "bias_head0" else case.bias[h * D:(h + 1) * D]
            out[b, :, h * D:(h + 1) * D] = y + bias
    return out


def measure_pair_contraction_error(seed=0):
    """max |err| / A of ``pair_dot`` on cut O(1) Gaussian operands against fp64 of the same fp32 operands, at the contraction lengths of the
    cases: K = 32 .. 256 (Q K^T; 256 x 256 outputs) and K = 64 .. 4096 with one non-negative operand (P V).  -> {K-label: figure}."""
    g = torch.Generator().manual_seed(seed)
    res = {}
    for label, K, positive in [("qk32", 32, False), ("qk64", 64, False), ("qk128", 128, False), ("qk256", 256, False),
                               ("pv64", 64, True), ("pv256", 256, True), ("pv1024", 1024, True), ("pv4096", 4096, True)]:
        a = torch.randn(256, K, generator=g)
        b = torch.randn(256, K, generator=g)
        if positive:
            b = b.abs()
        got = pair_dot(*cut_pairs(a), *cut_pairs(b)).double()
        ref, A = b.double() @ a.double().T, b.double().abs() @ a.double().abs().T
        res[label] = float(((got - ref).abs() / A).max())
    return res


# ------------------------------------------------------------------------------------------------------------------ the case lists
# Streaming shapes: all six (D, NW) forms, T in {64, 128, 192, 256}, H in {1, 2, 3}, grids 1 .. 15.
HEADS_SHAPES = [   # B, T, H, D        grid  route
    (1, 64, 1, 32),      # 1     heads<32,4>
    (1, 192, 2, 32),     # 6     heads<32,4>
    (5, 64, 3, 32),      # 15    heads<32,4>   head offsets 32, 64: not a power of two apart from 0
    (3, 128, 1, 64),     # 3     heads<64,8>
    (5, 256, 1, 64),     # 10    heads<64,8>
    (2, 192, 2, 64),     # 12    heads<64,4>
    (3, 192, 1, 128),    # 9     heads<128,4>
    (1, 256, 2, 128),    # 4     heads<128,8>
    (1, 128, 3, 32),     # 3     heads<32,8>
    (1, 256, 3, 32),     # 6     heads<32,8>
    (1, 64, 1, 128),     # 1     heads<128,4>
    (13, 64, 1, 64),     # 13    heads<64,4>
]
HEADS_PROFILES = ("random1", "uniform", "onehot", "ascending", "descending", "jump", "small_v", "small_qk", "random6", "random0.05")


def heads_case(shape, profile, seed=0):
    B, T, H, D = shape
    if profile.startswith("random"):
        return random_case("heads", B, T, H, D, float(profile[6:]), seed + T + 7 * H + D)
    if profile.startswith("small_"):
        return small_channel_case("heads", B, T, H, D, profile[6:], seed + T + D)
    return planted_case("heads", B, T, H, D, profile, seed + T + D + H)


def a256_case(B, C, profile, seed=0, band=(-19.0, -17.0)):
    if profile.startswith("random"):
        return random_case("a256", B, 256, 1, C, float(profile[6:]), seed + C + B)
    if profile.startswith("small_"):
        return small_channel_case("a256", B, 256, 1, C, profile[6:], seed + C)
    return planted_case("a256", B, 256, 1, C, profile, seed + C, band=band)


_SIX_FORMS = ((0, 4, 5, 6, 7, 8), (2, 3, 11, 10, 7, 9))    # two picks of HEADS_SHAPES, each with one shape per (D, NW) form


def grid_cases():
    """(shape index, profile) of the streaming matrix: every shape with the random recipe at gain 1, and every other profile on six
    shapes, one per (D, NW) form (the two picks alternate), so that each form meets each edge of the recurrence."""
    picks = [(i, "random1") for i in range(len(HEADS_SHAPES))]
    for n, prof in enumerate(HEADS_PROFILES[1:]):
        picks += [(i, prof) for i in _SIX_FORMS[n % 2]]
    return picks


A256_CASES = [   # B, C, profile: both instantiations with B in {1, 3} (grids 2 and 6), every profile that applies
    (1, 128, "random1"), (3, 128, "random6"), (1, 256, "random0.05"), (3, 256, "random1"),
    (1, 128, "uniform"), (3, 256, "uniform"), (1, 128, "onehot"), (1, 256, "onehot"),
    (1, 128, "small_v"), (1, 128, "small_qk"), (3, 256, "small_v"), (1, 256, "small_qk"),
]
BAND_T = (2048, 4096)                               # streaming band cases: B = 1, H = 1, D = 32
A256_BAND = (-17.5, -17.0)                          # attention256's band, narrowed toward -17 (T is fixed at 256)


def band_case(T):
    return planted_case("heads", 1, T, 1, 32, "band", 900 + T)


def a256_band_case(C=128):
    return planted_case("a256", 1, 256, 1, C, "band", 900 + C, band=A256_BAND)
