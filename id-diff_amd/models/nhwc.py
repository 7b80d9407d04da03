"""The NHWC executor the image score networks share: the primitive steps that do not know which network they serve.

An activation is a ``_T`` ([B, H*W, C] + geometry); every step is one or a few launches from libidiff_hip.so.  ``NCSNpp`` (and
``DDPM``) and ``BeatGANsUNetModel`` inherit ``NhwcExecutor`` and add what is theirs: the module list (= the reference's
``state_dict`` layout), the plan, the weight packing, FIR resampling.  Which kernel serves a 3x3 convolution is decided in one
place, ``CONV3X3_ROUTES`` / ``conv3x3_route``: host logic only, testable without a GPU.  A GroupNorm reaches its reader by one of
several kernels (its own pass, a convolution's tail or loader, a resampler's loader); whichever did it leaves the same ``NormedBy``
record on its output, and ``_conv`` returns one thing, a ``_T``, whether or not its tail applied the norm that follows.
"""
from typing import Callable, NamedTuple, Optional

import torch

from .. import _lib
from .base import HipScoreModel


def _pad4(c):
    return (c + 3) // 4 * 4


class PendingNorm(NamedTuple):
    """A GroupNorm that was NOT applied (NhwcExecutor._gn_act): the one 3x3 convolution that reads the tensor applies it in its loader."""
    coef: torch.Tensor       # [B, C, 2] from groupnorm_coef
    act: Optional[str]
    src: "_T"                # the norm's input
    gn: torch.nn.Module
    src2: Optional["_T"]     # the second source of a concatenation that was not made, or None

    def applied_by(self, route, B, H, W, cout):
        """Does the convolution of [B, H, W] to ``cout`` channels on ``route`` (still) apply this norm in its loader?  Asked by _defer_norm
        before it puts the pass off and again by _conv before it launches (a switch flipped in between: no, the pass after all)."""
        if route is None or route.name != "wino1d":
            return False
        if self.src2 is None:
            return _lib.conv2d_wino1d_normload_ok(B, H, W, self.src.C, cout)
        return _lib.conv2d_wino1d_normload_2src_ok(B, H, W, self.src.C, self.src2.C, cout)


class NormedBy(NamedTuple):
    """On the output of a GroupNorm (and kept through the resamplers): what HipScoreModel.pairs_admissible needs to decide whether the
    consumer may run on fp16 pairs.  Every kernel that applies a norm records it with ``of``; a resampler passes it ``through``."""
    gn: torch.nn.Module
    group_elems: int         # elements per normalised group
    gain: float              # absolute gain of what followed the norm
    modulated: bool          # a per-sample scale-shift followed it

    @classmethod
    def of(cls, gn, channels, pixels, modulated=False):
        """``gn`` over ``channels`` channels (of all its sources) on maps of ``pixels`` pixels."""
        return cls(gn, (channels // gn.num_groups) * pixels, 1.0, modulated)

    def through(self, gain):
        """Behind a linear map whose output stays within ``gain`` times its input's range (a FIR resampler's absolute tap sum)."""
        return self._replace(gain=self.gain * gain)


class _T:
    """An NHWC activation: buffer [B, H*W, C] + geometry (+ the per-tile column sums [B, nsplit, C, 2] its producing
    contraction wrote through epilogue.colstats, which let the consuming GroupNorm skip its statistics pass)."""
    __slots__ = ("buf", "H", "W", "C", "stats", "norm", "pending")

    def __init__(self, buf, H, W, C, stats=None, norm=None, pending=None):
        self.buf, self.H, self.W, self.C, self.stats = buf, H, W, C, stats
        # a PendingNorm where a GroupNorm was NOT applied: ``buf`` is still the norm's raw input
        self.pending = pending
        # a NormedBy on the output of a GroupNorm (and of the resamplers behind one)
        self.norm = norm

    @property
    def is_normed(self):
        """``buf`` holds a GroupNorm's output (not a convolution's that a norm is still to read, _conv's ``then_norm``)."""
        return self.norm is not None and self.pending is None


# the second source of a concatenation where there is none, as far as a norm reads one: no buffer, no channels, no column sums to add
_NO_SOURCE = NamedTuple("_NoSource", [(field, object) for field in ("buf", "C", "stats", "pending")])(None, 0, (None, 0), None)    # immutable


# ------------------------------------------------------------------------------------------------------------
# The 3x3 stride-1 pad-1 routes.  The thresholds are read at call time (tests set the *_MIN_WORKGROUPS to 1 to send test-sized
# batches through the large-batch kernels: they are speed rules, not correctness ones) and the ``_lib.*_ok`` predicates are asked
# per call (a switch flipped by ``thread_option`` between two forwards of one model takes effect).
# launches of fewer workgroups than this stay on the F(2x2, 3x3) kernel
WINO43_MIN_WORKGROUPS = 512
WINO43_PAIRS_MIN_WORKGROUPS = 256
# launches of fewer workgroups than this, and maps narrower than this, stay on the 2-D pair kernel
WINO1D_MIN_WORKGROUPS = 256
WINO1D_MIN_WIDTH = 4
# The x2 FIR of an up block's shortcut in Conv_1's tail (NhwcExecutor._up2_residual_taps) is routed where it was measured faster than the
# resampler's pass beyond the repetitions' spread (scripts/shortcut_shape_ab.py, profiles/shortcut_shape_ab.txt, B = 2240, 256 -> 256, us):
# 8 -> 16: 210 + 1090 against 1084 (-216, spread 30); 16 -> 32: 782 + 4404 against 4422 (-765, spread 64); 4 -> 8: 44 + 327 against 316
# (-55, spread 58: inside it, not routed although the kernel serves rows of 8 pixels).
RESUP_MIN_WIDTH = 16


def _wino43_workgroups(B, H, W, cout):
    """A workgroup takes 32 tiles of 4x4 pixels x 64 channels and a CU holds one."""
    return ((B * (H // 4) * (W // 4) + 31) // 32) * (cout // 64)


def _wino1d_serves(B, H, W, cin, cout, normed, per_image):
    """The row-wise F(4, 3) pair kernel (csrc/wino1d.hip: twice the matrix work of F(4x4, 3x3) for half the operand traffic) where it is served
    and measured at least as fast as the 2-D pair kernel: at one workgroup (512 pixels x 64 channels) per CU and more -- 1.08-1.23x on 16 x 16
    and 32 x 32 maps, 1.03-1.06x on 8 x 8, 1.00-1.01x on 4 x 4 (profiles/r05_wino1d_probe.txt, B = 2240); 64-pixel rows (config 5) likewise."""
    return (per_image and normed and W >= WINO1D_MIN_WIDTH and _lib.conv2d_wino1d_ok(B, H, W, cin, cout)
            and ((B * H * W + 511) // 512) * (cout // 64) >= WINO1D_MIN_WORKGROUPS)


def _wino43_pairs_serves(B, H, W, cin, cout, normed, per_image):
    """F(4x4, 3x3) on fp16 pairs (``normed`` inputs, see NhwcExecutor._conv): faster than F(2x2, 3x3) from one workgroup per CU on, 4x4
    maps included (127 us against 207, 209 against 370 at B = 2240, 256 / 512 -> 256 channels)."""
    return (per_image and normed and _lib.conv2d_winograd43h_ok(B, H, W, cin, cout)
            and _wino43_workgroups(B, H, W, cout) >= WINO43_PAIRS_MIN_WORKGROUPS)


def _wino43_fp32_serves(B, H, W, cin, cout, normed, per_image):
    """F(4x4, 3x3) with the contraction on the fp32 matrix cores: maps of 4x4 pixels (one tile per sample) or launches of fewer than two
    workgroups per CU stay on the 2x2 form (measured 0.87x there, 1.2-1.33x elsewhere: profiles/r04_wino43_time.txt)."""
    return (per_image and H >= 8 and W >= 8 and _lib.conv2d_winograd43_ok(B, H, W, cin, cout)
            and _wino43_workgroups(B, H, W, cout) >= WINO43_MIN_WORKGROUPS)


def _wino22_serves(B, H, W, cin, cout, normed, per_image):
    return _lib.conv2d_winograd_ok(B, H, W, cin, cout)


class Conv3x3Route(NamedTuple):
    """One kernel family.  ``pack`` / ``split`` / ``launch`` are NAMES of ``_lib`` functions, looked up on the module at the call
    (the benchmark's probe and the tests replace them by attribute).  ``form(B, H, W, cin, cout)``: the keyword that names the
    kernel form to both pack and launch; its value keys the bank beside ``id(wt)``."""
    name: str
    bank: str                # self._packed[bank]: dropped with the weights by _invalidate()
    serves: Callable         # (B, H, W, cin, cout, normed, per_image) -> bool; launches nothing
    pack: str
    split: str
    launch: str
    form: Callable


# first match wins; none of them: the implicit GEMM (conv2d_nhwc, any kernel size / stride / pad)
CONV3X3_ROUTES = (
    # Winograd F(4, 3) along the rows on fp16 pairs: 4.5 multiplications per output, half the operand traffic of the 2-D form
    Conv3x3Route("wino1d", "wino1d", _wino1d_serves, "wino1d_pack", "conv2d_wino1d_colstats_split", "conv2d_wino1d",
                 lambda *geom: {}),
    # Winograd F(4x4, 3x3): 2.25 multiplications per output (F(2x2, 3x3) below: 4, the implicit GEMM: 9)
    Conv3x3Route("wino43_pairs", "wino43", _wino43_pairs_serves, "winograd43_pack", "conv2d_winograd43_colstats_split",
                 "conv2d_winograd43", lambda *geom: {"pairs": True}),
    Conv3x3Route("wino43_fp32", "wino43", _wino43_fp32_serves, "winograd43_pack", "conv2d_winograd43_colstats_split",
                 "conv2d_winograd43", lambda *geom: {"pairs": False}),
    # Winograd F(2x2, 3x3): 2.25x fewer MFMA flops than the implicit GEMM
    Conv3x3Route("wino22", "wino", _wino22_serves, "winograd_pack", "conv2d_winograd_colstats_split", "conv2d_winograd",
                 lambda *geom: {}),
)


def conv3x3_route(B, H, W, cin, cout, normed, per_image):
    """The route of a 3x3 stride-1 pad-1 convolution of [B, H, W, cin] to cout channels, or None for the implicit GEMM.
    ``normed``: the input is a GroupNorm's output admitted to the fp16-pair kernels; ``per_image``: the epilogue's row groups are
    whole images (the per-sample time-embedding bias of the residual blocks)."""
    for route in CONV3X3_ROUTES:
        if route.serves(B, H, W, cin, cout, normed, per_image):
            return route
    return None


class NhwcExecutor(HipScoreModel):
    @staticmethod
    def _pack_conv(conv, cin_split=None):
        """[Cout, Cin, KH, KW] -> K-contiguous panel [Cout, KH, KW, Cin_pad]; optional split of Cin in two."""
        w = conv.weight.detach().float()
        cout, cin, kh, kw = w.shape
        parts = [w] if cin_split is None else [w[:, :cin_split], w[:, cin_split:]]
        out = []
        for part in parts:
            c = part.shape[1]
            buf = torch.zeros(cout, kh, kw, _pad4(c), device=w.device)
            buf[..., :c] = part.permute(0, 2, 3, 1)
            out.append(buf.contiguous())
        return out if cin_split is not None else out[0]

    def _new(self, B, H, W, C, like):
        return _T(torch.empty(B, H * W, C, device=like.device, dtype=torch.float32), H, W, C)

    @staticmethod
    def _colstats(y, ns, ep):
        """``y`` feeds a GroupNorm and the kernel that produces it writes ``ns`` per-tile column sums per sample (0: it cannot): allocate
        them, hand them to the epilogue ``ep``, keep them beside the activation."""
        if ns > 0:
            y.stats = (torch.empty(y.buf.shape[0] * ns * y.C * 2, device=y.buf.device, dtype=torch.float64), ns)
            ep["colstats"] = y.stats[0]

    def _gn_act(self, x, gn, act, x2=None, mod=None, conv_cout=None):
        """GroupNorm (+ scale-shift modulation ``mod`` [B, 2*Ctot]) (+activation) of x (or of cat[x, x2]).
        ``conv_cout``: the result's ONLY reader is a 3x3 stride-1 pad-1 convolution to that many channels whose epilogue groups are whole
        images.  Where that convolution takes the ``wino1d`` route on rows of 32 pixels, the norm is unmodulated, of one source with column
        sums, admitted to the fp16 pairs by ITS OWN gamma / beta (the record below: the tensor in memory stays the raw one) and the kernel's
        query routes the class (IDIFF_NO_FUSED_GN_LOAD answers no), the pass is not made: one small launch turns the column sums into an
        affine pair per (image, channel) and the tensor is handed on with a PendingNorm; _conv applies a x + b and the activation in its
        loader.  cat[x, x2] (both with column sums) goes the same way where the two-source query routes its class (its own switch,
        IDIFF_NO_FUSED_GN_LOAD_2SRC): neither the concatenated nor the normalised tensor is made, the record carries ``x2`` as ``src2`` and
        the tensor handed on is the first source under the concatenation's channel count (_defer_norm)."""
        B, HW, G = x.buf.shape[0], x.H * x.W, gn.num_groups
        s2 = _NO_SOURCE if x2 is None else x2
        C = x.C + s2.C
        norm = NormedBy.of(gn, C, HW, modulated=mod is not None)
        # every source carries the column sums its producing contraction wrote: no pass over the activations for the statistics
        summed = x.stats is not None and s2.stats is not None
        if conv_cout is not None and mod is None and summed:
            deferred = self._defer_norm(PendingNorm(None, act, x, gn, x2), norm, conv_cout)
            if deferred is not None:
                return deferred
        y = self._new(B, x.H, x.W, C, x.buf)
        y.norm = norm
        sources, affine = (x.buf, x.C, s2.buf, s2.C, B, HW, G), (gn.weight.detach(), gn.bias.detach(), act, y.buf)
        if summed and C <= 1024 and B <= 65535:
            # the statistics are finished inside the apply kernel (one launch per GroupNorm)
            _lib.groupnorm_apply_colstats(*sources, *x.stats, *s2.stats, gn.eps, *affine, mod=mod)
            return y
        stats = torch.empty(B * G * 2, device=x.buf.device, dtype=torch.float32)
        if summed:
            _lib.groupnorm_finalize(*x.stats, x.C, *s2.stats, s2.C, B, HW, G, gn.eps, stats)
        else:
            ws = torch.empty(B * _lib.groupnorm_nsplit(B, HW, C) * C * 2, device=x.buf.device, dtype=torch.float64)
            _lib.groupnorm_stats(*sources, gn.eps, ws, stats)
        _lib.groupnorm_apply(*sources, stats, *affine, mod=mod)
        return y

    def _pairs_ok(self, norm, transform, **asked):
        """May the consumer of what ``norm`` (a NormedBy) describes run on fp16 pairs?  ``asked``: fields to ask about instead of the record's."""
        norm = norm._replace(**asked)
        return self.pairs_admissible(norm.gn, norm.group_elems, gain=norm.gain, transform=transform, modulated=norm.modulated)

    def _defer_norm(self, pending, norm, conv_cout):
        """_gn_act's unmodulated norm of sources with column sums in front of a 3x3 convolution to ``conv_cout`` channels: the raw tensor
        with ``pending`` (and its coefficients) where the convolution's loader applies it (_gn_act's conditions), else None."""
        x, s2, gn = pending.src, pending.src2 or _NO_SOURCE, pending.gn
        B, C = x.buf.shape[0], x.C + s2.C
        if not (x.pending is None and s2.pending is None and x.W == 32 and _lib.ACT[pending.act] in (0, 1)
                and pending.applied_by(conv3x3_route(B, x.H, x.W, C, conv_cout, True, True), B, x.H, x.W, conv_cout)
                and self._pairs_ok(norm, transform=True)):
            return None
        coef = torch.empty(B * C * 2, device=x.buf.device, dtype=torch.float32)
        _lib.groupnorm_coef(*x.stats, x.C, *s2.stats, s2.C, B, x.H * x.W, gn.num_groups, gn.eps, gn.weight.detach(), gn.bias.detach(), coef)
        return _T(x.buf, x.H, x.W, C, norm=norm, pending=pending._replace(coef=coef))

    def _conv(self, x, wt, bias, stride=1, pad=1, pad_hi=None, normed=False, then_norm=None, residual_up2=None, **ep):
        """``then_norm``: what reads the output.  True: a GroupNorm -> ask the epilogue for the per-tile column sums (``stats``).
        ``residual_up2 = (lo, taps)``: the residual at half the resolution, upsampled x2 by the FIR of the polyphase weights ``taps`` in the
        convolution's tail (_lib.with_residual_up2); only the ``wino1d`` route serves it and the caller has asked (_up2_residual_taps).
        ``(gn, act)`` (_conv_gn_act's argument): that GroupNorm, unmodulated, and nothing else -> where the row-wise kernel applies it in
        its own tail the result is the GroupNorm's output (``is_normed``, no ``stats``), otherwise the convolution's with its column sums.
        ``normed=True``: the input is the output of a GroupNorm (+ activation, + FIR resampling), i.e. bounded by
        sqrt(group size) * |gamma| + |beta| -- only then may the Winograd contraction run on fp16 pairs, whose transformed input
        must stay below 65504 (include/idiff_hip.h), and only if THIS checkpoint's gamma / beta keep that bound inside the range
        (base.HipScoreModel.pairs_admissible, decided once per layer at pack time); any other input takes the fp32 contraction."""
        y, geom, route = self._conv_route(x, wt, stride, pad, pad_hi, normed, ep)
        x = self._settle_pending(x, route, geom)
        if route is not None:
            return self._conv3x3(route, x, wt, bias, y, geom, then_norm, ep, residual_up2)
        if residual_up2 is not None:
            raise RuntimeError("_conv: an upsampled residual for a convolution off the 3x3 routes")
        kh, kw = wt.shape[1:3]
        if then_norm:
            self._colstats(y, _lib.conv2d_colstats_split(*geom, kh, kw, stride, pad, pad_hi), ep)
        _lib.conv2d_nhwc(x.buf, wt, y.buf, *geom, kh, kw, stride, pad, epilogue=_lib.make_epilogue(bias=bias, **ep), pad_hi=pad_hi)
        return y

    def _conv_route(self, x, wt, stride, pad, pad_hi, normed, ep):
        """_conv's geometry: the output tensor, (B, H, W, cin, cout), the route (None: the implicit GEMM); ``ep`` gets its row groups."""
        cout, kh, kw, cin = wt.shape
        assert cin == x.C, (cin, x.C)
        if normed:
            assert x.norm is not None, "normed=True on a tensor that is not a GroupNorm's (resampled) output"
            normed = self._pairs_ok(x.norm, transform=True)
        ph = pad if pad_hi is None else pad_hi
        OH = (x.H + pad + ph - kh) // stride + 1
        OW = (x.W + pad + ph - kw) // stride + 1
        ep.setdefault("rows_per_group", OH * OW)
        geom = (x.buf.shape[0], x.H, x.W, cin, cout)
        route = None
        if (kh, kw, stride, pad, ph) == (3, 3, 1, 1, 1):
            route = conv3x3_route(*geom, normed, ep["rows_per_group"] == OH * OW)
        return self._new(geom[0], OH, OW, cout, x.buf), geom, route

    def _settle_pending(self, x, route, geom):
        """``x`` as the convolution on ``route`` may read it: itself, or, where its norm is pending and this is not the convolution
        _gn_act foresaw (a switch flipped in between), the pass after all -- never a raw tensor into a kernel that takes it for a normed one."""
        p = x.pending
        if p is None or p.applied_by(route, *geom[:3], geom[4]):
            return x
        return self._gn_act(p.src, p.gn, p.act, p.src2)

    def _up2_residual_taps(self, x, cout, taps):
        """``taps`` where the 3x3 convolution of ``x`` (a GroupNorm's output) to ``cout`` channels adds a residual given at half the
        resolution in its own tail: the ``wino1d`` route, no norm pending for its loader, the kernel's query (rows of 8 / 16 / 32 pixels;
        IDIFF_NO_FUSED_RES_UP answers no).  Otherwise None: the caller upsamples the residual itself."""
        if taps is None or x.pending is not None or x.norm is None or x.W < RESUP_MIN_WIDTH:
            return None
        geom = (x.buf.shape[0], x.H, x.W, x.C, cout)
        route = conv3x3_route(*geom, self._pairs_ok(x.norm, transform=True), True)
        if route is None or route.name != "wino1d" or not _lib.conv2d_wino1d_resup_ok(*geom):
            return None
        return taps

    def _conv3x3(self, route, x, wt, bias, y, geom, then_norm, ep, residual_up2=None):
        """_conv on one of CONV3X3_ROUTES: the filter bank, the epilogue with what rides beside it, one launch."""
        form = route.form(*geom)
        # the transformed filter bank is cached beside the panel; the entry keeps `wt` so that its id cannot be reused while it lives
        bank = self._packed.setdefault(route.bank, {})
        key = (id(wt), *form.values()) if form else id(wt)
        if key not in bank:
            bank[key] = (wt, getattr(_lib, route.pack)(wt, *geom[3:], **form))
        # the fused tail takes bias and the per-image bias only: an activation or a scale in front of the norm stays two launches
        fused = (isinstance(then_norm, tuple) and x.pending is None and route.name == "wino1d"
                 and _lib.conv2d_wino1d_gn_ok(*geom, then_norm[0].num_groups) and not (set(ep) - {"rowbias", "ld_rowbias", "rows_per_group"}))
        if then_norm and not fused:
            self._colstats(y, getattr(_lib, route.split)(*geom), ep)
        epilogue = _lib.make_epilogue(bias=bias, **ep)
        if fused:
            gn, act = then_norm
            epilogue = _lib.with_groupnorm(epilogue, gn.num_groups, gn.weight.detach(), gn.bias.detach(), gn.eps, act)
            y.norm = NormedBy.of(gn, y.C, y.H * y.W)
        elif x.pending is not None:
            p = x.pending
            epilogue = _lib.with_normload(epilogue, p.coef, p.act, *((None, None) if p.src2 is None else (p.src2.buf, p.src.C)))
        if residual_up2 is not None:        # (every launcher but conv2d_wino1d's plain form refuses the request: never dropped)
            epilogue = _lib.with_residual_up2(epilogue, *residual_up2)
        getattr(_lib, route.launch)(x.buf, bank[key][1], y.buf, *geom, epilogue=epilogue, **form)
        return y

    def _conv_gn_act(self, x, wt, bias, gn, act, mod=None, next_cout=None, **conv_args):
        """3x3 conv followed by GroupNorm ``gn`` (+ modulation ``mod``) + activation, the convolution's output read by nothing else
        (Conv_0 -> GroupNorm_1 of a residual block).  One launch where the convolution takes the ``wino1d`` route, the kernel's query admits
        the geometry and group count (maps of at most 256 pixels; IDIFF_NO_FUSED_GN answers no), the norm is unmodulated and the
        epilogue in front of it is bias + per-image bias only: the convolution's output then never reaches memory.  Otherwise the
        convolution with column sums and _gn_act, as two launches.  ``next_cout``: the norm's only reader is a 3x3 convolution to that many
        channels (_gn_act's ``conv_cout``: on 32-pixel rows that convolution's loader applies the norm)."""
        if mod is not None:
            return self._gn_act(self._conv(x, wt, bias, then_norm=True, **conv_args), gn, act, mod=mod)
        y = self._conv(x, wt, bias, then_norm=(gn, act), **conv_args)
        return y if y.is_normed else self._gn_act(y, gn, act, conv_cout=next_cout)

    def _pointwise(self, x, w, bias, stats=False, pairs=None, **ep):
        """1x1 conv / NIN on NHWC = plain GEMM over [B*HW, Cin]; w is [Cout, Cin].  ``pairs=(pk, act_scale)``: on fp16 pairs where that
        GEMM serves the shape, for an activation that is NOT a GroupNorm's output but whose scale is known: ``act_scale`` = device
        {s, 1 / s} (the attention output is a convex combination of the rows of v: never beyond v's range, so v's scale serves)."""
        B = x.buf.shape[0]
        cout, cin = w.shape
        assert cin == x.C, (cin, x.C)
        M = B * x.H * x.W
        on_pairs = pairs is not None and _lib.gemm_pairs_ok(M, cout, cin)
        y = self._new(B, x.H, x.W, cout, x.buf)
        if stats:
            self._colstats(y, _lib.gemm_colstats_split(M, cout, cin, cin, w.stride(0), x.H * x.W), ep)
        a, out = x.buf.view(-1, cin), y.buf.view(-1, cout)
        if on_pairs:
            _lib.gemm_pairs(a, w, _lib._pairs_scale_of(pairs[0], w), out, epilogue=_lib.make_epilogue(bias=bias, **ep), act_scale=pairs[1])
        else:
            _lib.gemm(a, w, out=out, epilogue=_lib.make_epilogue(bias=bias, **ep))
        return y

    def _attention(self, pk, x, n, wqk, bqk, wv, bv, wo, bo, cache, key, out_scale=1.0, heads=1):
        """Self-attention over ``n`` = a GroupNorm of ``x``: q|k projection (``wqk`` [2C, C], the two stacked), V^T,
        softmax(q k^T / sqrt(D)) v per head, output projection, (+ x) * out_scale.  The V bias is added after P.V (the rows of P sum
        to one), so V^T is produced directly in the K-contiguous layout that product wants.  ``cache[key]``: the operands' power-of-two
        scales, kept as long as the weights.  Head h owns rows [h D, (h + 1) D) of each of q, k (the halves of ``wqk``) and v,
        D = C / heads -- the callers permute their projection into that order at pack time; the projections do not know the heads.
        In between, ONE launch with the logits never written (csrc/attention.hip) where the norm is admitted to fp16 pairs and the
        kernel serves the shape: ``attention256`` for one head, the streaming ``attention_heads`` for more.  Otherwise
        the three-launch form once per head on column views of the same buffers."""
        B, HW, C = x.buf.shape[0], x.H * x.W, x.C
        D = C // heads
        gn = n.norm.gn
        pairs = self._pairs_ok(n.norm, transform=False, gain=1.0, modulated=False)     # the projections read the norm's own output
        dev = x.buf.device
        qk = torch.empty(B * HW, 2 * C, device=dev, dtype=torch.float32)
        _lib.gemm_normed(pk, n.buf.view(-1, C), wqk, qk, epilogue=_lib.make_epilogue(bias=bqk), pairs=pairs)    # n: a GroupNorm's output
        # V^T[b] = Wv^T-panel [C, Cin] x n[b]^T -> [C, HW], K-contiguous for the P.V product (bias deferred)
        vt = torch.empty(B, C, HW, device=dev, dtype=torch.float32)
        _lib.gemm_weight_times_normed_t(pk, wv, n.buf, vt, B, HW, C, pairs=pairs)
        mixed = _T(torch.empty(B, HW, C, device=dev, dtype=torch.float32), x.H, x.W, C)
        scale = float(D) ** (-0.5)                # BeatGANs: (q * s) . (k * s) with s = D^-1/4 (BeatGANsblocks.py:482, :517)
        if pairs and (_lib.attention256_ok(B, HW, C) if heads == 1 else _lib.attention_heads_ok(B, HW, heads, D)):
            # the operands' power-of-two scales from the projections' row norms (their input n has unit variance times gamma's scale)
            if key not in cache:
                gam = float(torch.sqrt((gn.weight.detach().double() ** 2).mean() + (gn.bias.detach().double() ** 2).mean()))
                cache[key] = (_lib.pairs_scale_from_rows(wqk, bqk, gam), _lib.pairs_scale_from_rows(wv, bv, gam))
            s_qk, s_v = cache[key]
            if heads == 1:
                _lib.attention256(qk, vt, mixed.buf, B, C, s_qk, s_v, scale, bias_v=bv)
            else:
                _lib.attention_heads(qk, vt, mixed.buf, B, HW, heads, D, s_qk, s_v, scale, bias_v=bv)
            return self._pointwise(mixed, wo, bo, pairs=(pk, s_v), residual=x.buf, out_scale=out_scale, stats=True)
        if heads > 1 and D % 4:
            raise NotImplementedError(f"attention heads of {D} channels: the GEMM takes a head as a column view only where its width "
                                      "is a multiple of 4")
        logits = torch.empty(B, HW, HW, device=dev, dtype=torch.float32)
        for h in range(heads):
            _lib.gemm(qk[:, h * D:], qk[:, C + h * D:], out=logits, M=HW, N=HW, K=D, lda=2 * C, ldb=2 * C, ldc=HW, batch=B,
                      stride_a=HW * 2 * C, stride_b=HW * 2 * C, stride_c=HW * HW)
            _lib.softmax_rows(logits, logits, B * HW, HW, scale)
            _lib.gemm(logits, vt[:, h * D:(h + 1) * D], out=mixed.buf[..., h * D:], M=HW, N=D, K=HW, lda=HW, ldb=HW, ldc=C, batch=B,
                      stride_a=HW * HW, stride_b=C * HW, stride_c=HW * C, epilogue=_lib.make_epilogue(bias=bv[h * D:(h + 1) * D]))
        return self._pointwise(mixed, wo, bo, residual=x.buf, out_scale=out_scale, stats=True)

    def _box(self, x, up):
        B = x.buf.shape[0]
        y = self._new(B, x.H * 2 if up else x.H // 2, x.W * 2 if up else x.W // 2, x.C, x.buf)
        _lib.resample2x_nhwc(x.buf, y.buf, B, x.H, x.W, x.C, up)
        y.norm = x.norm                                        # nearest x2 / 2x2 mean: never beyond the input's range
        return y

    def _add(self, a, b, scale):
        y = self._new(a.buf.shape[0], a.H, a.W, a.C, a.buf)
        _lib.add_scale(a.buf, b.buf, y.buf, a.buf.numel(), scale)
        return y

    def _cat(self, a, b):
        B = a.buf.shape[0]
        y = self._new(B, a.H, a.W, a.C + b.C, a.buf)
        _lib.concat_cols(a.buf, a.C, b.buf, b.C, y.buf, B * a.H * a.W)
        return y
