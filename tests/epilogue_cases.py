"""The CPU side of the epilogue matrices (tests/test_hip_epilogue_matrix.py, tests/test_hip_normfused_matrix.py and their host checks): the
product of epilogue terms, the fp64 reference of the header's epilogue and its per-element bound.  No GPU, no package import.

    out = (act(acc + bias + rowbias[g]) + residual) * out_scale * rowscale[g],   g = m // rows_per_group      (include/idiff_hip.h)

The bound and the origin of E are derived in the docstring of tests/test_hip_epilogue_matrix.py."""
import itertools

import torch

U32 = 2.0 ** -24
E_DIRECT, E_F4 = 1e-6, 4.5e-6
ACTS = ("none", "silu", "elu", "relu", "lrelu")
RESIDUALS = ("off", "dense", "slice")
SLICE_PAD = 32          # ld_residual = N + 32, the slice starts 16 columns in (64 bytes: still 16-byte aligned)
OUT_SCALE = 0.7071


def combos():
    """(bias, rowbias, act, residual, out_scale, rowscale): the full product, 240 entries."""
    return list(itertools.product((False, True), (False, True), ACTS, RESIDUALS, (1.0, OUT_SCALE), (False, True)))


def act64(name, v):
    if name == "silu":
        return v * torch.sigmoid(v)
    if name == "elu":
        return torch.where(v > 0, v, torch.expm1(v))
    if name == "relu":
        return v.clamp_min(0)
    if name == "lrelu":
        return torch.where(v > 0, v, 0.2 * v)
    return v


def epilogue_ref(acc64, A, terms, E):
    """(reference, per-element bound) of the header's epilogue, fp64 on the CPU.  acc64, A: [M, N] fp64; terms: bias [N] | None, rowbias
    [G, N] | None, rows_per_group, act, residual [M, N] | None, out_scale, rowscale [G] | None (all fp64)."""
    M = acc64.shape[0]
    grp = torch.arange(M) // terms["rows_per_group"]
    pre, mag = acc64, A
    if terms["bias"] is not None:
        pre, mag = pre + terms["bias"], mag + terms["bias"].abs()
    if terms["rowbias"] is not None:
        pre, mag = pre + terms["rowbias"][grp], mag + terms["rowbias"][grp].abs()
    a = act64(terms["act"], pre)
    s = torch.full((M, 1), float(terms["out_scale"]), dtype=torch.float64)
    if terms["rowscale"] is not None:
        s = s * terms["rowscale"][grp][:, None]
    small = a.abs()
    if terms["residual"] is not None:
        a, small = a + terms["residual"], small + terms["residual"].abs()
    return a * s, s.abs() * (1.1 * E * mag + 8 * U32 * small)
