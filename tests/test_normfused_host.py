"""CPU-side checks of the bounds tests/test_hip_normfused_matrix.py holds the GroupNorm-fused kernels to (tests/normfused_cases.py).

The bounds hold for the reference arithmetic alone: an fp32 replay of every case of the GPU module (z rounded to fp32 from the fp64 fma of
the fp32 operands, torch fp32 SiLU, torch fp32 direct convolution or an fp32 tap loop, the epilogue in fp32) stays inside its bound -- with
E = E_DIRECT = 1e-6, the class of the replay's direct contraction -- on every element.  And the bounds have teeth: each of the thirteen
mutated replays leaves the bound by a factor of at least 10 on at least one case.  The inputs' properties the mutations rely on are asserted,
the restated F(4, 3) matrices satisfy the bilinear identity, and the emulated fp16-pair contraction's error is measured here.

Printed maxima (python -m pytest -s tests/test_normfused_host.py), largest err / tol of the replays per form:
    REPLAY loader, one source      0.208        REPLAY loader, two sources     0.141        REPLAY statistics kinds   0.137
    REPLAY chain                   0.049        REPLAY tail norm               0.052        REPLAY FIR up / down      0.174 / 0.208
    REPLAY FIR chain               0.374
    EMUL   loader inputs 3.9e-7, tail-norm inputs 4.1e-7 (max |err| / A of the emulated row-wise F(4, 3) on fp16 pairs)
    COEF   exact GroupNorm against its fp32 coefficient form, conv output, / isolated tol (E_F4): benign 0.004 (|a| <= 1.5, |b| <= 3.7),
           |mean| / std = 30 0.096 (|b| <= 64), constant group 0.12 (|a| <= 1773, |b| <= 4434; four channels of 32, three images)
    CHAIN  coefficient term / (E A): benign 0.20, |mean| / std = 30 4.2 - 4.8, constant group 1.0e3
    MUTATION smallest factor beyond the bound over the thirteen: 6.9e3 (the neighbouring image's coefficients); every other above 2e4
"""
import numpy as np
import pytest
import torch

import norm_act_cases as nc
import normfused_cases as fc

PRINTED = {}


def note(key, value):
    PRINTED[key] = max(PRINTED.get(key, 0.0), value)
    print(f"\n{key}: {PRINTED[key]:.3g}")


HOST_COMBOS = [fc.BIAS_ONLY] + fc.PRODUCTION + [
    (False, False, "silu", "off", 1.0, False), (True, True, "silu", "slice", fc.OUT_SCALE, True), (False, True, "elu", "dense", 1.0, True),
    (True, False, "relu", "slice", fc.OUT_SCALE, False), (False, False, "lrelu", "dense", fc.OUT_SCALE, True), (False, False, "none", "off", 1.0, False)]
_loader = {}


def loader_case(shape, act, kind="benign", cpg=4, chain=False):
    """The operands, fp32 coefficients, reference terms (E_DIRECT: the replay's class) and replay contraction of one loader case."""
    key = (shape, act, kind, cpg, chain)
    if key not in _loader:
        B, H, C1, C2, Cout = shape
        Cin = C1 + C2
        G = 1 if cpg == 0 else Cin // cpg
        d = fc.raw_inputs(B, H * fc.W32, C1, C2, G, kind)
        w = fc.conv_weights(Cin, Cout)
        if chain:
            ws = fc.gn_colsums(nc.gn_full(d), H // 16)
            coef, extra = fc.coef_from_colsums(ws, d), fc.chain_extra_dz(d)
            acc, A = fc.loader_reference(d, H, w, fc.exact_coef(d), act, extra, E=fc.E_DIRECT)
        else:
            coef = fc.exact_coef(d).astype(np.float32)
            acc, A = fc.loader_reference(d, H, w, coef, act, E=fc.E_DIRECT)
        _loader[key] = dict(d=d, w=w, coef=coef, acc=acc, A=A, H=H, rpg=H * fc.W32,
                            ops=fc.epilogue_operands(B * H * fc.W32, Cout, B))
    return _loader[key]


def loader_ratio(c, act, combo, mutation=None, ep_mutation=None, coef=None):
    con = fc.loader_replay(c["d"], c["H"], c["w"], c["coef"] if coef is None else coef, act, mutation)
    N = con.shape[1]
    out = fc.epilogue_replay(con, c["ops"], combo, c["rpg"], ep_mutation)
    ref, tol = fc.epilogue_ref(c["acc"], c["A"], fc.epilogue_terms(c["ops"], combo, c["rpg"], N), fc.E_DIRECT)
    return fc.worst(out, ref, tol)


def test_restated_f43_matrices_are_the_bilinear_identity():
    assert fc.f43_identity_error() < 1e-12


def test_loader_tail_instantiations_are_enumerated():
    """r1_body<32, false, NL, S2> shares wino1d_kernel's tail, compiled for ACT x RES x SCALED x STATS: the loader cases x both loader
    activations x the product with and without column sums reach all 4 x 16 = 64, the two production ones (none, residual, scaled, stats)
    and (none, no residual, unscaled, stats) of every loader form included."""
    seen = fc.tail_instantiations()
    assert len(seen) == 64
    for nl in fc.NL_ACTS:
        for two in (False, True):
            assert (nl, two, False, True, True, True) in seen and (nl, two, False, False, False, True) in seen


@pytest.mark.parametrize("shape", fc.LOADER_CASES + [s for s, _, _ in fc.KIND_CASES[-1:]], ids=str)
def test_generated_inputs(shape):
    """every |beta| >= 0.7, x1's channel means positive and x2's negative, every operand finite"""
    B, H, C1, C2, Cout = shape
    for kind in ("benign", "mean30", "constgroup"):
        d = fc.raw_inputs(B, H * fc.W32, C1, C2, (C1 + C2) // 4, kind)
        for t in (d["x"], d["x2"], d["gamma"], d["beta"], fc.conv_weights(C1 + C2, Cout), fc.exact_coef(d)):
            assert t is None or bool(np.isfinite(t).all())
        assert float(np.abs(d["beta"]).min()) >= 0.7
        assert float(d["x"].mean((0, 1)).min()) > 0.5
        assert d["x2"] is None or float(d["x2"].mean((0, 1)).max()) < -0.5
        if kind == "constgroup":
            assert float(nc.gn_full(d)[:, :, 4:8].var()) == 0.0 and float(np.abs(fc.exact_coef(d)[:, 4:8, 0]).max()) > 500


@pytest.mark.parametrize("act", fc.NL_ACTS)
@pytest.mark.parametrize("shape", fc.LOADER_CASES, ids=str)
def test_loader_replay_inside_the_bound(shape, act):
    c = loader_case(shape, act)
    combos = fc.combos() if shape == (3, 16, 16, 0, 64) else HOST_COMBOS         # the whole product on the smallest case
    worst = max(loader_ratio(c, act, combo) for combo in combos)
    note("REPLAY loader, " + ("two sources" if shape[3] else "one source"), worst)
    assert worst < 1.0


@pytest.mark.parametrize("act", fc.NL_ACTS)
@pytest.mark.parametrize("shape,kind,cpg", fc.KIND_CASES, ids=str)
def test_statistics_kinds_replay_inside_the_bound(shape, kind, cpg, act):
    c = loader_case(shape, act, kind, cpg)
    worst = max(loader_ratio(c, act, combo) for combo in [fc.BIAS_ONLY] + fc.PRODUCTION)
    note("REPLAY statistics kinds", worst)
    assert worst < 1.0


@pytest.mark.parametrize("shape,G,kind", fc.CHAIN_CASES, ids=str)
def test_chain_replay_inside_the_bound(shape, G, kind):
    """The producer's stored output stands in as a random fp32 tensor: column sums at nsplit = H / 16, the coefficients formed from them in
    fp64 and rounded once, the consumer's replay; against the EXACT GroupNorm and the bound that carries the coefficient term."""
    Cin = shape[2] + shape[3]
    c = loader_case(shape, "silu", kind, Cin // G, chain=True)
    worst = max(loader_ratio(c, "silu", combo) for combo in [fc.BIAS_ONLY] + fc.PRODUCTION)
    note("REPLAY chain", worst)
    assert worst < 1.0
    d, H, w = c["d"], c["H"], c["w"]
    z, n, _ = fc.normed64(d, fc.exact_coef(d), "silu")
    _, A, Dc = fc.conv_terms(n, 1.1 * fc.chain_extra_dz(d), w, H)
    print(f"\nCHAIN {shape} G={G} {kind}: coefficient term / (E A) = {float((Dc / (fc.E_W1D * A)).max()):.3g}")


def test_emulated_contraction_error():
    """max |err| / A of the emulated row-wise F(4, 3) on fp16 pairs against fp64, on this module's inputs: E_W1D covers 4 x that."""
    worst = {"loader": 0.0, "tail": 0.0}
    cases = [(s, a, "benign", 4) for s in fc.LOADER_CASES for a in fc.NL_ACTS] + [(s, "silu", k, g) for s, k, g in fc.KIND_CASES]
    for shape, act, kind, cpg in cases:
        c = loader_case(shape, act, kind, cpg)
        _, n, _ = fc.normed64(c["d"], c["coef"], act)
        n32 = n.astype(np.float32)
        acc, A, _ = fc.conv_terms(n32.astype(np.float64), np.zeros_like(n), c["w"], c["H"])
        worst["loader"] = max(worst["loader"], float(((fc.wino1d_emulate(n32, c["w"], c["H"]).double() - acc).abs() / A).max()))
    for case in fc.TAIL_CASES:
        t = fc.tail_inputs(*case)
        acc, A = fc.tail_contraction(t)
        got = fc.wino1d_emulate(t["x"], t["w"], t["H"]).double().numpy().reshape(acc.shape)
        worst["tail"] = max(worst["tail"], float((np.abs(got - acc) / A).max()))
    print(f"\nEMUL loader inputs {worst['loader']:.3g}, tail-norm inputs {worst['tail']:.3g}; E_W1D = {fc.E_W1D:.3g}")
    measured = max(worst.values())
    assert 1e-8 < measured <= fc.E_EMULATED * 1.25, "the value the module docstring records (25 % for another CPU's summation order)"
    assert fc.E_W1D >= max(fc.E_F4, 4 * measured)


def test_coefficient_form_on_ill_conditioned_groups():
    """How far the fp32 coefficient pair alone moves the convolution's output from the exact GroupNorm, next to the isolated bound."""
    shape, got = (3, 32, 32, 0, 128), {}
    for kind in ("benign", "mean30", "constgroup"):
        c = loader_case(shape, "silu", kind)
        d, H, w = c["d"], c["H"], c["w"]
        ops = c["ops"]
        _, n32c, dn = fc.normed64(d, c["coef"], "silu")
        _, nex, _ = fc.normed64(d, fc.exact_coef(d), "silu")
        acc, A, D = fc.conv_terms(n32c, dn, w, H)
        accx, _, _ = fc.conv_terms(nex, dn, w, H)
        terms = fc.epilogue_terms(ops, fc.BIAS_ONLY, c["rpg"], 128)
        _, tol = fc.epilogue_ref(acc, A + D / fc.E_F4, terms, fc.E_F4)
        got[kind] = float(((acc - accx).abs() / tol).max())
        co = np.abs(c["coef"])
        print(f"\nCOEF {kind}: max |a| {co[..., 0].max():.4g} max |b| {co[..., 1].max():.4g}; exact GroupNorm against the fp32 coefficient "
              f"form / isolated tol = {got[kind]:.3g}")
    assert got["benign"] < got["mean30"] < got["constgroup"]


# ---------------------------------------------------------------------------------------------- mutations
MUT_SHAPES = [((3, 32, 32, 0, 128), "silu"), ((2, 32, 32, 48, 128), "silu"), ((3, 32, 16, 16, 64), "silu")]


@pytest.mark.parametrize("mutation", fc.LOADER_MUTATIONS)
def test_loader_mutations_leave_the_bound(mutation):
    worst = max(loader_ratio(loader_case(s, a), a, fc.BIAS_ONLY, mutation=mutation) for s, a in MUT_SHAPES)
    print(f"\nMUTATION loader {mutation}: err / tol = {worst:.3g}")
    assert worst >= 10.0


@pytest.mark.parametrize("mutation,combo", [("rowbias_wrong_image", fc.PRODUCTION[0]), ("scale_residual_only", fc.PRODUCTION[1]),
                                            ("residual_before_act", (True, False, "silu", "dense", 1.0, False))])
def test_epilogue_mutations_leave_the_bound(mutation, combo):
    worst = max(loader_ratio(loader_case(s, a), a, combo, ep_mutation=mutation) for s, a in MUT_SHAPES)
    print(f"\nMUTATION epilogue {mutation}: err / tol = {worst:.3g}")
    assert worst >= 10.0


def test_first_nsplit_slot_only_leaves_the_bound():
    worst = 0.0
    for shape, G, kind in fc.CHAIN_CASES[:2]:
        c = loader_case(shape, "silu", kind, (shape[2] + shape[3]) // G, chain=True)
        ws = fc.gn_colsums(nc.gn_full(c["d"]), c["H"] // 16)
        assert ws.shape[1] == 2
        worst = max(worst, loader_ratio(c, "silu", fc.BIAS_ONLY, coef=fc.coef_from_colsums(ws, c["d"], first_slot_only=True)))
    print(f"\nMUTATION first nsplit slot only: err / tol = {worst:.3g}")
    assert worst >= 10.0


# ---------------------------------------------------------------------------------------------- tail-norm form
@pytest.mark.parametrize("case", fc.TAIL_CASES, ids=str)
def test_tail_norm_replay_inside_the_bound(case):
    t = fc.tail_inputs(*case)
    acc, A = fc.tail_contraction(t)
    worst = 0.0
    for hb in (False, True):
        for hrb in (False, True):
            for act in fc.TAIL_ACTS:
                ref, tol = fc.tail_ref(t, acc, A, hb, hrb, act, E=fc.E_DIRECT)
                worst = max(worst, fc.worst(fc.tail_replay(t, hb, hrb, act), ref, tol))
    note("REPLAY tail norm", worst)
    assert worst < 1.0


@pytest.mark.parametrize("mutation", ["var_about_zero", "group_width_x2"])
def test_tail_norm_mutations_leave_the_bound(mutation):
    worst = 0.0
    for case in fc.TAIL_CASES[:5]:
        t = fc.tail_inputs(*case)
        acc, A = fc.tail_contraction(t)
        ref, tol = fc.tail_ref(t, acc, A, True, True, "silu", E=fc.E_DIRECT)
        worst = max(worst, fc.worst(fc.tail_replay(t, True, True, "silu", mutation), ref, tol))
    print(f"\nMUTATION tail norm {mutation}: err / tol = {worst:.3g}")
    assert worst >= 10.0


# ---------------------------------------------------------------------------------------------- FIR forms
def fir_case(mode, shape, kind):
    B, H, W, C = shape
    d = fc.fir_inputs(B, H, W, C, kind)
    return d, H, fc.exact_coef(d).astype(np.float32)


@pytest.mark.parametrize("kind", fc.FIR_KINDS)
@pytest.mark.parametrize("mode,shape", [(m, s) for m in fc.FIR_CASES for s in fc.FIR_CASES[m]], ids=str)
def test_fir_replay_inside_the_bound(mode, shape, kind):
    d, H, coef = fir_case(mode, shape, kind)
    worst = 0.0
    for act in fc.NL_ACTS:
        ref, tol = fc.fir_ref(d, H, coef, mode, act)
        up, down, p0, p1, _ = fc.FIR_MODES[mode]
        assert ref.shape[1:3] == (fc.fir_out_size(shape[1], up, down, p0, p1), fc.fir_out_size(shape[2], up, down, p0, p1))
        worst = max(worst, fc.worst(fc.fir_replay(d, H, coef, mode, act), ref, tol))
    note(f"REPLAY FIR {mode}", worst)
    assert worst < 1.0


@pytest.mark.parametrize("kind", fc.FIR_KINDS)
@pytest.mark.parametrize("mode", list(fc.FIR_CASES))
def test_fir_chain_replay_inside_the_bound(mode, kind):
    """[2, 32, 32, 64] with coefficients formed from column sums at nsplit = 2, against the exact GroupNorm and the chain's bound"""
    d, H, _ = fir_case(mode, (2, 32, 32, 64), kind)
    coef = fc.coef_from_colsums(fc.gn_colsums(d["x"], 2), d)
    worst = 0.0
    for act in fc.NL_ACTS:
        ref, tol = fc.fir_ref(d, H, fc.exact_coef(d), mode, act, fc.chain_extra_dz(d))
        worst = max(worst, fc.worst(fc.fir_replay(d, H, coef, mode, act), ref, tol))
    note("REPLAY FIR chain", worst)
    assert worst < 1.0


@pytest.mark.parametrize("mutation", fc.FIR_MUTATIONS)
@pytest.mark.parametrize("mode", list(fc.FIR_CASES))
def test_fir_mutations_leave_the_bound(mode, mutation):
    worst = 0.0
    for shape in fc.FIR_CASES[mode][:3]:
        d, H, coef = fir_case(mode, shape, "benign")
        ref, tol = fc.fir_ref(d, H, coef, mode, "silu")
        worst = max(worst, fc.worst(fc.fir_replay(d, H, coef, mode, "silu", mutation), ref, tol))
    print(f"\nMUTATION FIR {mode} {mutation}: err / tol = {worst:.3g}")
    assert worst >= 10.0


def test_fir_reference_is_the_oracles_resampling():
    """the numpy upfirdn of normfused_cases against the project's oracle (oracle/ops.py) on both modes, odd sizes included"""
    from oracle.ops import upfirdn2d_ref
    g = nc.rng(3)
    for mode, (up, down, p0, p1, gain) in fc.FIR_MODES.items():
        x = g.standard_normal((2, 6, 10, 4))
        k = fc.fir_taps(gain).astype(np.float64)
        want = upfirdn2d_ref(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(k), up, up, down, down, p0, p1, p0, p1).permute(0, 2, 3, 1)
        assert float(np.abs(fc.upfirdn(x, k, up, down, p0, p1) - want.numpy()).max()) < 1e-13
