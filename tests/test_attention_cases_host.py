"""The ground of tests/test_hip_attention_elementwise.py checked without a GPU (tests/attention_cases.py): the float32 replay of both
attention kernels stays inside the per-element bound on every case, ten deliberate errors of the replay leave it on named cases, the
constant E is four times what the replay's own contraction measures, the band cases can see a flushed or doubled subnormal
probability, and the chooser behind idiff_attention*_route names the form a launch takes and refuses what the launchers refuse."""
import functools

import pytest
import torch

import attention_cases as ac
from id_diff_amd import _lib


@functools.lru_cache(maxsize=None)
def built(key):
    """(case, fp64 outputs without bias, bound without the bias term) of a named case, computed once."""
    kind = key[0]
    if kind == "heads":
        case = ac.heads_case(ac.HEADS_SHAPES[key[1]], key[2])
    elif kind == "a256":
        case = ac.a256_case(key[1], key[2], key[3])
    elif kind == "band":
        case = ac.band_case(key[1])
    else:
        case = ac.a256_band_case(key[1])
    out, tol = ac.reference(case)
    return case, out, tol


def worst_ratio(case, out, tol, got):
    ref, t = ac.with_bias(case, out, tol)
    assert bool(torch.isfinite(got).all())
    return float(((got.double() - ref).abs() / t).max())


ALL_KEYS = ([("heads", i, prof) for i, prof in ac.grid_cases()] + [("band", T) for T in ac.BAND_T] + [("a256band", 128)]
            + [("a256", B, C, prof) for (B, C, prof) in ac.A256_CASES])


@pytest.mark.parametrize("key", ALL_KEYS, ids=lambda k: "-".join(str(x) for x in k))
def test_replay_stays_inside_the_bound(key):
    case, out, tol = built(key)
    r = worst_ratio(case, out, tol, ac.replay(case))
    print(f"{case.name} [{case.route}, grid {case.grid}]: replay max err / tol {r:.3f}")
    assert r < 1.0


def test_every_form_and_grid_residue_has_cases():
    cases = [ac.heads_case(ac.HEADS_SHAPES[i], "uniform") for i in range(len(ac.HEADS_SHAPES))]
    assert {c.route for c in cases} == {f"heads<{D},{NW}>" for D in (32, 64, 128) for NW in (4, 8)}
    assert {c.T for c in cases} == {64, 128, 192, 256} and {c.H for c in cases} == {1, 2, 3}
    assert {c.grid % 8 for c in cases} == set(range(1, 8)) and min(c.grid for c in cases) < 8 < max(c.grid for c in cases)
    assert any(c.H == 3 and c.D == 32 for c in cases)
    for prof in ac.HEADS_PROFILES:                  # every profile meets every form
        assert {ac.heads_case(ac.HEADS_SHAPES[i], "uniform").route for i, p in ac.grid_cases() if p == prof} == {c.route for c in cases}, prof
    assert {(B, C) for B, C, _ in ac.A256_CASES} == {(1, 128), (3, 128), (1, 256), (3, 256)}


def test_planted_profiles_are_what_they_claim():
    """Conditions on the INPUTS, from the fp64 logits: the edges of the streaming recurrence are really reached."""
    def logits(case):
        qk = case.qk.double().reshape(case.B, case.T, 2, case.H, case.D)
        return (qk[0, :, 0, 0] @ qk[0, :, 1, 0].T) * case.scale
    shape = (2, 192, 2, 64)
    idx = ac.HEADS_SHAPES.index(shape)
    x = logits(built(("heads", idx, "uniform"))[0])
    assert float(x.abs().max()) == 0.0
    cm = logits(ac.heads_case(shape, "ascending")).reshape(192, 3, 64).max(dim=2).values
    assert bool((cm[:, 1:] > cm[:, :-1] + 4).all())                                     # the maximum moves in every chunk
    x = logits(ac.heads_case(shape, "descending"))
    assert bool((x[:, :64].max(dim=1).values > x[:, 64:].max(dim=1).values + 1).all())  # and never after chunk 0
    x = logits(ac.heads_case(shape, "jump"))
    top = x.topk(2, dim=1)
    assert bool((top.indices[:, 0] == 192 - 3).all()) and float((top.values[:, 0] - top.values[:, 1]).min()) > 200
    x = logits(ac.heads_case(shape, "onehot"))
    top = x.topk(2, dim=1)
    assert torch.equal(top.indices[:, 0], ac.onehot_permutation(192)) and float((top.values[:, 0] - top.values[:, 1]).min()) > 100
    x = logits(ac.band_case(2048))
    assert bool((x[:, 0:1] - x[:, 1:] > 16.5).all()) and bool((x[:, 0:1] - x[:, 1:] < 19.5).all())
    p = torch.exp(x[:, 1:] - x[:, 0:1]) * 1024                                          # p 2^10 relative to the leading key: fp16 subnormal
    assert float(p.max()) < 2.0 ** -14 and float(p.min()) > 2.0 ** -24


# mutation -> the named cases on which it must leave the bound
MUTANTS = [
    ("drop_lo_hi", ("heads", 1, "random1")), ("drop_lo_hi", ("a256", 1, 128, "random1")),
    ("drop_hi_lo", ("heads", 1, "random1")), ("drop_hi_lo", ("a256", 1, 128, "random1")),
    ("flush_hi", ("band", 2048)), ("flush_hi", ("band", 4096)), ("flush_hi", ("a256", 1, 128, "small_v")),
    ("lo_eq_hi", ("band", 2048)), ("lo_eq_hi", ("band", 4096)), ("lo_eq_hi", ("heads", 4, "small_v")), ("lo_eq_hi", ("heads", 4, "small_qk")),
    ("lo_eq_hi", ("a256", 1, 128, "small_v")), ("lo_eq_hi", ("a256", 1, 128, "small_qk")),
    ("no_alpha_l", ("heads", 5, "ascending")), ("no_alpha_l", ("heads", 5, "jump")),
    ("no_alpha_o", ("heads", 5, "ascending")), ("no_alpha_o", ("heads", 5, "jump")),
    ("v_slot_order", ("heads", 7, "onehot")), ("v_slot_order", ("a256", 1, 128, "onehot")),
    ("scale_C", ("heads", 1, "random1")),
    ("bias_head0", ("heads", 1, "random1")),
    ("no_lane_sum", ("heads", 9, "uniform")), ("no_lane_sum", ("a256", 1, 128, "uniform")),
]


def test_every_mutation_is_listed():
    assert {m for m, _ in MUTANTS} == set(ac.MUTATIONS)


@pytest.mark.parametrize("mut,key", MUTANTS, ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in v))
def test_mutation_leaves_the_bound(mut, key):
    case, out, tol = built(key)
    assert worst_ratio(case, out, tol, ac.replay(case)) < 1.0
    r = worst_ratio(case, out, tol, ac.replay(case, mut))
    print(f"{mut} on {case.name}: max err / tol {r:.1f}")
    assert r > 1.0


def test_E_is_four_times_the_replays_own_contraction_error():
    m = ac.measure_pair_contraction_error()
    worst = max(m.values())
    print("max |err| / A of the three-product pair contraction:", {k: f"{v:.2e}" for k, v in m.items()})
    assert 4 * worst <= ac.E_PAIR <= 8 * worst


@pytest.mark.parametrize("T", ac.BAND_T)
def test_band_case_can_see_a_flushed_or_doubled_subnormal(T):
    """A condition on the inputs: the mass of the band's keys is at least 10 times the row's tolerance / max |v|."""
    case, out, tol = built(("band", T))
    mass, t = ac.band_visibility(case, out, tol)
    print(f"{case.name}: band mass {mass:.2e}, tol / max|v| {t:.2e}, ratio {mass / t:.1f}")
    assert mass >= 10 * t


def test_the_condition_cannot_hold_at_256_keys():
    """attention256 has T fixed at 256: even with the band narrowed to [-17.5, -17] its 255 keys carry 8e-6 of the mass, under 10 times the
    tolerance; the small-channel cases are that kernel's subnormal tests (lo_eq_hi and flush_hi leave the bound there, above).  At 1024
    keys the streaming band [-19, -17] does not reach 10 either, hence T = 2048 and 4096."""
    case, out, tol = built(("a256band", 128))
    mass, t = ac.band_visibility(case, out, tol)
    print(f"{case.name}: band mass {mass:.2e}, tol / max|v| {t:.2e}, ratio {mass / t:.1f}")
    assert mass < 10 * t
    c = ac.band_case(1024)
    mass, t = ac.band_visibility(c, *ac.reference(c))
    print(f"{c.name}: ratio {mass / t:.1f}")
    assert mass < 10 * t


# ------------------------------------------------------------------------------------------------------------------ the route queries
Q, V, O, S1, S2, BV = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000     # fabricated, 16-byte aligned: nothing is dereferenced


def test_attention_heads_route_names_the_instantiation():
    for D in (32, 64, 128):
        for T, NW in ((64, 4), (128, 8), (192, 4), (256, 8), (4096, 8), (4032, 4)):
            assert _lib.attention_heads_route(Q, 2 * 2 * D, V, BV, S1, S2, O, 3, T, 2, D) == f"heads<{D},{NW}>"
    assert _lib.attention_heads_route(Q, 132, V, None, S1, S2, O, 1, 64, 2, 32) == "heads<32,4>"           # pitched, no bias
    assert _lib.attention_heads_route(0, 0, 0, 0, 0, 0, 0, 0, 64, 2, 32) == "none"                         # B == 0: nothing to launch
    for bad in (dict(T=96), dict(T=32), dict(T=4160), dict(D=48), dict(D=256), dict(H=0), dict(H=16, D=128), dict(B=-1), dict(B=1 << 20, H=2),
                dict(ld=127), dict(ld=130), dict(ld=124), dict(qk=Q + 4), dict(vt=V + 4), dict(out=O + 4), dict(bias=BV + 4),
                dict(qk=0), dict(vt=0), dict(out=0), dict(s_qk=0), dict(s_v=0)):
        a = dict(qk=Q, ld=128, vt=V, bias=BV, s_qk=S1, s_v=S2, out=O, B=2, T=256, H=2, D=32)
        a.update(bad)
        assert _lib.attention_heads_route(a["qk"], a["ld"], a["vt"], a["bias"], a["s_qk"], a["s_v"], a["out"], a["B"], a["T"], a["H"],
                                          a["D"]) is None, bad
        assert _lib.lib().idiff_last_error().decode().startswith("attention_heads: "), bad


def test_attention256_route_names_the_instantiation():
    assert _lib.attention256_route(Q, 256, V, BV, S1, S2, O, 3, 256, 128) == "attention256<128>"
    assert _lib.attention256_route(Q, 512 + 32, V, None, S1, S2, O, 1 << 20, 256, 256) == "attention256<256>"
    assert _lib.attention256_route(0, 0, 0, 0, 0, 0, 0, 0, 192, 96) == "none"
    for bad in (dict(T=192), dict(T=512), dict(C=96), dict(C=64), dict(C=512), dict(B=-1), dict(B=(1 << 20) + 1), dict(ld=255), dict(ld=258),
                dict(ld=252), dict(qk=Q + 4), dict(vt=V + 4), dict(out=O + 4), dict(bias=BV + 4), dict(qk=0), dict(vt=0), dict(out=0),
                dict(s_qk=0), dict(s_v=0)):
        a = dict(qk=Q, ld=256, vt=V, bias=BV, s_qk=S1, s_v=S2, out=O, B=2, T=256, C=128)
        a.update(bad)
        assert _lib.attention256_route(a["qk"], a["ld"], a["vt"], a["bias"], a["s_qk"], a["s_v"], a["out"], a["B"], a["T"], a["C"]) is None, bad
        assert _lib.lib().idiff_last_error().decode().startswith("attention256: "), bad
