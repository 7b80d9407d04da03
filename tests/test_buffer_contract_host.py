"""tests/buffer_contract.py checked against itself, on the host: numpy stand-in "launchers" over host arenas, a clean one that
must pass and one per planted defect (a word of scratch read before it is written, an output element or a count left unwritten, a
store one element past the scratch or before an output, a modified input, an accumulation that does not start from zero) that
must fail with a message naming the buffer and the element."""
import numpy as np
import pytest

import buffer_contract as bc

N = 37          # elements of x and y
CH = 5          # elements per chunk: the last chunk is short
NCH = 8         # chunks = doubles of scratch


def _problem(seed):
    r = np.random.default_rng(seed)
    return {"x": r.standard_normal(N), "w": r.standard_normal(2)}


OUTPUTS = {"y": bc.Buf("f64", N), "total": bc.Buf("f64", 1, align=8), "count": bc.Buf("i32", 1, align=8)}
SCRATCH = {"part": bc.Buf("f64", NCH, align=8)}


def standin(bufs, defect=None):
    """y = w[0] x + w[1]; total = the sum of y through one partial sum per chunk in the scratch; count = the number of positive
    y.  ``defect`` plants one fault."""
    x, w = bufs["x"].f64(), bufs["w"].f64()
    y, total, count, part = bufs["y"].f64(), bufs["total"].f64(), bufs["count"].i32(), bufs["part"].f64()
    if defect == "past_scratch":
        a = bufs["part"]
        a.raw[a.offset + 8 * NCH:a.offset + 8 * NCH + 8] = 0          # part[NCH]
    if defect == "before_output":
        a = bufs["y"]
        a.raw[a.offset - 8:a.offset] = 0                              # y[-1]
    if defect == "modifies_input":
        x[11] = x[11] + 1.0
    v = w[0] * x + w[1]
    for c in range(NCH):
        lo, hi = c * CH, min(N, c * CH + CH)
        if defect == "scratch_read_first" and hi - lo < CH:
            continue                                                  # the short last chunk's slot is summed below all the same
        part[c] = v[lo:hi].sum()
    if defect == "accumulates":
        total[0] += part.sum()                                        # into an output nobody cleared
    else:
        total[0] = part.sum()
    keep = float(y[23])
    y[:] = v
    if defect == "unwritten":
        y[23] = keep
    if defect != "count_unwritten":
        count[0] = int((v > 0).sum())
    return 0


clean = standin


def _unwritten(bufs):
    return standin(bufs, "unwritten")


def _run(launch, **kw):
    return bc.run_contract(launch, _problem(1), OUTPUTS, SCRATCH, _problem(2), what="stand-in", **kw)


def test_arena_layout():
    for align in (8, 16, 256):
        a = bc.Arena(24, align)
        assert a.ptr % align == 0 and a.payload.size == 24
        assert a.offset >= bc.GUARD_BYTES and a.raw.size - a.offset - 24 >= bc.GUARD_BYTES
        assert a.intact() and a.damage() == ""
        a.fill(0xFF)
        assert a.intact() and np.isnan(a.f64()).all() and (a.i32() == -1).all() and (a.i64() == -1).all() and np.isnan(a.f32()).all()
        a.raw[a.offset + 24] = 0
        assert not a.intact() and "AFTER" in a.damage() and "byte 24" in a.damage()
    a = bc.Arena(0, 16)
    assert a.intact() and a.f64().size == 0


def test_clean_stand_in_passes():
    res = _run(clean)
    p = _problem(1)
    want = p["w"][0] * p["x"] + p["w"][1]
    assert (res.outputs["y"] == want).all() and abs(res.outputs["total"][0] - want.sum()) < 1e-12
    assert res.outputs["count"][0] == int((want > 0).sum())


def test_documented_unwritten_element_is_masked_and_must_keep_its_fill():
    _run(_unwritten, unwritten={"y": [23]})
    with pytest.raises(bc.ContractError, match=r"output 'y' element 22 is documented as not written but changed"):
        _run(clean, unwritten={"y": [22]})


@pytest.mark.parametrize("launch, pattern", [
    (lambda b: clean(b, "scratch_read_first"), r"output 'total' element 0 differs .* depends on what the outputs or the scratch held"),
    (_unwritten, r"output 'y' element 23 differs"),
    (lambda b: clean(b, "count_unwritten"), r"output 'count' element 0 differs .* never written"),
    (lambda b: clean(b, "past_scratch"), r"scratch 'part' was written outside its 64 bytes: .* AFTER the payload changed, the first at byte 64"),
    (lambda b: clean(b, "before_output"), r"output 'y' was written outside its 296 bytes: .* BEFORE the payload changed, the nearest 1 byte"),
    (lambda b: clean(b, "modifies_input"), r"read-only input 'x' was modified: element 11"),
    (lambda b: clean(b, "accumulates"), r"output 'total' element 0 differs .* accumulation that does not start from zero"),
], ids=["scratch_read_before_written", "output_element_unwritten", "count_unwritten", "one_past_scratch", "one_before_output",
        "input_modified", "accumulation_not_from_zero"])
def test_planted_defect_is_caught_and_named(launch, pattern):
    with pytest.raises(bc.ContractError, match=pattern):
        _run(launch)


def test_unwritten_element_is_told_from_a_dependence():
    """The element left out holds 0x00 after the first run and 0xFF after the third: the message says so."""
    with pytest.raises(bc.ContractError) as e:
        bc.run_contract(_unwritten, _problem(1), OUTPUTS, SCRATCH, _problem(1), what="stand-in")
    assert "never written" in str(e.value) and "'y' element 23" in str(e.value)


def test_return_code_and_zero_fill_only():
    with pytest.raises(bc.ContractError, match="return code 1001"):
        _run(lambda b: 1001)
    res = bc.run_zero_fill_only(clean, _problem(1), OUTPUTS, SCRATCH, what="stand-in")
    assert res.outputs["count"][0] == int((res.outputs["y"] > 0).sum())
    with pytest.raises(bc.ContractError, match="'part' was written outside"):
        bc.run_zero_fill_only(lambda b: clean(b, "past_scratch"), _problem(1), OUTPUTS, SCRATCH, what="stand-in")


def test_in_place_operand_and_documented_scratch():
    """An operand updated in place is reloaded before every run; a documented part of the scratch is compared like an output."""
    g0 = np.arange(6, dtype=np.float64)

    def launch(bufs):
        g, ws = bufs["g"].f64(), bufs["ws"].f64()
        ws[0] = g.sum()
        g *= 2.0
        return 0

    res = bc.run_contract(launch, {}, {"g": bc.Buf("f64", 6, init=g0)}, {"ws": bc.Buf("f64", 3)}, {}, documented={"ws": [0]})
    assert (res.outputs["g"] == 2 * g0).all() and res.scratch["ws"][0] == g0.sum()

    def leaky(bufs):
        bufs["ws"].f64()[0] += 1.0
        return 0

    with pytest.raises(bc.ContractError, match=r"scratch \(documented part\) 'ws' element 0 differs"):
        bc.run_contract(leaky, {}, {"g": bc.Buf("f64", 6, init=g0)}, {"ws": bc.Buf("f64", 3)}, {}, documented={"ws": [0]})


def test_torch_buffers_take_the_path_the_gpu_cases_take():
    """device="cpu": torch uint8 buffers and typed torch views, as on the GPU (where a copy back is a copy by itself)."""
    def launch(bufs, accumulate):
        x, y = bufs["x"].f64(), bufs["y"].f64()
        if accumulate:
            y += 2.0 * x
        else:
            y[:] = 2.0 * x
        return 0

    x = {"x": np.arange(5.0)}
    res = bc.run_contract(lambda b: launch(b, False), x, {"y": bc.Buf("f64", 5)}, {}, {"x": np.arange(5.0) + 1}, device="cpu")
    assert (res.outputs["y"] == 2.0 * x["x"]).all()
    with pytest.raises(bc.ContractError, match=r"output 'y' element 0 differs"):
        bc.run_contract(lambda b: launch(b, True), x, {"y": bc.Buf("f64", 5)}, {}, {"x": np.arange(5.0) + 1}, device="cpu")
