"""CPU-side checks of the C-ABI boundary: the library builds, loads and exports every declared symbol."""
import ctypes
import os
import re

import pytest

import id_diff_amd
from id_diff_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def library():
    if not os.path.exists(_lib.library_path()):
        _lib.build()
    return ctypes.CDLL(_lib.library_path())


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "idiff_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(idiff_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported(library):
    names = declared_symbols()
    assert len(names) >= 20
    for name in names:
        assert hasattr(library, name), f"{name} declared in include/idiff_hip.h but not exported"


def test_python_binding_covers_the_header():
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared_symbols()


def test_abi_version_and_loader(library):
    library.idiff_abi_version.restype = ctypes.c_int
    assert library.idiff_abi_version() == 1
    assert _lib.lib() is not None  # binds argtypes for every symbol


def test_epilogue_struct_layout_matches_header():
    # 8 + 8 + 8 + 4 + 4 + 8 + 8 + 4 (+4 pad) + 8 + 8
    assert ctypes.sizeof(_lib.Epilogue) == 72
    assert _lib.Epilogue.rowscale.offset == 56 and _lib.Epilogue.residual.offset == 32


def test_product_refuses_cpu_tensors():
    import torch
    from id_diff_amd import op
    with pytest.raises(RuntimeError, match="no CPU path"):
        op.upfirdn2d(torch.zeros(1, 1, 4, 4), torch.ones(2, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        op.fused_leaky_relu(torch.zeros(1, 2, 3), torch.zeros(2))


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "id-diff_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dirpath, f)


def test_no_kernel_spills_to_scratch_beyond_the_known_ones(library, tmp_path):
    """both GPU faults of the build were inside multi-workgroup kernels whose register allocation had spilled
    hundreds of bytes per lane to scratch; the rule since then is that no kernel of the library carries a scratch segment
    beyond a few dwords.  Read from the code objects."""
    import shutil, subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(f"{llvm}/llvm-objdump") and os.path.exists(f"{llvm}/llvm-readelf")):
        pytest.skip("no LLVM binutils")
    so = shutil.copy(_lib.library_path(), tmp_path / "lib.so")
    subprocess.run([f"{llvm}/llvm-objdump", "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    objs = [p for p in os.listdir(tmp_path) if "gfx950" in p]
    assert objs, "no gfx950 code object in the library"
    allowed = {}                            # no exceptions left since the factorisations keep two lanes per row
    seen = 0
    for o in objs:
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", str(tmp_path / o)], check=True, capture_output=True, text=True).stdout
        for name, size in re.findall(r"\.name:\s+(\S+)\s+\.private_segment_fixed_size:\s+(\d+)", notes):
            seen += 1
            limit = next((v for k, v in allowed.items() if k in name), 64)
            assert int(size) <= limit, f"{name}: {size} bytes of scratch per lane"
    assert seen >= 40


def test_thread_option_acts_on_the_calling_thread_only():
    """idiff_set_thread_option: the fail-soft re-solve selects a slower eigensolver form for ITS launch; another host thread's
    launches keep reading the process-wide value (checked through a host-only query that reads a switch)."""
    import threading
    ask = lambda: _lib.conv2d_winograd_ok(4, 16, 16, 64, 64)             # reads IDIFF_NO_WINOGRAD, no device call
    assert ask() is True
    seen = {}
    with _lib.thread_option("IDIFF_NO_WINOGRAD", 1):
        assert ask() is False
        t = threading.Thread(target=lambda: seen.setdefault("other", ask()))
        t.start(); t.join()
    assert seen["other"] is True and ask() is True
    with pytest.raises(KeyError):
        with _lib.thread_option("IDIFF_NO_SUCH_SWITCH", 1):
            pass


def test_diagnostic_builds_cannot_reach_the_production_path(library):
    """probe scripts used to rebuild libidiff_hip.so in place with timing-only kernels.  Now a build with extra flags must
    name a variant (its own file), the product library reports no variant flags, and no probe script patches or rewrites build.sh."""
    import subprocess
    library.idiff_variant_flags.restype = ctypes.c_char_p
    assert library.idiff_variant_flags() == b""
    build_sh = os.path.join(ROOT, "id-diff_amd", "csrc", "build.sh")
    out = subprocess.run(["bash", build_sh], env=dict(os.environ, IDIFF_VARIANT_FLAGS="-DIDIFF_W43H_DIAG_NO_U", IDIFF_VARIANT=""),
                         capture_output=True, text=True)
    assert out.returncode == 4 and "must name its own output file" in out.stderr          # refused before anything is compiled
    out = subprocess.run(["bash", build_sh], env=dict(os.environ, IDIFF_VARIANT="../x"), capture_output=True, text=True)
    assert out.returncode == 4
    scripts = os.path.join(ROOT, "scripts")
    for name in os.listdir(scripts):
        if name.endswith(".py") and name != "_variant.py":
            text = open(os.path.join(scripts, name)).read()
            assert "build.sh" not in text or "_variant" in text, f"scripts/{name} drives build.sh itself"
            assert "IDIFF_SCRATCH_LIMIT" not in text, f"scripts/{name} lifts the scratch limit of a build it does not name"


# ---- what the Winograd launchers refuse before any device call (csrc/wino_host.h and the four files in front of it)
_X, _U, _OUT, _RES, _ROWB, _GAMMA, _BETA = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000   # fabricated, 16-byte aligned
_B, _H, _W, _CIN, _COUT = 2, 8, 8, 64, 64            # a geometry all five convolution entry points serve
_CONVS = {"winograd": "conv2d_winograd", "winograd43": "conv2d_winograd43", "winograd43h": "conv2d_winograd43h",
          "wino1d": "conv2d_wino1d", "wino1d_gn": "conv2d_wino1d"}     # entry -> the name its shared checks report
_PACKERS = ("winograd43h_pack", "wino1d_pack")


def _refusal_cases():
    """(id, symbol, arguments, epilogue fields or None).  Each call violates exactly one of the launcher's conditions, with one exception
    the arithmetic forces: a residual pitch above 0x7fffffff / 4 also puts the residual beyond one buffer descriptor for any H * W >= 16."""
    cases = []
    for entry in _CONVS:
        def conv(tag, x=_X, u=_U, out=_OUT, B=_B, H=_H, ep=None, entry=entry):
            args = [x, u, out, B, H, _W, _CIN, _COUT, ep]
            if entry == "wino1d_gn":
                args += [32, _GAMMA, _BETA, 1e-6, 1]
            cases.append((f"{entry}-{tag}", f"idiff_conv2d_{entry}_f32", args))
        conv("null_x", x=0); conv("null_u", u=0); conv("null_out", out=0)
        conv("misaligned_x", x=_X + 4); conv("misaligned_u", u=_U + 8); conv("misaligned_out", out=_OUT + 4)
        conv("geometry", H=7 if entry == "winograd" else 6)
        conv("zero_batch", B=0)
        # bias and the per-group bias are read 16 bytes at a time by every tail
        conv("misaligned_bias", ep=dict(bias=_ROWB + 4))
        conv("misaligned_rowbias", ep=dict(rowbias=_ROWB + 8, ld_rowbias=_COUT, rows_per_group=_H * _W))
        conv("rowbias_pitch_not_4", ep=dict(rowbias=_ROWB, ld_rowbias=_COUT + 2, rows_per_group=_H * _W))
        if entry == "wino1d_gn":          # a residual, or a row group that is not the image, breaks a second condition of the fused GroupNorm
            continue
        conv("misaligned_residual", ep=dict(residual=_RES + 4, ld_residual=_COUT))
        conv("residual_pitch_not_4", ep=dict(residual=_RES, ld_residual=_COUT + 2))
        conv("residual_pitch_below_cout", ep=dict(residual=_RES, ld_residual=_COUT - 4))
        conv("residual_pitch_above_int", ep=dict(residual=_RES, ld_residual=0x7fffffff // 4 + 1))
        if entry != "winograd":           # F(2x2) serves any row group and splits a batch beyond one descriptor
            conv("not_per_image", ep=dict(rowbias=_ROWB, ld_rowbias=_COUT, rows_per_group=_H * _W // 2))
            conv("residual_beyond_descriptor", ep=dict(residual=_RES, ld_residual=1 << 23))
    for name in _PACKERS:
        def pack(tag, wt=_X, u=_U, Cin=32, Cout=64, name=name):
            cases.append((f"{name}-{tag}", f"idiff_{name}_f32", [wt, u, Cin, Cout]))
        pack("cin_granule", Cin=24); pack("cout_granule", Cout=96)
        pack("null_wt", wt=0); pack("null_u", u=0); pack("misaligned_u", u=_U + 4)
    return cases


def _call_refusal(handle, symbol, args):
    """The call on the null stream; -> (return code, idiff_last_error() when refused)."""
    args = list(args)
    for i, a in enumerate(args):
        if isinstance(a, dict):
            args[i] = ctypes.byref(_lib.Epilogue(**dict(dict(rows_per_group=1, out_scale=1.0), **a)))
    rc = getattr(handle, symbol)(*args, None)
    return rc, (handle.idiff_last_error().decode() if rc else "")


# Return code and idiff_last_error() of every case, recorded from the library of the commit before the launchers' host code was merged.
# (The bias / rowbias cases at the end of the table came later, with the checks they pin.)
# conv2d_winograd reported a bad residual in two texts of its own; it now says what the other three entries say, and for its four residual
# cases the words its old text has in common with theirs are what is pinned (_UNIFIED; the old text stands above each).
_REFUSALS = {
    'winograd-null_x': (1001, 'conv2d_winograd: null pointer'),
    'winograd-null_u': (1001, 'conv2d_winograd: null pointer'),
    'winograd-null_out': (1001, 'conv2d_winograd: null pointer'),
    'winograd-misaligned_x': (1001, 'conv2d_winograd: x, u and out must be 16-byte aligned'),
    'winograd-misaligned_u': (1001, 'conv2d_winograd: x, u and out must be 16-byte aligned'),
    'winograd-misaligned_out': (1001, 'conv2d_winograd: x, u and out must be 16-byte aligned'),
    'winograd-geometry': (1001, 'conv2d_winograd: geometry B=2 H=7 W=8 Cin=64 Cout=64 not supported (ask idiff_conv2d_winograd_ok)'),
    'winograd-zero_batch': (0, ''),
    # was: conv2d_winograd: residual must be 16-byte aligned with a row pitch that is a multiple of 4
    'winograd-misaligned_residual': (1001, 'residual must be 16-byte aligned with a row pitch'),
    # was: conv2d_winograd: residual must be 16-byte aligned with a row pitch that is a multiple of 4
    'winograd-residual_pitch_not_4': (1001, 'residual must be 16-byte aligned with a row pitch'),
    # was: conv2d_winograd: ld_residual 60 is not a row pitch for 64 channels
    'winograd-residual_pitch_below_cout': (1001, 'row pitch'),
    # was: conv2d_winograd: ld_residual 536870912 is not a row pitch for 64 channels
    'winograd-residual_pitch_above_int': (1001, 'row pitch'),
    'winograd43-null_x': (1001, 'conv2d_winograd43: null pointer'),
    'winograd43-null_u': (1001, 'conv2d_winograd43: null pointer'),
    'winograd43-null_out': (1001, 'conv2d_winograd43: null pointer'),
    'winograd43-misaligned_x': (1001, 'conv2d_winograd43: x, u and out must be 16-byte aligned'),
    'winograd43-misaligned_u': (1001, 'conv2d_winograd43: x, u and out must be 16-byte aligned'),
    'winograd43-misaligned_out': (1001, 'conv2d_winograd43: x, u and out must be 16-byte aligned'),
    'winograd43-geometry': (1001, 'conv2d_winograd43: geometry B=2 H=6 W=8 Cin=64 Cout=64 not supported (ask idiff_conv2d_winograd43_ok)'),
    'winograd43-zero_batch': (0, ''),
    'winograd43-misaligned_residual': (1001, 'conv2d_winograd43: residual must be 16-byte aligned with a row pitch >= Cout that is a multiple of 4'),
    'winograd43-residual_pitch_not_4': (1001, 'conv2d_winograd43: residual must be 16-byte aligned with a row pitch >= Cout that is a multiple of 4'),
    'winograd43-residual_pitch_below_cout': (1001, 'conv2d_winograd43: residual must be 16-byte aligned with a row pitch >= Cout that is a multiple of 4'),
    'winograd43-residual_pitch_above_int': (1001, 'conv2d_winograd43: residual must be 16-byte aligned with a row pitch >= Cout that is a multiple of 4'),
    'winograd43-not_per_image': (1001, 'conv2d_winograd43: per-row-group bias / scale only per image (rows_per_group = H * W = 64, got 32)'),
    'winograd43-residual_beyond_descriptor': (1001, 'conv2d_winograd43: residual beyond one buffer descriptor'),
    'winograd43h-null_x': (1001, 'conv2d_winograd43h: null pointer'),
    'winograd43h-null_u': (1001, 'conv2d_winograd43h: null pointer'),
    'winograd43h-null_out': (1001, 'conv2d_winograd43h: null pointer'),
    'winograd43h-misaligned_x': (1001, 'conv2d_winograd43h: x, u and out must be 16-byte aligned'),
    'winograd43h-misaligned_u': (1001, 'conv2d_winograd43h: x, u and out must be 16-byte aligned'),
    'winograd43h-misaligned_out': (1001, 'conv2d_winograd43h: x, u and out must be 16-byte aligned'),
    'winograd43h-geometry': (1001, 'conv2d_winograd43h: geometry B=2 H=6 W=8 Cin=64 Cout=64 not supported (ask idiff_conv2d_winograd43h_ok)'),
    'winograd43h-zero_batch': (0, ''),
    'winograd43h-misaligned_residual': (1001, 'conv2d_winograd43h: residual must be 16-byte aligned with a row pitch >= Cout that is a multiple of 4'),
    'winograd43h-residual_pitch_not_4': (1001, 'conv2d_winograd43h: residual must be 16-byte aligned with a row pitch >= Cout that is a multiple of 4'),
    'winograd43h-residual_pitch_below_cout': (1001, 'conv2d_winograd43h: residual must be 16-byte aligned with a row pitch >= Cout that is a multiple of 4'),
    'winograd43h-residual_pitch_above_int': (1001, 'conv2d_winograd43h: residual must be 16-byte aligned with a row pitch >= Cout that is a multiple of 4'),
    'winograd43h-not_per_image': (1001, 'conv2d_winograd43h: per-row-group bias / scale only per image (rows_per_group = H * W = 64, got 32)'),
    'winograd43h-residual_beyond_descriptor': (1001, 'conv2d_winograd43h: residual beyond one buffer descriptor'),
    'wino1d-null_x': (1001, 'conv2d_wino1d: null pointer'),
    'wino1d-null_u': (1001, 'conv2d_wino1d: null pointer'),
    'wino1d-null_out': (1001, 'conv2d_wino1d: null pointer'),
    'wino1d-misaligned_x': (1001, 'conv2d_wino1d: x, u and out must be 16-byte aligned'),
    'wino1d-misaligned_u': (1001, 'conv2d_wino1d: x, u and out must be 16-byte aligned'),
    'wino1d-misaligned_out': (1001, 'conv2d_wino1d: x, u and out must be 16-byte aligned'),
    'wino1d-geometry': (1001, 'conv2d_wino1d: geometry B=2 H=6 W=8 Cin=64 Cout=64 not supported (ask idiff_conv2d_wino1d_ok)'),
    'wino1d-zero_batch': (0, ''),
    'wino1d-misaligned_residual': (1001, 'conv2d_wino1d: residual must be 16-byte aligned with a row pitch >= Cout that is a multiple of 4'),
    'wino1d-residual_pitch_not_4': (1001, 'conv2d_wino1d: residual must be 16-byte aligned with a row pitch >= Cout that is a multiple of 4'),
    'wino1d-residual_pitch_below_cout': (1001, 'conv2d_wino1d: residual must be 16-byte aligned with a row pitch >= Cout that is a multiple of 4'),
    'wino1d-residual_pitch_above_int': (1001, 'conv2d_wino1d: residual must be 16-byte aligned with a row pitch >= Cout that is a multiple of 4'),
    'wino1d-not_per_image': (1001, 'conv2d_wino1d: per-row-group bias / scale only per image (rows_per_group = H * W = 64, got 32)'),
    'wino1d-residual_beyond_descriptor': (1001, 'conv2d_wino1d: residual beyond one buffer descriptor'),
    'wino1d_gn-null_x': (1001, 'conv2d_wino1d: null pointer'),
    'wino1d_gn-null_u': (1001, 'conv2d_wino1d: null pointer'),
    'wino1d_gn-null_out': (1001, 'conv2d_wino1d: null pointer'),
    'wino1d_gn-misaligned_x': (1001, 'conv2d_wino1d: x, u and out must be 16-byte aligned'),
    'wino1d_gn-misaligned_u': (1001, 'conv2d_wino1d: x, u and out must be 16-byte aligned'),
    'wino1d_gn-misaligned_out': (1001, 'conv2d_wino1d: x, u and out must be 16-byte aligned'),
    'wino1d_gn-geometry': (1001, 'conv2d_wino1d: geometry B=2 H=6 W=8 Cin=64 Cout=64 not supported (ask idiff_conv2d_wino1d_ok)'),
    'wino1d_gn-zero_batch': (0, ''),
    'winograd43h_pack-cin_granule': (1001, 'winograd43h_pack: Cin must be a multiple of 16 and Cout of 64 (got 24, 64)'),
    'winograd43h_pack-cout_granule': (1001, 'winograd43h_pack: Cin must be a multiple of 16 and Cout of 64 (got 32, 96)'),
    'winograd43h_pack-null_wt': (1001, 'winograd43h_pack: null pointer'),
    'winograd43h_pack-null_u': (1001, 'winograd43h_pack: null pointer'),
    'winograd43h_pack-misaligned_u': (1001, 'winograd43h_pack: u must be 16-byte aligned'),
    'wino1d_pack-cin_granule': (1001, 'wino1d_pack: Cin must be a multiple of 16 and Cout of 64 (got 24, 64)'),
    'wino1d_pack-cout_granule': (1001, 'wino1d_pack: Cin must be a multiple of 16 and Cout of 64 (got 32, 96)'),
    'wino1d_pack-null_wt': (1001, 'wino1d_pack: null pointer'),
    'wino1d_pack-null_u': (1001, 'wino1d_pack: null pointer'),
    'wino1d_pack-misaligned_u': (1001, 'wino1d_pack: u must be 16-byte aligned'),
    # since the Winograd front end checks what its tails read 16 bytes at a time beside the residual
    'winograd-misaligned_bias': (1001, 'conv2d_winograd: bias must be 16-byte aligned'),
    'winograd-misaligned_rowbias': (1001, 'conv2d_winograd: rowbias must be 16-byte aligned with a row pitch that is a multiple of 4'),
    'winograd-rowbias_pitch_not_4': (1001, 'conv2d_winograd: rowbias must be 16-byte aligned with a row pitch that is a multiple of 4'),
    'winograd43-misaligned_bias': (1001, 'conv2d_winograd43: bias must be 16-byte aligned'),
    'winograd43-misaligned_rowbias': (1001, 'conv2d_winograd43: rowbias must be 16-byte aligned with a row pitch that is a multiple of 4'),
    'winograd43-rowbias_pitch_not_4': (1001, 'conv2d_winograd43: rowbias must be 16-byte aligned with a row pitch that is a multiple of 4'),
    'winograd43h-misaligned_bias': (1001, 'conv2d_winograd43h: bias must be 16-byte aligned'),
    'winograd43h-misaligned_rowbias': (1001, 'conv2d_winograd43h: rowbias must be 16-byte aligned with a row pitch that is a multiple of 4'),
    'winograd43h-rowbias_pitch_not_4': (1001, 'conv2d_winograd43h: rowbias must be 16-byte aligned with a row pitch that is a multiple of 4'),
    'wino1d-misaligned_bias': (1001, 'conv2d_wino1d: bias must be 16-byte aligned'),
    'wino1d-misaligned_rowbias': (1001, 'conv2d_wino1d: rowbias must be 16-byte aligned with a row pitch that is a multiple of 4'),
    'wino1d-rowbias_pitch_not_4': (1001, 'conv2d_wino1d: rowbias must be 16-byte aligned with a row pitch that is a multiple of 4'),
    'wino1d_gn-misaligned_bias': (1001, 'conv2d_wino1d: bias must be 16-byte aligned'),
    'wino1d_gn-misaligned_rowbias': (1001, 'conv2d_wino1d: rowbias must be 16-byte aligned with a row pitch that is a multiple of 4'),
    'wino1d_gn-rowbias_pitch_not_4': (1001, 'conv2d_wino1d: rowbias must be 16-byte aligned with a row pitch that is a multiple of 4'),
}
_UNIFIED = ("winograd-misaligned_residual", "winograd-residual_pitch_not_4", "winograd-residual_pitch_below_cout",
            "winograd-residual_pitch_above_int")


@pytest.mark.parametrize("case", _refusal_cases(), ids=lambda c: c[0])
def test_winograd_launchers_refuse_before_any_device_call(case):
    """No GPU needed: every call here is turned away by host code in front of the first HIP call (the addresses are fabricated: a
    launcher that let one through would fault, not pass)."""
    ident, symbol, args = case
    want_rc, want_text = _REFUSALS[ident]
    rc, text = _call_refusal(_lib.lib(), symbol, args)
    assert rc == want_rc
    if ident in _UNIFIED:
        assert text.startswith("conv2d_winograd: ") and want_text in text
    else:
        assert text == want_text


def test_refusal_table_is_complete():
    assert sorted(_REFUSALS) == sorted(c[0] for c in _refusal_cases())
    for ident, (rc, text) in _REFUSALS.items():
        assert (rc, text) == (0, "") if ident.endswith("zero_batch") else rc == 1001 and text


# ---- what the five contraction entry points of csrc/igemm.hip refuse before any device call
_A, _A2, _BT, _C, _WS, _AS, _STATS = 0x10000, 0x18000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000     # fabricated, 16-byte aligned


def _igemm_refusal_cases():
    """(id, symbol, arguments, switches).  One violated condition per call; `zero_*` are the calls with nothing to do."""
    cases = []

    def gemm(tag, A=_A, lda=None, Bt=_BT, ldb=None, C=_C, ldc=None, M=256, N=64, K=64, batch=1, ep=None, switches=()):
        lda, ldb, ldc = K if lda is None else lda, K if ldb is None else ldb, N if ldc is None else ldc
        cases.append((f"gemm-{tag}", "idiff_gemm_f32", [A, lda, M * lda, Bt, ldb, N * ldb, C, ldc, M * ldc, M, N, K, batch, ep], switches))

    def pairs(tag, A=_A, lda=None, Bt=_BT, ldb=None, ws=_WS, C=_C, ldc=None, M=32768, N=128, K=64, batch=1, ep=None):
        lda, ldb, ldc = K if lda is None else lda, K if ldb is None else ldb, N if ldc is None else ldc
        cases.append((f"pairs-{tag}", "idiff_gemm_pairs_f32",
                      [A, lda, M * lda, Bt, ldb, N * ldb, ws, 0, _AS, C, ldc, M * ldc, M, N, K, batch, ep], ()))

    def two(tag, pair=False, A2=_A2, lda=None, K1=64, ldb=None, ldc=None, M=None, N=None, K=128, ep=None, switches=()):
        M, N = M or (32768 if pair else 256), N or (128 if pair else 64)
        lda, ldb, ldc = max(K1, K - K1) if lda is None else lda, K if ldb is None else ldb, N if ldc is None else ldc
        if pair:
            cases.append((f"pairs_2src-{tag}", "idiff_gemm_pairs_2src_f32", [_A, A2, lda, K1, _AS, _BT, ldb, _WS, _C, ldc, M, N, K, ep], switches))
        else:
            cases.append((f"2src-{tag}", "idiff_gemm_2src_f32", [_A, A2, lda, K1, _BT, ldb, _C, ldc, M, N, K, ep], switches))

    def conv(tag, x=_A, wt=_BT, out=_C, B=2, H=8, W=8, Cin=32, Cout=64, k=3, stride=1, pad=1, ep=None):
        cases.append((f"conv-{tag}", "idiff_conv2d_nhwc_f32", [x, wt, out, B, H, W, Cin, Cout, k, k, stride, pad, pad, ep], ()))

    for f in (gemm, pairs):
        f("negative_m", M=-1); f("k_zero", K=0); f("negative_batch", batch=-1)
        f("null_a", A=0); f("null_bt", Bt=0); f("null_c", C=0)
        f("lda_below_k", lda=60); f("ldb_below_k", ldb=60); f("ldc_below_n", ldc=60)
        f("zero_m", M=0)
    gemm("batch_above_grid", batch=65536)
    gemm("colstats_beyond_4gib", M=1_200_000, K=1024, ep=dict(colstats=_STATS, rows_per_group=128))
    gemm("colstats_general_kernel", K=101, ep=dict(colstats=_STATS, rows_per_group=64))
    gemm("colstats_partial_tile", M=300, N=72, ep=dict(colstats=_STATS, rows_per_group=100))
    pairs("not_served", M=300)
    pairs("misaligned_a", A=_A + 4)
    pairs("pitch_not_4", lda=66)
    pairs("slice_beyond_4gib", lda=40000)
    pairs("colstats_batched", batch=2, ep=dict(colstats=_STATS, rows_per_group=128))
    pairs("null_w_scale", ws=0)
    for pair in (False, True):
        two("k1_zero", pair, K1=0, lda=128); two("k1_equals_k", pair, K1=128, lda=128); two("k1_not_32", pair, K1=48, lda=80)
        two("lda_below_k1", pair, K1=64, K=96, lda=48); two("lda_below_k_minus_k1", pair, K1=32, K=128, lda=64)
        two("misaligned_a2", pair, A2=_A2 + 8)
    two("no_pipe", switches=("IDIFF_NO_PIPE",))
    two("colstats_beyond_4gib", M=1_200_000, lda=1024, ep=dict(colstats=_STATS, rows_per_group=128))
    # both sources beyond one descriptor by their pitch, one row group of an odd number of rows: no row to cut at
    two("cut_inside_row_group", M=2049, lda=1 << 20, ep=dict(rowscale=_STATS, rows_per_group=2049))
    two("not_served", True, M=300)
    conv("bad_stride", stride=0); conv("negative_pad", pad=-1)
    conv("cin_not_4", Cin=30)
    conv("null_x", x=0); conv("null_wt", wt=0); conv("null_out", out=0)
    conv("misaligned_x", x=_A + 4); conv("misaligned_wt", wt=_BT + 8)
    conv("empty_output", H=1, W=1, pad=0)
    conv("rows_beyond_int32", B=40000, H=256, W=256, Cin=4, k=1, pad=0)
    conv("colstats_not_pipelined", Cin=8, ep=dict(colstats=_STATS, rows_per_group=64))
    conv("zero_batch", B=0)
    return cases


# Return code and idiff_last_error() of every case, recorded from the library of the commit before the five entry points got one front end.
# idiff_gemm_pairs_2src_f32 now reports an unserved shape and unfit operands in the words of idiff_gemm_pairs_f32; for those two cases the
# words both texts share are what is pinned (_IGEMM_UNIFIED; the old text stands above each).
_IGEMM_REFUSALS = {
    'gemm-negative_m': (1001, 'gemm: bad sizes M=-1 N=64 K=64 batch=1'),
    'gemm-k_zero': (1001, 'gemm: bad sizes M=256 N=64 K=0 batch=1'),
    'gemm-negative_batch': (1001, 'gemm: bad sizes M=256 N=64 K=64 batch=-1'),
    'gemm-null_a': (1001, 'gemm: null pointer'),
    'gemm-null_bt': (1001, 'gemm: null pointer'),
    'gemm-null_c': (1001, 'gemm: null pointer'),
    'gemm-lda_below_k': (1001, 'gemm: leading dimension smaller than the row length'),
    'gemm-ldb_below_k': (1001, 'gemm: leading dimension smaller than the row length'),
    'gemm-ldc_below_n': (1001, 'gemm: leading dimension smaller than the row length'),
    'gemm-zero_m': (0, ''),
    'pairs-negative_m': (1001, 'gemm_pairs: bad sizes M=-1 N=128 K=64 batch=1'),
    'pairs-k_zero': (1001, 'gemm_pairs: bad sizes M=32768 N=128 K=0 batch=1'),
    'pairs-negative_batch': (1001, 'gemm_pairs: bad sizes M=32768 N=128 K=64 batch=-1'),
    'pairs-null_a': (1001, 'gemm_pairs: null pointer'),
    'pairs-null_bt': (1001, 'gemm_pairs: null pointer'),
    'pairs-null_c': (1001, 'gemm_pairs: null pointer'),
    'pairs-lda_below_k': (1001, 'gemm_pairs: leading dimension smaller than the row length'),
    'pairs-ldb_below_k': (1001, 'gemm_pairs: leading dimension smaller than the row length'),
    'pairs-ldc_below_n': (1001, 'gemm_pairs: leading dimension smaller than the row length'),
    'pairs-zero_m': (0, ''),
    'gemm-batch_above_grid': (1001, 'gemm: batch 65536 exceeds grid.y'),
    'gemm-colstats_beyond_4gib': (1001, 'gemm: colstats is not available for operands beyond 4 GiB'),
    'gemm-colstats_general_kernel': (1001, 'gemm: colstats requested for a problem the pipelined kernel does not take (ask idiff_gemm_colstats_split first)'),
    'gemm-colstats_partial_tile': (1001, 'gemm: colstats with M = 300 rows in tiles of 64: no whole tiles (ask idiff_gemm_colstats_split first)'),
    'pairs-not_served': (1001, 'gemm_pairs: M=300 N=128 K=64 batch=1 not served (ask idiff_gemm_pairs_ok)'),
    'pairs-misaligned_a': (1001, 'gemm_pairs: operands must be 16-byte aligned with row pitches and batch strides that are multiples of 4, one batch slice inside 4 GiB'),
    'pairs-pitch_not_4': (1001, 'gemm_pairs: operands must be 16-byte aligned with row pitches and batch strides that are multiples of 4, one batch slice inside 4 GiB'),
    'pairs-slice_beyond_4gib': (1001, 'gemm_pairs: operands must be 16-byte aligned with row pitches and batch strides that are multiples of 4, one batch slice inside 4 GiB'),
    'pairs-colstats_batched': (1001, 'gemm_pairs: colstats only for unbatched problems'),
    'pairs-null_w_scale': (1001, 'gemm_pairs: null pointer'),
    '2src-k1_zero': (1001, 'gemm_2src: bad sizes M=256 N=64 K=128 K1=0'),
    '2src-k1_equals_k': (1001, 'gemm_2src: bad sizes M=256 N=64 K=128 K1=128'),
    '2src-k1_not_32': (1001, 'gemm_2src: the split column K1 = 48 must be a multiple of 32'),
    '2src-lda_below_k1': (1001, 'gemm_2src: leading dimension smaller than the row length'),
    '2src-lda_below_k_minus_k1': (1001, 'gemm_2src: leading dimension smaller than the row length'),
    '2src-misaligned_a2': (1001, 'gemm_2src: operands must be 16-byte aligned with K % 4 == 0 and lda % 4 == 0 (use two idiff_gemm_f32 calls)'),
    'pairs_2src-k1_zero': (1001, 'gemm_pairs_2src: bad sizes M=32768 N=128 K=128 K1=0'),
    'pairs_2src-k1_equals_k': (1001, 'gemm_pairs_2src: bad sizes M=32768 N=128 K=128 K1=128'),
    'pairs_2src-k1_not_32': (1001, 'gemm_pairs_2src: the split column K1 = 48 must be a multiple of 32'),
    'pairs_2src-lda_below_k1': (1001, 'gemm_pairs_2src: leading dimension smaller than the row length'),
    'pairs_2src-lda_below_k_minus_k1': (1001, 'gemm_pairs_2src: leading dimension smaller than the row length'),
    # was: gemm_pairs_2src: operands must be 16-byte aligned with row pitches that are multiples of 4 and lie inside 4 GiB
    'pairs_2src-misaligned_a2': (1001, 'operands must be 16-byte aligned with row pitches'),
    '2src-no_pipe': (1001, 'gemm_2src: operands must be 16-byte aligned with K % 4 == 0 and lda % 4 == 0 (use two idiff_gemm_f32 calls)'),
    '2src-colstats_beyond_4gib': (1001, 'gemm_2src: colstats is not available for operands beyond 4 GiB'),
    '2src-cut_inside_row_group': (1001, 'gemm_2src: cannot split 2049 rows inside an epilogue row group of 2049'),
    # was: gemm_pairs_2src: M=300 N=128 K=128 not served (ask idiff_gemm_pairs_ok)
    'pairs_2src-not_served': (1001, 'not served (ask idiff_gemm_pairs_ok)'),
    'conv-bad_stride': (1001, 'conv2d: bad geometry'),
    'conv-negative_pad': (1001, 'conv2d: bad geometry'),
    'conv-cin_not_4': (1001, 'conv2d: Cin must be a multiple of 4 (pad the channels), got 30'),
    'conv-null_x': (1001, 'conv2d: null pointer'),
    'conv-null_wt': (1001, 'conv2d: null pointer'),
    'conv-null_out': (1001, 'conv2d: null pointer'),
    'conv-misaligned_x': (1001, 'conv2d: x and wt must be 16-byte aligned'),
    'conv-misaligned_wt': (1001, 'conv2d: x and wt must be 16-byte aligned'),
    'conv-empty_output': (1001, 'conv2d: empty output'),
    'conv-rows_beyond_int32': (1001, 'conv2d: B*OH*OW overflows int32'),
    'conv-colstats_not_pipelined': (1001, 'conv2d: colstats requested for a problem the pipelined kernel does not take (ask idiff_conv2d_colstats_split first)'),
    'conv-zero_batch': (0, ''),
}
_IGEMM_UNIFIED = ("pairs_2src-misaligned_a2", "pairs_2src-not_served")


@pytest.mark.parametrize("case", _igemm_refusal_cases(), ids=lambda c: c[0])
def test_igemm_entry_points_refuse_before_any_device_call(case):
    """As the Winograd table above, for idiff_gemm_f32, idiff_gemm_pairs_f32, idiff_gemm_2src_f32, idiff_gemm_pairs_2src_f32 and
    idiff_conv2d_nhwc_f32: sizes, null pointers, pitches, alignment, operands beyond one buffer descriptor and column sums the
    pipelined kernel cannot give are turned away by the host front end."""
    import contextlib
    ident, symbol, args, switches = case
    want_rc, want_text = _IGEMM_REFUSALS[ident]
    with contextlib.ExitStack() as stack:
        for s in switches:
            stack.enter_context(_lib.thread_option(s, 1))
        rc, text = _call_refusal(_lib.lib(), symbol, args)
    assert rc == want_rc
    if ident in _IGEMM_UNIFIED:
        assert text.startswith(symbol[len("idiff_"):-len("_f32")] + ": ") and want_text in text
    else:
        assert text == want_text


def test_igemm_refusal_table_is_complete():
    assert sorted(_IGEMM_REFUSALS) == sorted(c[0] for c in _igemm_refusal_cases())
    for ident, (rc, text) in _IGEMM_REFUSALS.items():
        assert (rc, text) == (0, "") if ident.split("-")[1].startswith("zero_") else rc == 1001 and text
