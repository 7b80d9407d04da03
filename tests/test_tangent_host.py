"""Host-side logic of the tangent-space basis (no GPU): the C ABI lists the entry points, the width of a point's basis is decided
from its spectrum on the host, and the one-rank restriction is enforced before anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import id_diff_amd
from id_diff_amd import _lib, dim_reduction, parallel, plot_utils
from id_diff_amd.configs.utils import read_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("idiff_sym_lowvecs_scratch_doubles", "idiff_sym_lowvecs_f64")


def test_entry_points_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "idiff_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/idiff_hip.h"
    assert _lib._SIGNATURES["idiff_sym_lowvecs_scratch_doubles"] == (ctypes.c_int64, [ctypes.c_int] * 2)
    res, args = _lib._SIGNATURES["idiff_sym_lowvecs_f64"]
    assert res is ctypes.c_int and len(args) == 8 and args[1] is ctypes.c_int and args[2] is ctypes.c_int
    if not os.path.exists(_lib.library_path()):
        _lib.build()
    for name in NAMES:
        assert hasattr(_lib.lib(), name)


def test_scratch_size_and_refusals_need_no_device():
    """Both entry points turn bad arguments away in host code, in front of the first HIP call (fabricated addresses)."""
    lib = _lib.lib()
    D, k = 300, 7
    chunks = -(-D // 256)
    assert lib.idiff_sym_lowvecs_scratch_doubles(D, k) >= D * D + 2 * D * k + chunks * k * k + 2 * k * k
    for bad_D, bad_k in [(300, 0), (300, -3), (300, 129), (128, 128), (5, 9)]:
        assert lib.idiff_sym_lowvecs_scratch_doubles(bad_D, bad_k) == 0
        assert lib.idiff_sym_lowvecs_f64(0x10000, bad_D, bad_k, 0x20000, 0x30000, 0x40000, 0x50000, None) != 0
        assert "sym_lowvecs" in lib.idiff_last_error().decode()
    for hole in range(5):
        ptrs = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000]
        ptrs[hole] = 0
        assert lib.idiff_sym_lowvecs_f64(ptrs[0], D, k, ptrs[1], ptrs[2], ptrs[3], ptrs[4], None) != 0
        assert lib.idiff_last_error().decode() == "sym_lowvecs: null pointer"


def _spectrum_with_gap(n, d, high=5.0, low=1e-3):
    """n singular values, descending, whose one large gap sits before the last d of them."""
    return np.concatenate([np.linspace(2 * high, high, n - d), np.linspace(2 * low, low, d)]).tolist()


@pytest.mark.parametrize("n,d", [(100, 10), (1024, 1), (1024, 128), (40, 37)])
def test_width_is_the_id_where_a_basis_is_served(n, d):
    sv = _spectrum_with_gap(n, d)
    assert plot_utils.estimate_dim(sv) == d                  # the hand-made spectrum says what it was made to say
    assert dim_reduction.tangent_width(sv, n) == (d, d)


def test_width_is_none_outside_what_is_served():
    assert _lib.TANGENT_MAX == 128
    sv = _spectrum_with_gap(1024, 129)
    assert dim_reduction.tangent_width(sv, 1024) == (129, None)                # above the cap
    assert dim_reduction.tangent_width(sv, 1024, cap=200) == (129, 129)
    assert dim_reduction.tangent_width(_spectrum_with_gap(1024, 500), 1024) == (500, None)
    assert dim_reduction.tangent_width([3.0, 1.0], 100) == (-1, None)          # fewer than three singular values: no ID, no basis
    sv = _spectrum_with_gap(30, 12)
    assert dim_reduction.tangent_width(sv, 12) == (12, None)                   # a basis must be narrower than the space


def _ksphere_config(tmp_path):
    cfg = read_config('configs/dimension_estimation/paper/euclidean_data/ksphere/10dim.py')
    cfg.model.name = 'ksphere_exact'
    cfg.data.data_samples = 2000
    cfg.device = 'cuda'
    cfg.logging.log_path = str(tmp_path)
    return cfg


def _no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the driver went on to set up the model")
    monkeypatch.setattr(dim_reduction, "setup_model", touched)
    monkeypatch.setattr(dim_reduction, "create_lightning_datamodule", touched)


def test_two_ranks_are_refused_before_any_device_work(tmp_path, monkeypatch):
    _no_device(monkeypatch)
    monkeypatch.setattr(parallel, "rank_world", lambda: (1, 2))
    cfg = _ksphere_config(tmp_path)
    with pytest.raises(NotImplementedError, match="variable-width bases"):
        dim_reduction.get_manifold_dimension(cfg, return_svd=True, return_tangent=True)
    cfg.dim_estimation.save_tangent = True
    with pytest.raises(NotImplementedError, match="world size 2"):
        dim_reduction.get_manifold_dimension(cfg, name="x")
    assert not os.listdir(tmp_path)                    # refused before the output directory was made


def test_row_sharding_is_refused_on_one_rank_too(tmp_path, monkeypatch):
    _no_device(monkeypatch)
    cfg = _ksphere_config(tmp_path)
    cfg.dim_estimation.shard = 'rows'
    with pytest.raises(NotImplementedError, match="shard = 'rows'"):
        dim_reduction.get_manifold_dimension(cfg, return_svd=True, return_tangent=True)


def test_tangent_without_svd_is_a_usage_error(tmp_path, monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="return_svd"):
        dim_reduction.get_manifold_dimension(_ksphere_config(tmp_path), return_tangent=True)
