"""Host-side logic of the intrinsic-dimension driver (no GPU): what `get_manifold_dimension` hands back or writes for each
combination of its flags, how points are grouped into launches, and how many singular values a point keeps."""
import itertools
import os
import pickle
import types

import pytest
import torch

import id_diff_amd
from id_diff_amd import dim_reduction
from id_diff_amd.configs.config_dict import ConfigDict
from id_diff_amd.configs.utils import read_config


# ------------------------------------------------------------------------------------------ the exit, on an empty point list
def _empty_run(tmp_path, monkeypatch, **dim_estimation):
    """A config with num_datapoints = 1 (the reference's loop body never runs) over a stubbed model set-up: no device work."""
    cfg = read_config('configs/dimension_estimation/paper/euclidean_data/ksphere/10dim.py')
    cfg.logging.log_path = str(tmp_path)
    cfg.dim_estimation = ConfigDict(dict(num_datapoints=1, **dim_estimation))
    data = types.SimpleNamespace(train_dataloader=lambda: [])
    module = types.SimpleNamespace(sde=None, sampling_eps=1e-5)
    monkeypatch.setattr(dim_reduction, "setup_model", lambda config: (data, module, None, torch.device("cpu")))
    return cfg


@pytest.mark.parametrize("return_dims,return_tangent", itertools.product((False, True), repeat=2))
def test_empty_point_list_returns_what_a_non_empty_call_returns(tmp_path, monkeypatch, return_dims, return_tangent):
    cfg = _empty_run(tmp_path, monkeypatch)
    got = dim_reduction.get_manifold_dimension(cfg, return_svd=True, return_dims=return_dims, return_tangent=return_tangent)
    info = {'singular_values': []}
    want = {(False, False): info, (True, False): (info, []), (False, True): (info, []), (True, True): (info, [], [])}
    assert got == want[return_dims, return_tangent]
    assert isinstance(got, tuple) == (return_dims or return_tangent)
    assert not os.listdir(tmp_path)                              # return_svd writes nothing


@pytest.mark.parametrize("save_tangent", [False, True])
def test_empty_point_list_writes_the_pickles(tmp_path, monkeypatch, save_tangent):
    cfg = _empty_run(tmp_path, monkeypatch, save_tangent=save_tangent)
    assert dim_reduction.get_manifold_dimension(cfg, name="empty") is None
    folder = os.path.join(str(tmp_path), cfg.logging.log_name, 'svd')
    assert sorted(os.listdir(folder)) == ["empty.pkl"] + (["empty_tangent.pkl"] if save_tangent else [])
    with open(os.path.join(folder, "empty.pkl"), "rb") as f:
        assert pickle.load(f) == {'singular_values': []}
    if save_tangent:
        with open(os.path.join(folder, "empty_tangent.pkl"), "rb") as f:
            assert pickle.load(f) == {'tangent': [], 'dims': []}


# ------------------------------------------------------------------------------------------ the grouping rule
def _groups(points, ids, **dim_estimation):
    cfg = ConfigDict(dict(dim_estimation=ConfigDict(dim_estimation)))
    return dim_reduction._launch_groups(cfg, points, ids)


def test_small_points_of_one_batch_size_share_launches():
    points = [(torch.zeros(10), 5)] * 9
    ids = [0, 2, 3, 4, 5, 7, 8]                                  # a rank's share: any 7 ids
    assert _groups(points, ids, points_per_launch=3) == (True, [[0, 2, 3], [4, 5, 7], [8]])
    assert _groups(points, ids, points_per_launch=1) == (True, [[p] for p in ids])     # still the batched route
    assert _groups(points, ids, points_per_launch=0) == (True, [[p] for p in ids])
    assert _groups(points, [], points_per_launch=3) == (False, [])                     # a rank without points


def test_large_points_and_mixed_batch_sizes_go_one_by_one():
    ids = list(range(7))
    large = [(torch.zeros(4097), 5)] * 7
    assert _groups(large, ids, points_per_launch=3) == (False, [[p] for p in ids])
    assert _groups([(torch.zeros(4096), 5)] * 7, ids, points_per_launch=3)[0] is True  # the threshold itself is small
    mixed = [(torch.zeros(10), 5)] * 6 + [(torch.zeros(10), 4)]                        # a short last loader batch
    assert _groups(mixed, ids, points_per_launch=3) == (False, [[p] for p in ids])
    assert _groups(mixed, ids[:6], points_per_launch=3) == (True, [[0, 1, 2], [3, 4, 5]])   # decided on the ids given


def test_default_group_size_is_131072_rows_capped_by_the_ids():
    rows = dim_reduction.batching((100,), 500)[2]
    assert rows == 1501 and 131072 // rows == 87
    points = [(torch.zeros(100), 500)] * 200
    assert [len(g) for g in _groups(points, list(range(200)))[1]] == [87, 87, 26]
    assert [len(g) for g in _groups(points, list(range(40)))[1]] == [40]
    # more rows in a point than in a launch: one point per launch, by max(1, ...)
    rows = dim_reduction.batching((4096,), 140000)[2]
    assert rows > 131072
    assert _groups([(torch.zeros(4096), 140000)] * 3, [0, 1, 2]) == (True, [[0], [1], [2]])


# ------------------------------------------------------------------------------------------ singular values kept per point
@pytest.mark.parametrize("shape,batchsize,count", [((100,), 500, 100), ((3, 32, 32), 128, 3072), ((3, 64, 64), 128, 12288)])
def test_singular_value_count_on_the_baseline_shapes(shape, batchsize, count):
    x = torch.zeros(shape)
    assert dim_reduction._sv_count(x.shape, batchsize) == min(dim_reduction.batching(shape, batchsize)[2], x.numel()) == count


def test_singular_value_count_of_a_short_loader_batch():
    # torch.linalg.svd gives min(M, D) values: a loader batch of 2 leaves a 100-vector M = 3 * 2 + 1 = 7 rows for D = 100 columns
    assert dim_reduction.batching((100,), 2)[2] == 7 and dim_reduction._sv_count((100,), 2) == 7
