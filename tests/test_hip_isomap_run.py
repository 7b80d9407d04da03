"""GPU: ``isomap.run(config, embed=True)`` and the ``--embed`` switch of the CLI through a stand-in DataModule: the files written with
labels, without labels, and when the eigenvector plan refuses the largest n_components.

The data: the first 200 points of the roll257 fixture as the train loader (batches of 64, connected at 8 neighbours: checked with
scikit-learn), the other 57 as the test loader; the two classes are the sign of scikit-learn's first Isomap coordinate of all 257
points, so a classifier on a faithful embedding separates them (scikit-learn's own pipeline scores 0.93-0.98 here; chance is 0.5).
"""
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

import id_diff_amd
from id_diff_amd import _lib, isomap
from id_diff_amd.lightning_data_modules import utils as data_utils

pytestmark = pytest.mark.gpu
N_TRAIN, NN, KS = 200, 8, [1, 2, 3, 11]


class Loaders:
    """What ``run`` asks of a DataModule; batches are (x, y) pairs, or bare tensors when ``labels`` is off."""

    def __init__(self, X, y, labels):
        self.X, self.y, self.labels = torch.from_numpy(X), torch.from_numpy(y), labels

    def setup(self):
        pass

    def _batches(self, lo, hi):
        for a in range(lo, hi, 64):
            b = min(a + 64, hi)
            yield [self.X[a:b].reshape(b - a, 3, 4), self.y[a:b]] if self.labels else self.X[a:b]      # shaped: run flattens

    def train_dataloader(self):
        return self._batches(0, N_TRAIN)

    def test_dataloader(self):
        return self._batches(N_TRAIN, len(self.X))


@pytest.fixture(scope="module")
def data(golden):
    X = golden("isomap.npz")["roll257_X"]
    y = (golden("isomap_embed.npz")["roll257_k3_emb"][:, 0] > 0).astype(np.int64)
    return X, y


def _patch(monkeypatch, data, labels):
    monkeypatch.setattr(data_utils, "create_lightning_datamodule", lambda config: Loaders(data[0], data[1], labels))


def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def test_run_with_labels_writes_embeddings_and_scores(monkeypatch, tmp_path, data):
    _patch(monkeypatch, data, labels=True)
    plain, out = str(tmp_path / "plain"), str(tmp_path / "embed")
    ks0, err0 = isomap.run(None, N=N_TRAIN, ks=KS, out_dir=plain, n_neighbors=NN)
    assert sorted(os.listdir(plain)) in (["reconstruction_error.pkl"], ["reconstruction_error.pkl", "reconstruction_error.png"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # nothing to warn about here
        ks1, err1 = isomap.run(None, N=N_TRAIN, ks=KS, out_dir=out, n_neighbors=NN, embed=True)
    assert (ks1, err1) == (ks0, err0) == (KS, _load(os.path.join(out, "reconstruction_error.pkl")))      # the curve is what it was
    emb, scores = _load(os.path.join(out, "embedding.pkl")), _load(os.path.join(out, "clf_scores.pkl"))
    assert sorted(emb) == [2, 3] and emb[2].shape == (N_TRAIN, 2) and emb[3].shape == (N_TRAIN, 3)
    # one fit at 11 components serves them all: its first 3 columns are the embedding a fit at 3 components returns; either basis
    # has a residual within 1e-9 lambda_1 sqrt(k), so they differ by at most twice 10 (1e-9 / g_min) max|Z| (test_hip_isomap_embed.py)
    direct = isomap.Isomap(NN, 3).fit(data[0][:N_TRAIN])
    lam = isomap.reconstruction_errors(data[0][:N_TRAIN], [3], n_neighbors=NN, return_eigenvalues=True)[1]
    gmin = float(np.min((lam[:3] - lam[1:4]) / lam[0]))
    Z = direct.embedding_.cpu().numpy()
    diff = np.abs(emb[3] - Z).max()
    print(f"g_min = {gmin:.3g}: |columns of the fit at 11 - fit at 3| / max|Z| = {diff / np.abs(Z).max():.3g}; scores {scores}")
    assert diff <= 2 * 10 * (1e-9 / gmin) * np.abs(Z).max()
    assert np.array_equal(emb[2], emb[3][:, :2])
    assert sorted(scores) == KS and all(isinstance(v, float) and 0.8 <= v <= 1.0 for v in scores.values())


def test_run_without_labels_warns_once_and_writes_no_scores(monkeypatch, tmp_path, data):
    _patch(monkeypatch, data, labels=False)
    out = str(tmp_path / "out")
    with pytest.warns(UserWarning, match="no classifier scores .the loaders yield no labels.") as seen:
        isomap.run(None, N=N_TRAIN, ks=KS, out_dir=out, n_neighbors=NN, embed=True)
    assert len([w for w in seen if "isomap" in str(w.message)]) == 1
    assert sorted(_load(os.path.join(out, "embedding.pkl"))) == [2, 3]
    assert not os.path.exists(os.path.join(out, "clf_scores.pkl"))


def test_a_refused_plan_costs_that_k_only(monkeypatch, tmp_path, data):
    """The plan of 11 components is made to fail the way a flat spectrum fails: one warning names 11, the rest is written."""
    _patch(monkeypatch, data, labels=True)
    real = _lib.topvecs_plan

    def plan(eigvals, k):
        if k >= 11:
            raise ValueError(f"topvecs_plan: lambda_{k} = 1.0 and lambda_{k + 17} = 1.0 are too close")
        return real(eigvals, k)
    monkeypatch.setattr(_lib, "topvecs_plan", plan)
    out = str(tmp_path / "out")
    with pytest.warns(UserWarning, match=r"no embedding for n_components \[11\]: topvecs_plan: lambda_11") as seen:
        isomap.run(None, N=N_TRAIN, ks=KS, out_dir=out, n_neighbors=NN, embed=True)
    assert len(seen) == 1
    assert sorted(_load(os.path.join(out, "clf_scores.pkl"))) == [1, 2, 3]
    assert sorted(_load(os.path.join(out, "embedding.pkl"))) == [2, 3]


def test_cli_embed_switch(monkeypatch, tmp_path, data, capsys):
    from id_diff_amd.configs import utils as config_utils
    _patch(monkeypatch, data, labels=True)
    monkeypatch.setattr(config_utils, "read_config", lambda path: None)
    monkeypatch.setattr(isomap, "DEFAULT_KS", [1, 2, 3])
    out = str(tmp_path / "cli")
    isomap.main(["--config", "unused.py", "--N", str(N_TRAIN), "--n_neighbors", str(NN), "--out_dir", out, "--embed"])
    assert "k = 3  reconstruction error:" in capsys.readouterr().out
    assert sorted(_load(os.path.join(out, "clf_scores.pkl"))) == [1, 2, 3] and sorted(_load(os.path.join(out, "embedding.pkl"))) == [2, 3]
