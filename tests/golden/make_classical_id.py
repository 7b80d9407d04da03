"""Generate tests/golden/classical_id.npz: the classical ID estimators of the reference, run on two small sets.

Run once, in the build container only (``/root/reference`` and sklearn are not on the GPU box)::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_classical_id.py

The reference's mle.py (Levina-Bickel on sklearn's ball tree) is imported read-only from /root/reference; sklearn's
``PCA(n_components='mle')`` gives the PPCA rank.  The two sets are rebuilt by the tests from this project's own
generators (``make_sets``) rather than stored (a 1 MiB limit per committed file); their sums and first rows are stored
to pin them.  Stored per set (prefix ``a::`` / ``b::``):
    dist, ind                the 20 neighbour columns after the self column of kneighbors(n_neighbors=21)
    sw5                      intrinsic_dim_sample_wise(X, k=5)
    si                       intrinsic_dim_scale_interval(X, 10, 20)
    boot_F, boot_T, Rs       bootstrap_intrinsic_dim_scale_interval(X, nb_iter=10, random_state=0, average=False / True)
    boot_idx, boot_off       the bootstrap subsets of that seed, concatenated, and their offsets
    ppca_n, ppca_ev, ppca_ll sklearn's n_components_, the whole explained_variance_ spectrum and _assess_dimension per rank
"""
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
NB_ITER = 10
SEED = 0


def make_sets():
    """Set A: k-sphere, k = 10 in R^100, N = 2000, noise 0.01 (KSphereDataset); set B: 600 smooth 16 x 16 images of an
    8-dimensional latent (SyntheticImages), D = 256.  Both fp32 [N, D] numpy."""
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import id_diff_amd  # noqa: F401
    from id_diff_amd.configs.config_dict import ConfigDict
    from id_diff_amd.lightning_data_modules.KSphereDataset import KSphereDataset
    from id_diff_amd.lightning_data_modules.SyntheticImages import smooth_decoder_images
    cfg = ConfigDict()
    cfg.data = ConfigDict(data_samples=2000, n_spheres=1, ambient_dim=100, manifold_dim=10, noise_std=0.01,
                          embedding_type='random_isometry')
    torch.manual_seed(0)
    a = KSphereDataset(cfg).data.float().numpy()
    b = smooth_decoder_images(600, [1, 16, 16], 8, 0).reshape(600, -1).numpy()
    return {"a": np.ascontiguousarray(a), "b": np.ascontiguousarray(b)}


def pin(X):
    """Sums and first rows that identify a set."""
    X64 = X.astype(np.float64)
    return np.array([X64.sum(), (X64 * X64).sum()]), X[:4].copy()


def main():
    import pandas as pd
    from sklearn.decomposition import PCA
    from sklearn.decomposition._pca import _assess_dimension, _infer_dimension
    from sklearn.neighbors import NearestNeighbors
    sys.path.insert(0, REF)
    import mle as ref_mle
    out = {}
    for name, X in make_sets().items():
        df = pd.DataFrame(X)
        dist, ind = NearestNeighbors(n_neighbors=21, n_jobs=1, algorithm='ball_tree').fit(X).kneighbors(X)
        assert np.all(dist[:, 0] == 0) and np.all(ind[:, 0] == np.arange(len(X)))
        out[f"{name}::sums"], out[f"{name}::head"] = pin(X)
        out[f"{name}::dist"] = dist[:, 1:]
        out[f"{name}::ind"] = ind[:, 1:].astype(np.int32)
        out[f"{name}::sw5"] = ref_mle.intrinsic_dim_sample_wise(df, k=5)
        out[f"{name}::si"] = np.array(ref_mle.intrinsic_dim_scale_interval(df, 10, 20))
        res_f, Rs = ref_mle.bootstrap_intrinsic_dim_scale_interval(df, nb_iter=NB_ITER, random_state=SEED, average=False)
        res_t, Rs_t = ref_mle.bootstrap_intrinsic_dim_scale_interval(df, nb_iter=NB_ITER, random_state=SEED, average=True)
        assert np.array_equal(Rs, Rs_t)
        out[f"{name}::boot_F"], out[f"{name}::boot_T"], out[f"{name}::Rs"] = np.asarray(res_f), np.asarray(res_t), np.asarray(Rs)
        rng = np.random.RandomState(SEED)           # the subsets the reference drew (mle.py:88)
        subsets = [np.unique(rng.randint(0, len(X) - 1, size=len(X))) for _ in range(NB_ITER)]
        out[f"{name}::boot_idx"] = np.concatenate(subsets).astype(np.int32)
        out[f"{name}::boot_off"] = np.cumsum([0] + [len(s) for s in subsets])
        pca = PCA(n_components='mle').fit(X.astype(np.float64))
        ev = PCA().fit(X.astype(np.float64)).explained_variance_   # the whole spectrum ('mle' keeps n_components_ of it)
        assert _infer_dimension(ev, len(X)) == pca.n_components_
        out[f"{name}::ppca_n"] = np.array(pca.n_components_)
        out[f"{name}::ppca_ev"] = ev
        out[f"{name}::ppca_ll"] = np.array([-np.inf] + [_assess_dimension(ev, r, len(X)) for r in range(1, len(ev))])
        print(name, X.shape, "si", np.round(out[f"{name}::si"][[0, -1]], 3), "ppca", pca.n_components_)
    np.savez_compressed(os.path.join(HERE, "classical_id.npz"), **out)


if __name__ == "__main__":
    main()
