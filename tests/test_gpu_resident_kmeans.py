"""``ResidentPredictor.kmeans`` / ``kmeans_file`` on the GPU: the clusters are ``ops.kmeans_rows``' on the batch's embedding, bit for
bit, with ``classify``'s calls beside them, and they are the ``clusters`` the per-cluster calls take as they come."""
import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as F

import scdeepsort_amd as sda
from scdeepsort_amd import ops

from test_gpu_resident_doublets import BUNDLE_SEED, _counts
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
B, K = 60, 4


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(km, rows_run):
    np.testing.assert_array_equal(km.cluster, rows_run.label.cpu().numpy())
    np.testing.assert_array_equal(_bits(km.sq_distance), _bits(rows_run.d2.cpu().numpy()))
    np.testing.assert_array_equal(_bits(km.centers), _bits(rows_run.centers.cpu().numpy()))
    np.testing.assert_array_equal(km.size, rows_run.size.cpu().numpy())
    np.testing.assert_array_equal(km.seed_cells, rows_run.seed_row.cpu().numpy())
    assert (km.n_iter, km.converged, list(km.inertia_trace)) == (rows_run.n_iter, rows_run.converged, list(rows_run.inertia_trace))
    assert km.inertia == rows_run.inertia_trace[-1]


@pytest.mark.parametrize("n_layers", [1, 2])
def test_kmeans_end_to_end(tmp_path, n_layers):
    root, G = _random_bundle(tmp_path, n_layers, hidden=12, seed=BUNDLE_SEED[n_layers])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G)
    assert counts.shape[0] == B
    label, prob, _ = rp.classify(counts, genes=genes, normalize="lognorm")
    kw = dict(genes=genes, normalize="lognorm")

    for space in ("hidden", "features"):
        emb = rp.embed(counts, space=space, **kw)
        km = rp.kmeans(counts, K, space=space, seed=1, **kw)
        assert isinstance(km, sda.KMeans) and km.space == space and km.metric == "euclidean" and km.n_clusters == K
        assert km.cluster.dtype == np.int64 and km.cluster.shape == (B,) and km.sq_distance.dtype == np.float32
        assert km.centers.shape == (K, emb.shape[1]) and km.size.sum() == B and km.cluster.min() >= 0
        _same(km, ops.kmeans_rows(emb, K, seed=1))
        np.testing.assert_array_equal(km.label, label); np.testing.assert_array_equal(km.max_prob, prob)
        again = rp.kmeans(counts, K, space=space, seed=1, **kw)
        _same(again, ops.kmeans_rows(emb, K, seed=1))
        np.testing.assert_array_equal(again.cluster, km.cluster)
        np.testing.assert_array_equal(_bits(again.centers), _bits(km.centers))
    emb = rp.embed(counts, **kw)
    cos = rp.kmeans(counts, K, metric="cosine", **kw)
    _same(cos, ops.kmeans_rows(F.normalize(emb, dim=1), K))
    assert cos.metric == "cosine"
    # an init array, in the space's own width; max_iter
    start = emb[[0, 1, 2, 3]].cpu().numpy()
    given = rp.kmeans(counts, K, init=start, max_iter=1, **kw)
    assert given.seed_cells is None and given.n_iter == 1 and not given.converged
    want = ops.kmeans_rows(emb, K, init=start, max_iter=1)
    np.testing.assert_array_equal(given.cluster, want.label.cpu().numpy())
    np.testing.assert_array_equal(_bits(given.centers), _bits(want.centers.cpu().numpy()))

    # the table, and the clusters as the per-cluster calls take them
    km = rp.kmeans(counts, K, **kw)
    assert km.cluster_names == ["c0000", "c0001", "c0002", "c0003"] and km.composition().to_numpy().sum() == B
    assert len(km.frame()) == B and f"{B} cells in {K} clusters" in str(km.summary())
    calls = rp.annotate(counts, km.cluster, n_clusters=K, **kw)
    assert calls.tally[:, 0].cpu().numpy().tolist() == km.size.tolist()
    named = rp.annotate(counts, [km.cluster_names[k] for k in km.cluster], cluster_names=km.cluster_names, **kw)
    assert torch.equal(named.votes, calls.votes) and torch.equal(named.prob_sum, calls.prob_sum)
    comp = km.composition().to_numpy()
    np.testing.assert_array_equal(calls.votes.cpu().numpy(), comp[:, :-1])       # annotate's votes are the table's counts
    bulk = rp.pseudobulk(counts, genes, km.cluster, normalize="lognorm", n_clusters=K)
    assert bulk.frame()["n_cells"].tolist() == km.size.tolist()
    ranks = rp.rank_genes(counts, groups=km.cluster, n_groups=K, **kw)
    assert [int(n) for n in ranks.n_cells] == km.size.tolist()


def test_kmeans_file_feeds_annotate_file(tmp_path):
    root, G = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=30, seed=1)
    cells = [f"C{j}" for j in range(30)]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    out = rp.kmeans_file(data, K, normalize="lognorm", save_path=tmp_path / "res")
    km = rp.kmeans(counts, K, genes=genes, normalize="lognorm", index=cells)
    assert (km.size > 0).all()                                          # else the file's sorted names would skip a cluster
    assert list(out.columns) == ["index", "cell", "cluster"] and out["cell"].tolist() == cells
    assert out["cluster"].tolist() == [km.cluster_names[k] for k in km.cluster]
    written = tmp_path / "res" / "mouse_Rand_kmeans.csv"
    by_file = rp.annotate_file(data, written, normalize="lognorm")
    want = rp.annotate(counts, km.cluster, cluster_names=km.cluster_names, genes=genes, normalize="lognorm").frame()
    pd.testing.assert_frame_equal(by_file, want)
    bulk = rp.pseudobulk_file(data, written)
    pd.testing.assert_frame_equal(bulk, rp.pseudobulk(counts, genes, km.cluster, normalize="lognorm",
                                                      cluster_names=km.cluster_names).frame())


def test_kmeans_argument_errors(tmp_path):
    root, G = _random_bundle(tmp_path, 1, hidden=12, seed=1)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    counts, genes = _counts(rp, G, n=8)
    kw = dict(genes=genes, normalize="lognorm")
    for bad in (dict(n_clusters=0), dict(n_clusters=9), dict(n_clusters=5000), dict(n_clusters=2, space="pca"),
                dict(n_clusters=2, metric="manhattan"), dict(n_clusters=2, init="random"), dict(n_clusters=2, max_iter=0),
                dict(n_clusters=2, index=["a"]), dict(n_clusters=2, init=np.zeros((2, 5), np.float32))):
        with pytest.raises(ValueError):
            rp.kmeans(counts, **bad, **kw)
    rp.hidden, rp.hidden_padded = 260, 260               # what a wider bundle sets: the refusal comes before any launch
    with pytest.raises(ValueError, match="fused kernels only"):
        rp.kmeans(counts, 2, **kw)
