"""``ResidentPredictor.leiden`` / ``leiden_file`` on the GPU: the communities are ``ops.leiden_graph``'s on the shared-neighbour graph of
``knn``'s own lists, with ``classify``'s calls beside them; every one of them is connected on that graph, and they are the
``clusters`` / ``groups`` the per-cluster calls take as they come."""
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import ops

import leiden_reference as L
from test_gpu_resident_doublets import BUNDLE_SEED, _counts
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
B, KNN = 60, 6


def _same(table, rows_run):
    np.testing.assert_array_equal(table.cluster, rows_run.cluster.cpu().numpy())
    assert len(table.level_labels) == len(rows_run.level_labels) and len(table.refined_labels) == len(rows_run.refined_labels)
    assert len(table.refined_labels) == len(table.levels)
    for mine, theirs in zip(list(table.level_labels) + list(table.refined_labels), rows_run.level_labels + rows_run.refined_labels):
        np.testing.assert_array_equal(mine, theirs.cpu().numpy())
    assert (table.levels, table.modularity, table.resolution, table.converged) == \
        (rows_run.levels, rows_run.modularity, rows_run.resolution, rows_run.converged)
    np.testing.assert_array_equal(table.size, np.bincount(table.cluster[table.cluster >= 0]))
    assert table.method == "leiden"


def _connected(lists, weights, cluster):
    rowptr, col, _ = ops.snn_graph(lists, weights)
    return L.disconnected(rowptr.cpu().numpy(), col.cpu().numpy(), cluster) == 0


@pytest.mark.parametrize("n_layers", [1, 2])
def test_leiden_end_to_end(tmp_path, n_layers):
    root, G = _random_bundle(tmp_path, n_layers, hidden=12, seed=BUNDLE_SEED[n_layers])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G)
    assert counts.shape[0] == B
    label, prob, _ = rp.classify(counts, genes=genes, normalize="lognorm")
    kw = dict(genes=genes, normalize="lognorm")
    dev = rp.device

    for space, metric, weights in (("hidden", "euclidean", "snn"), ("features", "euclidean", "unit"), ("hidden", "cosine", "snn")):
        graph = rp.knn(counts, k=KNN, space=space, metric=metric, **kw)
        out = rp.leiden(counts, k=KNN, weights=weights, space=space, metric=metric, **kw)
        assert isinstance(out, sda.Communities) and (out.space, out.metric, out.weights, out.k) == (space, metric, weights, KNN)
        assert out.cluster.dtype == np.int64 and out.cluster.shape == (B,) and out.cluster.min() >= 0
        assert out.n_clusters == len(out.size) >= 2 and out.size.sum() == B and (np.diff(out.size) <= 0).all()
        lists = torch.from_numpy(graph.indices).to(dev)
        want = ops.leiden_graph(*ops.snn_graph(lists, weights))
        _same(out, want)
        assert _connected(lists, weights, out.cluster)
        np.testing.assert_array_equal(out.label, label); np.testing.assert_array_equal(out.max_prob, prob)
        # graph= skips the search: a NeighborGraph brings its own space and metric, an array keeps the arguments'
        given = rp.leiden(counts, weights=weights, graph=graph, **kw)
        _same(given, want)
        assert (given.space, given.metric, given.k) == (space, metric, KNN)
        _same(rp.leiden(counts, weights=weights, graph=graph.indices.astype(np.int32), **kw), want)
        _same(rp.leiden(counts, weights=weights, graph=graph.indices, **kw), want)
        _same(rp.leiden(counts, k=KNN, weights=weights, space=space, metric=metric, **kw), want)       # two calls, the same bits
        # louvain stays louvain
        assert rp.louvain(counts, weights=weights, graph=graph, **kw).method == "louvain"

    out = rp.leiden(counts, k=KNN, resolution=0.8, index=[f"C{j}" for j in range(B)], **kw)
    graph = rp.knn(counts, k=KNN, **kw)
    assert out.resolution == Fraction(4, 5)
    _same(out, ops.leiden_graph(*ops.snn_graph(torch.from_numpy(graph.indices).to(dev)), resolution=0.8))

    # the table
    K = out.n_clusters
    assert out.cluster_names == [f"c{k:04d}" for k in range(K)] and out.composition().to_numpy().sum() == B
    frame = out.frame()
    assert len(frame) == B and frame["index"].tolist() == [f"C{j}" for j in range(B)] and frame["cluster_size"].tolist() == out.size[out.cluster].tolist()
    assert f"{B} cells in {K} Leiden communities" in str(out.summary()) and out.summary()["method"] == "leiden"
    np.testing.assert_array_equal(out.at_level(-1), out.cluster)
    first = out.at_level(0)
    assert first.max() + 1 == out.levels[0]["communities"]
    # ... and the communities as the per-cluster calls take them, without conversion
    calls = rp.annotate(counts, out.cluster, n_clusters=K, **kw)
    assert calls.tally[:, 0].cpu().numpy().tolist() == out.size.tolist()
    np.testing.assert_array_equal(calls.votes.cpu().numpy(), out.composition().to_numpy()[:, :-1])
    sil = rp.silhouette(counts, groups=out.cluster, n_groups=K, **kw)
    np.testing.assert_array_equal(sil.size, out.size)
    ranks = rp.rank_genes(counts, groups=out.cluster, n_groups=K, **kw)
    assert [int(n) for n in ranks.n_cells] == out.size.tolist()
    bulk = rp.pseudobulk(counts, genes, out.cluster, normalize="lognorm", n_clusters=K)
    assert bulk.frame()["n_cells"].tolist() == out.size.tolist()


def test_leiden_file_feeds_annotate_file(tmp_path):
    root, G = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=30, seed=1)
    cells = [f"C{j}" for j in range(30)]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    out = rp.leiden_file(data, k=5, normalize="lognorm", save_path=tmp_path / "res")
    table = rp.leiden(counts, k=5, genes=genes, normalize="lognorm", index=cells)
    assert list(out.columns) == ["index", "cell", "cluster"] and out["cell"].tolist() == cells
    assert out["cluster"].tolist() == [table.cluster_names[k] for k in table.cluster]
    written = tmp_path / "res" / "mouse_Rand_leiden.csv"
    by_file = rp.annotate_file(data, written, normalize="lognorm")
    want = rp.annotate(counts, table.cluster, cluster_names=table.cluster_names, genes=genes, normalize="lognorm").frame()
    pd.testing.assert_frame_equal(by_file, want)
    bulk = rp.pseudobulk_file(data, written)
    pd.testing.assert_frame_equal(bulk, rp.pseudobulk(counts, genes, table.cluster, normalize="lognorm",
                                                      cluster_names=table.cluster_names).frame())
    assert len(rp.silhouette_file(data, written, normalize="lognorm")) == 30


def test_leiden_argument_errors(tmp_path):
    root, G = _random_bundle(tmp_path, 1, hidden=12, seed=1)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    counts, genes = _counts(rp, G, n=8)
    kw = dict(genes=genes, normalize="lognorm")
    for bad in (dict(weights="jaccard"), dict(k=0), dict(k=65), dict(resolution=0), dict(resolution=float("nan")),
                dict(space="pca"), dict(metric="manhattan"), dict(max_sweeps=0), dict(index=["a"]),
                dict(graph=np.zeros((7, 3), np.int64)), dict(graph=np.zeros((8, 3), np.float32)), dict(graph=np.full((8, 3), 8)),
                dict(graph=np.zeros((8, 65), np.int64))):
        with pytest.raises(ValueError):
            rp.leiden(counts, **bad, **kw)
    rp.hidden, rp.hidden_padded = 260, 260               # what a wider bundle sets: the refusal comes before any launch
    with pytest.raises(ValueError, match="leiden runs on the fused kernels only"):
        rp.leiden(counts, **kw)
