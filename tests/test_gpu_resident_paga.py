"""``ResidentPredictor.paga`` / ``paga_file`` on the GPU: the tables are ``ops.group_edges`` on ``knn``'s own lists and the numpy
restatement's (tests/geodesic_reference.py) exact rationals, for the predicted types and for ``leiden``'s communities; graph
reuse, ``directed`` by ``pseudotime``, the file round trip and the argument errors."""
import numpy as np
import pandas as pd
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import ops

import geodesic_reference as G
from test_gpu_resident_doublets import BUNDLE_SEED, _counts
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
B, KNN = 60, 6


def _same(table, lists, group, K, dev):
    """``table`` against ``ops.group_edges`` run by hand and against the restatement's tables."""
    by_hand = ops.group_edges(torch.from_numpy(lists).to(dev), torch.from_numpy(group).to(dev), K)
    np.testing.assert_array_equal(table.edges, by_hand.edges.cpu().numpy())
    np.testing.assert_array_equal(table.size, by_hand.size.cpu().numpy())
    edges, size = G.group_edges(lists, group, K)
    np.testing.assert_array_equal(table.edges, edges); np.testing.assert_array_equal(table.size, size)
    out_edges, expected, conn = G.paga(edges, size)
    np.testing.assert_array_equal(table.out_edges, out_edges)
    np.testing.assert_array_equal(table.expected, expected)
    np.testing.assert_array_equal(table.connectivities, conn)
    assert table.edges.dtype == table.size.dtype == table.out_edges.dtype == np.int64 and table.connectivities.dtype == np.float64
    np.testing.assert_array_equal(table.connectivities, table.connectivities.T)
    assert (np.diag(table.connectivities) == 0).all() and table.connectivities.max() <= 1.0
    np.testing.assert_array_equal(table.group, group)
    assert table.n_skipped == (group < 0).sum() and len(table.group_names) == K


@pytest.mark.parametrize("n_layers", [1, 2])
def test_paga_end_to_end(tmp_path, n_layers):
    root, n_genes = _random_bundle(tmp_path, n_layers, hidden=12, seed=BUNDLE_SEED[n_layers])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, n_genes)
    assert counts.shape[0] == B
    label, prob, _ = rp.classify(counts, genes=genes, normalize="lognorm")
    kw = dict(genes=genes, normalize="lognorm")
    dev = rp.device
    C = len(rp.id2label)
    predicted = np.where(label >= 0, label, -1).astype(np.int64)

    for space, metric in (("hidden", "euclidean"), ("features", "euclidean"), ("hidden", "cosine")):
        graph = rp.knn(counts, k=KNN, space=space, metric=metric, **kw)
        out = rp.paga(counts, k=KNN, space=space, metric=metric, **kw)
        assert isinstance(out, sda.Abstraction) and (out.space, out.metric, out.k) == (space, metric, KNN)
        assert list(out.group_names) == list(rp.id2label)
        _same(out, graph.indices, predicted, C, dev)
        # graph= skips the search: a NeighborGraph brings its own space and metric, an array keeps the arguments'
        given = rp.paga(counts, graph=graph, **kw)
        _same(given, graph.indices, predicted, C, dev)
        assert (given.space, given.metric, given.k) == (space, metric, KNN)
        _same(rp.paga(counts, graph=graph.indices, **kw), graph.indices, predicted, C, dev)
        _same(rp.paga(counts, graph=graph.indices.astype(np.int32), **kw), graph.indices, predicted, C, dev)

    # leiden's communities feed it as they come
    graph = rp.knn(counts, k=KNN, **kw)
    lc = rp.leiden(counts, graph=graph, **kw)
    K = lc.n_clusters
    out = rp.paga(counts, groups=lc.cluster, n_groups=K, graph=graph, **kw)
    _same(out, graph.indices, lc.cluster, K, dev)
    assert out.size.tolist() == lc.size.tolist() and out.n_skipped == 0 and out.edges.sum() == (graph.indices >= 0).sum()
    named = rp.paga(counts, groups=torch.from_numpy(lc.cluster), group_names=lc.cluster_names, graph=graph, **kw)
    np.testing.assert_array_equal(named.connectivities, out.connectivities)
    assert list(named.group_names) == lc.cluster_names
    some = lc.cluster.copy()
    some[::4] = -1                                                      # cells the caller skips
    _same(rp.paga(counts, groups=some, n_groups=K, graph=graph, **kw), graph.indices, some, K, dev)

    # the table: the spanning forest, the frame, and the pairs oriented by pseudotime
    tree, frame = out.tree(), out.frame()
    inter = out.edges + out.edges.T
    pairs = [(a, b) for a in range(K) for b in range(a + 1, K) if inter[a, b] > 0]
    assert list(zip(frame["a"], frame["b"])) == [(str(a), str(b)) for a, b in pairs]
    assert frame["edges"].tolist() == [int(inter[a, b]) for a, b in pairs]
    assert frame["connectivity"].tolist() == [out.connectivities[a, b] for a, b in pairs]
    assert frame["in_tree"].tolist() == [bool(tree[a, b]) for a, b in pairs]
    np.testing.assert_array_equal(tree, tree.T)
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    n_comp = connected_components(csr_matrix(inter > 0), directed=False)[0]
    assert tree.sum() // 2 == K - n_comp == out.summary()["n_tree_edges"] and out.summary()["n_components"] == n_comp
    pt = rp.pseudotime(counts, 0, graph=graph, **kw)
    directed = out.directed(pt)
    reached = ~np.isnan(pt.pseudotime)
    median = {str(a): np.median(pt.pseudotime[(lc.cluster == a) & reached]) if ((lc.cluster == a) & reached).any() else np.nan
              for a in range(K)}
    assert [{a, b} for a, b in zip(directed["a"], directed["b"])] == [{a, b} for a, b in zip(frame["a"], frame["b"])]
    assert not any(median[a] > median[b] for a, b in zip(directed["a"], directed["b"]))
    np.testing.assert_array_equal(directed["median_a"], [median[a] for a in directed["a"]])
    np.testing.assert_array_equal(directed["median_b"], [median[b] for b in directed["b"]])
    # turned round: time that runs the other way turns every pair whose medians differ
    back = out.directed(1.0 - pt.pseudotime)
    for (a, b), (c, d) in zip(zip(directed["a"], directed["b"]), zip(back["a"], back["b"])):
        assert (c, d) == ((b, a) if median[a] < median[b] else (min(a, b, key=int), max(a, b, key=int)))
    layout = np.random.default_rng(0).normal(size=(B, 2)).astype(np.float32)
    np.testing.assert_allclose(out.centroids(layout), np.stack([layout[lc.cluster == a].astype(np.float64).mean(0) for a in range(K)]),
                               rtol=1e-12)
    assert f"{B} cells in {K} non-empty groups" in str(out.summary())


def test_paga_file_round_trip(tmp_path):
    root, n_genes = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, n_genes, n=30, seed=1)
    cells = [f"C{j}" for j in range(30)]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    kw = dict(genes=genes, normalize="lognorm")
    rp.leiden_file(data, k=5, normalize="lognorm", save_path=tmp_path / "res")
    clusters = rp.leiden(counts, k=5, index=cells, **kw)
    out = rp.paga_file(data, tmp_path / "res" / "mouse_Rand_leiden.csv", k=5, normalize="lognorm", save_path=tmp_path / "res")
    want = rp.paga(counts, groups=clusters.cluster, group_names=clusters.cluster_names, k=5, **kw).frame()
    pd.testing.assert_frame_equal(out, want)
    written = pd.read_csv(tmp_path / "res" / "mouse_Rand_paga.csv", float_precision="round_trip", dtype={"a": str, "b": str})
    assert list(written.columns) == ["a", "b", "edges", "expected", "connectivity", "in_tree"] and len(written) == len(want)
    assert written["a"].tolist() == want["a"].tolist() and written["edges"].tolist() == want["edges"].tolist()
    np.testing.assert_array_equal(written["connectivity"], want["connectivity"])
    np.testing.assert_array_equal(written["expected"], want["expected"])
    # no clusters file: the predicted types
    pd.testing.assert_frame_equal(rp.paga_file(data, k=5, normalize="lognorm"), rp.paga(counts, k=5, **kw).frame())


def test_paga_argument_errors(tmp_path):
    root, n_genes = _random_bundle(tmp_path, 1, hidden=12, seed=1)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    counts, genes = _counts(rp, n_genes, n=8)
    kw = dict(genes=genes, normalize="lognorm")
    short = rp.knn(counts[:7], k=3, **kw)
    ids = np.arange(8) % 2
    for bad in (dict(k=0), dict(k=65), dict(space="pca"), dict(metric="manhattan"), dict(index=["a"]), dict(groups="clusters"),
                dict(groups=ids), dict(groups=ids, n_groups=1), dict(groups=ids[:7], n_groups=2), dict(groups=ids * 0.5, n_groups=2),
                dict(groups=ids - 2, n_groups=2), dict(groups=ids, n_groups=2, group_names=["a"]), dict(groups=ids, n_groups=4097),
                dict(graph=np.zeros((7, 3), np.int64)), dict(graph=np.zeros((8, 3), np.float32)), dict(graph=np.full((8, 3), 8)),
                dict(graph=np.zeros((8, 65), np.int64)), dict(graph=short)):
        with pytest.raises(ValueError):
            rp.paga(counts, **bad, **kw)
    rp.hidden, rp.hidden_padded = 260, 260               # what a wider bundle sets: the refusal comes before any launch
    with pytest.raises(ValueError, match="paga runs on the fused kernels only"):
        rp.paga(counts, **kw)
