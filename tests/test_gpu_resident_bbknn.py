"""``ResidentPredictor.bbknn`` / ``bbknn_file`` and ``NeighborGraph.lisi`` on the GPU: the batch-balanced graph is
``ops.knn_segments`` on ``embed``'s rows bit for bit, with a single batch it is ``knn``'s graph, and every ``graph=`` argument
takes it as the ``NeighborGraph`` it is."""
import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as F

import scdeepsort_amd as sda
from scdeepsort_amd import ops

import bbknn_reference as BR
from test_gpu_resident_doublets import BUNDLE_SEED, _counts
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
B, S, KW = 60, 3, 3


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _batches():
    """One name per cell, three samples of 24, 21 and 15 cells dealt over the rows."""
    ids = np.random.default_rng(2).permutation(np.repeat(np.arange(S), (24, 21, 15)))
    return np.array([f"sample{i}" for i in ids]), ids


def _predictor(tmp_path, n_layers=2):
    root, G = _random_bundle(tmp_path, n_layers, hidden=12, seed=BUNDLE_SEED[n_layers])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G)
    assert counts.shape[0] == B
    return rp, counts, genes, dict(genes=genes, normalize="lognorm")


@pytest.mark.parametrize("n_layers", [1, 2])
def test_bbknn_is_knn_segments_on_the_embedding(tmp_path, n_layers):
    rp, counts, genes, kw = _predictor(tmp_path, n_layers)
    names, ids = _batches()
    label, prob, _ = rp.classify(counts, **kw)
    for space in ("hidden", "features"):
        for metric in ("euclidean", "cosine"):
            bg = rp.bbknn(counts, names, k_within=KW, space=space, metric=metric, **kw)
            assert isinstance(bg, sda.BatchGraph) and isinstance(bg, sda.NeighborGraph)
            assert (bg.k, bg.k_within, bg.space, bg.metric) == (S * KW, KW, space, metric)
            assert bg.batch_names == [f"sample{i}" for i in range(S)] and bg.batch.dtype == np.int64
            np.testing.assert_array_equal(bg.batch, ids)
            np.testing.assert_array_equal(bg.label, label); np.testing.assert_array_equal(bg.max_prob, prob)
            rows = rp.embed(counts, space=space, **kw)
            if metric == "cosine":
                rows = F.normalize(rows, dim=1)
            want = ops.knn_segments(rows, torch.from_numpy(ids).to(rows.device), S, KW)
            assert bg.indices.dtype == bg.by_batch_indices.dtype == np.int64 and bg.sq_distances.dtype == np.float32
            np.testing.assert_array_equal(bg.indices, want.merged_idx.cpu().numpy())
            np.testing.assert_array_equal(_u32(bg.sq_distances), _u32(want.merged_d2.cpu().numpy()))
            np.testing.assert_array_equal(bg.by_batch_indices, want.idx.cpu().numpy())
            np.testing.assert_array_equal(_u32(bg.by_batch_sq_distances), _u32(want.d2.cpu().numpy()))
            # the merged list is the blocked lists under (distance, index); a block lists its own batch
            merged = BR.merge(bg.by_batch_indices, bg.by_batch_sq_distances)
            np.testing.assert_array_equal(bg.indices, merged[0]); np.testing.assert_array_equal(_u32(bg.sq_distances), _u32(merged[1]))
            listed = bg.by_batch_indices >= 0
            assert (ids[bg.by_batch_indices] == np.arange(S)[None, :, None])[listed].all()
            full = listed.all(axis=(1, 2))                                        # a cell without a read may have no usable row
            assert full.sum() >= B - 1 and (bg.batch_share()[full] == (S - 1) / S).all()
            again = rp.bbknn(counts, names, k_within=KW, space=space, metric=metric, **kw)          # two calls: the same bits
            np.testing.assert_array_equal(again.indices, bg.indices)
            np.testing.assert_array_equal(_u32(again.sq_distances), _u32(bg.sq_distances))
    # integer ids with their names, or their number, give the same graph
    bg = rp.bbknn(counts, names, k_within=KW, **kw)
    for given in (dict(batch_names=bg.batch_names), dict(n_batches=S)):
        same = rp.bbknn(counts, torch.from_numpy(ids), k_within=KW, **given, **kw)
        np.testing.assert_array_equal(same.indices, bg.indices)
    table, summary = bg.by_batch(), bg.summary()
    assert table["n_cells"].tolist() == [24, 21, 15] and (table["n_short"] == 0).all() and np.isfinite(table.iloc[:, 3:].values).all()
    assert summary["batch_sizes"] == {"sample0": 24, "sample1": 21, "sample2": 15} and "3 batches" in str(summary)
    assert len(bg.frame()) == B
    # a single batch: knn's graph
    one = rp.bbknn(counts, np.zeros(B, np.int64), k_within=5, n_batches=1, **kw)
    plain = rp.knn(counts, k=5, **kw)
    np.testing.assert_array_equal(one.indices, plain.indices)
    np.testing.assert_array_equal(_u32(one.sq_distances), _u32(plain.sq_distances))
    assert np.isnan(one.batch_share()).sum() == 0 and (one.batch_share() == 0).all()
    # a batch with fewer cells than k_within: short lists, the share follows what is listed
    few = np.zeros(B, np.int64); few[[3, 17]] = 1
    short = rp.bbknn(counts, few, k_within=4, n_batches=2, **kw)
    listed = (short.by_batch_indices >= 0).sum(axis=2)
    assert (listed[:, 0] == 4).all() and (listed[:, 1] == np.where(few == 1, 1, 2)).all()
    assert short.summary()["n_short"] == B and short.by_batch()["n_short"].tolist() == [58, 2]


def test_every_graph_argument_takes_a_batch_graph(tmp_path):
    rp, counts, genes, kw = _predictor(tmp_path)
    names, ids = _batches()
    bg = rp.bbknn(counts, names, k_within=KW, **kw)
    plain = sda.NeighborGraph(indices=bg.indices, sq_distances=bg.sq_distances, k=bg.k, space=bg.space, metric=bg.metric,
                              label=bg.label, max_prob=bg.max_prob, index=bg.index, id2label=bg.id2label, label_map=bg.label_map)
    for method in (rp.louvain, rp.leiden):
        a, b, c = method(counts, graph=bg, **kw), method(counts, graph=bg.indices, **kw), method(counts, graph=plain, **kw)
        np.testing.assert_array_equal(a.cluster, b.cluster); np.testing.assert_array_equal(a.cluster, c.cluster)
        assert a.k == S * KW and a.modularity == b.modularity
    a, b = rp.umap(counts, graph=bg, n_epochs=20, init="hash", **kw), rp.umap(counts, graph=plain, n_epochs=20, init="hash", **kw)
    np.testing.assert_array_equal(_u32(a.coords), _u32(b.coords))
    np.testing.assert_array_equal(a.col, b.col); np.testing.assert_array_equal(_u32(a.weight), _u32(b.weight))
    assert a.k == S * KW and np.isfinite(a.coords).all()
    a, b = rp.pseudotime(counts, 0, graph=bg, **kw), rp.pseudotime(counts, 0, graph=plain, **kw)
    np.testing.assert_array_equal(_u32(a.distance), _u32(b.distance))
    assert a.k == S * KW
    a, b = rp.paga(counts, graph=bg, **kw), rp.paga(counts, graph=plain, **kw)
    np.testing.assert_array_equal(a.edges, b.edges)
    a, b = rp.diffmap(counts, n_comps=5, graph=bg, **kw), rp.diffmap(counts, n_comps=5, graph=plain, **kw)
    np.testing.assert_array_equal(a.coords.view(np.uint64), b.coords.view(np.uint64))
    assert a.k == S * KW
    # and smooth its lists
    sm = rp.smooth(counts, genes, bg.indices, normalize="lognorm")
    assert (sm.n_neighbors == S * KW).all()


def test_lisi_of_the_plain_graph_and_of_the_balanced_one(tmp_path):
    rp, counts, genes, kw = _predictor(tmp_path)
    names, ids = _batches()
    graph = rp.knn(counts, k=9, **kw)
    n_types = len(graph.id2label)
    got = graph.lisi("predicted", n_labels=n_types)
    want = BR.lisi(graph.indices, graph.distances(), graph.label, 3.0, n_types)
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    # between 1 and the number of types where every neighbour has a call; an unsure neighbour is a stranger and lifts the index
    # beyond that, and a cell whose neighbours are all unsure has none
    called = (graph.label[graph.indices] >= 0).all(axis=1)
    assert not np.isnan(got[called]).any() and (got[called] >= 1.0 - 1e-12).all() and (got[called] <= n_types + 1e-12).all()
    assert np.isnan(got[(graph.label[graph.indices] < 0).all(axis=1)]).all() and (got[~np.isnan(got)] >= 1.0 - 1e-12).all()
    # over the batches: one id per cell on the plain graph; "batch" on the balanced one, which knows its own
    mixing = graph.lisi(ids)
    np.testing.assert_array_equal(mixing.view(np.uint64), BR.lisi(graph.indices, graph.distances(), ids, 3.0, S).view(np.uint64))
    assert (mixing >= 1.0 - 1e-12).all() and (mixing <= S + 1e-12).all()
    bg = rp.bbknn(counts, names, k_within=KW, **kw)
    np.testing.assert_array_equal(bg.lisi("batch").view(np.uint64), bg.lisi(ids).view(np.uint64))
    with pytest.raises(ValueError, match="predicted"):
        graph.lisi("batch")


def test_bbknn_file_feeds_smooth_file(tmp_path):
    root, G = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=30, seed=1)
    cells = [f"C{j}" for j in range(30)]
    batch = [f"run{j % 2}" for j in range(30)]
    data, batch_file = tmp_path / "mouse_Rand7_data.csv", tmp_path / "mouse_Rand7_batches.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    pd.DataFrame({"Cell": cells, "Batch": batch}).to_csv(batch_file)
    out = rp.bbknn_file(data, batch_file, k_within=2, normalize="lognorm", save_path=tmp_path / "res")
    graph = rp.bbknn(counts, batch, k_within=2, genes=genes, normalize="lognorm", index=cells)
    assert list(out.columns) == ["cell"] + [f"n{j}" for j in range(4)] and out["cell"].tolist() == cells
    assert out.iloc[:, 1:].values.tolist() == [[cells[j] for j in row] for row in graph.indices]
    smoothed = rp.smooth_file(data, tmp_path / "res" / "mouse_Rand_bbknn.csv")
    pd.testing.assert_frame_equal(smoothed, rp.smooth(counts, genes, graph.indices, normalize="lognorm", index=cells).frame())
    with pytest.raises(ValueError, match="cell order"):
        pd.DataFrame({"Cell": cells[::-1], "Batch": batch}).to_csv(batch_file)
        rp.bbknn_file(data, batch_file, k_within=2, normalize="lognorm")


def test_refusals(tmp_path):
    root, G = _random_bundle(tmp_path, 1, hidden=12, seed=1)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    counts, genes = _counts(rp, G, n=8)
    kw = dict(genes=genes, normalize="lognorm")
    two = np.arange(8) % 2
    with pytest.raises(ValueError, match="65 batches with k_within = 1"):                  # too many batches
        rp.bbknn(counts, two, k_within=1, n_batches=65, **kw)
    with pytest.raises(ValueError, match="22 batches with k_within = 3"):                  # n_batches * k_within > 64
        rp.bbknn(counts, two, k_within=3, n_batches=22, **kw)
    with pytest.raises(ValueError, match="2 batches with k_within = 33"):
        rp.bbknn(counts, two, k_within=33, n_batches=2, **kw)
    with pytest.raises(ValueError, match="k_within = 0"):
        rp.bbknn(counts, two, k_within=0, n_batches=2, **kw)
    with pytest.raises(ValueError, match="-1 is not taken"):                               # a cell without a batch
        rp.bbknn(counts, np.where(np.arange(8) == 3, -1, two), n_batches=2, **kw)
    for bad in (two[:7], two.astype(np.float32), two + 1):                                 # a wrong length, no ids, out of range
        with pytest.raises(ValueError):
            rp.bbknn(counts, bad, n_batches=2, **kw)
    with pytest.raises(ValueError):                                                        # integer ids need names or their number
        rp.bbknn(counts, two, **kw)
    for bad in (dict(space="pca"), dict(metric="manhattan"), dict(index=list("abc"))):
        with pytest.raises(ValueError):
            rp.bbknn(counts, two, n_batches=2, **bad, **kw)
    rp.hidden, rp.hidden_padded = 260, 260               # what a wider bundle sets: the refusal comes before any launch
    with pytest.raises(ValueError, match="fused kernels only"):
        rp.bbknn(counts, two, n_batches=2, **kw)
