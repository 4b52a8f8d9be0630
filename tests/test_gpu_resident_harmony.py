"""``ResidentPredictor.harmony`` / ``harmony_file`` on the GPU, on the small bundle the other resident tests use: the table is
``ops.harmony_rows`` on ``embed``'s rows bit for bit with ``classify``'s calls beside it, its graphs are ``NeighborGraph``s that
know the batches and that every ``graph=`` argument takes, ``graph_before`` is ``knn(metric="cosine")``'s, and two calls give the
same bits."""
import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as F

import scdeepsort_amd as sda
from scdeepsort_amd import ops

from test_gpu_resident_bbknn import B, S, _batches, _predictor, _u32
from test_gpu_resident_doublets import BUNDLE_SEED, _counts
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
K = 9


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("n_layers", [1, 2])
def test_harmony_is_harmony_rows_on_the_embedding(tmp_path, n_layers):
    rp, counts, genes, kw = _predictor(tmp_path, n_layers)
    names, ids = _batches()
    label, prob, _ = rp.classify(counts, **kw)
    h = rp.harmony(counts, names, k=K, **kw)
    assert isinstance(h, sda.Harmonized) and sda.Harmonized is sda.api.Harmonized is sda.tables.Harmonized
    np.testing.assert_array_equal(h.label, label); np.testing.assert_array_equal(h.max_prob, prob)
    np.testing.assert_array_equal(h.batch, ids)
    assert h.batch_names == [f"sample{i}" for i in range(S)] and h.batch.dtype == np.int64 and h.space == "hidden"
    rows = rp.embed(counts, **kw)
    run = ops.harmony_rows(rows.contiguous(), torch.from_numpy(ids).to(rows.device), S)
    assert h.coords.dtype == np.float32 and h.coords.shape == (B, rows.shape[1]) and h.cluster_prob.dtype == np.float64
    np.testing.assert_array_equal(_u32(h.coords), _u32(run.coords.float().cpu().numpy()))
    np.testing.assert_array_equal(_u32(h.embedding), _u32(rows.cpu().numpy()))
    np.testing.assert_array_equal(_u64(h.cluster_prob), _u64(run.R.cpu().numpy()))
    np.testing.assert_array_equal(_u64(h.centers), _u64(run.centers.cpu().numpy()))
    np.testing.assert_array_equal(h.cluster, h.cluster_prob.argmax(axis=1))
    assert h.cluster_prob.shape == (B, ops.harmony_default_clusters(B)) and list(h.objective) == run.objective
    assert (h.n_iter, h.converged) == (run.n_iter, run.converged) and 1 <= h.n_iter <= 10
    # the graphs: the corrected unit rows, and knn's own cosine lists
    for g in (h.graph, h.graph_before):
        assert isinstance(g, sda.NeighborGraph) and (g.k, g.metric, g.space) == (K, "cosine", "hidden")
        assert g.indices.dtype == np.int64 and g.indices.shape == (B, K) and g.batch_names == h.batch_names
        np.testing.assert_array_equal(g.batch, ids)
        np.testing.assert_array_equal(g.lisi("batch").view(np.uint64), g.lisi(ids, n_labels=S).view(np.uint64))
    idx, d2 = ops.knn_rows(F.normalize(run.coords.float(), dim=1), K)
    np.testing.assert_array_equal(h.graph.indices, idx.cpu().numpy()); np.testing.assert_array_equal(_u32(h.graph.sq_distances), _u32(d2.cpu().numpy()))
    plain = rp.knn(counts, k=K, metric="cosine", **kw)
    np.testing.assert_array_equal(h.graph_before.indices, plain.indices)
    np.testing.assert_array_equal(_u32(h.graph_before.sq_distances), _u32(plain.sq_distances))
    # two calls: the same bits; integer ids with their number: the same table
    for again in (rp.harmony(counts, names, k=K, **kw), rp.harmony(counts, torch.from_numpy(ids), k=K, n_batches=S, **kw)):
        np.testing.assert_array_equal(_u32(again.coords), _u32(h.coords))
        np.testing.assert_array_equal(_u64(again.cluster_prob), _u64(h.cluster_prob))
        np.testing.assert_array_equal(again.graph.indices, h.graph.indices)
        assert list(again.objective) == list(h.objective)
    # the host tables
    mix, by, frame, summary = h.mixing(), h.by_batch(), h.frame(), h.summary()
    assert list(mix.columns) == ["index", "batch_lisi_before", "batch_lisi_after", "type_lisi_before", "type_lisi_after"] and len(mix) == B
    np.testing.assert_array_equal(mix["batch_lisi_after"].to_numpy().view(np.uint64), h.graph.lisi("batch", n_labels=S).view(np.uint64))
    assert by["batch"].tolist() == h.batch_names and by["n_cells"].tolist() == [24, 21, 15] and (by["median_shift"] >= 0).all()
    assert list(frame.columns)[:7] == ["index", "cell_type", "prob", "batch", "cluster", "cluster_prob", "shift"]
    assert list(frame.columns)[7:] == [f"h{j + 1}" for j in range(h.coords.shape[1])] and len(frame) == B
    np.testing.assert_array_equal(frame["shift"].to_numpy(), h.shift())
    assert summary["batch_sizes"] == {"sample0": 24, "sample1": 21, "sample2": 15} and summary["k"] == K
    text = str(summary)
    assert "3 batches" in text and "median batch LISI" in text
    assert ("WARNING" in text) == (summary["type_lisi_after"] > summary["type_lisi_before"])


def test_skipped_graphs_and_one_batch(tmp_path):
    rp, counts, genes, kw = _predictor(tmp_path)
    names, ids = _batches()
    full = rp.harmony(counts, names, k=K, **kw)
    no_before = rp.harmony(counts, names, k=K, compare=False, **kw)
    assert no_before.graph_before is None and np.array_equal(no_before.graph.indices, full.graph.indices)
    assert np.isnan(no_before.mixing()["batch_lisi_before"]).all() and "not compared" in str(no_before.summary())
    bare = rp.harmony(counts, names, k=None, **kw)
    assert bare.graph is None and bare.graph_before is None
    np.testing.assert_array_equal(_u32(bare.coords), _u32(full.coords))
    with pytest.raises(ValueError, match="k=None"):
        bare.mixing()
    assert "LISI" not in str(bare.summary()) and len(bare.frame()) == B
    one = rp.harmony(counts, np.zeros(B, np.int64), n_batches=1, k=K, **kw)     # nothing to correct: the input's bits
    np.testing.assert_array_equal(_u32(one.coords), _u32(one.embedding))
    assert one.n_iter == 0 and one.cluster_prob.shape == (B, 0) and (one.shift() == 0).all() and (one.cluster == 0).all()
    np.testing.assert_array_equal(one.graph.indices, one.graph_before.indices)
    assert len(one.frame()) == B and "1 batches" in str(one.summary())


def test_every_graph_argument_takes_the_corrected_graph(tmp_path):
    rp, counts, genes, kw = _predictor(tmp_path)
    names, ids = _batches()
    g = rp.harmony(counts, names, k=K, **kw).graph
    plain = sda.NeighborGraph(indices=g.indices, sq_distances=g.sq_distances, k=g.k, space=g.space, metric=g.metric,
                              label=g.label, max_prob=g.max_prob, index=g.index, id2label=g.id2label, label_map=g.label_map)
    for method in (rp.louvain, rp.leiden):
        a, b = method(counts, graph=g, **kw), method(counts, graph=plain, **kw)
        np.testing.assert_array_equal(a.cluster, b.cluster)
        assert a.k == K
    a, b = rp.umap(counts, graph=g, n_epochs=20, init="hash", **kw), rp.umap(counts, graph=plain, n_epochs=20, init="hash", **kw)
    np.testing.assert_array_equal(_u32(a.coords), _u32(b.coords))
    assert a.k == K and np.isfinite(a.coords).all()
    a, b = rp.pseudotime(counts, 0, graph=g, **kw), rp.pseudotime(counts, 0, graph=plain, **kw)
    np.testing.assert_array_equal(_u32(a.distance), _u32(b.distance))
    np.testing.assert_array_equal(rp.paga(counts, graph=g, **kw).edges, rp.paga(counts, graph=plain, **kw).edges)
    a, b = rp.diffmap(counts, n_comps=5, graph=g, **kw), rp.diffmap(counts, n_comps=5, graph=plain, **kw)
    np.testing.assert_array_equal(a.coords.view(np.uint64), b.coords.view(np.uint64))
    assert (rp.smooth(counts, genes, g.indices, normalize="lognorm").n_neighbors == K).all()


def test_harmony_file_writes_the_coordinates(tmp_path):
    root, G = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=30, seed=1)
    cells = [f"C{j}" for j in range(30)]
    batch = [f"run{j % 2}" for j in range(30)]
    data, batch_file = tmp_path / "mouse_Rand7_data.csv", tmp_path / "mouse_Rand7_batches.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    pd.DataFrame({"Cell": cells, "Batch": batch}).to_csv(batch_file)
    out = rp.harmony_file(data, batch_file, normalize="lognorm", save_path=tmp_path / "res", theta=1.0)
    h = rp.harmony(counts, batch, genes=genes, normalize="lognorm", index=cells, theta=1.0, k=None)
    assert list(out.columns) == ["cell"] + [f"h{j + 1}" for j in range(h.coords.shape[1])] and out["cell"].tolist() == cells
    np.testing.assert_array_equal(_u32(out.iloc[:, 1:].to_numpy(np.float32)), _u32(h.coords))
    written = pd.read_csv(tmp_path / "res" / "mouse_Rand_harmony.csv")
    assert written["cell"].tolist() == cells and written.shape == out.shape
    with pytest.raises(ValueError, match="cell order"):
        pd.DataFrame({"Cell": cells[::-1], "Batch": batch}).to_csv(batch_file)
        rp.harmony_file(data, batch_file, normalize="lognorm")


def test_refusals(tmp_path):
    root, G = _random_bundle(tmp_path, 1, hidden=12, seed=1)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    counts, genes = _counts(rp, G, n=8)
    kw = dict(genes=genes, normalize="lognorm")
    two = np.arange(8) % 2
    with pytest.raises(ValueError, match="65 batches"):
        rp.harmony(counts, two, n_batches=65, **kw)
    with pytest.raises(ValueError, match="-1 is not taken"):
        rp.harmony(counts, np.where(np.arange(8) == 3, -1, two), n_batches=2, **kw)
    for bad in (two[:7], two.astype(np.float32), two + 1):             # a wrong length, no ids, out of range
        with pytest.raises(ValueError):
            rp.harmony(counts, bad, n_batches=2, **kw)
    with pytest.raises(ValueError):                                    # integer ids need names or their number
        rp.harmony(counts, two, **kw)
    for bad in (dict(space="pca"), dict(k=0), dict(k=65), dict(index=list("abc")), dict(n_clusters=9), dict(sigma=0.0),
                dict(theta=-1.0), dict(n_blocks=65)):
        with pytest.raises(ValueError):
            rp.harmony(counts, two, n_batches=2, **bad, **kw)
    rp.hidden, rp.hidden_padded = 260, 260               # what a wider bundle sets: the refusal comes before any launch
    with pytest.raises(ValueError, match="fused kernels only"):
        rp.harmony(counts, two, n_batches=2, **kw)
