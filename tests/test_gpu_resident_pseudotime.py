"""``ResidentPredictor.pseudotime`` / ``pseudotime_file`` on the GPU: the table is ``ops.geodesic_rows`` on ``ops.distance_graph`` of
``knn``'s own lists, with ``classify``'s calls beside it; the root in all four forms, graph reuse, a cell that is not reached,
the file round trip and the argument errors."""
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


def _same(table, rows_run, roots):
    np.testing.assert_array_equal(table.distance.view(np.uint32), rows_run.dist.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(table.pred, rows_run.pred.cpu().numpy())
    assert table.distance.dtype == np.float32 and table.pred.dtype == np.int64 and table.pseudotime.dtype == np.float64
    assert (table.rounds, table.converged, table.reached) == (rows_run.rounds, rows_run.converged, rows_run.reached)
    assert table.root.tolist() == sorted(set(roots))
    d = table.distance.astype(np.float64)
    fin = np.isfinite(d)
    np.testing.assert_array_equal(table.pseudotime[fin], d[fin] / d[fin].max())
    assert np.isnan(table.pseudotime[~fin]).all() and table.reached == fin.sum()


@pytest.mark.parametrize("n_layers", [1, 2])
def test_pseudotime_end_to_end(tmp_path, n_layers):
    root, n_genes = _random_bundle(tmp_path, n_layers, hidden=12, seed=BUNDLE_SEED[n_layers])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, n_genes)
    assert counts.shape[0] == B
    label, prob, _ = rp.classify(counts, genes=genes, normalize="lognorm")
    kw = dict(genes=genes, normalize="lognorm")
    dev = rp.device

    for space, metric, roots in (("hidden", "euclidean", [0]), ("features", "euclidean", [3, 40]), ("hidden", "cosine", [59])):
        graph = rp.knn(counts, k=KNN, space=space, metric=metric, **kw)
        out = rp.pseudotime(counts, roots if len(roots) > 1 else roots[0], k=KNN, space=space, metric=metric, **kw)
        assert isinstance(out, sda.Pseudotime) and (out.space, out.metric, out.k) == (space, metric, KNN)
        # ops by hand on knn()'s own graph, and the restatement on the same lists
        lengths = ops.distance_graph(torch.from_numpy(graph.indices).to(dev), torch.from_numpy(graph.sq_distances).to(dev))
        want = ops.geodesic_rows(*lengths, roots)
        _same(out, want, roots)
        ref = G.geodesic_rows(*G.distance_graph(graph.indices, graph.sq_distances), roots)
        np.testing.assert_array_equal(out.distance.view(np.uint32), ref.dist.view(np.uint32))
        np.testing.assert_array_equal(out.pred, ref.pred)
        assert (out.rounds, out.converged, out.reached) == (ref.rounds, True, ref.reached)
        np.testing.assert_array_equal(out.label, label); np.testing.assert_array_equal(out.max_prob, prob)
        # graph= skips the search and brings its own k, space and metric
        given = rp.pseudotime(counts, roots, graph=graph, **kw)
        _same(given, want, roots)
        assert (given.space, given.metric, given.k) == (space, metric, KNN)
        _same(rp.pseudotime(counts, roots, k=KNN, space=space, metric=metric, **kw), want, roots)      # two calls, the same bits
        np.testing.assert_array_equal(out.hops(), G.hops(ref.pred, ref.dist))

    # the root in its four forms
    cells = [f"C{j}" for j in range(B)]
    graph = rp.knn(counts, k=KNN, **kw)
    by_position = rp.pseudotime(counts, 7, graph=graph, index=cells, **kw)
    for root_arg in (np.int64(7), [7], (7, 7), np.array([7]), torch.tensor([7]), "C7"):
        other = rp.pseudotime(counts, root_arg, graph=graph, index=cells, **kw)
        np.testing.assert_array_equal(other.distance, by_position.distance)
        assert other.root.tolist() == [7]
    called = int(label[label >= 0][0])
    own = np.flatnonzero(label == called)
    best = int(own[np.argmax(prob[own])])                               # the first of equal maxima: the lowest position
    typed = rp.pseudotime(counts, {"type": rp.id2label[called]}, graph=graph, **kw)
    assert typed.root.tolist() == [best] and typed.distance[best] == 0
    np.testing.assert_array_equal(typed.distance, rp.pseudotime(counts, best, graph=graph, **kw).distance)
    absent = [t for i, t in enumerate(rp.id2label) if not (label == i).any()]
    for bad in ({"type": "NoSuchType"}, {"kind": "x"}, "C7", "nobody") + (({"type": absent[0]},) if absent else ()):
        with pytest.raises(ValueError):
            rp.pseudotime(counts, bad, graph=graph, **kw)                # a name needs index=
    with pytest.raises(ValueError):
        rp.pseudotime(counts, "nobody", graph=graph, index=cells, **kw)

    # max_rounds
    cut = rp.pseudotime(counts, 7, graph=graph, max_rounds=1, **kw)
    assert (cut.rounds, cut.converged) == (1, False) and cut.reached == 1 + len(set(np.flatnonzero(cut.pred == 7)))
    # the table
    out = by_position
    frame = out.frame()
    assert list(frame.columns) == ["index", "pseudotime", "distance", "pred", "label", "max_prob"] and frame["index"].tolist() == cells
    types = out.by_type()
    assert list(types.columns) == ["cell_type", "n_cells", "median", "min", "max"] and (np.diff(types["median"]) >= 0).all()
    assert types["n_cells"].sum() == ((label >= 0) & np.isfinite(out.distance)).sum()
    far = int(np.nanargmax(out.pseudotime))
    path = out.path(far)
    assert path[0] == 7 and path[-1] == far and len(path) == out.hops()[far] + 1 and out.pseudotime[far] == 1.0
    assert f"{B} cells ordered by geodesic distance" in str(out.summary()) and out.summary()["rounds"] == out.rounds


def test_a_nan_row_is_not_reached(tmp_path):
    root, n_genes = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, n_genes)
    kw = dict(genes=genes, normalize="lognorm")
    emb = rp.embed(counts, **kw).clone()
    emb[5] = float("nan")
    idx, d2 = ops.knn_rows(emb, KNN)                                     # knn lists a NaN row nowhere, and nobody for it
    assert (idx[5] == -1).all() and not (idx == 5).any()
    graph = rp.knn(counts, k=KNN, **kw)
    graph.indices, graph.sq_distances = idx.cpu().numpy().astype(np.int64), d2.cpu().numpy()
    out = rp.pseudotime(counts, 0, graph=graph, **kw)
    assert np.isinf(out.distance[5]) and np.isnan(out.pseudotime[5]) and out.pred[5] == -1 and out.hops()[5] == -1
    assert out.converged and out.reached == int(np.isfinite(out.distance).sum()) <= B - 1 and len(out.path(5)) == 0
    assert np.nanmax(out.pseudotime) == 1.0 and out.summary()["n_unreached"] == B - out.reached


def test_pseudotime_file_round_trip(tmp_path):
    root, n_genes = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, n_genes, n=30, seed=1)
    cells = [f"C{j}" for j in range(30)]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    out = rp.pseudotime_file(data, "C4", k=5, normalize="lognorm", save_path=tmp_path / "res")
    table = rp.pseudotime(counts, 4, k=5, genes=genes, normalize="lognorm", index=cells)
    assert list(out.columns) == ["cell", "pseudotime"] and out["cell"].tolist() == cells
    np.testing.assert_array_equal(out["pseudotime"].to_numpy(), table.pseudotime)
    written = pd.read_csv(tmp_path / "res" / "mouse_Rand_pseudotime.csv", float_precision="round_trip")
    assert list(written.columns) == ["cell", "pseudotime"] and written["cell"].tolist() == cells
    np.testing.assert_array_equal(written["pseudotime"].to_numpy(), table.pseudotime)
    # a cell that is not reached is written empty, not refused: k = 1 leaves several components
    lone = rp.pseudotime_file(data, 4, k=1, normalize="lognorm", save_path=tmp_path / "res1")
    assert lone["pseudotime"].isna().any()
    text = (tmp_path / "res1" / "mouse_Rand_pseudotime.csv").read_text().splitlines()
    assert sum(line.endswith(",") for line in text[1:]) == int(lone["pseudotime"].isna().sum())


def test_pseudotime_argument_errors(tmp_path):
    root, n_genes = _random_bundle(tmp_path, 1, hidden=12, seed=1)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    counts, genes = _counts(rp, n_genes, n=8)
    kw = dict(genes=genes, normalize="lognorm")
    graph = rp.knn(counts, k=3, **kw)
    short = rp.knn(counts[:7], k=3, **kw)
    for bad in (dict(k=0), dict(k=65), dict(space="pca"), dict(metric="manhattan"), dict(index=["a"]), dict(max_rounds=-1),
                dict(graph=graph.indices), dict(graph=np.zeros((8, 3), np.int64)), dict(graph=short)):
        with pytest.raises(ValueError):
            rp.pseudotime(counts, 0, **bad, **kw)
    for bad_root in (-1, 8, [0, 8], [], 0.5, [0.5], None, np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            rp.pseudotime(counts, bad_root, graph=graph, **kw)
    rp.hidden, rp.hidden_padded = 260, 260               # what a wider bundle sets: the refusal comes before any launch
    with pytest.raises(ValueError, match="pseudotime runs on the fused kernels only"):
        rp.pseudotime(counts, 0, **kw)
