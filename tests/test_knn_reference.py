"""CPU checks of the k-nearest-neighbour graph: the fp64 reference (tests/knn_reference.py) on a hand-made case, the exact ties
and the near-tie budget of the fixtures the GPU tests use, ``NeighborGraph``'s host methods, and the host logic of
``ResidentPredictor.knn`` / ``knn_file`` with ``ops.knn_rows`` replaced by the reference."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import api, ops, tables

import knn_reference as R


def test_reference_on_five_points():
    x = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 2, 0, 0], [1, 0, 0, 0], [0, 0, 0, 3]], np.float32)
    idx, d2 = R.knn(x, 3)
    np.testing.assert_array_equal(idx, [[1, 3, 2], [3, 0, 2], [0, 1, 3], [1, 0, 2], [0, 1, 3]])      # ties: the lower index
    np.testing.assert_array_equal(d2, [[1, 1, 4], [0, 1, 5], [4, 5, 5], [0, 1, 5], [9, 10, 10]])
    idx, d2 = R.knn(x, 6)                                              # four candidates: the tail
    assert (idx[:, 4:] == -1).all() and np.isinf(d2[:, 4:]).all() and (idx[:, :4] >= 0).all()
    idx, d2 = R.knn(x, 2, self_offset=None)                            # nothing left out: the cell first, then its duplicate
    np.testing.assert_array_equal(idx, [[0, 1], [1, 3], [2, 0], [1, 3], [4, 0]])
    np.testing.assert_array_equal(d2[:, 0], 0)
    idx, d2 = R.knn(x, 2, queries=x[2:4], self_offset=2)               # a sub-range of the rows as queries
    np.testing.assert_array_equal(idx, [[0, 1], [1, 0]])
    far = np.array([[5, 0, 0, 0]], np.float32)
    np.testing.assert_array_equal(R.knn(x, 2, queries=far, self_offset=None)[0], [[1, 3]])
    bad = x.copy(); bad[1, 2] = np.nan
    idx, d2 = R.knn(bad, 4)
    assert not (idx == 1).any() and idx[1].tolist() == [-1] * 4 and idx[0].tolist() == [3, 2, 4, -1]
    assert R.gamma(256) == pytest.approx(259 * 2.0 ** -24, rel=1e-4)


@pytest.mark.parametrize("D", R.LATTICE_DIMS)
def test_lattice_fixture_is_exact_in_float32_and_has_ties(D):
    x = R.lattice(D)
    assert x.shape == (R.LATTICE_N, D) and np.abs(x).max() <= 4 and (x * 8 == np.round(x * 8)).all()
    assert (x[50] == x[7]).all() and (x[120] == x[7]).all() and (x[121] == x[8]).all()
    d = R.sq_distances(x, x)
    units = d * 64
    assert (units == np.round(units)).all() and units.max() < 2 ** 18          # every partial f32 sum is exact, in any order
    idx, d2 = R.reference("lattice", 16, D)
    assert d2[7, 0] == d2[7, 1] == 0 and idx[7, :2].tolist() == [50, 120] and idx[50, :2].tolist() == [7, 120]
    tied = (np.diff(d2, axis=1) == 0).any(axis=1)
    print(f"D={D}: {int(tied.sum())} rows with an exact tie among their first 16 distances, largest distance {int(units.max())} / 64")
    assert tied.sum() >= 5                                             # the five duplicate rows at the least
    if D == 256:
        assert tied.sum() > 5                                          # and ties between distinct rows


@pytest.mark.parametrize("case", R.REAL_CASES)
def test_near_tie_budget_of_the_real_fixtures(case):
    x = R.real(*case)
    near = R.near_ties(x, 15)
    share = near.mean()
    print(f"{case}: near-tie positions {int(near.sum())} of {near.size} = {100 * share:.3f} %")
    assert share <= 0.02


def _graph():
    # 0 <-> 1 mutual, 2 -> 0 one-way, 3 alone, 4 -> (2, 3)
    indices = np.array([[1, 2], [0, -1], [0, 1], [-1, -1], [2, 3]], np.int64)
    d2 = np.array([[1, 4], [1, np.inf], [4, 9], [np.inf, np.inf], [16, 25]], np.float32)
    label = np.array([0, 0, 1, -1, -1], np.int64)
    return tables.NeighborGraph(indices=indices, sq_distances=d2, k=2, space="hidden", metric="euclidean", label=label,
                                max_prob=np.full(5, 0.5, np.float32), index=[f"c{i}" for i in range(5)], id2label=["A", "B"])


def test_neighbor_graph_methods():
    g = _graph()
    assert sda.NeighborGraph is api.NeighborGraph is tables.NeighborGraph and "NeighborGraph" in sda.__all__
    np.testing.assert_array_equal(g.distances(), np.array([[1, 2], [1, np.inf], [2, 3], [np.inf, np.inf], [4, 5]], np.float32))
    m = g.to_scipy()
    assert m.shape == (5, 5) and m.nnz == 7 and m.indptr.tolist() == [0, 2, 3, 5, 5, 7]
    assert m.indices.tolist() == [1, 2, 0, 0, 1, 2, 3] and m.data.tolist() == [1, 2, 1, 2, 3, 4, 5]
    np.testing.assert_array_equal(g.mutual(), [[True, True], [True, False], [True, False], [False, False], [False, False]])
    agree = g.label_agreement()
    np.testing.assert_array_equal(agree[[0, 1, 2, 4]], [0.5, 1.0, 0.0, 0.0])       # unsure neighbours, and an unsure cell's, disagree
    assert np.isnan(agree[3])
    by = g.by_type()
    assert list(by.columns) == ["cell_type", "n_cells", "median_nearest", "median_kth", "mutual", "agreement"]
    assert by["cell_type"].tolist() == ["A", "B", "unsure"] and by["n_cells"].tolist() == [2, 1, 2]
    assert by["median_nearest"].tolist() == [1.0, 2.0, 4.0] and by["median_kth"].tolist() == [1.5, 3.0, 5.0]
    assert by["mutual"].tolist() == [1.0, 0.5, 0.0] and by["agreement"].tolist() == [0.75, 0.0, 0.0]
    f = g.frame()
    assert list(f.columns) == ["index", "cell_type", "prob", "n_neighbors", "nearest", "nearest_distance", "kth_distance", "n_mutual",
                               "label_agreement"]
    assert f["n_neighbors"].tolist() == [2, 1, 2, 0, 2] and f["nearest"].tolist() == ["c1", "c0", "c0", None, "c2"]
    assert f["kth_distance"].tolist()[:3] == [2.0, 1.0, 3.0] and np.isnan(f["kth_distance"][3]) and f["n_mutual"].tolist() == [2, 1, 1, 0, 0]
    s = g.summary()
    assert s["n_cells"] == 5 and s["n_edges"] == 7 and s["n_without"] == 1 and s["mutual_share"] == pytest.approx(4 / 7)
    assert "k = 2" in str(s) and "hidden" in str(s)
    cos = tables.NeighborGraph(**{**g.__dict__, "metric": "cosine"})
    np.testing.assert_array_equal(cos.distances()[0], [0.5, 2.0])                  # 1 - cos = d2 / 2
    # the lists are smooth's `neighbors` as they stand
    ptr, members = api._neighbor_lists(g.indices, 5, include_self=False)
    assert ptr.tolist() == [0, 2, 3, 5, 5, 7] and members.tolist() == [1, 2, 0, 0, 1, 2, 3]


def _fake_predictor(monkeypatch, rows: np.ndarray, n_classes=3, hidden=8):
    """A ResidentPredictor without a GPU: the fields ``knn`` reads, the call and the embedding faked, ``ops.knn_rows`` replaced by
    the reference."""
    B = rows.shape[0]
    rp = api.ResidentPredictor.__new__(api.ResidentPredictor)
    rp.species, rp.tissue, rp.file_type, rp.threshold = "mouse", "Fake", "csv", 0
    rp.device = torch.device("cpu")
    rp.n_layers, rp.n_genes, rp.n_classes, rp.hidden, rp.hidden_padded = 1, 6, n_classes, hidden, hidden
    rp.id2gene = [f"G{i}" for i in range(6)]
    rp.id2label = [f"type{i}" for i in range(n_classes)]
    rp.normalize = None
    rp.bundle = SimpleNamespace(label_map=lambda: None)
    pred = np.arange(B, dtype=np.int64) % n_classes
    pred[0] = -1
    seen = {}

    def fake_knn_rows(x, k, **kw):
        seen["rows"], seen["kw"] = x.clone(), kw
        idx, d2 = R.knn(x.numpy(), k)
        return torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(d2.astype(np.float32))

    def fake_embed(self, csr, space):
        seen["space"] = space
        return torch.from_numpy(rows)

    monkeypatch.setattr(ops, "knn_rows", fake_knn_rows)
    monkeypatch.setattr(api.ResidentPredictor, "_embed", fake_embed)
    monkeypatch.setattr(api.ResidentPredictor, "_classify_on_device",
                        lambda self, expr: (pred, np.full(B, 0.75, np.float32), torch.zeros(B, n_classes), None))
    monkeypatch.setattr(api.ResidentPredictor, "_over_genes", lambda self, expr, genes, normalize: sp.csr_matrix(np.asarray(expr)))
    monkeypatch.setattr(torch.cuda, "device", contextlib.nullcontext)          # the entries' device context, without a device
    return rp, pred, seen


def test_knn_host_logic_with_the_reference_as_kernel(monkeypatch):
    rows = R.real(197, 36, 1)[:40, :8].copy()
    rp, pred, seen = _fake_predictor(monkeypatch, rows)
    X = np.ones((40, 6), np.float32)
    g = rp.knn(X, k=5)
    want_idx, want_d2 = R.knn(rows, 5)
    assert isinstance(g, sda.NeighborGraph) and g.k == 5 and g.space == "hidden" and g.metric == "euclidean"
    assert g.indices.dtype == np.int64 and g.sq_distances.dtype == np.float32 and seen["space"] == "hidden" and seen["kw"] == {}
    np.testing.assert_array_equal(g.indices, want_idx)
    np.testing.assert_array_equal(g.sq_distances, want_d2.astype(np.float32))
    np.testing.assert_array_equal(g.label, pred)
    assert list(g.index) == list(range(40)) and g.id2label == rp.id2label
    assert torch.equal(seen["rows"], torch.from_numpy(rows))
    # cosine: the normalised rows through the same kernel
    c = rp.knn(X, k=5, metric="cosine", space="features", index=[f"c{i}" for i in range(40)])
    unit = torch.nn.functional.normalize(torch.from_numpy(rows), dim=1)
    assert torch.equal(seen["rows"], unit) and seen["space"] == "features" and c.metric == "cosine" and list(c.index)[3] == "c3"
    np.testing.assert_array_equal(c.indices, R.knn(unit.numpy(), 5)[0])
    np.testing.assert_allclose(c.distances(), 1 - (unit.numpy() @ unit.numpy().T)[np.arange(40)[:, None], c.indices], atol=1e-6)
    # fewer cells than k + 1: the tail
    few = rp.knn(X, k=64)
    assert (few.indices[:, 39:] == -1).all() and np.isinf(few.sq_distances[:, 39:]).all() and (few.indices[:, :39] >= 0).all()
    for bad in (dict(k=0), dict(k=65), dict(space="pca"), dict(metric="manhattan"), dict(index=["a"])):
        with pytest.raises(ValueError):
            rp.knn(X, **bad)
    with pytest.raises(ValueError, match="space"):
        rp.embed(X, space="pca")
    rp.hidden, rp.hidden_padded = 300, 300
    for call in (lambda: rp.knn(X), lambda: rp.embed(X)):
        with pytest.raises(ValueError, match="fused kernels only"):
            call()


def test_knn_file_writes_what_smooth_file_reads(monkeypatch, tmp_path):
    rows = R.real(197, 36, 1)[:12, :8].copy()
    rp, _, _ = _fake_predictor(monkeypatch, rows)
    cells = [f"cell{i}" for i in range(12)]
    data = tmp_path / "mouse_Fake7_data.csv"
    pd.DataFrame(np.ones((6, 12), np.float32), index=rp.id2gene, columns=cells).to_csv(data)
    out = rp.knn_file(data, k=4, save_path=tmp_path / "res")
    want = R.knn(rows, 4)[0]
    assert list(out.columns) == ["cell", "n0", "n1", "n2", "n3"] and out["cell"].tolist() == cells
    assert out["n0"].tolist() == [cells[j] for j in want[:, 0]]
    written = tmp_path / "res" / "mouse_Fake_neighbors.csv"
    assert written.exists()
    # a short list: fields left empty
    short = rp.knn_file(data, k=15, save_path=tmp_path / "res15")
    assert (short[["n11", "n14"]] == "").all().all() and (short["n10"] != "").all()
    # smooth_file's reader gives the lists back
    got = {}
    monkeypatch.setattr(api.ResidentPredictor, "smooth", lambda self, counts, genes, neighbors, **kw:
                        got.update(neighbors=neighbors, kw=kw) or SimpleNamespace(frame=lambda: pd.DataFrame({"index": cells})))
    rp.smooth_file(data, written)
    np.testing.assert_array_equal(got["neighbors"], want)
    rp.smooth_file(data, tmp_path / "res15" / "mouse_Fake_neighbors.csv")
    np.testing.assert_array_equal(got["neighbors"], R.knn(rows, 15)[0])
