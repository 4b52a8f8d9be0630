"""``ResidentPredictor.diffmap`` / ``dpt`` and their ``*_file`` methods on the GPU: the tables are the ops composed by hand on
``knn``'s own lists - and the numpy restatement (tests/diffusion_reference.py) on the same graph - bit for bit, with ``classify``'s
calls beside them; the root in its forms, graph and map reuse, a cell outside the component, the hand-over to ``umap`` and
``paga``, the file round trips and the argument errors."""
import numpy as np
import pandas as pd
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import ops

import diffusion_reference as R
from test_gpu_resident_doublets import BUNDLE_SEED, _counts
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
B, KNN = 60, 6


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _by_hand(rp, graph, n_comps, n_steps=None, seed=0):
    """``diffmap``'s composition from ``knn``'s lists on: ``(coords, eigenvalues, residual, mask, run, fuzzy)``."""
    dev = rp.device
    fuzzy = ops.fuzzy_graph(torch.from_numpy(graph.indices).to(dev), torch.from_numpy(graph.sq_distances).to(dev))
    lowest = ops.graph_components(fuzzy.rowptr, fuzzy.col)
    size = torch.bincount(lowest, minlength=len(lowest))
    mask = lowest == int(torch.nonzero(size == size.max())[0, 0])
    op = ops.diffusion_operator(fuzzy.rowptr, fuzzy.col, fuzzy.w)
    run = ops.lanczos_graph(fuzzy.rowptr, fuzzy.col, op.t, op.z, mask, n_steps=n_steps, seed=seed)
    theta, S, res = ops.lanczos_ritz(run.alpha, run.beta, run.n_run)
    n_found = min(n_comps, run.n_run + 1)
    coords = ops.basis_combine(run.V, S[:, :n_found - 1]).cpu().numpy()
    coords[~mask.cpu().numpy()] = np.nan
    return coords, np.concatenate([[1.0], theta[:n_found - 1]]), np.concatenate([[0.0], res[:n_found - 1]]), mask.cpu().numpy(), run, fuzzy


@pytest.mark.parametrize("n_layers", [1, 2])
def test_diffmap_and_dpt_end_to_end(tmp_path, n_layers):
    root, n_genes = _random_bundle(tmp_path, n_layers, hidden=12, seed=BUNDLE_SEED[n_layers])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, n_genes)
    assert counts.shape[0] == B
    label, prob, _ = rp.classify(counts, genes=genes, normalize="lognorm")
    kw = dict(genes=genes, normalize="lognorm")

    for space, metric, n_comps, n_steps in (("hidden", "euclidean", 8, None), ("features", "cosine", 5, 20)):
        graph = rp.knn(counts, k=KNN, space=space, metric=metric, **kw)
        dm = rp.diffmap(counts, n_comps=n_comps, k=KNN, space=space, metric=metric, n_steps=n_steps, **kw)
        assert isinstance(dm, sda.DiffusionMap) and (dm.space, dm.metric, dm.k, dm.seed) == (space, metric, KNN, 0)
        coords, lam, res, mask, run, fuzzy = _by_hand(rp, graph, n_comps, n_steps)
        np.testing.assert_array_equal(_u64(dm.coords), _u64(coords))
        np.testing.assert_array_equal(_u64(dm.eigenvalues), _u64(lam)); np.testing.assert_array_equal(_u64(dm.residual), _u64(res))
        np.testing.assert_array_equal(dm.in_component, mask)
        assert (dm.n_steps, dm.breakdown, dm.n_found) == (run.n_run, run.breakdown, coords.shape[1]) and dm.n_found == n_comps
        assert dm.coords.dtype == np.float64 and dm.eigenvalues[0] == 1.0 and dm.residual[0] == 0.0 and (np.diff(dm.eigenvalues) <= 0).all()
        assert dm.converged == bool((dm.residual <= 1e-8).all())
        np.testing.assert_array_equal(dm.label, label); np.testing.assert_array_equal(dm.max_prob, prob)
        # the numpy restatement on the device's own graph
        ref = R.diffmap(fuzzy.rowptr.cpu().numpy(), fuzzy.col.cpu().numpy(), fuzzy.w.cpu().numpy(), n_comps, run.V.shape[0] - 1)
        np.testing.assert_array_equal(_u64(dm.coords[mask]), _u64(ref.Y[mask]))
        np.testing.assert_array_equal(_u64(dm.eigenvalues), _u64(ref.eigenvalues))
        assert ref.n_components == dm.n_components and np.array_equal(ref.mask, mask)
        # unit eigenvectors of the operator, up to the reported residual
        np.testing.assert_allclose(np.linalg.norm(dm.coords[mask], axis=0), 1.0, atol=1e-12)
        # graph= skips the search and brings its own k, space and metric; two calls give the same bits
        given = rp.diffmap(counts, n_comps=n_comps, graph=graph, n_steps=n_steps, **kw)
        np.testing.assert_array_equal(_u64(given.coords), _u64(dm.coords))
        assert (given.space, given.metric, given.k) == (space, metric, KNN)
        again = rp.diffmap(counts, n_comps=n_comps, k=KNN, space=space, metric=metric, n_steps=n_steps, **kw)
        np.testing.assert_array_equal(_u64(again.coords), _u64(dm.coords))
        other = rp.diffmap(counts, n_comps=n_comps, graph=graph, n_steps=n_steps, seed=3, **kw)
        assert other.seed == 3 and not np.array_equal(_u64(other.coords), _u64(dm.coords))

    # dpt: the distance is ops.diffusion_distance on the map, and the map is reused or made
    cells = [f"C{j}" for j in range(B)]
    graph = rp.knn(counts, k=KNN, **kw)
    dm = rp.diffmap(counts, n_comps=8, graph=graph, index=cells, **kw)
    inside = np.flatnonzero(dm.in_component)
    r0 = int(inside[0])
    full = rp.dpt(counts, r0, n_dcs=6, n_comps=8, graph=graph, index=cells, **kw)
    reused = rp.dpt(counts, r0, n_dcs=6, diffmap=dm)
    assert isinstance(full, sda.DiffusionPseudotime) and (full.n_dcs, full.roots.tolist()) == (6, [r0])
    np.testing.assert_array_equal(_u64(full.distance), _u64(reused.distance))
    np.testing.assert_array_equal(_u64(full.pseudotime), _u64(reused.pseudotime))
    assert list(reused.index) == cells
    np.testing.assert_array_equal(full.label, label); np.testing.assert_array_equal(full.max_prob, prob)
    g = R.diffusion_weights(dm.eigenvalues[:6])
    want = ops.diffusion_distance(torch.from_numpy(dm.coords[:, :6].copy()).to(rp.device), g, r0).cpu().numpy()
    np.testing.assert_array_equal(_u64(full.distance), _u64(want))
    np.testing.assert_array_equal(_u64(full.distance), _u64(R.diffusion_distance(dm.coords[:, :6], g, r0)))
    on = dm.in_component
    assert full.distance[r0] == 0 and np.isfinite(full.distance[on]).all() and np.isnan(full.distance[~on]).all()
    assert np.nanmax(full.pseudotime) == 1.0 and np.isnan(full.pseudotime[~on]).all() and full.pseudotime.dtype == np.float64
    # the root in its forms
    for root_arg in (np.int64(r0), [r0], (r0, r0), np.array([r0]), torch.tensor([r0]), f"C{r0}"):
        other = rp.dpt(counts, root_arg, n_dcs=6, diffmap=dm, index=cells)
        np.testing.assert_array_equal(_u64(other.distance), _u64(full.distance))
    r1 = int(inside[-1])
    two = rp.dpt(counts, [r1, r0], n_dcs=6, diffmap=dm)
    assert two.roots.tolist() == [r0, r1] and (two.distance[on] <= full.distance[on]).all() and two.distance[r1] == 0
    called = int(label[on & (label >= 0)][0])
    own = np.flatnonzero(label == called)
    best = int(own[np.argmax(prob[own])])
    if dm.in_component[best]:
        typed = rp.dpt(counts, {"type": rp.id2label[called]}, n_dcs=6, diffmap=dm)
        assert typed.roots.tolist() == [best] and typed.distance[best] == 0
    for bad in ({"type": "NoSuchType"}, {"kind": "x"}, "nobody", -1, B, [], 0.5):
        with pytest.raises(ValueError):
            rp.dpt(counts, bad, n_dcs=6, diffmap=dm, index=cells)
    with pytest.raises(ValueError):
        rp.dpt(counts, f"C{r0}", n_dcs=6, diffmap=dm)                    # a name needs index=
    for n_dcs in (1, dm.n_found + 1):
        with pytest.raises(ValueError, match="n_dcs"):
            rp.dpt(counts, r0, n_dcs=n_dcs, diffmap=dm)
    with pytest.raises(ValueError, match="DiffusionMap of this batch"):
        rp.dpt(counts[:-1], r0, n_dcs=6, diffmap=dm)

    # the tables
    frame = full.frame()
    assert list(frame.columns) == ["index", "pseudotime", "distance", "label", "max_prob"] and frame["index"].tolist() == cells
    types = full.by_type()
    assert list(types.columns) == ["cell_type", "n_cells", "median", "min", "max"] and (np.diff(types["median"]) >= 0).all()
    assert types["n_cells"].sum() == ((label >= 0) & on).sum()
    assert list(full.by_group(np.arange(B) % 3).columns) == ["group", "n_cells", "median", "min", "max"]
    assert list(full.pseudotime_frame().columns) == ["cell", "pseudotime"]
    assert f"{B} cells ordered by diffusion distance" in str(full.summary()) and full.summary()["n_ordered"] == on.sum()
    assert list(dm.frame().columns) == ["index", "in_component"] + [f"dc{c}" for c in range(1, 8)] + ["label", "max_prob"]
    assert list(dm.coords_frame().columns) == ["cell"] + [f"dc{c}" for c in range(1, 8)]
    assert list(dm.by_type().columns) == ["cell_type", "n_cells"] + [f"dc{c}" for c in range(1, 8)]
    assert dm.by_type()["n_cells"].sum() == on.sum()
    assert f"{B} cells" in str(dm.summary()) and dm.summary()["n_found"] == 8 and dm.summary()["n_in_component"] == on.sum()

    # the hand-over: a spectral start for umap, a direction for paga
    start = dm.spectral_init()
    assert start.dtype == np.float32 and start.shape == (B, 2) and np.abs(start).max() == np.float32(10.0) and (start[~on] == 0).all()
    scale = 10.0 / np.abs(dm.coords[on][:, 1:3]).max()
    np.testing.assert_array_equal(start[on], (dm.coords[on][:, 1:3] * scale).astype(np.float32))
    layout = rp.umap(counts, graph=graph, init=start, n_epochs=5, a=1.577, b=0.895, **kw)
    assert layout.init == "array" and np.isfinite(layout.coords).all()
    directed = rp.paga(counts, graph=graph, **kw).directed(full)
    assert {"median_a", "median_b"} <= set(directed.columns) and (directed["median_a"].fillna(0) <= directed["median_b"].fillna(1)).all()


def test_a_nan_row_and_other_components_fall_outside(tmp_path):
    root, n_genes = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, n_genes)
    kw = dict(genes=genes, normalize="lognorm")
    emb = rp.embed(counts, **kw).clone()
    emb[5] = float("nan")
    idx, d2 = ops.knn_rows(emb, KNN)                                     # knn lists a NaN row nowhere, and nobody for it
    graph = rp.knn(counts, k=KNN, **kw)
    graph.indices, graph.sq_distances = idx.cpu().numpy().astype(np.int64), d2.cpu().numpy()
    dm = rp.diffmap(counts, n_comps=4, graph=graph, **kw)
    assert not dm.in_component[5] and np.isnan(dm.coords[5]).all() and np.isfinite(dm.coords[dm.in_component]).all()
    assert dm.n_components >= 2 and dm.summary()["n_outside"] == (~dm.in_component).sum() >= 1
    assert (dm.spectral_init()[5] == 0).all()
    inside = int(np.flatnonzero(dm.in_component)[0])
    out = rp.dpt(counts, inside, n_dcs=4, diffmap=dm)
    assert np.isnan(out.distance[5]) and np.isnan(out.pseudotime[5]) and np.nanmax(out.pseudotime) == 1.0
    with pytest.raises(ValueError, match="outside the component"):
        rp.dpt(counts, 5, n_dcs=4, diffmap=dm)
    with pytest.raises(ValueError, match="outside the component"):
        rp.dpt(counts, [inside, 5], n_dcs=4, diffmap=dm)
    # k = 1 leaves many small components: fewer diffusion components than asked for are reported, not raised
    small = rp.diffmap(counts, n_comps=15, k=1, **kw)
    n_c = int(small.in_component.sum())
    assert small.n_components > 1 and 2 <= small.n_found == min(15, small.n_steps + 1) <= n_c and small.breakdown
    assert np.isfinite(small.coords[small.in_component]).all() and small.eigenvalues.shape == small.residual.shape == (small.n_found,)
    with pytest.raises(ValueError, match="n_dcs"):
        rp.dpt(counts, int(np.flatnonzero(small.in_component)[0]), n_dcs=small.n_found + 1, diffmap=small)


def test_diffmap_and_dpt_file_round_trips(tmp_path):
    root, n_genes = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, n_genes, n=30, seed=1)
    cells = [f"C{j}" for j in range(30)]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    kw = dict(genes=genes, normalize="lognorm", index=cells)
    dm = rp.diffmap(counts, n_comps=4, k=5, **kw)
    out = rp.diffmap_file(data, n_comps=4, k=5, normalize="lognorm", save_path=tmp_path / "res")
    assert list(out.columns) == ["cell", "dc1", "dc2", "dc3"] and out["cell"].tolist() == cells
    np.testing.assert_array_equal(_u64(out[["dc1", "dc2", "dc3"]].to_numpy()), _u64(dm.coords[:, 1:]))
    written = pd.read_csv(tmp_path / "res" / "mouse_Rand_diffmap.csv", float_precision="round_trip")
    assert list(written.columns) == ["cell", "dc1", "dc2", "dc3"] and written["cell"].tolist() == cells
    np.testing.assert_array_equal(_u64(written[["dc1", "dc2", "dc3"]].to_numpy()), _u64(dm.coords[:, 1:]))
    inside = int(np.flatnonzero(dm.in_component)[0])
    table = rp.dpt(counts, inside, n_dcs=4, diffmap=dm)
    out = rp.dpt_file(data, f"C{inside}", n_dcs=4, n_comps=4, k=5, normalize="lognorm", save_path=tmp_path / "res")
    assert list(out.columns) == ["cell", "pseudotime"] and out["cell"].tolist() == cells
    np.testing.assert_array_equal(_u64(out["pseudotime"].to_numpy()), _u64(table.pseudotime))
    written = pd.read_csv(tmp_path / "res" / "mouse_Rand_dpt.csv", float_precision="round_trip")
    assert list(written.columns) == ["cell", "pseudotime"]
    np.testing.assert_array_equal(_u64(written["pseudotime"].to_numpy()), _u64(table.pseudotime))
    # a cell outside the component is written empty, not refused: k = 1 leaves several components
    lone = rp.diffmap(counts, n_comps=2, k=1, **kw)
    first = int(np.flatnonzero(lone.in_component)[0])
    out = rp.dpt_file(data, first, n_dcs=2, n_comps=2, k=1, normalize="lognorm", save_path=tmp_path / "res1")
    assert out["pseudotime"].isna().sum() == (~lone.in_component).sum() > 0
    text = (tmp_path / "res1" / "mouse_Rand_dpt.csv").read_text().splitlines()
    assert sum(line.endswith(",") for line in text[1:]) == int(out["pseudotime"].isna().sum())


def test_diffmap_argument_errors(tmp_path):
    root, n_genes = _random_bundle(tmp_path, 1, hidden=12, seed=1)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    counts, genes = _counts(rp, n_genes, n=8)
    kw = dict(genes=genes, normalize="lognorm")
    graph = rp.knn(counts, k=3, **kw)
    short = rp.knn(counts[:7], k=3, **kw)
    for bad in (dict(k=0), dict(k=65), dict(space="pca"), dict(metric="manhattan"), dict(index=["a"]), dict(n_comps=1), dict(n_comps=65),
                dict(n_steps=0), dict(n_steps=1025), dict(seed=-1), dict(seed=2 ** 32), dict(tol=-1.0), dict(tol=float("nan")),
                dict(graph=graph.indices), dict(graph=np.zeros((8, 3), np.int64)), dict(graph=short)):
        with pytest.raises(ValueError):
            rp.diffmap(counts, **bad, **kw)
        with pytest.raises(ValueError):
            rp.dpt(counts, 0, n_dcs=2, **bad, **kw)
    with pytest.raises(ValueError, match="distances"):
        rp.diffmap(counts, graph=graph.indices, **kw)                   # a bare index array carries none
    rp.hidden, rp.hidden_padded = 260, 260               # what a wider bundle sets: the refusal comes before any launch
    with pytest.raises(ValueError, match="diffmap runs on the fused kernels only"):
        rp.diffmap(counts, **kw)
