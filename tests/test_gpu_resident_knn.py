"""``ResidentPredictor.embed`` / ``knn`` / ``knn_file`` on the GPU: the embedding is the headless layer chain bit for bit and
reproduces ``classify``'s logits, the graph is the reference's on that embedding, and its lists are ``smooth``'s neighbours."""
import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as F

import scdeepsort_amd as sda
from scdeepsort_amd import api, ops

import knn_reference as R
from test_gpu_resident_doublets import BUNDLE_SEED, _counts
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
B, K = 60, 9


def _agrees(graph, rows: np.ndarray, k: int):
    """``graph`` against the reference run on ``rows``: a position may differ only at a near-tie; the distances within gamma."""
    want, _ = R.knn(rows, k)
    differs = graph.indices != want
    assert not (differs & ~R.near_ties(rows, k)).any()
    listed = graph.indices >= 0
    exact = R.sq_distances(rows, rows)[np.arange(rows.shape[0])[:, None], np.where(listed, graph.indices, 0)]
    err = np.abs(graph.sq_distances.astype(np.float64) - exact)
    assert (err[listed] <= R.gamma(rows.shape[1]) * exact[listed]).all()


@pytest.mark.parametrize("n_layers", [1, 2])
def test_embed_and_knn_end_to_end(tmp_path, monkeypatch, n_layers):
    root, G = _random_bundle(tmp_path, n_layers, hidden=12, seed=BUNDLE_SEED[n_layers])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G)
    assert counts.shape == (B, 302)
    label, prob, logits = rp.classify(counts, genes=genes, normalize="lognorm")
    rowptr, col, raw = rp.align(counts, genes, normalize="lognorm")

    # the hidden space: the layers as classify runs them, every launch headless
    emb = rp.embed(counts, genes=genes, normalize="lognorm")
    assert emb.shape == (B, rp.hidden) and emb.dtype == torch.float32 and emb.is_cuda and (emb >= 0).all()
    h = ops.predict_rows(rowptr, col, raw, rp.tables[0], rp.alpha, rp.biases[0])
    for l in range(1, n_layers):
        h = ops.predict_rows(rowptr, col, raw, rp.tables[l], rp.alpha, rp.biases[l], self_rows=ops.linear_fwd(h, rp.self_weights[l]))
    assert torch.equal(emb, h[:, :rp.hidden])
    # ... and the vector the head reads: every logit within the bound of a float32 dot product of H + 1 terms
    h64, w64, b64 = emb.double().cpu().numpy(), rp.w_head[:, :rp.hidden].double().cpu().numpy(), rp.b_head.double().cpu().numpy()
    n = rp.hidden + 1
    g = n * R.U / (1 - n * R.U)
    bound = g * (np.abs(h64[:, None, :] * w64[None, :, :]).sum(-1) + np.abs(b64)[None, :])
    err = np.abs(h64 @ w64.T + b64 - logits.double().cpu().numpy())
    print(f"layers {n_layers}: largest logit error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()

    # the features space: the model's input features of the aligned batch
    feats = rp.embed(counts, genes=genes, normalize="lognorm", space="features")
    assert feats.shape == (B, rp.gene_feat.shape[1])
    assert torch.equal(feats, sda.CellGeneGraph.cell_features(rowptr, col, raw, rp.gene_feat))
    # a batch over the bundle's own ids gives the same rows
    assert torch.equal(rp.embed((rowptr, col, raw)), emb)

    # the graph: the reference on the embedding, classify's labels
    for space, rows in (("hidden", emb), ("features", feats)):
        graph = rp.knn(counts, k=K, genes=genes, normalize="lognorm", space=space)
        assert isinstance(graph, sda.NeighborGraph) and graph.k == K and graph.space == space and graph.metric == "euclidean"
        assert graph.indices.shape == (B, K) and graph.indices.dtype == np.int64 and graph.sq_distances.dtype == np.float32
        np.testing.assert_array_equal(graph.label, label); np.testing.assert_array_equal(graph.max_prob, prob)
        _agrees(graph, rows.cpu().numpy(), K)
        again = rp.knn(counts, k=K, genes=genes, normalize="lognorm", space=space)
        np.testing.assert_array_equal(again.indices, graph.indices)
        np.testing.assert_array_equal(again.sq_distances.view(np.uint32), graph.sq_distances.view(np.uint32))
    graph = rp.knn(counts, k=K, genes=genes, normalize="lognorm")
    assert (graph.indices >= 0).all() and (graph.indices != np.arange(B)[:, None]).all() and len(graph.frame()) == B
    assert f"{B} cells" in str(graph.summary())

    # cosine: the Euclidean graph of the normalised rows, bit for bit
    cos = rp.knn(counts, k=K, genes=genes, normalize="lognorm", metric="cosine")
    idx, d2 = ops.knn_rows(F.normalize(emb, dim=1), K)
    np.testing.assert_array_equal(cos.indices, idx.cpu().numpy())
    np.testing.assert_array_equal(cos.sq_distances.view(np.uint32), d2.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(cos.distances(), cos.sq_distances / np.float32(2))

    # the lists are smooth's neighbours as they come
    sm = rp.smooth(counts, genes, graph.indices, normalize="lognorm")
    plain = rp.smooth(counts, genes, np.array(graph.indices.tolist()), normalize="lognorm")
    assert torch.equal(sm.logits, plain.logits)
    for name in ("smooth_label", "smooth_prob", "n_neighbors", "n_reads", "hood_ptr", "members"):
        np.testing.assert_array_equal(getattr(sm, name), getattr(plain, name), err_msg=name)
    assert (sm.n_neighbors == K).all()

    # chunked and unchunked: the same bits.  The embedding of a deeper model runs 7 cells per launch; the search would be cut
    # over query ranges if it kept partial lists (a batch of one candidate tile is scanned in one range and keeps none:
    # tests/test_gpu_knn_rows.py chunks the op)
    monkeypatch.setattr(api, "STABILITY_CHUNK_BYTES", rp.hidden_padded * 4 * 3 * 7)
    monkeypatch.setattr(ops, "KNN_WORKSPACE_BYTES", 8 * K * 11)
    assert torch.equal(rp.embed(counts, genes=genes, normalize="lognorm"), emb)
    chunked = rp.knn(counts, k=K, genes=genes, normalize="lognorm")
    np.testing.assert_array_equal(chunked.indices, graph.indices)
    np.testing.assert_array_equal(chunked.sq_distances.view(np.uint32), graph.sq_distances.view(np.uint32))


def test_knn_file_feeds_smooth_file(tmp_path):
    root, G = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=30, seed=1)
    cells = [f"C{j}" for j in range(30)]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    out = rp.knn_file(data, k=5, normalize="lognorm", save_path=tmp_path / "res")
    graph = rp.knn(counts, k=5, genes=genes, normalize="lognorm", index=cells)
    assert list(out.columns) == ["cell"] + [f"n{j}" for j in range(5)] and out["cell"].tolist() == cells
    assert out.iloc[:, 1:].values.tolist() == [[cells[j] for j in row] for row in graph.indices]
    smoothed = rp.smooth_file(data, tmp_path / "res" / "mouse_Rand_neighbors.csv")
    pd.testing.assert_frame_equal(smoothed, rp.smooth(counts, genes, graph.indices, normalize="lognorm", index=cells).frame())


def test_a_hidden_width_above_256_is_refused(tmp_path):
    root, G = _random_bundle(tmp_path, 1, hidden=12, seed=1)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    counts, genes = _counts(rp, G, n=8)
    rp.hidden, rp.hidden_padded = 260, 260               # what a wider bundle sets: the refusal comes before any launch
    for call in (lambda: rp.embed(counts, genes=genes, normalize="lognorm"), lambda: rp.knn(counts, k=3, genes=genes, normalize="lognorm"),
                 lambda: rp.embed(counts, genes=genes, normalize="lognorm", space="features")):
        with pytest.raises(ValueError, match="fused kernels only"):
            call()
