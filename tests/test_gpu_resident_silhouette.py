"""``ResidentPredictor.silhouette`` / ``silhouette_file`` on the GPU: the figures are ``ops.silhouette_rows``' on the batch's embedding,
bit for bit, with ``classify``'s calls beside them; ``kmeans``' clusters feed it as they come."""
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
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(sil, rows_run):
    """The table's arrays are the op's, bit for bit (NaN bits included: both come from one kernel)."""
    for got, want in ((sil.a, rows_run.a), (sil.b, rows_run.b), (sil.score, rows_run.score)):
        np.testing.assert_array_equal(_bits(got), _bits(want.cpu().numpy()))
    np.testing.assert_array_equal(sil.nearest, rows_run.nearest.cpu().numpy())
    np.testing.assert_array_equal(sil.size, rows_run.size.cpu().numpy())


@pytest.mark.parametrize("n_layers", [1, 2])
def test_silhouette_end_to_end(tmp_path, n_layers):
    root, G = _random_bundle(tmp_path, n_layers, hidden=12, seed=BUNDLE_SEED[n_layers])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G)
    assert counts.shape[0] == B
    label, prob, _ = rp.classify(counts, genes=genes, normalize="lognorm")
    kw = dict(genes=genes, normalize="lognorm")
    dev = rp.device
    ids = np.arange(B) % K
    ids[5] = -1

    for space in ("hidden", "features"):
        emb = rp.embed(counts, space=space, **kw)
        sil = rp.silhouette(counts, groups=ids, n_groups=K, space=space, **kw)
        assert isinstance(sil, sda.Silhouette) and sil.space == space and sil.metric == "euclidean"
        assert sil.score.dtype == np.float64 and sil.score.shape == (B,) and sil.nearest.dtype == np.int64
        _same(sil, ops.silhouette_rows(emb, torch.from_numpy(ids).to(dev), K))
        np.testing.assert_array_equal(sil.label, label); np.testing.assert_array_equal(sil.max_prob, prob)
        np.testing.assert_array_equal(sil.group, ids)
        assert sil.n_skipped == 1 and np.isnan(sil.score[5]) and sil.nearest[5] == -1 and sil.size.sum() == B - 1
        again = rp.silhouette(counts, groups=ids, n_groups=K, space=space, **kw)
        np.testing.assert_array_equal(_bits(again.score), _bits(sil.score))
        # kmeans' clusters as they come
        km = rp.kmeans(counts, K, space=space, seed=1, **kw)
        fed = rp.silhouette(counts, groups=km.cluster, n_groups=K, space=km.space, metric=km.metric, **kw)
        _same(fed, ops.silhouette_rows(emb, torch.from_numpy(km.cluster).to(dev), K))
        np.testing.assert_array_equal(fed.size, km.size)
    emb = rp.embed(counts, **kw)
    cos = rp.silhouette(counts, groups=ids, n_groups=K, metric="cosine", **kw)
    _same(cos, ops.silhouette_rows(F.normalize(emb, dim=1), torch.from_numpy(ids).to(dev), K))
    assert cos.metric == "cosine"

    # the predicted types: unsure cells are skipped; integer ids and names agree
    C = len(rp.id2label)
    assert len(set(label[label >= 0].tolist())) >= 2 and (label < 0).any()       # these bundles call several types and leave cells unsure
    pred = rp.silhouette(counts, **kw)
    assert list(pred.group_names) == list(rp.id2label)
    np.testing.assert_array_equal(pred.group, label)
    assert pred.n_skipped == int((label < 0).sum()) and np.isnan(pred.score[label < 0]).all()
    by_id = rp.silhouette(counts, groups=label, n_groups=C, **kw)
    by_name = rp.silhouette(counts, groups=label, group_names=list(rp.id2label), **kw)
    np.testing.assert_array_equal(_bits(by_id.score), _bits(pred.score))
    np.testing.assert_array_equal(_bits(by_name.score), _bits(pred.score))
    np.testing.assert_array_equal(by_name.nearest, pred.nearest)
    assert list(by_id.group_names) == [str(i) for i in range(C)]

    # the table is consistent with its arrays
    sil = rp.silhouette(counts, groups=ids, group_names=["w", "x", "y", "z"], index=[f"C{j}" for j in range(B)], **kw)
    on = ids >= 0
    assert sil.mean() == float(sil.score[on].mean())
    per = sil.by_group()
    assert per["group"].tolist() == ["w", "x", "y", "z"] and per["n_cells"].tolist() == sil.size.tolist()
    for k in range(K):
        m = ids == k
        assert per["mean"][k] == sil.score[m].mean() and per["median"][k] == np.median(sil.score[m])
        assert per["negative"][k] == (sil.score[m] < 0).mean()
        neg = m & (sil.score < 0)
        want = None if not neg.any() else ["w", "x", "y", "z"][int(np.argmax(np.bincount(sil.nearest[neg], minlength=K)))]
        assert per["nearest"][k] == want or (want is None and per["nearest"][k] is None)
    frame = sil.frame()
    assert len(frame) == B and frame["index"].tolist() == [f"C{j}" for j in range(B)] and frame["group"][5] is None
    assert frame["group"][0] == "w" and frame["nearest"][0] == ["w", "x", "y", "z"][sil.nearest[0]]
    np.testing.assert_array_equal(_bits(frame["score"].to_numpy()), _bits(sil.score))
    for cut in (0.0, 0.5, 2.0):
        bad = sil.misplaced(cut)
        assert len(bad) == int((on & (sil.score < cut)).sum()) and bad["score"].is_monotonic_increasing
        assert (bad["score"] < cut).all() and bad["group"].notna().all()
    assert len(sil.misplaced(2.0)) == B - 1
    summary = sil.summary()
    assert summary["n_cells"] == B - 1 and summary["n_groups"] == K and summary["n_skipped"] == 1 and summary["mean"] == sil.mean()
    assert summary["n_misplaced"] == int((sil.score[on] < 0).sum()) and f"{B - 1} cells in {K} non-empty groups" in str(summary)
    assert summary["worst_mean"] == per["mean"].min() and summary["best_mean"] == per["mean"].max()


def test_silhouette_file(tmp_path):
    root, G = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=30, seed=1)
    cells = [f"C{j}" for j in range(30)]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    rp.kmeans_file(data, K, normalize="lognorm", save_path=tmp_path / "res")
    km = rp.kmeans(counts, K, genes=genes, normalize="lognorm", index=cells)
    assert (km.size > 0).all()                                          # else the file's sorted names would skip a cluster
    out = rp.silhouette_file(data, tmp_path / "res" / "mouse_Rand_kmeans.csv", normalize="lognorm", save_path=tmp_path / "res")
    want = rp.silhouette(counts, groups=km.cluster, group_names=km.cluster_names, genes=genes, normalize="lognorm", index=cells)
    pd.testing.assert_frame_equal(out, want.frame())
    written = pd.read_csv(tmp_path / "res" / "mouse_Rand_silhouette.csv")
    assert written["score"].notna().sum() == 30 and set(written["group"]) == set(km.cluster_names)
    np.testing.assert_allclose(written["score"].to_numpy(), want.score, rtol=1e-12)
    label, _, _ = rp.classify(counts, genes=genes, normalize="lognorm")
    assert len(set(label[label >= 0].tolist())) >= 2 and (label < 0).any()
    typed = rp.silhouette_file(data, normalize="lognorm", space="features")    # without a clusters file: the predicted types
    want = rp.silhouette(counts, genes=genes, normalize="lognorm", space="features", index=cells)
    pd.testing.assert_frame_equal(typed, want.frame())
    assert typed["group"].isna().sum() == int((label < 0).sum()) == want.n_skipped


def test_silhouette_argument_errors(tmp_path):
    root, G = _random_bundle(tmp_path, 1, hidden=12, seed=1)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    counts, genes = _counts(rp, G, n=8)
    kw = dict(genes=genes, normalize="lognorm")
    ids = np.arange(8) % 2
    for bad in (dict(groups=ids, n_groups=2, space="pca"), dict(groups=ids, n_groups=2, metric="manhattan"),
                dict(groups=ids, n_groups=2, index=["a"]), dict(groups=ids), dict(groups=ids, n_groups=1),
                dict(groups=ids[:5], n_groups=2), dict(groups=ids.astype(float), n_groups=2), dict(groups="clusters"),
                dict(groups=ids, n_groups=5000), dict(groups=ids, n_groups=3, group_names=["a", "b"])):
        with pytest.raises(ValueError):
            rp.silhouette(counts, **bad, **kw)
    # fewer than two non-empty groups
    for one in (np.zeros(8, np.int64), np.full(8, -1), np.where(np.arange(8) < 3, 1, -1)):
        with pytest.raises(ValueError, match="two non-empty groups"):
            rp.silhouette(counts, groups=one, n_groups=3, **kw)
    rp.hidden, rp.hidden_padded = 260, 260               # what a wider bundle sets: the refusal comes before any launch
    with pytest.raises(ValueError, match="fused kernels only"):
        rp.silhouette(counts, groups=ids, n_groups=2, **kw)
