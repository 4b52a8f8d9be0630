"""``ResidentPredictor.pseudobulk`` on the GPU: a cluster's call is bit for bit ``classify`` of the host-summed count matrix, the
pooled counts are the host sums, and the form of the operands, ``into=`` and the order of the caller's genes change nothing."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import api

from test_gpu_resident_predict import _random_bundle
from test_gpu_resident_doublets import BUNDLE_SEED, _counts

pytestmark = pytest.mark.gpu
B, K = 60, 7


def _clusters(n=B):
    """One id per cell: clusters 0..5 of uneven size, cluster 6 without cells, three cells skipped."""
    ids = np.random.default_rng(2).integers(0, 6, n)
    ids[[1, 17, 40]] = -1
    return ids


def _host_sums(counts, ids, k=K):
    summed = np.zeros((k, counts.shape[1]), np.float64)
    np.add.at(summed, ids[ids >= 0], counts[ids >= 0].astype(np.float64))
    return summed.astype(np.float32)                                  # small integers: exact


def _same(x: api.Pseudobulk, y: api.Pseudobulk, calls=True):
    assert list(x.names) == list(y.names)
    for name in ("n_cells", "n_reads", "n_genes") + (("label", "max_prob") if calls else ()):
        np.testing.assert_array_equal(getattr(x, name), getattr(y, name), err_msg=name)
    for name in ("rowptr", "col", "val", "cnt") + (("logits",) if calls else ()):
        assert torch.equal(getattr(x, name), getattr(y, name)), name


@pytest.mark.parametrize("n_layers", [1, 2])
def test_pseudobulk_end_to_end(tmp_path, n_layers):
    root, G = _random_bundle(tmp_path, n_layers, hidden=12, seed=BUNDLE_SEED[n_layers])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G)
    ids = _clusters()
    names = [f"c{k}" for k in range(K)]
    pb = rp.pseudobulk(counts, genes, ids, normalize="lognorm", cluster_names=names)
    # the calls: classify of the host-summed [K, n_cols] count matrix, bit for bit
    summed = _host_sums(counts, ids)
    label, prob, logits = rp.classify(summed, genes=genes, normalize="lognorm")
    np.testing.assert_array_equal(pb.label, label); np.testing.assert_array_equal(pb.max_prob, prob)
    assert torch.equal(pb.logits, logits)
    assert pb.label.dtype == np.int64 and pb.max_prob.dtype == np.float32
    np.testing.assert_array_equal(pb.n_reads, summed.sum(axis=1, dtype=np.float64).astype(np.int64))
    np.testing.assert_array_equal(pb.n_cells, np.bincount(ids[ids >= 0], minlength=K))
    assert list(pb.names) == names and pb.n_cells[6] == 0 and pb.n_reads[6] == 0 and pb.n_genes[6] == 0
    # counts(): the host sums restricted to the bundle's genes
    gene_ids = rp.gene_map(genes).cpu().numpy()
    inside = gene_ids >= 0
    want = np.zeros((K, G), np.int64)
    want[:, gene_ids[inside]] = summed[:, inside].astype(np.int64)
    pooled = pb.counts()
    assert pooled.shape == (K, G) and pooled.dtype == np.int64
    np.testing.assert_array_equal(pooled.toarray(), want)
    np.testing.assert_array_equal(pb.n_genes, (want > 0).sum(axis=1))
    assert (pb.n_reads >= want.sum(axis=1)).all() and (pb.n_reads > want.sum(axis=1)).any()        # reads outside the bundle
    # the same from names, a scipy CSR, a gene map made once, n_clusters in place of names
    by_name = rp.pseudobulk(counts, genes, np.asarray([f"c{k}" if k >= 0 else "c6" for k in ids]), normalize="lognorm")
    assert list(by_name.names) == names                              # factorised in sorted order; the skipped cells went to c6
    assert by_name.n_cells[6] == 3
    named = np.asarray([f"c{max(k, 0)}" for k in ids], dtype=object)
    _same(rp.pseudobulk(counts[ids >= 0], genes, named[ids >= 0], normalize="lognorm", cluster_names=names), pb)
    _same(rp.pseudobulk(sp.csr_matrix(counts), rp.gene_map(genes), ids, normalize="lognorm", cluster_names=names), pb)
    numbered = rp.pseudobulk(counts, genes, torch.from_numpy(ids), normalize=api.LogNormalize(), n_clusters=K)
    assert list(numbered.names) == [str(k) for k in range(K)]
    numbered.names = names
    _same(numbered, pb)
    # the caller's genes in another order: the same pooled rows (sorted by bundle id), the same calls
    perm = np.random.default_rng(1).permutation(len(genes))
    shuffled = rp.pseudobulk(counts[:, perm], [genes[j] for j in perm], ids, normalize="lognorm", cluster_names=names)
    _same(shuffled, pb)
    # into: two halves equal the whole, bit for bit
    half = rp.pseudobulk(counts[:B // 2], genes, ids[:B // 2], normalize="lognorm", cluster_names=names)
    assert half.n_cells.sum() < pb.n_cells.sum()
    assert rp.pseudobulk(counts[B // 2:], genes, ids[B // 2:], normalize="lognorm", into=half) is half
    _same(half, pb)
    with pytest.raises(ValueError, match="into"):
        rp.pseudobulk(counts, genes, ids, normalize="lognorm", cluster_names=names[:-1] + ["other"], into=half)
    with pytest.raises(ValueError, match="into"):
        rp.pseudobulk(counts, genes, ids, normalize="lognorm", n_clusters=K - 1, into=half)
    # the tables
    frame = pb.frame()
    assert list(frame.columns) == ["cluster", "n_cells", "n_reads", "n_genes", "cell_type", "cell_subtype", "probability"]
    assert pb.calls()[6] == -2 and frame["cell_type"][6] == "empty" and np.isnan(frame["probability"][6])
    np.testing.assert_array_equal(pb.calls()[:6], label[:6])
    calls = rp.annotate(counts, ids, cluster_names=names, genes=genes, normalize="lognorm")
    both = pb.frame(calls=calls)
    vote, _ = calls.consensus()
    assert both["agrees"].tolist() == (vote == pb.calls()).tolist() and bool(both["agrees"][6]) and "vote_type" in both.columns
    assert f"{K} clusters pooled from {B - 3} cells" in str(pb.summary())


def test_pseudobulk_refusals(tmp_path):
    root, G = _random_bundle(tmp_path, 1, hidden=12, seed=BUNDLE_SEED[1])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=20)
    ids = np.arange(20) % 3
    with pytest.raises(ValueError, match="genes="):
        rp.pseudobulk(counts, None, ids, normalize="lognorm", n_clusters=3)
    with pytest.raises(ValueError, match="normalize"):
        rp.pseudobulk(counts, genes, ids, n_clusters=3)
    doubled = genes[:-1] + [genes[0]]
    merged = rp.gene_map(doubled, duplicates="sum")
    assert isinstance(merged, api.GeneMap)
    with pytest.raises(ValueError, match="merged"):
        rp.pseudobulk(counts, merged, ids, normalize="lognorm", n_clusters=3)
    with pytest.raises(sda.WgnnError, match="cell 3"):
        bad = counts.copy(); bad[3, 0] = 2.5
        rp.pseudobulk(bad, genes, ids, normalize="lognorm", n_clusters=3)
    with pytest.raises(sda.WgnnError, match="cell 4 holds a count above 2\\^23"):
        bad = counts.copy(); bad[4, 1] = 2.0 ** 23 + 1
        rp.pseudobulk(bad, genes, ids, normalize="lognorm", n_clusters=3)
    with pytest.raises(ValueError, match="clusters lists 19 cells"):
        rp.pseudobulk(counts, genes, ids[:19], normalize="lognorm", n_clusters=3)
    with pytest.raises(ValueError, match="out of range"):
        rp.pseudobulk(counts, genes, ids, normalize="lognorm", n_clusters=2)


def test_pseudobulk_file_writes_the_table(tmp_path):
    root, G = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=30, seed=1)
    cells = [f"C{j}" for j in range(counts.shape[0])]
    clusters = [f"k{j % 4} " for j in range(counts.shape[0])]         # a trailing blank: names are stripped
    data, cfile = tmp_path / "mouse_Rand7_data.csv", tmp_path / "mouse_Rand7_clusters.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    pd.DataFrame({"Cell": cells, "Cluster": clusters}).to_csv(cfile)
    out = rp.pseudobulk_file(data, cfile, save_path=tmp_path / "res")
    written = pd.read_csv(tmp_path / "res" / "mouse_Rand_pseudobulk.csv")
    cols = ["cluster", "n_cells", "n_reads", "n_genes", "cell_type", "cell_subtype", "probability"]
    assert list(out.columns) == cols and list(written.columns) == cols and len(written) == len(out) == 4
    want = rp.pseudobulk(counts, genes, [c.strip() for c in clusters], normalize="lognorm").frame()
    pd.testing.assert_frame_equal(out, want)
    assert written["cluster"].tolist() == ["k0", "k1", "k2", "k3"] and written["n_cells"].tolist() == [8, 8, 7, 7]
    np.testing.assert_allclose(written["probability"], want["probability"])
    pd.DataFrame({"Cell": cells[::-1], "Cluster": clusters}).to_csv(cfile)
    with pytest.raises(ValueError, match="cell order"):
        rp.pseudobulk_file(data, cfile)
