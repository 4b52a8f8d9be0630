"""``ResidentPredictor.doublets`` on the GPU: a pair's call is bit for bit ``classify`` of the host-summed count matrix, the
partners are the numpy rule's, and further draws, chunking and the order of the caller's genes change nothing."""
import numpy as np
import pandas as pd
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import api

import pairs_reference as P
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
B, D = 60, 4
BUNDLE_SEED = {1: 35, 2: 31}            # random bundles whose calls on _counts' cells spread over several types and unsure


def _counts(rp, G, n=B, seed=3):
    """Raw counts over 300 of the bundle's genes IN BUNDLE ORDER, and two columns outside the bundle that hold reads.  The cells
    come from three expression programs (each deep on its own hundred genes), so that the model calls more than one type."""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.permutation(G)[:300])
    genes = [rp.id2gene[i] for i in ids] + ["NotAGene1", "NotAGene2"]
    counts = rng.geometric(0.5, (n, len(genes))) * (rng.random((n, len(genes))) < 0.2)
    program = np.arange(n) % 3
    for k in range(3):
        block = slice(100 * k, 100 * (k + 1))
        counts[program == k, block] += rng.geometric(0.05, ((program == k).sum(), 100)) * (rng.random(((program == k).sum(), 100)) < 0.6)
    counts[5] = 0                                                     # a cell without a read
    return counts.astype(np.float32), genes


def _same(x: api.Doublets, y: api.Doublets):
    assert x.n_partners == y.n_partners and x.seed == y.seed and x.across == y.across
    for name in ("label", "max_prob", "partner", "draw_label", "draw_prob"):
        np.testing.assert_array_equal(getattr(x, name), getattr(y, name), err_msg=name)


@pytest.mark.parametrize("n_layers", [1, 2])
def test_doublets_end_to_end(tmp_path, monkeypatch, n_layers):
    root, G = _random_bundle(tmp_path, n_layers, hidden=12, seed=BUNDLE_SEED[n_layers])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G)
    label, prob, _ = rp.classify(counts, genes=genes, normalize="lognorm")
    assert len(np.unique(label[label >= 0])) > 1 and (label < 0).any()          # two called types at least, and unsure cells
    for across in ("types", "any"):
        db = rp.doublets(counts, genes, normalize="lognorm", n_partners=D, across=across, seed=11)
        np.testing.assert_array_equal(db.label, label); np.testing.assert_array_equal(db.max_prob, prob)      # the call as given
        assert db.partner.dtype == np.int32 and db.draw_label.dtype == np.int32 and db.draw_prob.dtype == np.float32
        assert db.partner.shape == db.draw_label.shape == db.draw_prob.shape == (B, D)
        np.testing.assert_array_equal(db.partner, P.partners(label, D, 11, across))
        # the pairs' calls: classify of the host-summed count matrix, bit for bit
        summed = counts[np.repeat(np.arange(B), D)] + counts[db.partner.ravel()]
        want_label, want_prob, _ = rp.classify(summed, genes=genes, normalize="lognorm")
        np.testing.assert_array_equal(db.draw_label.ravel(), want_label)
        np.testing.assert_array_equal(db.draw_prob.ravel(), want_prob)
        assert db.pair_table().sum() == B * D and len(db.frame()) > 0 and 0 <= db.caught() <= 1
        assert "heterotypic pairs" in str(db.summary())
    types = rp.doublets(counts, genes, normalize="lognorm", n_partners=D, seed=11)                 # across="types" is the default
    _same(types, rp.doublets(counts, genes, normalize="lognorm", n_partners=D, across="types", seed=11))
    assert (label[types.partner] != label[:, None]).all()
    # into: 2 draws and 2 more are 4 at once
    half = rp.doublets(counts, genes, normalize="lognorm", n_partners=2, seed=11)
    assert rp.doublets(counts, genes, normalize="lognorm", n_partners=2, seed=11, into=half) is half
    _same(half, types)
    with pytest.raises(ValueError, match="into"):
        rp.doublets(counts, genes, normalize="lognorm", n_partners=2, seed=12, into=half)
    # chunked by a tiny byte budget (a few pairs per chunk): the same bits
    monkeypatch.setattr(api, "DOUBLETS_CHUNK_BYTES", 8 * 400)
    _same(rp.doublets(counts, genes, normalize="lognorm", n_partners=D, seed=11), types)
    monkeypatch.undo()
    # the caller's genes in another order: the rows are sorted by bundle id, the pairs' calls are the same
    perm = np.random.default_rng(1).permutation(len(genes))
    shuffled = rp.doublets(counts[:, perm], [genes[j] for j in perm], normalize="lognorm", n_partners=D, seed=11)
    np.testing.assert_array_equal(shuffled.partner, types.partner)
    np.testing.assert_array_equal(shuffled.draw_label, types.draw_label)
    # from a CSR over the caller's columns, and with a gene map made once
    import scipy.sparse as sp
    _same(rp.doublets(sp.csr_matrix(counts), rp.gene_map(genes), normalize="lognorm", n_partners=D, seed=11), types)


def test_doublets_refusals(tmp_path):
    root, G = _random_bundle(tmp_path, 1, hidden=12, seed=BUNDLE_SEED[1])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=20)
    with pytest.raises(ValueError, match="genes="):
        rp.doublets(counts, None, normalize="lognorm")
    with pytest.raises(ValueError, match="normalize"):
        rp.doublets(counts, genes)
    with pytest.raises(ValueError, match="across"):
        rp.doublets(counts, genes, normalize="lognorm", across="clusters")
    with pytest.raises(ValueError, match="n_partners"):
        rp.doublets(counts, genes, normalize="lognorm", n_partners=0)
    with pytest.raises(ValueError, match="index"):
        rp.doublets(counts, genes, normalize="lognorm", index=["a", "b"])
    doubled = genes[:-1] + [genes[0]]
    merged = rp.gene_map(doubled, duplicates="sum")
    assert isinstance(merged, api.GeneMap)
    with pytest.raises(ValueError, match="merged"):
        rp.doublets(counts, merged, normalize="lognorm")
    with pytest.raises(sda.WgnnError, match="cell 3"):
        bad = counts.copy(); bad[3, 0] = 2.5
        rp.doublets(bad, genes, normalize="lognorm")
    with pytest.raises(sda.WgnnError, match="cell 4 holds a count above 2\\^23"):
        bad = counts.copy(); bad[4, 1] = 2.0 ** 23 + 1
        rp.doublets(bad, genes, normalize="lognorm")
    one_type = np.tile(counts[:1], (6, 1))                            # every cell the same: one group
    with pytest.raises(ValueError, match="across=\"any\""):
        rp.doublets(one_type, genes, normalize="lognorm")
    assert rp.doublets(one_type, genes, normalize="lognorm", across="any", n_partners=2).draw_label.shape == (6, 2)


def test_doublets_file_writes_the_table(tmp_path):
    root, G = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=30, seed=1)
    cells = [f"C{j}" for j in range(counts.shape[0])]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    out = rp.doublets_file(data, n_partners=D, seed=3, save_path=tmp_path / "res")
    written = pd.read_csv(tmp_path / "res" / "mouse_Rand_doublets.csv")
    cols = ["type_a", "type_b", "n", "parent_share", "third_share", "unsure_share", "top_third", "mean_prob"]
    assert list(out.columns) == cols and list(written.columns) == cols and len(written) == len(out) > 0
    want = rp.doublets(counts, genes, normalize="lognorm", n_partners=D, seed=3).frame()
    pd.testing.assert_frame_equal(out, want)
    np.testing.assert_allclose(written["parent_share"], want["parent_share"])
