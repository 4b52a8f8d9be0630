"""``ResidentPredictor.ambient`` on the GPU: a draw's call is bit for bit ``classify`` of the host-materialised contaminated count
matrix (the soup reads drawn by tests/soup_reference.py), and further draws, chunking, the form of the batch and the order of the
caller's genes change nothing."""
import numpy as np
import pandas as pd
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import api

import soup_reference as S
from test_gpu_resident_doublets import BUNDLE_SEED, _counts
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
B, D = 60, 3
RHO = (0.1, 0.3)
SEED = 11


def _profile(rp, genes, weights):
    """``(cdf uint64 [G + 2], column of every bin)`` of one weight per caller column: the bundle's genes where they sit, the columns
    outside the bundle folded into the last bin, whose reads are placed on the first of them."""
    G = rp.n_genes
    ids = rp.gene_map(genes).cpu().numpy()
    bins = np.zeros(G + 1, np.int64)
    np.add.at(bins, np.where(ids >= 0, ids, G), np.asarray(weights, np.int64))
    column = np.full(G + 1, -1, np.int64)
    column[ids[ids >= 0]] = np.flatnonzero(ids >= 0)
    column[G] = int(np.flatnonzero(ids < 0)[0])
    return S.cdf_of(bins), column


def _n_add(counts, rho):
    return np.floor(counts.sum(axis=1, dtype=np.float64) * (rho / (1.0 - rho)) + 0.5).astype(np.int64)


def _materialised(counts, cdf, column, rho, n_draws, seed, draw0=0):
    """float32 [B * n_draws, n_cols]: every cell's counts with its soup reads of every draw added, and the reads per unit that fell
    on bundle genes."""
    n_add = _n_add(counts, rho)
    G = len(cdf) - 2
    out = np.repeat(counts.astype(np.float64), n_draws, axis=0)
    mapped = np.zeros(len(out), np.int64)
    for r in range(counts.shape[0]):
        for d in range(n_draws):
            bins = S.draws(seed, r, draw0 + d, int(n_add[r]), cdf)
            np.add.at(out[r * n_draws + d], column[bins], 1.0)
            mapped[r * n_draws + d] = (bins < G).sum()
    return out.astype(np.float32), mapped, n_add


def _same(x: api.Ambient, y: api.Ambient, given=True):
    assert x.rho == y.rho and x.seed == y.seed and x.n_draws == y.n_draws
    assert x.soup_label == y.soup_label and x.soup_prob == y.soup_prob and x.profile[1] == y.profile[1]
    np.testing.assert_array_equal(x.profile[0], y.profile[0])
    for name in ("draw_label", "draw_prob", "n_added", "n_mapped") + (("label", "max_prob") if given else ()):
        np.testing.assert_array_equal(getattr(x, name), getattr(y, name), err_msg=name)


@pytest.mark.parametrize("n_layers", [1, 2])
def test_ambient_end_to_end(tmp_path, monkeypatch, n_layers):
    root, G = _random_bundle(tmp_path, n_layers, hidden=12, seed=BUNDLE_SEED[n_layers])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G)
    assert counts.shape == (B, 302) and counts[5].sum() == 0 and counts[:, 300:].sum() > 0
    label, prob, _ = rp.classify(counts, genes=genes, normalize="lognorm")
    assert len(np.unique(label[label >= 0])) > 1 and (label < 0).any()          # two called types at least, and unsure cells
    am = rp.ambient(counts, genes, normalize="lognorm", rho=RHO, n_draws=D, seed=SEED)
    np.testing.assert_array_equal(am.label, label); np.testing.assert_array_equal(am.max_prob, prob)      # the call as given
    L = len(RHO)
    assert am.rho == RHO and am.n_draws == D and am.seed == SEED
    assert am.draw_label.dtype == np.int32 and am.draw_prob.dtype == np.float32 and am.n_mapped.dtype == np.int32
    assert am.n_added.dtype == np.int64 and am.draw_label.shape == am.draw_prob.shape == am.n_mapped.shape == (B, L, D)
    assert am.n_added.shape == (B, L) and am.profile[0].shape == (G,) and am.profile[0].dtype == np.int64
    # profile="batch": the batch's own column sums, the two outside columns in the rest bin
    sums = counts.sum(axis=0).astype(np.int64)
    cdf, column = _profile(rp, genes, sums)
    np.testing.assert_array_equal(np.diff(cdf.astype(np.int64))[:G], am.profile[0])
    assert am.profile[1] == int(sums[300:].sum()) > 0
    _same(rp.ambient(counts, genes, normalize="lognorm", rho=RHO, n_draws=D, seed=SEED, profile=sums), am)
    # every unit: classify of the host-materialised contaminated counts, bit for bit
    for l, rho in enumerate(RHO):
        x, mapped, n_add = _materialised(counts, cdf, column, rho, D, SEED)
        np.testing.assert_array_equal(am.n_added[:, l], n_add)
        np.testing.assert_array_equal(am.n_mapped[:, l].ravel(), mapped)
        assert n_add[5] == 0 and n_add.max() > 64
        want_label, want_prob, _ = rp.classify(x, genes=genes, normalize="lognorm")
        np.testing.assert_array_equal(am.draw_label[:, l].ravel(), want_label)
        np.testing.assert_array_equal(am.draw_prob[:, l].ravel(), want_prob)
    # the soup itself: classify of the profile as a one-cell batch
    s_label, s_prob, _ = rp.classify(sums[None, :].astype(np.float32), genes=genes, normalize="lognorm")
    assert am.soup_label == int(s_label[0]) and am.soup_prob == float(s_prob[0])
    # rho = 0: the call as given in every draw (levels come sorted and once each)
    zero = rp.ambient(counts, genes, normalize="lognorm", rho=(0.3, 0.0, 0.3), n_draws=2, seed=SEED)
    assert zero.rho == (0.0, 0.3) and (zero.n_added[:, 0] == 0).all() and (zero.n_mapped[:, 0] == 0).all()
    np.testing.assert_array_equal(zero.draw_label[:, 0], np.repeat(label[:, None], 2, axis=1))
    np.testing.assert_array_equal(zero.draw_prob[:, 0], np.repeat(prob[:, None], 2, axis=1))
    np.testing.assert_array_equal(zero.draw_label[:, 1], am.draw_label[:, 1, :2])          # and the draws do not depend on the levels
    called = label >= 0
    assert (zero.agreement()[called, 0] == 1).all() and np.isnan(zero.agreement()[~called]).all()
    # the host logic on top
    agree = am.agreement()
    assert agree.shape == am.mean_prob().shape == (B, L) and ((agree[called] >= 0) & (agree[called] <= 1)).all()
    want = (am.draw_label == label[:, None, None]).mean(axis=2)
    np.testing.assert_array_equal(agree[called], want[called])
    ids, share = am.flips_to()
    assert ids.shape == share.shape == (B, L) and ((ids == -1) == (share == 0)).all() and (ids[called] != label[called, None]).all()
    assert am.fragile().shape == (B,) and not am.fragile()[~called].any() and am.sinks().shape == (L, len(rp.id2label))
    by_type = am.by_type()
    assert list(by_type.columns) == ["rho", "cell_type", "n_cells", "retained", "unsure", "becomes"]
    assert len(by_type) == L * len(np.unique(label[called])) and by_type["n_cells"].sum() == L * called.sum()
    frame = am.frame()
    assert len(frame) == B and {"index", "cell_type", "prob", "added_0.1", "agree_0.3", "prob_0.1", "flip_0.3", "flip_share_0.1"} <= set(frame.columns)
    text = str(am.summary())
    assert "the soup itself is called" in text and "rho 0.1" in text and "rho 0.3" in text
    # into: 2 draws and 1 more are 3 at once
    part = rp.ambient(counts, genes, normalize="lognorm", rho=RHO, n_draws=2, seed=SEED)
    assert rp.ambient(counts, genes, normalize="lognorm", rho=RHO, n_draws=1, seed=SEED, into=part) is part
    _same(part, am)
    with pytest.raises(ValueError, match="into"):
        rp.ambient(counts, genes, normalize="lognorm", rho=RHO, n_draws=1, seed=SEED + 1, into=part)
    with pytest.raises(ValueError, match="into"):
        rp.ambient(counts, genes, normalize="lognorm", rho=(0.1,), n_draws=1, seed=SEED, into=part)
    with pytest.raises(ValueError, match="another soup profile"):
        rp.ambient(counts, genes, normalize="lognorm", rho=RHO, n_draws=1, seed=SEED, into=part, profile=sums + 1)
    assert part.n_draws == D
    # chunked by a tiny byte budget (a cell or two per chunk): the same bits
    monkeypatch.setattr(api, "AMBIENT_CHUNK_BYTES", 8 * 400 * D)
    _same(rp.ambient(counts, genes, normalize="lognorm", rho=RHO, n_draws=D, seed=SEED), am)
    monkeypatch.undo()
    # the caller's genes in another order: a draw does not depend on it, and the contaminated rows leave by bundle id
    perm = np.random.default_rng(1).permutation(len(genes))
    shuffled = rp.ambient(counts[:, perm], [genes[j] for j in perm], normalize="lognorm", rho=RHO, n_draws=D, seed=SEED)
    _same(shuffled, am, given=False)
    np.testing.assert_array_equal(shuffled.label, am.label)
    # from a CSR over the caller's columns, and with a gene map made once
    import scipy.sparse as sp
    _same(rp.ambient(sp.csr_matrix(counts), rp.gene_map(genes), normalize="lognorm", rho=RHO, n_draws=D, seed=SEED), am)


def test_ambient_refusals(tmp_path):
    root, G = _random_bundle(tmp_path, 1, hidden=12, seed=BUNDLE_SEED[1])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=20)
    with pytest.raises(ValueError, match="genes="):
        rp.ambient(counts, None, normalize="lognorm")
    with pytest.raises(ValueError, match="normalize"):
        rp.ambient(counts, genes)
    for bad in (1.0, -0.1, (0.1, 1.5), float("nan"), ()):
        with pytest.raises(ValueError, match="rho"):
            rp.ambient(counts, genes, normalize="lognorm", rho=bad)
    with pytest.raises(ValueError, match="n_draws"):
        rp.ambient(counts, genes, normalize="lognorm", n_draws=0)
    with pytest.raises(ValueError, match="index"):
        rp.ambient(counts, genes, normalize="lognorm", index=["a", "b"])
    doubled = genes[:-1] + [genes[0]]
    merged = rp.gene_map(doubled, duplicates="sum")
    assert isinstance(merged, api.GeneMap)
    with pytest.raises(ValueError, match="merged"):
        rp.ambient(counts, merged, normalize="lognorm")
    with pytest.raises(sda.WgnnError, match="cell 3"):
        bad = counts.copy(); bad[3, 0] = 2.5
        rp.ambient(bad, genes, normalize="lognorm")
    with pytest.raises(sda.WgnnError, match="cell 4 holds a count above 2\\^23"):
        bad = counts.copy(); bad[4, 1] = 2.0 ** 23 + 1
        rp.ambient(bad, genes, normalize="lognorm")
    with pytest.raises(sda.WgnnError, match="cell 4 would take more than 2\\^23 soup reads"):
        bad = counts.copy(); bad[4, 1] = 2.0 ** 22
        rp.ambient(bad, genes, normalize="lognorm", rho=0.9)
    ones = np.ones(len(genes))
    for bad, word in ((-ones, "non-negative"), (ones * 0.5, "integer"), (ones * np.inf, "non-negative integer"), (ones[:-1], "weights"),
                      (ones * 2.0 ** 41, "2\\^40"), (0 * ones, "all-zero"), ("empty", "profile"), (ones[None, :], "vector")):
        with pytest.raises(ValueError, match=word):
            rp.ambient(counts, genes, normalize="lognorm", profile=bad)
    with pytest.raises(ValueError, match="all-zero"):
        rp.ambient(0 * counts, genes, normalize="lognorm")              # profile="batch" of a batch without a read
    only_outside = 0 * ones
    only_outside[-1] = 5                                                # a soup that never hits a bundle gene is a soup
    out = rp.ambient(counts, genes, normalize="lognorm", rho=0.2, n_draws=2, profile=only_outside)
    assert (out.n_mapped == 0).all() and out.profile[1] == 5 and (out.n_added[counts.sum(axis=1) > 0] > 0).all()


def test_ambient_file_writes_the_table(tmp_path):
    root, G = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=30, seed=1)
    cells = [f"C{j}" for j in range(counts.shape[0])]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    out = rp.ambient_file(data, rho=RHO, n_draws=D, seed=3, save_path=tmp_path / "res")
    written = pd.read_csv(tmp_path / "res" / "mouse_Rand_ambient.csv")
    assert list(written.columns) == list(out.columns) and len(written) == len(out) == 30 and list(out["index"]) == cells
    want = rp.ambient(counts, genes, normalize="lognorm", rho=RHO, n_draws=D, seed=3, index=cells).frame()
    pd.testing.assert_frame_equal(out, want)
    np.testing.assert_allclose(written["agree_0.3"], want["agree_0.3"])
