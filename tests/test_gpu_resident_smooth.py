"""``ResidentPredictor.smooth`` on the GPU: a pooled cell's call is bit for bit ``classify`` of the host-summed count matrix
``(A + I) @ counts``, and the form of the neighbour graph, chunking, the form of the batch and the order of the caller's genes
change nothing."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import api

from test_gpu_resident_doublets import BUNDLE_SEED, _counts
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
B, K = 60, 9
NEIGHBOR_SEED = 12         # a seed at which, for both bundles, the HOST-materialised route changes a call and rescues an unsure cell


def _neighbors(seed=NEIGHBOR_SEED, n=B):
    """int64 [n, K]: ragged lists of 0 to 9 neighbours (-1 = none), most of them of the cell's own expression program (``_counts``
    deals the programs out by ``cell % 3``), the others of any; cell 7 has none, cell 5 - the cell without a read - has some."""
    rng = np.random.default_rng(70_000 + seed)
    out = np.full((n, K), -1, np.int64)
    for i in range(n):
        k = 0 if i == 7 else int(rng.integers(0, K + 1)) if i != 5 else 4
        own = np.array([j for j in range(n) if j != i and j % 3 == i % 3])
        others = np.array([j for j in range(n) if j != i])
        picked = []
        while len(picked) < k:
            j = int(rng.choice(own if rng.random() < 0.7 else others))
            if j not in picked:
                picked.append(j)
        out[i, :k] = picked
    return out


def _indicator(nb, include_self):
    """The neighbour graph as a dense float64 ``[B, B]`` indicator (``A``, or ``A + I``)."""
    n = nb.shape[0]
    a = np.zeros((n, n))
    for i in range(n):
        a[i, nb[i][nb[i] >= 0]] = 1.0
    return a + np.eye(n) if include_self else a


def _same(x: api.Smoothed, y: api.Smoothed, given=True, order=True):
    """Equal bits; ``given``: the call as given too, ``order``: the neighbours come in the same order too."""
    assert x.include_self == y.include_self and torch.equal(x.logits, y.logits)
    for name in ("smooth_label", "smooth_prob", "n_neighbors", "n_reads", "n_genes", "smooth_n_genes", "hood_ptr") + \
            (("label", "max_prob") if given else ()) + (("members",) if order else ()):
        np.testing.assert_array_equal(getattr(x, name), getattr(y, name), err_msg=name)


@pytest.mark.parametrize("n_layers", [1, 2])
def test_smooth_end_to_end(tmp_path, monkeypatch, n_layers):
    root, G = _random_bundle(tmp_path, n_layers, hidden=12, seed=BUNDLE_SEED[n_layers])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G)
    assert counts.shape == (B, 302) and counts[5].sum() == 0 and counts[:, 300:].sum() > 0
    label, prob, _ = rp.classify(counts, genes=genes, normalize="lognorm")
    assert len(np.unique(label[label >= 0])) > 1 and (label < 0).any()          # two called types at least, and unsure cells
    nb = _neighbors()
    n_nb = (nb >= 0).sum(axis=1)
    assert n_nb.min() == 0 and n_nb.max() == K and n_nb[7] == 0 and n_nb[5] > 0 and len(np.unique(n_nb)) > 5
    C = len(rp.id2label)
    by_self = {}
    for include_self in (True, False):
        # the host route: the summed float32 count matrix through classify
        summed = (_indicator(nb, include_self) @ counts.astype(np.float64)).astype(np.float32)
        want_label, want_prob, want_logits = rp.classify(summed, genes=genes, normalize="lognorm")
        if include_self:                               # the fixture shows what the method is for, by the host route alone
            assert ((label >= 0) & (want_label >= 0) & (label != want_label)).any(), "no call changes: pick another NEIGHBOR_SEED"
            assert ((label < 0) & (want_label >= 0)).any(), "no cell is rescued: pick another NEIGHBOR_SEED"
        sm = by_self[include_self] = rp.smooth(counts, genes, nb, normalize="lognorm", include_self=include_self)
        np.testing.assert_array_equal(sm.label, label); np.testing.assert_array_equal(sm.max_prob, prob)      # the call as given
        np.testing.assert_array_equal(sm.smooth_label, want_label)
        np.testing.assert_array_equal(sm.smooth_prob, want_prob)
        assert sm.logits.shape == (B, C) and sm.logits.dtype == want_logits.dtype and torch.equal(sm.logits, want_logits)
        assert sm.smooth_label.dtype == sm.n_reads.dtype == sm.n_neighbors.dtype == np.int64 and sm.smooth_prob.dtype == np.float32
        np.testing.assert_array_equal(sm.n_neighbors, n_nb)
        np.testing.assert_array_equal(sm.n_reads, summed.astype(np.float64).sum(axis=1).astype(np.int64))      # outside columns included
        np.testing.assert_array_equal(sm.n_genes, (counts[:, :300] > 0).sum(axis=1))
        np.testing.assert_array_equal(sm.smooth_n_genes, (summed[:, :300] > 0).sum(axis=1))      # the threshold is 0: all are kept
        # the other forms of the graph: a tensor, a scipy matrix with weights and a diagonal, lists with the cell itself in them
        _same(rp.smooth(counts, genes, torch.from_numpy(nb), normalize="lognorm", include_self=include_self), sm)
        a = sp.csr_matrix(_indicator(nb, False) * 0.25 + 3.0 * np.eye(B))
        _same(rp.smooth(counts, genes, a, normalize="lognorm", include_self=include_self), sm, order=False)      # by column there
        with_self = np.concatenate([np.arange(B)[:, None], nb], axis=1)
        _same(rp.smooth(counts, genes, with_self, normalize="lognorm", include_self=include_self), sm)
    sm, bare = by_self[True], by_self[False]
    # a cell without a neighbour keeps its own call's bits - or, without itself, is the empty row; so is the cell without a read
    assert sm.smooth_label[7] == label[7] and sm.smooth_prob[7] == prob[7] and sm.n_reads[7] == counts[7].sum()
    assert torch.equal(sm.logits[7], rp.classify(counts, genes=genes, normalize="lognorm")[2][7])
    assert bare.n_reads[7] == 0 and bare.smooth_n_genes[7] == 0 and bare.n_neighbors[7] == 0
    assert sm.n_genes[5] == 0 and sm.smooth_n_genes[5] > 0 and sm.n_reads[5] > 0
    # the host logic on top
    for s in (sm, bare):
        own, pooled = s.label, s.smooth_label
        np.testing.assert_array_equal(s.rescued(), (own < 0) & (pooled >= 0))
        np.testing.assert_array_equal(s.lost(), (own >= 0) & (pooled < 0))
        np.testing.assert_array_equal(s.changed(), (own >= 0) & (pooled >= 0) & (own != pooled))
        t = s.transitions()
        assert t.shape == (C + 1, C + 1) and t.dtype == np.int64 and t.sum() == B
        assert t[C, :C].sum() == s.rescued().sum() and t[:C, C].sum() == s.lost().sum()
        assert t[:C, :C].sum() - np.trace(t[:C, :C]) == s.changed().sum() and t[C, C] == ((own < 0) & (pooled < 0)).sum()
        for i, j in ((0, 1), (1, 0), (2, 2)):
            assert t[i, j] == ((own == i) & (pooled == j)).sum()
        agree = s.neighbor_agreement()
        want = np.full(B, np.nan)
        for i in range(B):
            mine = nb[i][nb[i] >= 0]
            if len(mine) and pooled[i] >= 0:
                want[i] = (own[mine] == pooled[i]).mean()
        np.testing.assert_array_equal(agree, want)
        by_type = s.by_type()
        assert list(by_type.columns) == ["cell_type", "n_cells", "kept", "unsure", "becomes"] and by_type["n_cells"].sum() == B
        assert len(by_type) == len(np.unique(own)) and by_type["cell_type"].iloc[-1] == "unsure"
        frame = s.frame()
        assert len(frame) == B and list(frame.columns) == ["index", "cell_type", "prob", "smooth_type", "smooth_prob", "n_neighbors",
                                                            "n_reads", "n_genes", "smooth_n_genes", "neighbor_agreement"]
        text = str(s.summary())
        assert f"{int(s.rescued().sum())} rescued" in text and f"{int(s.lost().sum())} lost" in text
        assert ("with the cell itself" in text) == s.include_self
    assert sm.rescued().any() and sm.changed().any()
    # chunked by a tiny byte budget (a cell or two per chunk): the same bits
    monkeypatch.setattr(api, "SMOOTH_CHUNK_BYTES", 8 * 400)
    _same(rp.smooth(counts, genes, nb, normalize="lognorm"), sm)
    monkeypatch.undo()
    # the caller's genes in another order: a pooled row does not depend on it, it leaves by bundle id
    perm = np.random.default_rng(1).permutation(len(genes))
    shuffled = rp.smooth(counts[:, perm], [genes[j] for j in perm], nb, normalize="lognorm")
    _same(shuffled, sm, given=False)
    np.testing.assert_array_equal(shuffled.label, sm.label)
    # from a CSR over the caller's columns, and with a gene map made once
    _same(rp.smooth(sp.csr_matrix(counts), rp.gene_map(genes), nb, normalize="lognorm"), sm)
    named = rp.smooth(counts, genes, nb, normalize="lognorm", index=[f"C{i}" for i in range(B)])
    assert list(named.frame()["index"]) == [f"C{i}" for i in range(B)]


def test_smooth_refusals(tmp_path):
    root, G = _random_bundle(tmp_path, 1, hidden=12, seed=BUNDLE_SEED[1])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=20)
    nb = _neighbors(n=20)
    with pytest.raises(ValueError, match="genes="):
        rp.smooth(counts, None, nb, normalize="lognorm")
    with pytest.raises(ValueError, match="normalize"):
        rp.smooth(counts, genes, nb)
    with pytest.raises(ValueError, match="index"):
        rp.smooth(counts, genes, nb, normalize="lognorm", index=["a", "b"])
    doubled = genes[:-1] + [genes[0]]
    merged = rp.gene_map(doubled, duplicates="sum")
    assert isinstance(merged, api.GeneMap)
    with pytest.raises(ValueError, match="merged"):
        rp.smooth(counts, merged, nb, normalize="lognorm")
    by_sum = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2, duplicates="sum")
    with pytest.raises(ValueError, match="merged"):
        by_sum.smooth(counts, genes, nb, normalize="lognorm")
    with pytest.raises(sda.WgnnError, match="cell 3"):
        bad = counts.copy(); bad[3, 0] = 2.5
        rp.smooth(bad, genes, nb, normalize="lognorm")
    with pytest.raises(sda.WgnnError, match="cell 4 holds a count above 2\\^23"):
        bad = counts.copy(); bad[4, 1] = 2.0 ** 23 + 1
        rp.smooth(bad, genes, nb, normalize="lognorm")
    twice = nb.copy(); twice[2, :2] = 11
    with pytest.raises(ValueError, match="cell 2 lists the neighbour 11 twice"):
        rp.smooth(counts, genes, twice, normalize="lognorm")
    for bad_index in (20, -2):
        outside = nb.copy(); outside[6, 0] = bad_index
        with pytest.raises(ValueError, match=f"cell 6 lists the index {bad_index}"):
            rp.smooth(counts, genes, outside, normalize="lognorm")
    with pytest.raises(ValueError, match="the batch holds 20 cells"):
        rp.smooth(counts, genes, sp.csr_matrix((21, 21)), normalize="lognorm")
    with pytest.raises(ValueError, match="neighbors"):
        rp.smooth(counts, genes, nb.astype(np.float32), normalize="lognorm")
    with pytest.raises(ValueError, match="neighbors"):
        rp.smooth(counts, genes, nb[:-1], normalize="lognorm")
    # more than 255 neighbours: a batch of 300 cells, one of which lists 256
    many, many_genes = _counts(rp, G, n=300)
    wide = np.full((300, 256), -1)
    wide[9] = np.delete(np.arange(257), 9)
    with pytest.raises(ValueError, match="cell 9 lists 256 neighbours, more than 255"):
        rp.smooth(many, many_genes, wide, normalize="lognorm")
    full = rp.smooth(many, many_genes, wide[:, :255], normalize="lognorm")              # 255 and the cell itself: a unit of 256
    assert full.n_neighbors[9] == 255 and full.n_reads[9] == many[:256].sum(dtype=np.float64) and full.n_neighbors.sum() == 255


def test_smooth_file_round_trips_a_neighbours_file(tmp_path):
    root, G = _random_bundle(tmp_path, 2, hidden=12, seed=BUNDLE_SEED[2])
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G, n=30, seed=1)
    nb = _neighbors(n=30)
    cells = [f"C{j}" for j in range(30)]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    # the cells in another order, a cell without a line, empty fields where a list is short
    order = np.random.default_rng(2).permutation(30)
    lines = [[cells[i]] + [cells[j] if j >= 0 else "" for j in nb[i]] for i in order if i != 7]
    graph = tmp_path / "mouse_Rand7_neighbors.csv"
    pd.DataFrame(lines, columns=["cell"] + [f"n{k}" for k in range(K)]).to_csv(graph, index=False)
    for include_self in (True, False):
        out = rp.smooth_file(data, graph, include_self=include_self, save_path=tmp_path / "res")
        written = pd.read_csv(tmp_path / "res" / "mouse_Rand_smoothed.csv")
        assert list(written.columns) == list(out.columns) and len(written) == len(out) == 30 and list(out["index"]) == cells
        want = rp.smooth(counts, genes, nb, normalize="lognorm", include_self=include_self, index=cells).frame()
        pd.testing.assert_frame_equal(out, want)
        np.testing.assert_array_equal(written["n_reads"], want["n_reads"])
    stranger = tmp_path / "stranger.csv"
    pd.DataFrame([["C1", "C2", "Nobody"]], columns=["cell", "n0", "n1"]).to_csv(stranger, index=False)
    with pytest.raises(ValueError, match="'Nobody' is not a cell"):
        rp.smooth_file(data, stranger)
    pd.DataFrame([["C1", "C2"], ["C1", "C3"]], columns=["cell", "n0"]).to_csv(stranger, index=False)
    with pytest.raises(ValueError, match="'C1' has two lines"):
        rp.smooth_file(data, stranger)
