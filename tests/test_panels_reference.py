"""CPU side of ``ResidentPredictor.panels``: the fp64 restatement of tests/panels_reference.py against its own special panels
(all genes, none, a materialised sub-row, the zeroed count matrix), the packed membership words, the share of unclear pairs of
every GPU case, and the host logic - name resolution, the ``PanelCalls`` tables and the refusals of ``renormalize=True``."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from scdeepsort_amd import api

import panels_reference as N
import stability_reference as R
import thin_reference as T


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def test_membership_and_pack_round_trip():
    G = R.G_CASE
    for P in (1, 3, 33, 64):
        member = N.membership(G, P)
        words = N.pack(member)
        assert words.dtype == np.uint64 and words.shape == (G,)
        np.testing.assert_array_equal(N.unpack(words, P), member)
        if P < 64:
            assert not (words >> np.uint64(P)).any()
    m64 = N.membership(G, 64)
    assert m64[0].all() and not m64[1].any() and m64[2].sum() == G // 2 and m64[3].sum() == G // 2
    assert (N.pack(m64) >> np.uint64(63)).any()                      # bit 63 is in use
    np.testing.assert_array_equal(N.membership(G, 9), m64[:9])       # a panel does not depend on how many there are
    np.testing.assert_array_equal(api._member_words(m64).view(np.uint64), N.pack(m64))     # the predictor packs the same words


@pytest.mark.parametrize("H,explicit", [(12, False), (64, True)])
def test_all_genes_is_the_unmasked_layer_and_none_is_the_empty_row(H, explicit):
    P, C = 9, 16
    c = N.panel_case(H, C, explicit, P)
    m, B = c["m"], c["m"].shape[0]
    sr = c["self_rows"]
    full = R.layer_draw(m, np.ones(m.nnz, bool), c["table"], c["alpha"], c["bias"], None if sr is None else sr[0::P])
    np.testing.assert_array_equal(c["out"][0::P], full)
    z = c["bias"].astype(np.float64)[None, :] + (0 if sr is None else float(c["alpha"][-1]) * sr[1::P].astype(np.float64))
    np.testing.assert_allclose(c["out"][1::P], np.broadcast_to(np.maximum(z, 0.0), (B, H)), rtol=0, atol=1e-15)
    assert c["empty"][:, 1].all() and not c["entries"][:, 1].any()
    np.testing.assert_array_equal(c["entries"][:, 0], np.diff(m.indptr))
    assert c["empty"][1].all()                                       # the empty cell is empty in every panel


@pytest.mark.parametrize("p", [2, 3, 5, 7])
def test_a_panel_equals_the_reference_on_the_materialised_sub_row(p):
    H, C, P = 32, 16, 9
    c = N.panel_case(H, C, True, P)
    m = c["m"]
    sub = R.thinned(m, N.kept_entries(m, c["member"][p]))
    assert sub.nnz == int(c["entries"][:, p].sum()) and 0 < sub.nnz < m.nnz
    want = R.layer_draw(sub, np.ones(sub.nnz, bool), c["table"], c["alpha"], c["bias"], c["self_rows"][p::P])
    np.testing.assert_allclose(c["out"][p::P], want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("vthr", [0.0, 1.5])
def test_counts_reference_equals_the_lognorm_reference_of_the_zeroed_matrix(vthr):
    H, C, P = 64, 16, 9
    c = N.count_case(H, C, False, P, vthr)
    m, rest, member = c["m"], c["rest"], c["member"]
    B, G = m.shape
    dropped = False
    for p in range(P):
        x = N.zeroed_dense(m, rest, member[p], p % 2 == 1)
        np.testing.assert_array_equal(x.sum(axis=1).astype(np.int64), c["lib"][:, p])       # align's total is the panel's reads
        zeroed = sp.csr_matrix(x[:, :G]); zeroed.sort_indices()
        batch = T.lognorm_batch(zeroed, x[:, -1].astype(np.int64), T.SCALE, vthr)
        want = R.layer_draw(batch, np.ones(batch.nnz, bool), c["table"], c["alpha"], c["bias"], None)
        np.testing.assert_allclose(c["out"][p::P], want, rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(c["entries"][:, p], np.diff(batch.indptr))
        dropped |= batch.nnz < zeroed.nnz
    assert dropped == (vthr > 0)                                     # the positive threshold drops entries
    assert (c["lib"][:, 1] == np.asarray(rest)).all() and c["empty"][:, 1].all()             # the empty panel holds `rest` alone
    assert (c["lib"][:, 0] == np.asarray(m.sum(axis=1)).ravel()).all()


@pytest.mark.parametrize("case", N.PANEL_CASES, ids=str)
def test_share_of_unclear_pairs(case):
    """A condition on the inputs: the GPU test may leave out only the pairs ``unclear`` marks, and only from the label
    comparison, so they must be few (the sibling GPU tests' cap)."""
    H, C, explicit, _, P = case
    c = N.panel_case(H, C, explicit, P)
    share = float(c["unclear"].mean())
    print(f"case {case}: unclear pairs {share:.4f}")
    assert share <= 0.05


# ------------------------------------------------------------------------------------------------
# name resolution
# ------------------------------------------------------------------------------------------------
GENE2ID = {f"G{i}": i for i in range(8)}


def test_panels_resolve_against_the_bundle_vocabulary():
    names, comp, genes, cols, missing = api._resolve_panels(
        {"small": ["G1", "G3", "nope", 5], "ens": ["ENSG3", "ENSX"]}, {"mito": ["G0", "G7", "mt-Zz"]}, GENE2ID,
        aliases={"ENSG3": "G3", "ENSX": "NotInBundle"})
    assert names == ["small", "ens", "mito"] and comp.tolist() == [False, False, True] and cols is None
    assert genes[0].tolist() == [False, True, False, True, False, False, False, False]
    assert genes[1].tolist() == [False, False, False, True, False, False, False, False]
    assert genes[2].tolist() == [False, True, True, True, True, True, True, False]
    assert missing == {"small": ["nope", "5"], "ens": ["ENSX"], "mito": ["mt-Zz"]}


def test_panels_resolve_against_the_callers_columns():
    columns = ["G5", "Other", "ENSG3", "G1", "Spike"]                 # shuffled, two outside the bundle, one by alias
    ids = api._resolve_genes(columns, GENE2ID, {"ENSG3": "G3"})[0]
    assert ids.tolist() == [5, -1, 3, 1, -1]
    names, comp, genes, cols, missing = api._resolve_panels(
        {"a": ["G3", "Spike", "G2"], "b": ["ENSG3", "G5"]}, {"w": ["Other", "G1", "G7"]}, GENE2ID, {"ENSG3": "G3"}, columns, ids)
    assert cols[0].tolist() == [False, False, True, False, True]      # G3 by its bundle id, Spike by its name; G2 is no column
    assert cols[1].tolist() == [True, False, True, False, False]
    assert cols[2].tolist() == [True, False, True, False, True]       # the complement over the CALLER's columns
    assert np.flatnonzero(genes[0]).tolist() == [3] and np.flatnonzero(genes[1]).tolist() == [3, 5]
    assert np.flatnonzero(genes[2]).tolist() == [3, 5]
    assert missing == {"a": ["G2"], "b": [], "w": ["G7"]}
    # a gene map without names: the panel's names can only resolve through the bundle
    _, _, genes2, cols2, missing2 = api._resolve_panels({"a": ["G3", "Spike"]}, None, GENE2ID, None, None, ids)
    assert cols2[0].tolist() == [False, False, True, False, False] and missing2 == {"a": ["Spike"]}
    assert np.flatnonzero(genes2[0]).tolist() == [3]


def test_panel_specifications_that_are_refused():
    with pytest.raises(ValueError, match="at least one"):
        api._resolve_panels(None, None, GENE2ID)
    with pytest.raises(ValueError, match="at least one"):
        api._resolve_panels({}, {}, GENE2ID)
    with pytest.raises(ValueError, match="twice"):
        api._resolve_panels({"x": ["G1"]}, {"x": ["G2"]}, GENE2ID)
    with pytest.raises(ValueError, match="one string"):
        api._resolve_panels({"x": "G1"}, None, GENE2ID)


# ------------------------------------------------------------------------------------------------
# PanelCalls on hand-built tables
# ------------------------------------------------------------------------------------------------
def _calls(n_reads=None):
    #        cell:  0  1  2  3  4   5  6
    label = np.array([0, 0, 0, 1, 1, -1, 2])
    panel = np.array([[0, 0], [0, 1], [-1, 1], [1, 1], [0, 1], [-1, 0], [2, -1]])      # [B, P]: panels "keep" and "drop"
    prob = np.linspace(0.3, 0.95, 14, dtype=np.float32).reshape(7, 2)
    return api.PanelCalls(names=["keep", "drop"], missing={"keep": ["Zzz"], "drop": []}, n_genes=np.array([300, 5900]),
                          n_columns=None, label=label, max_prob=np.full(7, 0.8, np.float32), panel_label=panel, panel_prob=prob,
                          n_entries=np.arange(14).reshape(7, 2), n_reads=n_reads, index=list("abcdefg"),
                          id2label=["T0", "T1", "T2"], renormalize=n_reads is not None)


def test_panel_calls_agreement_confusion_by_type_and_lost():
    pc = _calls()
    np.testing.assert_allclose(pc.agreement(), [4 / 6, 3 / 6])        # cell 5 has no full call and does not count
    conf = pc.confusion("keep")
    assert conf.shape == (4, 4) and conf.sum() == 7
    assert conf.tolist() == [[2, 0, 0, 1], [1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    assert pc.confusion("drop").tolist() == [[1, 2, 0, 0], [0, 2, 0, 0], [0, 0, 0, 1], [1, 0, 0, 0]]
    with pytest.raises(ValueError, match="no panel"):
        pc.confusion("other")
    t = pc.by_type()
    assert list(t.columns) == ["panel", "cell_type", "n_cells", "retained", "unsure", "other", "other_share"]
    assert t["panel"].tolist() == ["keep"] * 3 + ["drop"] * 3 and t["cell_type"].tolist() == ["T0", "T1", "T2"] * 2
    assert t["n_cells"].tolist() == [3, 2, 1, 3, 2, 1]
    np.testing.assert_allclose(t["retained"], [2 / 3, 0.5, 1, 1 / 3, 1, 0])
    np.testing.assert_allclose(t["unsure"], [1 / 3, 0, 0, 0, 0, 1])
    assert t["other"].tolist() == [None, "T0", None, "T1", None, None]
    np.testing.assert_allclose(t["other_share"], [0, 0.5, 0, 2 / 3, 0, 0])
    lost = pc.lost()
    assert list(zip(lost["panel"], lost["cell_type"])) == [("keep", "T0"), ("keep", "T1"), ("drop", "T0"), ("drop", "T2")]
    assert list(zip(*[pc.lost(0.4)[k] for k in ("panel", "cell_type")])) == [("drop", "T0"), ("drop", "T2")]
    s = pc.summary()
    assert s["n_cells"] == 7 and s["n_called"] == 6 and s["n_lost_types"] == [2, 2] and s["n_missing"] == [1, 0]
    text = str(s)
    assert len(text.splitlines()) == 3 and "1 names not found" in text and "re-normalised" not in text


def test_panel_calls_frame():
    pc = _calls()
    f = pc.frame()
    assert list(f.columns) == ["index", "cell_type", "prob", "call_keep", "prob_keep", "entries_keep", "call_drop", "prob_drop",
                               "entries_drop"]
    assert f["cell_type"].tolist() == ["T0", "T0", "T0", "T1", "T1", "unsure", "T2"]
    assert f["call_keep"].tolist() == ["T0", "T0", "unsure", "T1", "T0", "unsure", "T2"] and f["index"].tolist() == list("abcdefg")
    assert f["entries_drop"].tolist() == [1, 3, 5, 7, 9, 11, 13]
    reads = _calls(np.arange(14).reshape(7, 2) * 100)
    assert "reads_keep" in reads.frame().columns and "re-normalised per panel" in str(reads.summary())
    none = api.PanelCalls(**{**_calls().__dict__, "label": np.full(7, -1)})
    assert np.isnan(none.agreement()).all() and len(none.by_type()) == 0


# ------------------------------------------------------------------------------------------------
# the refusals, before anything is launched
# ------------------------------------------------------------------------------------------------
def test_panels_argument_errors():
    class Fake(api.ResidentPredictor):                              # the checks run before the device is touched
        def __init__(self, hidden=12):
            self.hidden_padded, self.n_classes, self.id2label = hidden, 3, ["T0", "T1", "T2"]
            self.normalize, self.duplicates, self.aliases = None, "error", None
            self._gene2id = {f"g{i}": i for i in range(7)}

    rp, batch, genes = Fake(), np.zeros((4, 7), np.float32), [f"g{i}" for i in range(7)]
    spec = dict(panels={"a": ["g1"]})
    with pytest.raises(ValueError, match="genes="):
        rp.panels(batch, renormalize=True, normalize="lognorm", **spec)              # no gene list
    with pytest.raises(ValueError, match="normalize"):
        rp.panels(batch, renormalize=True, genes=genes, **spec)                      # no normalize spec
    with pytest.raises(ValueError, match="library_size"):
        rp.panels(batch, renormalize=True, genes=genes, normalize=api.LogNormalize(library_size=np.ones(4)), **spec)
    ids = torch.zeros(7, dtype=torch.int32)
    merged = api.GeneMap(ids=ids, col_group=ids, group_ptr=torch.tensor([0, 2], dtype=torch.int32),
                         group_cols=torch.tensor([0, 1], dtype=torch.int32), n_groups=1, n_merged_columns=2)
    with pytest.raises(ValueError, match="merged"):
        rp.panels(batch, renormalize=True, genes=merged, normalize="lognorm", **spec)
    rp.duplicates = "sum"
    with pytest.raises(ValueError, match="merged"):
        rp.panels(batch, renormalize=True, genes=genes, normalize="lognorm", **spec)
    rp.duplicates = "error"
    with pytest.raises(ValueError, match="at least one"):
        rp.panels(batch, genes=genes)
    with pytest.raises(ValueError, match="twice"):
        rp.panels(batch, genes=genes, panels={"a": ["g1"]}, without={"a": ["g2"]})
    with pytest.raises(ValueError, match="index"):
        rp.panels(batch, genes=genes, index=["x"], **spec)
    with pytest.raises(ValueError, match="fused kernels"):
        Fake(hidden=260).panels(batch, genes=genes, **spec)
    with pytest.raises(ValueError, match="normalize"):
        rp.panels_file("nowhere.csv", renormalize=True, **spec)
