"""CPU side of ``ResidentPredictor.signatures``: the ``rankdata`` reference of tests/signatures_reference.py against hand-worked
rows and against the kernel's counting definition restated in numpy; the host step ``api._signature_scores``; ``read_gmt``; the
refusals, which come before the device is touched; and the ``SignatureScores`` methods on a small constructed table."""
import numpy as np
import pytest

import scdeepsort_amd as sda
from scdeepsort_amd import api

import signatures_reference as S

# a 7-gene vocabulary; the cell stores g0 .. g4 with the values 3, 1, 2, 2, 5: ranks 2, 5, 3.5, 3.5, 1 and 6.5 for g5, g6
ROW = (np.array([0, 5], np.int64), np.arange(5, dtype=np.int32), np.array([3, 1, 2, 2, 5], np.float32))
EMPTY = (np.array([0, 0], np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))


def _sets(*genes):
    member = np.zeros((len(genes), 7), bool)
    for p, g in enumerate(genes):
        member[p, list(g)] = True
    return member


def test_a_row_with_a_tie_by_hand():
    np.testing.assert_array_equal(S.dense_ranks(ROW[1], ROW[2], 7), [2, 5, 3.5, 3.5, 1, 6.5, 6.5])
    r2, present, score = S.rank_sets(*ROW, 7, _sets([0, 2], [2, 5], [5, 6]), max_rank=10)
    assert r2.tolist() == [[11, 7, 0]] and present.tolist() == [[2, 1, 0]]            # the last set: nothing present
    # U = 2 + 3.5 - 3, 3.5 + 6.5 - 3, 6.5 + 6.5 - 3 over n * max_rank = 20
    assert score.tolist() == [[1 - 2.5 / 20, 1 - 7 / 20, 1 - 10 / 20]]


def test_an_empty_row_and_the_cap_by_hand():
    r2, present, score = S.rank_sets(*EMPTY, 7, _sets([1, 2]), max_rank=10)           # every gene at rank (7 + 1) / 2 = 4
    assert r2.tolist() == [[0]] and present.tolist() == [[0]] and score.tolist() == [[1 - 5 / 20]]
    assert S.rank_sets(*EMPTY, 7, _sets([1, 2]), max_rank=2)[2].tolist() == [[1 - 3 / 4]]      # capped at rank 3
    # max_rank = 2 on the stored row: g4 keeps rank 1, g0 rank 2, everything else counts as 3
    r2, present, score = S.rank_sets(*ROW, 7, _sets([4, 1], [0, 6], []), max_rank=2)
    assert r2.tolist() == [[2 + 6, 4, 0]] and present.tolist() == [[2, 1, 0]]
    assert score[0, :2].tolist() == [1 - 1 / 4, 1 - 2 / 4] and np.isnan(score[0, 2])   # a set of no gene scores NaN


def test_key_order():
    v = np.array([np.nan, np.inf, 2.0, 0.0, -0.0, -1.0, -np.inf], np.float32)
    v = np.concatenate([v, -v[:1]])                                                   # ... and a NaN with the sign bit set
    k = S.key32(v)
    assert k.dtype == np.uint32 and np.all(k[:-1] > k[1:])                            # one strict total order, -0.0 below +0.0
    x = np.random.default_rng(0).standard_normal(1000).astype(np.float32)
    assert np.array_equal(np.argsort(S.key32(x), kind="stable"), np.argsort(x, kind="stable"))


def _random_rows(G=120, B=200, seed=3):
    rng = np.random.default_rng(seed)
    indptr, indices, data = [0], [], []
    for r in range(B):
        n = 0 if r % 17 == 0 else int(rng.integers(1, G + 1))
        counts = rng.integers(1, 6, n)                                                # small counts: many ties
        indices.append(rng.permutation(G)[:n].astype(np.int32))
        data.append(np.log1p(counts / max(counts.sum(), 1) * 1e4).astype(np.float32))
        indptr.append(indptr[-1] + n)
    return np.asarray(indptr, np.int64), np.concatenate(indices), np.concatenate(data)


@pytest.mark.parametrize("max_rank", [15, 1500])
def test_the_counting_definition_equals_the_rankdata_reference(max_rank):
    G = 120
    indptr, indices, data = _random_rows(G)
    member = S.membership(G, 9)[:, :G]
    member[3, 15:] = False                                                            # one set no larger than the small max_rank
    want_r2, want_present, want_score = S.rank_sets(indptr, indices, data, G, member, max_rank)
    r2, present = S.count_form(indptr, indices, data, member, max_rank)
    np.testing.assert_array_equal(r2, want_r2)
    np.testing.assert_array_equal(present, want_present)
    np.testing.assert_array_equal(S.rank_sets(indptr, indices, data, G, member, max_rank, by_key=True)[0], want_r2)
    # the host step on the integer sums gives the reference's fp64 score, to the bit
    score = api._signature_scores(r2, present, np.diff(indptr), member.sum(axis=1), G, max_rank)
    assert score.dtype == np.float64 and np.array_equal(score, want_score, equal_nan=True)
    assert np.isnan(score[:, S.EMPTY_SET]).all()
    fits = (member.sum(axis=1) > 0) & (member.sum(axis=1) <= max_rank)                # UCell's precondition: then 0 <= score <= 1
    assert fits[3] and score[:, fits].min() >= 0 and score[:, fits].max() <= 1


def test_pack_matches_the_api():
    member = S.membership(50, 64)
    assert np.array_equal(api._member_words(member).view(np.uint64), S.pack(member))


def test_read_gmt(tmp_path):
    path = tmp_path / "sets.gmt"
    path.write_text("T cell\tCD3 complex\tCD3E\tCD3D\tTRAC\n\nB cell\t\tCD79A\t\tMS4A1 \r\nnone\tno gene\n")
    assert sda.read_gmt(path) == {"T cell": ["CD3E", "CD3D", "TRAC"], "B cell": ["CD79A", "MS4A1"], "none": []}
    assert list(sda.read_gmt(str(path))) == ["T cell", "B cell", "none"]
    path.write_text("a\td\tg1\na\td\tg2\n")
    with pytest.raises(ValueError, match="twice"):
        sda.read_gmt(path)
    path.write_text("\td\tg1\n")
    with pytest.raises(ValueError, match="without a name"):
        sda.read_gmt(path)


# ------------------------------------------------------------------------------------------------
# the refusals, before anything is launched
# ------------------------------------------------------------------------------------------------
def test_signatures_argument_errors():
    class Fake(api.ResidentPredictor):                              # the checks run before the device is touched
        def __init__(self):
            self.hidden_padded, self.n_classes, self.id2label = 12, 3, ["T0", "T1", "T2"]
            self.normalize, self.duplicates, self.aliases = None, "error", None
            self._gene2id = {f"g{i}": i for i in range(7)}

    rp, batch, genes = Fake(), np.zeros((4, 7), np.float32), [f"g{i}" for i in range(7)]
    sets = {"a": ["g1", "g2"], "b": ["g3"]}
    with pytest.raises(ValueError, match="at least one set"):
        rp.signatures(batch, {}, genes=genes)
    with pytest.raises(ValueError, match="at least one set"):
        rp.signatures(batch, None, genes=genes)
    with pytest.raises(ValueError, match="twice"):
        rp.signatures(batch, {1: ["g1"], "1": ["g2"]}, genes=genes)
    with pytest.raises(ValueError, match="one string"):
        rp.signatures(batch, {"a": "g1"}, genes=genes)
    with pytest.raises(ValueError, match="more than max_rank"):
        rp.signatures(batch, sets, genes=genes, max_rank=1)
    with pytest.raises(ValueError, match="more than max_rank"):
        rp.signatures(batch, sets, max_rank=1)                      # resolved against the vocabulary
    for bad in (0, -3, 2 ** 30 + 1):
        with pytest.raises(ValueError, match="max_rank"):
            rp.signatures(batch, sets, genes=genes, max_rank=bad)
    with pytest.raises(ValueError, match="the set 'c'"):
        rp.signatures(batch, sets, genes=genes, expected={"T0": "c"})
    with pytest.raises(ValueError, match="the cell type 'T9'"):
        rp.signatures(batch, sets, genes=genes, expected={"T9": "a"})
    with pytest.raises(ValueError, match="index"):
        rp.signatures(batch, sets, genes=genes, index=["x"])
    with pytest.raises(ValueError, match="normalize needs genes="):
        rp.signatures(batch, sets, normalize="lognorm")


# ------------------------------------------------------------------------------------------------
# SignatureScores on a constructed table
# ------------------------------------------------------------------------------------------------
def _scores(expected="default"):
    # sets:           A     B     C     D (no gene)
    score = np.array([[0.9, 0.2, 0.5, np.nan],       # a  T0  own A, best A by 0.4 over C; rival B: concordant by 0.7
                      [0.3, 0.3, 0.1, np.nan],       # b  T0  A ties B: best = A (the lower index), margin 0, concordant at 0
                      [0.1, 0.6, 0.8, np.nan],       # c  T0  own A = 0.1, rival B = 0.6: discordant; best C
                      [0.7, 0.4, 0.9, np.nan],       # d  T1  own B = 0.4, rival A = 0.7: discordant; best C
                      [0.2, 0.5, 0.1, np.nan],       # e  T1  own B, rival A: concordant by 0.3
                      [0.6, 0.1, 0.2, np.nan],       # f  unsure
                      [0.2, 0.3, 0.4, np.nan]])      # g  T2  no expected set
    if expected == "default":
        expected = {"T0": "A", "T1": "B"}
    return api.SignatureScores(names=["A", "B", "C", "D"], missing={"A": [], "B": ["x"], "C": [], "D": ["y", "z"]},
                               set_size=np.array([3, 2, 4, 0]), score=score, n_present=np.zeros((7, 4), np.int64),
                               n_genes=np.arange(7) * 10, label=np.array([0, 0, 0, 1, 1, -1, 2]),
                               max_prob=np.linspace(0.3, 0.9, 7).astype(np.float32), index=list("abcdefg"),
                               id2label=["T0", "T1", "T2"], max_rank=20, expected=expected)


def test_signature_scores_best_own_and_concordant():
    s = _scores()
    ids, margin = s.best()
    assert ids.tolist() == [0, 0, 2, 2, 1, 0, 2]
    np.testing.assert_allclose(margin, [0.4, 0.0, 0.2, 0.2, 0.3, 0.4, 0.1])
    own = s.own()
    np.testing.assert_array_equal(own[:5], [0.9, 0.3, 0.1, 0.4, 0.5])
    assert np.isnan(own[5:]).all()
    assert s.concordant().tolist() == [True, True, False, False, True, False, False]
    assert s.concordant(0.3).tolist() == [True, False, False, False, True, False, False]
    assert s.concordant(0.5).tolist() == [True, False, False, False, False, False, False]
    # one expected set only: its type's cells are concordant whatever the others score
    assert _scores({"T1": "B"}).concordant().tolist() == [False, False, False, True, True, False, False]
    none = _scores(None)
    assert not none.concordant().any() and np.isnan(none.own()).all()
    one = api.SignatureScores(**{**_scores().__dict__, "score": _scores().score[:, 3:], "names": ["D"], "set_size": np.array([0]),
                                 "expected": None})
    assert one.best()[0].tolist() == [-1] * 7 and np.isnan(one.best()[1]).all()
    two = api.SignatureScores(**{**_scores().__dict__, "score": _scores().score[:, 2:], "names": ["C", "D"],
                                 "set_size": np.array([4, 0]), "expected": None})
    assert two.best()[0].tolist() == [0] * 7 and np.isnan(two.best()[1]).all()         # no runner-up: no margin


def test_signature_scores_tables():
    s = _scores()
    t = s.by_type()
    assert list(t.columns) == ["cell_type", "n_cells", "expected", "median_own", "concordant", "other", "other_share"]
    assert t["cell_type"].tolist() == ["T0", "T1", "T2"] and t["n_cells"].tolist() == [3, 2, 1]
    assert t["expected"].tolist() == ["A", "B", None]
    np.testing.assert_allclose(t["median_own"], [0.3, 0.45, np.nan])
    np.testing.assert_allclose(t["concordant"], [2 / 3, 0.5, np.nan])
    assert t["other"].tolist() == ["C", "A", "C"]                    # T0 without A: C, B, C; T1 without B: C, A - the lower index
    np.testing.assert_allclose(t["other_share"], [2 / 3, 0.5, 1.0])
    f = s.frame()
    assert list(f.columns) == ["index", "cell_type", "prob", "n_genes", "best", "margin", "own", "concordant", "score_A", "score_B",
                               "score_C", "score_D"]
    assert f["cell_type"].tolist() == ["T0", "T0", "T0", "T1", "T1", "unsure", "T2"] and f["best"].tolist() == list("AACCBAC")
    assert f["index"].tolist() == list("abcdefg") and f["n_genes"].tolist() == [0, 10, 20, 30, 40, 50, 60]
    d = s.discordant()
    assert d["index"].tolist() == ["c", "d"] and s.discordant(0.3)["index"].tolist() == ["b", "c", "d"]
    assert "own" not in _scores(None).frame().columns and len(_scores(None).discordant()) == 0
    m = s.summary()
    assert m["n_cells"] == 7 and m["n_called"] == 6 and m["n_best"] == [3, 1, 3, 0] and m["n_missing"] == [0, 1, 0, 2]
    assert m["n_expected"] == 5 and m["concordant"] == 3 / 5 and np.isnan(m["median_score"][3])
    text = str(m)
    assert len(text.splitlines()) == 5 and "2 names not found" in text and "0.600 of them concordant" in text
    assert "concordant" not in str(_scores(None).summary())
    with pytest.raises(ValueError, match="no set"):
        _scores({"T0": "Z"}).own()
