"""The reference of ``wgnn_rank_genes_groups`` (tests/rank_genes_reference.py) against the header's counting identities and
against ``scipy.stats.mannwhitneyu``, the host step of ``ResidentPredictor.rank_genes`` against it bit for bit, Benjamini-Hochberg
against a hand-worked vector, and ``GeneRanks.top`` / ``frame`` / ``compare`` / ``summary`` on a hand-built table.  No GPU."""
import numpy as np
import pytest
import torch
from scipy.stats import mannwhitneyu

import scdeepsort_amd as sda
from scdeepsort_amd import api

import rank_genes_reference as R

LENGTHS = (0, 1, 2, 63, 64, 65, 200, 399, 400)
K = 5


@pytest.fixture(scope="module")
def case():
    """400 cells x 9 genes of 0 .. 400 stored entries, heavy ties, 5 groups (one empty, one of a single cell) and skipped cells."""
    rowptr, col, val = R.column_case(400, LENGTHS, len(LENGTHS), seed=4)
    group = R.groups_of(400, K, seed=5)
    return rowptr, col, val, group, R.tables(rowptr, col, val, group, K, len(LENGTHS))


def _dense(rowptr, col, val, G):
    x = np.zeros((len(rowptr) - 1, G), np.float32)
    x[np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)), col] = val
    return x


def test_reference_integers_are_the_counting_identities(case):
    rowptr, col, val, group, (r2, count, tie, size) = case
    G = len(LENGTHS)
    x = _dense(rowptr, col, val, G)
    stored = _dense(rowptr, col, np.ones_like(val), G) > 0
    part = group >= 0
    x, stored, grp = x[part], stored[part], group[part]
    N = len(grp)
    assert size.tolist() == np.bincount(grp, minlength=K).tolist() and size[1] == 0 and size[2] == 1 and (group < 0).any()
    for g in range(G):
        v = x[:, g]
        lt = (v[None, :] < v[:, None]).sum(axis=1)
        eq = (v[None, :] == v[:, None]).sum(axis=1)
        twice = 2 * lt + eq + 1
        assert np.bincount(grp, weights=twice, minlength=K).astype(np.int64).tolist() == r2[:, g].tolist()
        assert int((eq.astype(np.int64) ** 2 - 1).sum()) == tie[g]
        assert np.bincount(grp[stored[:, g]], minlength=K).tolist() == count[:, g].tolist()
        # the implicit zeros as the header words them: every stored value here is > 0
        z = N - int(stored[:, g].sum())
        r2_zero = z + 1
        for k in range(K):
            own = stored[:, g] & (grp == k)
            assert r2[k, g] == twice[own].sum() + (size[k] - count[k, g]) * r2_zero
        eq_stored = eq[stored[:, g]].astype(np.int64)
        assert tie[g] == (eq_stored ** 2 - 1).sum() + z * (z * z - 1)


def test_u_and_p_are_scipys(case):
    rowptr, col, val, group, (r2, count, tie, size) = case
    G = len(LENGTHS)
    x = _dense(rowptr, col, val, G)
    U, auc, z, p = R.host_stats(r2, tie, size)
    worst, seen = 0.0, 0
    for k in range(K):
        a, b = x[group == k], x[(group >= 0) & (group != k)]
        if not len(a) or not len(b):
            assert np.isnan(z[k]).all() and np.isnan(p[k]).all() and np.isnan(auc[k]).all()
            continue
        for g in range(G):
            want = mannwhitneyu(a[:, g], b[:, g], use_continuity=False, method="asymptotic")
            assert U[k, g] == want.statistic
            if len(np.unique(np.concatenate([a[:, g], b[:, g]]))) == 1:
                assert (z[k, g], p[k, g], auc[k, g]) == (0.0, 1.0, 0.5)                 # every value tied
                continue
            rel = abs(p[k, g] - want.pvalue) / want.pvalue
            print(f"group {k} gene {g}: p {p[k, g]!r} scipy {want.pvalue!r} rel {rel:.3g}")
            worst, seen = max(worst, rel), seen + 1
            assert 0.0 <= auc[k, g] <= 1.0 and (z[k, g] > 0) == (auc[k, g] > 0.5)
    print(f"largest relative difference of p: {worst!r} over {seen} tests")
    assert seen >= 20 and worst <= max(16 * R.P_REL_MEASURED, 4 * np.finfo(np.float64).eps)


def test_the_host_step_is_the_references_bit_for_bit(case):
    _, _, _, _, (r2, count, tie, size) = case
    for got, want in zip(api._rank_genes_stats(r2, tie, size), R.host_stats(r2, tie, size)):
        assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True)


def test_edge_cases():
    rowptr, col, val = R.column_case(50, (0, 50, 20, 7), 4, seed=2, tied_gene=1)
    # group 1 is empty, group 0 holds every participating cell: nothing to test against
    group = np.zeros(50, np.int64)
    group[:5] = -1
    r2, count, tie, size = R.tables(rowptr, col, val, group, 2, 4)
    assert size.tolist() == [45, 0] and (r2[1] == 0).all() and (count[1] == 0).all()
    assert r2[0].tolist() == [45 * 46] * 4                                              # all ranks of 45 values, doubled
    for stats in (R.host_stats(r2, tie, size), api._rank_genes_stats(r2, tie, size)):
        for t in stats[1:]:
            assert np.isnan(t).all()
    # two groups: a gene nobody expresses and a gene whose values all tie have var == 0
    group = np.arange(50) % 2
    r2, count, tie, size = R.tables(rowptr, col, val, group, 2, 4)
    assert tie[0] == tie[1] == 50 ** 3 - 50 and (count[:, 0] == 0).all() and (count[:, 1] == 25).all()
    for U, auc, z, p in (R.host_stats(r2, tie, size), api._rank_genes_stats(r2, tie, size)):
        assert (z[:, :2] == 0).all() and (p[:, :2] == 1).all() and (auc[:, :2] == 0.5).all()
        assert (U[:, :2] == 25 * 25 / 2).all() and not np.isnan(z).any()
        assert np.array_equal(z[0], -z[1]) and np.array_equal(U[0] + U[1], np.full(4, 625.0))   # two groups mirror each other
    # keys: -0.0 sorts below the implicit +0.0, a negative below both, a NaN above everything
    rowptr = np.array([0, 1, 2, 3, 4, 4, 4], np.int64)
    val = np.array([-0.0, -1.5, np.nan, 2.0], np.float32)
    r2, count, tie, size = R.tables(rowptr, np.zeros(4, np.int32), val, np.array([0, 1, 2, 3, 4, 4]), 5, 1)
    assert size.tolist() == [1, 1, 1, 1, 2] and r2[:, 0].tolist() == [4, 2, 12, 10, 7 + 7] and tie[0] == 6


def test_benjamini_hochberg_against_a_hand_worked_vector():
    p = np.array([0.01, 0.04, 0.03, 0.005])
    # ascending: 0.005 * 4 / 1, 0.01 * 4 / 2, 0.03 * 4 / 3, 0.04 * 4 / 4 = 0.02, 0.02, 0.04, 0.04; already monotone
    np.testing.assert_allclose(R.benjamini_hochberg(p), [0.02, 0.04, 0.04, 0.02], rtol=1e-14)
    # 0.5 * 3 / 2 = 0.75 is pulled down to its successor's 0.6 * 3 / 3; 0.9 * 2 / 1 is capped at 1
    np.testing.assert_allclose(R.benjamini_hochberg([0.5, 0.6, 0.001]), [0.6, 0.6, 0.003], rtol=1e-14)
    np.testing.assert_allclose(R.benjamini_hochberg([0.9, 0.95]), [0.95, 0.95], rtol=1e-14)
    rng = np.random.default_rng(0)
    q = rng.random((3, 40)) ** 3
    q[1] = np.nan                                                                       # an empty group's row stays NaN
    got = api._benjamini_hochberg(q)
    assert np.isnan(got[1]).all()
    for i in (0, 2):
        assert np.array_equal(got[i], R.benjamini_hochberg(q[i]))


@pytest.fixture(scope="module")
def table():
    """12 cells in 3 groups of 4 over 6 genes: gene g < 3 is group g's marker, gene 3 is in every cell at one value, gene 4 in
    none, gene 5 is group 0's weaker second marker."""
    x = np.zeros((12, 6), np.float32)
    for k in range(3):
        x[4 * k:4 * k + 4, k] = [2.0, 2.5, 3.0, 3.5]
    x[:, 3] = 1.0
    x[0:3, 5] = [1.0, 1.5, 2.0]
    x[8, 5] = 1.2
    group = np.repeat(np.arange(3), 4)
    rowptr, col, val = R.csr_of(x > 0, x)
    r2, count, tie, size = R.tables(rowptr, col, val, group, 3, 6)
    mean = np.stack([x[group == k].astype(np.float64).mean(axis=0) for k in range(3)])
    rest = np.stack([x[group != k].astype(np.float64).mean(axis=0) for k in range(3)])
    return sda.GeneRanks(group_names=["a", "b", "c"], id2gene=[f"G{i}" for i in range(6)], n_cells=size, n_skipped=0,
                         rank2_sum=r2, expr_count=count, tie_sum=tie, mean=mean, mean_rest=rest)


def test_gene_ranks_top_and_frame(table):
    z = table.z()
    genes, score = table.top(3)
    assert genes.shape == (3, 3) and genes[:, 0].tolist() == [0, 1, 2]
    assert genes[0].tolist() == [0, 5, 3]                       # then the weaker marker, then z == 0 by ascending gene id
    assert z[0, 3] == z[0, 4] == 0 and score[0].tolist() == [z[0, 0], z[0, 5], 0.0]
    assert table.top(2, min_fraction=0.5)[0].tolist() == [[0, 5], [1, 3], [2, 3]]
    assert table.top(8)[0][0].tolist() == [0, 5, 3, 4, 1, 2, -1, -1]        # z ties (genes 1 and 2) by ascending gene id
    assert table.top(3, min_logfc=1.0)[0].tolist() == [[0, 5, -1], [1, -1, -1], [2, -1, -1]]
    assert table.top(3, max_padj=0.1)[0][:, 0].tolist() == [0, 1, 2]
    with pytest.raises(ValueError, match="positive"):
        table.top(0)
    np.testing.assert_array_equal(table.fraction()[0], [1, 0, 0, 1, 0, 0.75])
    np.testing.assert_array_equal(table.fraction_rest()[0], [0, 0.5, 0.5, 1, 0, 0.125])
    assert table.auc()[0, 0] == 1.0 and table.auc()[1, 0] == 0.25 and table.u()[0, 0] == 32.0
    lf = table.logfc()
    assert lf[0, 0] > 20 and lf[1, 0] < -20 and lf[0, 3] == 0 and lf[0, 4] == 0
    adj = table.pvals_adj()
    for k in range(3):
        assert np.array_equal(adj[k], R.benjamini_hochberg(table.pvals()[k]))
    f = table.frame(2)
    assert list(f.columns) == ["group", "rank", "gene", "z", "auc", "logfc", "p", "p_adj", "fraction", "fraction_rest", "mean"]
    assert f["group"].tolist() == ["a", "a", "b", "b", "c", "c"] and f["rank"].tolist() == [1, 2] * 3
    assert f["gene"].tolist() == ["G0", "G5", "G1", "G3", "G2", "G3"]
    assert f["z"][0] == z[0, 0] and f["mean"][0] == 2.75 and f["p_adj"][1] == adj[0, 5]
    s = table.summary(alpha=0.1)
    assert s["n_cells"] == 12 and s["top_gene"] == ["G0", "G1", "G2"] and s["group_cells"] == [4, 4, 4]
    assert "a: 4 cells" in str(s) and "top G0" in str(s)


def test_gene_ranks_compare(table):
    score = torch.zeros((3, 6), dtype=torch.float64)
    score[0, 0], score[0, 1] = 4.0, 2.0                         # the model leans on G0 and G1 for a
    score[1, 5] = 1.0                                           # on G5 for b
    markers = sda.MarkerTable(group_names=["a", "b", "c"], id2gene=table.id2gene, n_cells=np.array([4, 4, 4]), n_skipped=0,
                              score_sum=score, expr_count=(score != 0).to(torch.int32) * 4, base_sum=np.zeros(3),
                              logit_sum=np.zeros(3))
    c = table.compare(markers, k=2)
    assert list(c.columns) == ["group", "n_model", "n_data", "n_shared", "jaccard", "model_only", "data_only"]
    assert c["n_model"].tolist() == [2, 1, 0] and c["n_data"].tolist() == [2, 2, 2] and c["n_shared"].tolist() == [1, 0, 0]
    assert c["jaccard"].tolist() == [1 / 3, 0.0, 0.0]
    assert c["model_only"].tolist() == [["G1"], ["G5"], []] and c["data_only"].tolist() == [["G5"], ["G1", "G3"], ["G2", "G3"]]
    markers.group_names = ["a", "b", "x"]
    with pytest.raises(ValueError, match="group names"):
        table.compare(markers)
    markers.group_names, markers.id2gene = ["a", "b", "c"], [f"H{i}" for i in range(6)]
    with pytest.raises(ValueError, match="gene names"):
        table.compare(markers)
