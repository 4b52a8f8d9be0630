"""CPU side of ``ops.pool_rows`` / ``ResidentPredictor.pseudobulk``: the numpy reference against hand-computed vectors, against
the pair reference (a group of two is a pair) and against the cell's own row (a group of one), what the shared cases hold, the
share of fragile values of every GPU case, the ``Pseudobulk`` table arithmetic on hand-made arrays and the argument errors of
``pseudobulk`` that are raised before the device is touched."""
import math

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import api

import pairs_reference as P
import pool_reference as R


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def test_reference_by_hand():
    # three cells over 6 genes; cell 1 lists gene 4 twice and is not sorted; cell 2 is skipped
    rowptr = [0, 2, 5, 6]
    col = [1, 4, 4, 0, 4, 1]
    cnt = [3, 1, 2, 5, 7, 100]
    lib = [10, 14, 500]
    out = R.pool_rows(rowptr, col, cnt, lib, [1, 1, -1], 3, 0.0)
    assert out.rowptr.tolist() == [0, 0, 3, 3] and out.col.tolist() == [0, 1, 4] and out.cnt.tolist() == [5, 3, 10]
    assert out.total.tolist() == [0, 24, 0] and out.n_cells.tolist() == [0, 2, 0]
    want = [math.log1p(c / 24 * 1e4) for c in (5, 3, 10)]
    np.testing.assert_array_equal(out.v64, want)
    np.testing.assert_array_equal(out.val, np.asarray(want).astype(np.float32))
    # log1p(3 / 24 * 1e4) = 7.13 is the smallest of the three: a threshold of 7.2 drops it alone
    high = R.pool_rows(rowptr, col, cnt, lib, [1, 1, -1], 3, 7.2)
    assert high.col.tolist() == [0, 4] and high.cnt.tolist() == [5, 10] and high.total.tolist() == [0, 24, 0]
    # pooled on top of an earlier result: cell 2 joins group 1, gene 1 grows, the totals and cell numbers add
    more = R.pool_rows(rowptr, col, cnt, lib, [-1, -1, 1], 3, 0.0, seed=out)
    assert more.cnt.tolist() == [5, 103, 10] and more.total.tolist() == [0, 524, 0] and more.n_cells.tolist() == [0, 3, 0]
    both = R.pool_rows(rowptr, col, cnt, lib, [1, 1, 1], 3, 0.0)
    np.testing.assert_array_equal(more.v64, both.v64)
    # a total of 0 leaves nothing, whatever the row holds
    assert R.pool_rows(rowptr, col, cnt, [0, 0, 0], [0, 0, 0], 1, 0.0).rowptr.tolist() == [0, 0]


def test_the_value_takes_the_count_in_fp64():
    total = R.big_total()
    assert 10 ** 11 <= total < 10 ** 11 + 1000
    exact = np.float32(math.log1p(float(R.BIG_COUNT) / total * 1e4))
    through_f32 = np.float32(math.log1p(float(np.float32(R.BIG_COUNT)) / total * 1e4))
    assert float(np.float32(R.BIG_COUNT)) == 2.0 ** 24 and exact != through_f32
    c = R.case(0.0)
    k = R.GROUP_BIG
    row = slice(c.ref.rowptr[k], c.ref.rowptr[k + 1])
    at = int(np.flatnonzero(c.ref.col[row] == R.BIG_GENE)[0])
    assert c.ref.cnt[row][at] == 16_777_217 and c.ref.total[k] == total
    assert c.ref.val[row][at] == exact and not R.fragile(c.ref.v64[row])[at]


def test_groups_of_two_are_pair_rows_and_a_group_of_one_is_the_row():
    m = P.batch()
    rng = np.random.default_rng(4)
    for thr in P.THRESHOLDS:
        a = rng.permutation(m.B)[:m.B // 2 * 2].astype(np.int32)
        a, b = a[::2], a[1::2]
        group = np.full(m.B, -1, np.int32)
        group[a] = np.arange(len(a)); group[b] = np.arange(len(a))
        pooled = R.pool_rows(m.rowptr, m.col, m.cnt, m.lib, group, len(a), thr)
        rowptr, col, val, v64 = P.pair_rows(m.rowptr, m.col, m.cnt, m.lib, a, b, thr)
        np.testing.assert_array_equal(pooled.rowptr, rowptr); np.testing.assert_array_equal(pooled.col, col)
        np.testing.assert_array_equal(pooled.v64, v64); np.testing.assert_array_equal(pooled.val, val)
        np.testing.assert_array_equal(pooled.total, m.lib[a] + m.lib[b])
        # every cell a group of its own: the self pair's row (2c / 2T == c / T), the cell's own counts
        own = R.pool_rows(m.rowptr, m.col, m.cnt, m.lib, np.arange(m.B), m.B, thr)
        same = np.arange(m.B, dtype=np.int32)
        rowptr, col, val, v64 = P.pair_rows(m.rowptr, m.col, m.cnt, m.lib, same, same, thr)
        np.testing.assert_array_equal(own.rowptr, rowptr); np.testing.assert_array_equal(own.col, col)
        np.testing.assert_array_equal(own.v64, v64)
        if thr == 0:
            lens = np.where(m.lib > 0, np.diff(m.rowptr), 0)
            np.testing.assert_array_equal(np.diff(own.rowptr), lens)
            np.testing.assert_array_equal(own.cnt, m.cnt.astype(np.int64))
        np.testing.assert_array_equal(own.total, m.lib); assert (own.n_cells == 1).all()


def test_reference_is_align_on_the_summed_matrix():
    from lognorm_reference import lognorm_dense
    c = R.case(1.5)
    x, gmap = R.summed_dense(c.m, c.group, c.K)
    small = R.small_groups(c.m, c.group, c.K)
    assert small.tolist() == [k != R.GROUP_BIG for k in range(c.K)]
    np.testing.assert_array_equal(x[small].sum(axis=1, dtype=np.float64), c.ref.total[small].astype(np.float64))
    rowptr, col, val, v64 = lognorm_dense(x[small], gmap, 1.5, fp64=True)
    keep = np.repeat(small, np.diff(c.ref.rowptr))
    np.testing.assert_array_equal(np.diff(rowptr), np.diff(c.ref.rowptr)[small])
    np.testing.assert_array_equal(col, c.ref.col[keep]); np.testing.assert_array_equal(v64, c.ref.v64[keep])


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def test_the_cases_hold_what_the_gpu_tests_need():
    m, g = R.batch(), R.groups()
    assert m.G == 300 and m.B == P.batch().B + 6 and len(g) == m.B
    sizes = np.bincount(g[g >= 0], minlength=R.N_GROUPS)
    assert sizes.tolist() == [0, 2, 1, 1, 2, 2, 4, 5, 9, 3] and (g < 0).sum() == 5
    # with cells_per_unit = 4 the member list is cut at 4, 8, ...: windows that hold several groups, groups that span windows
    starts = np.concatenate([[0], np.cumsum(sizes)])
    assert any(s % 4 and e - s > 1 and s // 4 != (e - 1) // 4 for s, e in zip(starts, starts[1:]))       # a group across a cut
    assert any(s % 4 == 0 and e - s == 4 for s, e in zip(starts, starts[1:]))                            # a group that is a window
    assert (m.cnt == np.floor(m.cnt)).all() and m.cnt.min() >= 1 and m.cnt.max() == 2 ** 23
    row = lambda r: m.col[m.rowptr[r]:m.rowptr[r + 1]]
    assert (np.diff(row(m.ROW_UNSORTED)) < 0).all() and len(row(m.ROW_UNSORTED)) > 20
    assert len(row(m.ROW_TWICE)) > len(set(row(m.ROW_TWICE).tolist()))
    assert len(row(m.ROW_EMPTY_2)) == 0 and m.lib[m.ROW_EMPTY_2] == 0
    c = R.case(0.0)
    kept = np.diff(c.ref.rowptr)
    assert kept[R.GROUP_NO_CELLS] == kept[R.GROUP_EMPTY_ROWS] == kept[R.GROUP_FOREIGN_ONLY] == 0
    assert c.ref.total[R.GROUP_FOREIGN_ONLY] == 7 and c.ref.total[R.GROUP_EMPTY_ROWS] == 0
    assert kept[R.GROUP_EVEN_ODD] == 300 and kept[R.GROUP_TWINS] == 130 and kept[R.GROUP_NINE] == 300
    nine = c.ref.cnt[c.ref.rowptr[R.GROUP_NINE]:c.ref.rowptr[R.GROUP_NINE + 1]]
    assert nine.max() > 2 ** 23                                        # ROW_ALL's 2^23 and more on top: beyond a cell's range
    # slabs of 128 genes: three over 300 genes, the last one partial
    assert -(-m.G // 128) == 3 and m.G % 128
    everything = R.case(0.0, "all")
    assert everything.K == 1 and everything.ref.n_cells.tolist() == [m.B - 3] and np.diff(everything.ref.rowptr).tolist() == [300]
    in_it = everything.group >= 0
    assert everything.ref.total[0] == m.lib[in_it].sum()
    assert everything.ref.cnt.sum() == int(m.cnt.astype(np.int64).sum()) - (2 ** 24 + 1 + 4 + 1 + 7 + 2 + 1)


@pytest.mark.parametrize("threshold", R.THRESHOLDS)
@pytest.mark.parametrize("which", ["groups", "all"])
def test_fragile_values_of_the_gpu_cases_stay_under_the_cap(threshold, which):
    c = R.case(threshold, which)
    assert c.ref.v64.size > 0 and R.fragile(c.ref.v64).mean() <= R.FRAGILE_CAP
    if threshold > 0:
        assert c.ref.v64.size < R.case(0.0, which).ref.v64.size and c.ref.val.min() > threshold


# ------------------------------------------------------------------------------------------------
# the Pseudobulk table and pseudobulk's argument errors (before the device is touched)
# ------------------------------------------------------------------------------------------------
def _table():
    return api.Pseudobulk(names=["a", "b", "c"], n_cells=np.array([3, 0, 2]), n_reads=np.array([900, 0, 40]),
                          n_genes=np.array([2, 0, 1]), label=np.array([1, 0, -1]), max_prob=np.array([.9, .5, .4], np.float32),
                          logits=torch.zeros(3, 2), rowptr=torch.tensor([0, 2, 2, 3]), col=torch.tensor([0, 3, 1], dtype=torch.int32),
                          val=torch.tensor([1., 2., 3.]), cnt=torch.tensor([5, 2 ** 40, 7]), id2label=["T0", "T1"],
                          id2gene=["g0", "g1", "g2", "g3"])


def test_pseudobulk_table_arithmetic():
    t = _table()
    counts = t.counts()
    assert counts.shape == (3, 4) and counts.dtype == np.int64
    assert counts.toarray().tolist() == [[5, 0, 0, 2 ** 40], [0, 0, 0, 0], [0, 7, 0, 0]]
    assert t.calls().tolist() == [1, -2, -1]
    f = t.frame()
    assert list(f.columns) == ["cluster", "n_cells", "n_reads", "n_genes", "cell_type", "cell_subtype", "probability"]
    assert f["cell_type"].tolist() == ["T1", "empty", "unsure"] and np.isnan(f["probability"][1]) and f["n_reads"].tolist() == [900, 0, 40]
    calls = api.ClusterCalls(["a", "b", "c"], ["T0", "T1"], torch.zeros(3, 2, dtype=torch.float64), torch.zeros(3, dtype=torch.float64),
                             torch.tensor([[0, 3], [0, 0], [2, 0]], dtype=torch.int32), torch.tensor([[3, 0, 0], [0, 0, 0], [2, 0, 0]], dtype=torch.int32))
    g = t.frame(calls=calls)
    assert g["vote_type"].tolist() == ["T1", "empty", "T0"] and g["agrees"].tolist() == [True, True, False]
    calls.cluster_names = ["a", "b", "z"]
    with pytest.raises(ValueError, match="cluster names"):
        t.frame(calls=calls)
    s = t.summary()
    assert (s["n_clusters"], s["n_cells"], s["n_called"], s["n_unsure"], s["n_empty"], s["min_reads"]) == (3, 5, 1, 1, 1, 40)
    assert "3 clusters pooled from 5 cells" in str(s)
    assert sda.Pseudobulk is api.Pseudobulk and {"pool_rows", "Pseudobulk"} <= set(sda.__all__)


def test_pseudobulk_argument_errors():
    class Fake(api.ResidentPredictor):
        def __init__(self):
            self.hidden_padded, self.n_classes, self.id2label, self.id2gene = 12, 2, ["T0", "T1"], ["g0", "g1", "g2", "g3"]
            self.normalize, self.duplicates, self.aliases, self.threshold = None, "error", None, 0

    rp, batch, genes = Fake(), np.zeros((5, 7), np.float32), [f"g{i}" for i in range(7)]
    clusters = ["a", "b", "a", "c", "c"]
    with pytest.raises(ValueError, match="genes="):
        rp.pseudobulk(batch, None, clusters, normalize="lognorm")
    with pytest.raises(ValueError, match="normalize"):
        rp.pseudobulk(batch, genes, clusters)
    ids = torch.zeros(7, dtype=torch.int32)
    merged = api.GeneMap(ids=ids, col_group=ids, group_ptr=torch.tensor([0, 2], dtype=torch.int32),
                         group_cols=torch.tensor([0, 1], dtype=torch.int32), n_groups=1, n_merged_columns=2)
    with pytest.raises(ValueError, match="merged"):
        rp.pseudobulk(batch, merged, clusters, normalize="lognorm")
    rp.duplicates = "sum"
    with pytest.raises(ValueError, match="merged"):
        rp.pseudobulk(batch, genes, clusters, normalize="lognorm")
    rp.duplicates = "error"
    with pytest.raises(ValueError, match="clusters lists 4 cells"):
        rp.pseudobulk(batch, genes, clusters[:4], normalize="lognorm")
    with pytest.raises(ValueError, match="cluster_names or n_clusters"):
        rp.pseudobulk(batch, genes, [0, 1, 0, 2, 2], normalize="lognorm")
    with pytest.raises(ValueError, match="out of range"):
        rp.pseudobulk(batch, genes, [0, 1, 0, 2, 3], normalize="lognorm", n_clusters=3)
    with pytest.raises(ValueError, match="not one of the table's"):
        rp.pseudobulk(batch, genes, ["a", "b", "a", "q", "c"], normalize="lognorm", into=_table())
    with pytest.raises(ValueError, match="into"):
        rp.pseudobulk(batch, genes, clusters, normalize="lognorm", into="nothing")
    other = _table(); other.id2label = ["T0", "T9"]
    with pytest.raises(ValueError, match="another bundle"):
        rp.pseudobulk(batch, genes, clusters, normalize="lognorm", into=other)
    rp.threshold = 0.5
    with pytest.raises(ValueError, match="threshold of 0"):
        rp.pseudobulk(batch, genes, clusters, normalize="lognorm", into=_table())
