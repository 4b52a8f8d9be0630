"""Host side of the merging alignment: name resolution (``aliases=``) and the duplicate rule (``duplicates=``) of
``ResidentPredictor.gene_map``, and the fp64 restatement of tests/merge_reference.py checked against itself - merging by the
reference equals summing the member columns on the host and running tests/lognorm_reference.py unchanged.  No GPU."""
import numpy as np
import pytest

from scdeepsort_amd import api

import lognorm_reference as L
import merge_reference as M

GENE2ID = {"Actb": 0, "Cd3e": 1, "Cd4": 2, "Gapdh": 3, "Ptprc": 4}
#          0        1                     2       3      4       5                     6       7       8
NAMES = ["Cd4", "ENSMUSG00000032093", "Xist", "Actb", "Cd3e", "ENSMUSG00000023274", "Ly5", "Cd45", "Gapdh"]
ALIASES = {"ENSMUSG00000032093": "Cd3e", "ENSMUSG00000023274": "Cd4", "Ly5": "Ptprc", "Cd45": "Ptprc"}
PLAIN = np.array([2, -1, -1, 0, 1, -1, -1, -1, 3], np.int32)             # without aliases: exact names only
ALIASED = np.array([2, 1, -1, 0, 1, 2, 4, 4, 3], np.int32)               # Cd4 at 0 / 5, Cd3e at 1 / 4, Ptprc at 6 / 7


def test_without_a_collision_the_map_is_the_plain_one_whatever_duplicates_is():
    for mode in api.DUPLICATES:
        ids, groups = api._resolve_genes(NAMES, GENE2ID, None, mode)
        assert groups is None and ids.dtype == np.int32
        np.testing.assert_array_equal(ids, PLAIN)
        np.testing.assert_array_equal(api._gene_map_ids(NAMES, GENE2ID, duplicates=mode), PLAIN)
    np.testing.assert_array_equal(api._gene_map_ids(NAMES, GENE2ID), PLAIN)
    # aliases that hit nothing colliding: still a plain map
    ids, groups = api._resolve_genes(NAMES, GENE2ID, {"Ly5": "Ptprc"}, "sum")
    assert groups is None
    np.testing.assert_array_equal(ids, np.where(np.arange(9) == 6, 4, PLAIN))


def test_error_raises_the_unchanged_message():
    with pytest.raises(ValueError) as e:
        api._resolve_genes(NAMES, GENE2ID, ALIASES, "error")
    assert str(e.value) == ("positions 1 and 4 of the gene list both name bundle gene 1 ('ENSMUSG00000032093'): "
                            "a cell may list a gene once")
    with pytest.raises(ValueError, match="positions 0 and 2 of the gene list both name bundle gene 2"):
        api._gene_map_ids(["Cd4", "Actb", "Cd4"], GENE2ID)                                 # the default, no aliases
    with pytest.raises(ValueError, match="none of the 2 gene names is a gene of the bundle"):
        api._resolve_genes(["a", "b"], GENE2ID, ALIASES, "sum")
    with pytest.raises(ValueError, match="duplicates = 'merge'"):
        api._resolve_genes(NAMES, GENE2ID, ALIASES, "merge")


def test_drop_first_and_sum():
    ids, groups = api._resolve_genes(NAMES, GENE2ID, ALIASES, "drop")
    assert groups is None
    np.testing.assert_array_equal(ids, [-1, -1, -1, 0, -1, -1, -1, -1, 3])
    ids, groups = api._resolve_genes(NAMES, GENE2ID, ALIASES, "first")
    assert groups is None
    np.testing.assert_array_equal(ids, [2, 1, -1, 0, -1, -1, 4, -1, 3])
    ids, groups = api._resolve_genes(NAMES, GENE2ID, ALIASES, "sum")
    np.testing.assert_array_equal(ids, ALIASED)
    col_group, group_ptr, group_cols = groups
    assert all(a.dtype == np.int32 for a in groups)
    np.testing.assert_array_equal(col_group, [1, 0, -1, -1, 0, 1, 2, 2, -1])               # groups by ascending gene id
    np.testing.assert_array_equal(group_ptr, [0, 2, 4, 6])
    np.testing.assert_array_equal(group_cols, [1, 4, 0, 5, 6, 7])
    for got, want in zip(groups, M.group_tables(ALIASED)):                                 # the reference's own loop
        np.testing.assert_array_equal(got, want)


def test_an_alias_never_overrides_an_exact_bundle_name():
    ids, groups = api._resolve_genes(["Cd4", "Actb"], GENE2ID, {"Cd4": "Gapdh", "Actb": "nothing"}, "error")
    assert groups is None
    np.testing.assert_array_equal(ids, [2, 0])


def test_an_alias_to_a_name_outside_the_bundle_stays_unmatched():
    ids, _ = api._resolve_genes(["Cd4", "Foo", 7], GENE2ID, {"Foo": "Bar", "7": "Actb"}, "error")
    np.testing.assert_array_equal(ids, [2, -1, 0])                                         # names compare as str


def test_drop_is_the_freq_1_rule_of_pre_process_r():
    """pre-process.R:13-31 / 43-63 by hand: a non-symbol becomes the symbol it is the unique synonym of, then every name that
    occurs more than once goes (``genedata1$Freq == 1``)."""
    symbols = ["A", "B", "C", "D"]
    synonym_of = {"a1": "A", "b1": "B", "b2": "B"}
    rows = ["A", "a1", "B", "x", "C", "b1", "b2", "D", "D"]
    renamed = [n if n in symbols else synonym_of.get(n, n) for n in rows]                  # exact symbols first
    freq = {n: renamed.count(n) for n in renamed}
    kept = [i for i, n in enumerate(renamed) if freq[n] == 1 and n in symbols]
    assert kept == [4]                                                                     # only C survives
    ids = api._gene_map_ids(rows, {s: i for i, s in enumerate(symbols)}, synonym_of, "drop")
    np.testing.assert_array_equal(np.flatnonzero(ids >= 0), kept)
    assert ids[4] == 2


class _Host(api.ResidentPredictor):
    """The predictor's host half: no bundle, no device."""
    def __init__(self, **kw):
        self.normalize, self.aliases, self.duplicates, self.threshold = None, None, "error", 0
        self._gene2id, self.device = GENE2ID, "cpu"
        self.__dict__.update(kw)


def test_sum_without_normalisation_raises_on_the_host():
    x = np.ones((2, len(NAMES)), np.float32)
    with pytest.raises(ValueError, match='duplicates="sum" needs normalize='):
        _Host(aliases=ALIASES, duplicates="sum")._align(x, NAMES, None)
    gm = _Host().gene_map(NAMES, ALIASES, "sum")
    assert isinstance(gm, api.GeneMap) and gm.n_groups == 3 and gm.n_merged_columns == 6
    with pytest.raises(ValueError, match='duplicates="sum" needs normalize='):
        _Host()._align(x, gm, None)
    with pytest.raises(ValueError, match="groups belongs to normalize"):
        from scdeepsort_amd import ops
        ops.align_rows(x, gm.ids, 5, 0.0, groups=gm.groups)
    with pytest.raises(ValueError, match="duplicates = 'add'"):
        api.ResidentPredictor("mouse", "Testis", duplicates="add")
    assert isinstance(_Host().gene_map(NAMES, ALIASES, "drop"), api.torch.Tensor)


# ------------------------------------------------------------------------------------------------
# the reference against itself
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    return M.merge_case(11, 24, 700, 900)


@pytest.mark.parametrize("thr", [0.0, M.JOINT_THRESHOLD])
def test_merging_equals_summing_on_the_host_dense(case, thr):
    c = case
    assert c.x.max() < 2 ** 24 and (c.x == np.round(c.x)).all()
    pre = M.premerge_dense(c.x, c.col_group)
    want = L.lognorm_dense(pre, c.gene_map, thr, library_size=L.totals(c.x))
    got = M.merge_dense(c.x, c.gene_map, c.col_group, thr)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    plain = L.lognorm_dense(c.x, c.gene_map, thr)
    assert len(got[1]) < len(plain[1])                                                     # something was merged
    kept = np.diff(got[0])
    assert kept[M.ROW_EMPTY] == 0 and kept[M.ROW_NO_MEMBER] > 0
    quad_gene = c.gene_map[M.GROUP_QUAD[0]]
    joint = got[1][got[0][M.ROW_JOINT]: got[0][M.ROW_JOINT + 1]]
    assert (quad_gene in joint) == True and (thr == 0 or quad_gene not in
                                             plain[1][plain[0][M.ROW_JOINT]: plain[0][M.ROW_JOINT + 1]])


def test_merging_equals_summing_on_the_host_csr(case):
    c = case
    for rowptr, col, val in (L.to_csr(c.x), M.shuffled_csr(c.x, 5)):
        pre = M.premerge_csr(rowptr, col, val, c.col_group)
        want = L.lognorm_csr(rowptr, col, pre, c.gene_map, 0.0, library_size=L.totals(c.x))
        got = M.merge_csr(rowptr, col, val, c.gene_map, c.col_group, 0.0)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
    dense = M.merge_dense(c.x, c.gene_map, c.col_group, 0.0)
    for g, w in zip(M.merge_csr(*L.to_csr(c.x), c.gene_map, c.col_group, 0.0), dense):    # column order: the same rows
        np.testing.assert_array_equal(g, w)
    shuffled = M.merge_csr(*M.shuffled_csr(c.x, 5), c.gene_map, c.col_group, 0.0)
    assert not np.array_equal(shuffled[1], dense[1])                                       # the input-order rule shows


def test_the_case_holds_the_layouts_it_names(case):
    c = case
    for grp in M.FIXED_GROUPS:
        assert len(set(c.col_group[list(grp)])) == 1 and c.col_group[grp[0]] >= 0
        assert len(set(c.gene_map[list(grp)])) == 1 and c.gene_map[grp[0]] >= 0
    a, b = M.GROUP_QUAD
    assert a // 4 == b // 4                                                                # one float4
    assert M.GROUP_STEPS[0] // 64 != M.GROUP_STEPS[1] // 64 and M.GROUP_STEPS[1] < 256     # steps of one chunk
    assert len({j // 256 for j in M.GROUP_CHUNKS}) == 3 and len(M.GROUP_FIVE) == 5
    assert (c.x[:, list(M.GROUP_ZERO)] == 0).all()
    assert (c.x[M.ROW_EMPTY] == 0).all()
    assert (c.x[M.ROW_NO_MEMBER, c.col_group >= 0] == 0).all() and (c.x[M.ROW_NO_MEMBER] > 0).any()
    for grp in c.groups:
        if tuple(grp) != M.GROUP_ZERO:
            assert c.x[M.ROW_FIRST_ZERO, grp[0]] == 0 and c.x[M.ROW_FIRST_ZERO, grp[-1]] > 0
    both = [(c.x[:, grp] > 0).sum(axis=1).max() for grp in c.groups]
    assert max(both) == 5 and sorted(both)[1] >= 2                                          # groups do meet in a row
    assert L.totals(c.x)[M.ROW_JOINT] == M.JOINT_TOTAL


def test_binade_case_is_exact_and_never_fragile():
    """The GPU test's non-integer case: every partial sum is exact in fp64, and no value of the reference lies within 16 fp64
    ulps of a float32 rounding midpoint - its exception (at most 1 entry in 1 000) excuses nothing for this seed."""
    c = M.merge_case(23, 24, 700, 900, integer=False)
    assert ((c.x * 1024) == np.round(c.x * 1024)).all() and c.x.max() < 2 ** 15 and (c.x != np.round(c.x)).any()
    lo, hi = c.x[c.x > 0].min(), c.x.max()
    assert hi / lo >= 2 ** 18                                                              # many binades
    want = M.merge_dense(c.x, c.gene_map, c.col_group, 0.0, fp64=True)
    assert len(want[3]) > 3000 and L.fragile(want[3]).sum() * 1000 <= len(want[3])
    assert not L.fragile(want[3]).any()
    sh = M.merge_csr(*M.shuffled_csr(c.x, 7), c.gene_map, c.col_group, 0.0, fp64=True)
    assert not L.fragile(sh[3]).any()
