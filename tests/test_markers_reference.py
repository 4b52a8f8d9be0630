"""CPU side of the per-group gene tables: the C ABI of ``wgnn_group_gene_reduce`` without a GPU, the fp64 reference of
tests/markers_reference.py against a brute-force dense loop and the completeness identity, ``MarkerTable``'s host logic on
CPU tensors, and the premises of the operands the GPU suite uses."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib

import attrib_reference as R
import markers_reference as M

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------
# 1. the ABI
# ------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for s in ("wgnn_group_gene_reduce", "wgnn_group_gene_reduce_workspace"):
        assert re.search(rf"\b{s}\s*\(", text), f"{s} is not declared in wgnn.h"
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert int(re.search(r"#define\s+WGNN_MARKERS_ACCUMULATE\s+(\d+)", text).group(1)) == _lib.MARKERS_ACCUMULATE
    assert lib.wgnn_version() == 206
    from scdeepsort_amd import build
    assert "wgnn_markers.hip" in {p.name for p in build.SRC}


def test_bad_arguments_return_error_codes_without_gpu():
    lib = _lib.lib()
    one = C.c_void_p(16)          # fake, aligned, never dereferenced: validation happens first

    def run(sum_=one, count=one, n_rows=4, K=3, G=5, flags=0, t_rowptr=one, ws_bytes=0):
        return lib.wgnn_group_gene_reduce(t_rowptr, one, one, one, n_rows, K, G, sum_, count, None, ws_bytes, flags, None)

    assert run(sum_=None) == -1 and b"sum and count" in lib.wgnn_last_error_string(-1)
    assert run(count=None) == -1
    assert run(K=0) == -1 and b"n_groups" in lib.wgnn_last_error_string(-1)
    assert run(K=-2) == -1
    assert run(G=0) == -1 and b"n_genes" in lib.wgnn_last_error_string(-1)
    assert run(n_rows=-1) == -1 and b"n_rows" in lib.wgnn_last_error_string(-1)
    assert run(n_rows=2 ** 31) == -1
    assert run(flags=1) == -1 and b"WGNN_MARKERS_ACCUMULATE" in lib.wgnn_last_error_string(-1)
    assert run(t_rowptr=None) == -1
    assert run(K=2 ** 20 + 1) == -3
    assert run(ws_bytes=-1) == -4
    assert run(sum_=C.c_void_p(20)) == -2
    assert lib.wgnn_last_error_string(-1) == b"bad argument (null pointer, negative size or bad enum)"   # handed out once
    nb = C.c_int64(-7)
    assert lib.wgnn_group_gene_reduce_workspace(100, 5000, 16, 200, C.addressof(nb)) == 0 and nb.value >= 0
    assert lib.wgnn_group_gene_reduce_workspace(100, 5000, 16, 200, None) == -1
    assert lib.wgnn_group_gene_reduce_workspace(-1, 5000, 16, 200, C.addressof(nb)) == -1
    assert lib.wgnn_group_gene_reduce_workspace(100, -1, 16, 200, C.addressof(nb)) == -1
    assert lib.wgnn_group_gene_reduce_workspace(100, 5000, 0, 200, C.addressof(nb)) == -1
    assert lib.wgnn_group_gene_reduce_workspace(100, 5000, 16, 0, C.addressof(nb)) == -1


def test_wrapper_refuses_cpu_tensors():
    z = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.group_gene_reduce(z, z[:0], torch.zeros(0), z[:2], 2, 5)


# ------------------------------------------------------------------------------------------------
# 2. the reference itself
# ------------------------------------------------------------------------------------------------
def _brute(m, scores, group, K):
    G = m.shape[1]
    total, count = np.zeros((K, G)), np.zeros((K, G), np.int32)
    for i in range(m.shape[0]):
        if group[i] < 0:
            continue
        for j in range(m.indptr[i], m.indptr[i + 1]):
            total[group[i], m.indices[j]] += float(scores[j])
            count[group[i], m.indices[j]] += 1
    return total, count


@pytest.mark.parametrize("K", [1, 5, 40])
def test_reference_equals_brute_force(K):
    rng = np.random.default_rng(K)
    m = R.ragged_batch(rng, 40, 6000)
    group = rng.integers(-1, K, 40)
    scores = M.lattice(rng, m.nnz)                           # exact in any order: the two must be equal bit for bit
    total, count, mag = M.reduce(m.indptr, m.indices, scores, group, K, 6000)
    want_t, want_c = _brute(m, scores, group, K)
    assert np.array_equal(total, want_t) and np.array_equal(count, want_c)
    assert M.exact_premise(mag)
    flt = rng.standard_normal(m.nnz).astype(np.float32)
    total, count, mag = M.reduce(m.indptr, m.indices, flt, group, K, 6000)
    want_t, _ = _brute(m, flt, group, K)
    assert (np.abs(total - want_t) <= M.bound(count, mag)).all()
    assert count.sum() == np.diff(m.indptr)[group >= 0].sum()


@pytest.mark.parametrize("n_layers", [1, 2])
def test_group_sums_keep_the_completeness_identity(n_layers):
    """sum_g sum[k, g] + base_sum[k] == logit_sum[k] in fp64, on attrib_reference.attribution output."""
    rng = np.random.default_rng(40 + n_layers)
    G, B, H, C_ = 6000, 40, 16, 5
    m = R.ragged_batch(rng, B, G)
    tables = [(0.5 * rng.standard_normal((G, H))).astype(np.float32) for _ in range(n_layers)]
    biases = [(0.1 * rng.standard_normal(H)).astype(np.float32) for _ in range(n_layers)]
    selfw = [None] + [(rng.standard_normal((H, H)) / np.sqrt(H)).astype(np.float32) for _ in range(n_layers - 1)]
    alpha = rng.uniform(0.5, 1.5, G + 2).astype(np.float32)
    w, b = (rng.standard_normal((C_, H)) / np.sqrt(H)).astype(np.float32), (0.1 * rng.standard_normal(C_)).astype(np.float32)
    ref = R.attribution(m, tables, alpha, biases, selfw, w, b)
    group = ref.target.copy()
    group[::7] = -1
    total, count, mag = M.reduce(m.indptr, m.indices, ref.scores, group, C_, G)
    n_cells, n_skipped, base_sum, logit_sum = M.group_stats(group, ref.base, ref.logit, C_)
    assert n_skipped == len(group[::7]) and n_cells.sum() == B - n_skipped
    scale = mag.sum(1) + np.abs(base_sum) + 1.0
    assert (np.abs(total.sum(1) + base_sum - logit_sum) <= 1e-12 * scale).all()


# ------------------------------------------------------------------------------------------------
# 3. MarkerTable on CPU tensors
# ------------------------------------------------------------------------------------------------
def _table(score_sum, count, n_cells, names=None):
    K, G = np.asarray(score_sum).shape
    return sda.MarkerTable(group_names=names or [f"g{i}" for i in range(K)], id2gene=[f"Gene{i}" for i in range(G)],
                           n_cells=np.asarray(n_cells, np.int64), n_skipped=0,
                           score_sum=torch.tensor(score_sum, dtype=torch.float64), expr_count=torch.tensor(count, dtype=torch.int32),
                           base_sum=np.zeros(K), logit_sum=np.zeros(K))


def test_mean_fraction_and_an_empty_group():
    t = _table([[2.0, -4.0, 0.0], [0.0, 0.0, 0.0]], [[1, 4, 0], [0, 0, 0]], [4, 0])
    assert torch.equal(t.mean_score(), torch.tensor([[0.5, -1.0, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64))
    assert torch.equal(t.fraction(), torch.tensor([[0.25, 1.0, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64))
    genes, scores = t.top(2)
    np.testing.assert_array_equal(genes, [[0, 1], [-1, -1]])         # gene 2 is not expressed; the empty group lists nothing
    np.testing.assert_array_equal(scores, np.array([[0.5, -1.0], [0.0, 0.0]], np.float32))
    assert genes.dtype == np.int64 and scores.dtype == np.float32


def test_top_tie_rule_padding_and_min_fraction():
    #           gene:   0     1     2     3     4     5
    s = [[3.0, 6.0, 6.0, 1.0, 6.0, 9.0]]
    c = [[2, 4, 4, 1, 4, 0]]                                          # gene 5: the best sum, but no cell expresses it
    t = _table(s, c, [4])
    genes, scores = t.top(8)
    np.testing.assert_array_equal(genes, [[1, 2, 4, 0, 3, -1, -1, -1]])        # equal scores by the lower gene id, -1 padding
    np.testing.assert_array_equal(scores, np.array([[1.5, 1.5, 1.5, 0.75, 0.25, 0, 0, 0]], np.float32))
    genes, _ = t.top(3, min_fraction=0.5)
    np.testing.assert_array_equal(genes, [[1, 2, 4]])
    genes, _ = t.top(5, min_fraction=0.75)
    np.testing.assert_array_equal(genes, [[1, 2, 4, -1, -1]])
    # keys are float32(mean): two fp64 means that round to one f32 tie, and the lower gene id wins
    t = _table([[1.0, 1.0 + 2.0 ** -40]], [[1, 1]], [1])
    np.testing.assert_array_equal(t.top(2)[0], [[0, 1]])
    with pytest.raises(ValueError):
        t.top(0)


def test_frame_columns():
    t = _table([[3.0, 6.0, 0.0], [0.0, -2.0, 8.0]], [[2, 4, 0], [0, 1, 2]], [4, 2], names=["B cell", "T cell"])
    f = t.frame(k=2)
    assert list(f.columns) == ["group", "n_cells", "rank", "gene", "mean_score", "fraction"]
    assert f["group"].tolist() == ["B cell", "B cell", "T cell", "T cell"]
    assert f["rank"].tolist() == [1, 2, 1, 2] and f["gene"].tolist() == ["Gene1", "Gene0", "Gene2", "Gene1"]
    assert f["n_cells"].tolist() == [4, 4, 2, 2]
    assert f["mean_score"].tolist() == [1.5, 0.75, 4.0, -1.0] and f["fraction"].tolist() == [1.0, 0.5, 1.0, 0.5]


def test_into_mismatches_and_host_sums():
    t = _table(np.zeros((2, 3)), np.zeros((2, 3), np.int32), [0, 0], names=["a", "b"])
    genes = [f"Gene{i}" for i in range(3)]
    t._require_same(["a", "b"], 3, genes)
    with pytest.raises(ValueError, match="groups"):
        t._require_same(["a", "b", "c"], 3, genes)
    with pytest.raises(ValueError, match="genes"):
        t._require_same(["a", "b"], 4, genes + ["Gene3"])
    with pytest.raises(ValueError, match="group names"):
        t._require_same(["a", "c"], 3, genes)
    with pytest.raises(ValueError, match="gene names"):
        t._require_same(["a", "b"], 3, ["Gene0", "Gene1", "other"])
    t._add_cells(np.array([0, -1, 1, 1]), np.array([1.0, 2.0, 3.0, 4.0], np.float32), np.array([10.0, 20.0, 30.0, 40.0], np.float32))
    t._add_cells(np.array([-1, 0]), np.array([5.0, 6.0], np.float32), np.array([50.0, 60.0], np.float32))
    assert t.n_cells.tolist() == [2, 2] and t.n_skipped == 2
    assert t.base_sum.tolist() == [7.0, 7.0] and t.logit_sum.tolist() == [70.0, 70.0] and t.base_sum.dtype == np.float64


# ------------------------------------------------------------------------------------------------
# 4. premises of the GPU suite's operands
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", M.GENES)
@pytest.mark.parametrize("K", M.GROUPS)
def test_lattice_cases_are_exact_in_fp64(K, G):
    for i64 in (False, True):
        c = M.case(K, G, i64)
        _, count, mag = M.reduce(c.rowptr, c.col, c.lat, c.group, K, G)
        assert M.exact_premise(mag)
        assert np.all(c.lat.astype(np.float64) / M.UNIT == np.round(c.lat.astype(np.float64) / M.UNIT))
        assert np.abs(c.lat).max() <= 1024
        # what the case is there for: empty rows, the long row, skipped cells, a group without a cell, an awkward B
        lens = np.diff(c.rowptr)
        assert (lens == 0).sum() >= 2 and lens.max() == min(5000, G) and (c.group < 0).any() and c.B % 2 == 1
        assert c.group[3] >= 0 and count.max() >= 1
        if K >= 2:
            assert not (c.group == K // 2).any()


@pytest.mark.parametrize("name", M.SPECIAL)
def test_special_cases_are_exact_in_fp64(name):
    c = M.special(name)
    _, count, mag = M.reduce(c.rowptr, c.col, c.lat, c.group, c.K, c.G)
    assert M.exact_premise(mag)
    if name == "one_group":
        assert (c.group == 9).all() and count[9].sum() == c.rowptr[-1]
    else:
        assert count.sum() == 0 and (c.B == 0 or (c.group < 0).all())


def test_ranking_case_leaves_out_at_most_two_percent():
    """The share of (group, rank) pairs the GPU ranking test skips, on the reference alone."""
    c = M.ranking_case()
    total, count, _ = M.reduce(c.rowptr, c.col, c.flt, c.group, c.K, c.G)
    n_cells = np.bincount(c.group[c.group >= 0], minlength=c.K)
    clear, exists = M.clear_pairs(M.ranking(total, count, n_cells), 20)
    assert exists.sum() >= 0.9 * c.K * 20
    assert (exists & ~clear).sum() <= 0.02 * exists.sum()
