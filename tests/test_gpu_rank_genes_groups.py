"""``ops.rank_genes_groups`` / ``wgnn_rank_genes_groups`` on the GPU: all three integer tables exactly the ``rankdata``
reference's (tests/rank_genes_reference.py) - gene lengths at the wave, vector and owner-block edges, 1 to 1 500 groups with
skipped cells, an empty group and a group of one cell, both rowptr widths, guarded outputs, two launches, genes around the
16 384-key slab, permuted cells and genes, the key order, stray entries, and the wrapper's refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops
from scdeepsort_amd.graph import _ptr, _stream

import rank_genes_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 40
GUARD = -7777


@functools.lru_cache(maxsize=None)
def _edge():
    return R.edge_case()


@functools.lru_cache(maxsize=None)
def _edge_want(K):
    group = R.groups_of(600, K, seed=K)
    return group, R.tables(*_edge(), group, K, G)


@functools.lru_cache(maxsize=None)
def _slab():
    rowptr, col, val = R.slab_case()
    group = R.groups_of(17000, 13, seed=3)
    return rowptr, col, val, group, R.tables(rowptr, col, val, group, 13, 6)


def _run(rowptr, col, val, group, K, n_genes, width=torch.int64, **kw):
    out = sda.rank_genes_groups(torch.from_numpy(np.asarray(rowptr)).to(DEV, width), torch.from_numpy(col).to(DEV),
                                torch.from_numpy(val).to(DEV), torch.from_numpy(np.asarray(group)).to(DEV), K, n_genes, **kw)
    return tuple(t.cpu().numpy() for t in out)


def _same(got, want):
    for g, w, dt in zip(got, want, (np.int64, np.int32, np.int64, np.int64)):
        assert g.dtype == dt and g.shape == w.shape
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("K", [1, 2, 13, 300, 1500])
def test_edge_lengths_and_groups_with_guards(K):
    """K = 1 500 is past the 1 024 bins of one pass of the block reduction."""
    rowptr, col, val = _edge()
    group, want = _edge_want(K)
    assert sorted(set(np.bincount(col, minlength=G).tolist())) == sorted(R.GENE_LENGTHS)
    if K >= 3:
        assert want[3][1] == 0 and want[3][2] == 1 and (group < 0).any()
    got = _run(rowptr, col, val, group, K, G)
    _same(got, want)
    # int32 row pointers, into guarded views with ld > G
    r2 = torch.full((K + 2, G + 5), GUARD, dtype=torch.int64, device=DEV)
    cnt = torch.full((K + 2, G + 3), GUARD, dtype=torch.int32, device=DEV)
    tie = torch.full((G + 4,), GUARD, dtype=torch.int64, device=DEV)
    out = (r2[1:K + 1, 2:G + 2], cnt[1:K + 1, 2:G + 2], tie[2:G + 2])
    again = _run(rowptr, col, val, group, K, G, width=torch.int32, out=out)
    _same(again, want)                                                             # and two launches are bit-identical
    for t in (r2, cnt, tie):
        guard = torch.ones_like(t, dtype=torch.bool)
        if t.dim() == 2:
            guard[1:K + 1, 2:G + 2] = False
        else:
            guard[2:G + 2] = False
        assert bool((t[guard] == GUARD).all())


def test_genes_around_the_slab_limit():
    rowptr, col, val, group, want = _slab()
    assert np.bincount(col, minlength=6).tolist() == [16384, 16385, 17000, 16385, 100, 0]
    got = _run(rowptr, col, val, group, 13, 6)
    _same(got, want)
    _same(_run(rowptr, col, val, group, 13, 6), got)
    n = int((group >= 0).sum())
    assert want[2][5] == n ** 3 - n and want[2][3] > want[2][1]                    # nobody's gene; the all-tied gene


def test_cell_order_and_gene_order_do_not_matter():
    rowptr, col, val = _edge()
    group, want = _edge_want(13)
    rng = np.random.default_rng(11)
    # the cells permuted (their groups with them)
    perm = rng.permutation(600)
    deg = np.diff(rowptr)
    p_rowptr = np.concatenate([[0], np.cumsum(deg[perm])]).astype(np.int64)
    take = np.concatenate([np.arange(rowptr[i], rowptr[i + 1]) for i in perm])
    _same(_run(p_rowptr, col[take], val[take], group[perm], 13, G), want)
    # the genes permuted inside every cell
    take = np.concatenate([rng.permutation(np.arange(rowptr[i], rowptr[i + 1])) for i in range(600)])
    assert (take != np.arange(len(col))).any()
    _same(_run(rowptr, col[take], val[take], group, 13, G), want)


def test_key_order_negatives_signed_zeros_and_a_nan():
    rng = np.random.default_rng(5)
    mask = rng.random((90, 5)) < 0.6
    mask[:, 4] = True
    mask[7, 1] = True
    values = rng.choice(np.array([-2.5, -1.0, -0.0, 0.0, 0.5, 1.0, 3.0], np.float32), size=mask.shape)
    values[7, 1] = np.nan
    values[:, 4] = rng.choice(np.array([-0.0, 0.0], np.float32), size=90)
    rowptr, col, val = R.csr_of(mask, values)
    assert np.isnan(val).sum() == 1 and (np.signbit(val) & (val == 0)).any() and (~np.signbit(val) & (val == 0)).any()
    group = R.groups_of(90, 4, seed=6)
    want = R.tables(rowptr, col, val, group, 4, 5)
    _same(_run(rowptr, col, val, group, 4, 5), want)
    # -0.0 is not the implicit +0.0: a gene holding only signed zeros still has two tie groups
    n = int((group >= 0).sum())
    assert want[2][4] < n ** 3 - n


def test_stray_groups_take_no_part():
    rowptr, col, val = _edge()
    group, _ = _edge_want(13)
    stray = group.copy()
    stray[::7] = 13 + (np.arange(len(stray[::7])) % 3) * 1000                       # out of range above, several values
    stray[3::50] = -5                                                              # and below
    want = R.tables(rowptr, col, val, stray, 13, G)
    assert want[3].sum() < (group >= 0).sum()
    with pytest.raises(ValueError, match="out of range"):
        _run(rowptr, col, val, stray, 13, G)
    _same(_run(rowptr, col, val, stray, 13, G, check=False), want)
    # around the slab limit, where a gene with a stray is compacted chunk by chunk
    rowptr, col, val, group, _ = _slab()
    stray = group.copy()
    stray[100::997] = 13
    _same(_run(rowptr, col, val, stray, 13, 6, check=False), R.tables(rowptr, col, val, stray, 13, 6))


def test_stray_cell_ids_at_the_c_abi():
    """The gene-major operand handed to the export directly, some cell ids outside [0, n_rows): those ENTRIES take no part,
    their cells still hold an implicit zero."""
    rowptr, col, val = _edge()
    group, _ = _edge_want(13)
    B, K = 600, 13
    rng = np.random.default_rng(2)
    rows = np.repeat(np.arange(B), np.diff(rowptr))
    order = np.lexsort((rows, col))                                                # gene-major, cells ascending
    t_cell, t_val = rows[order].astype(np.int32), val[order]
    t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=G))]).astype(np.int32)
    bad = rng.random(len(t_cell)) < 0.02
    t_bad = t_cell.copy()
    t_bad[bad] = rng.choice(np.array([-1, B, B + 7, 2 ** 31 - 1, -2 ** 31], np.int64), size=int(bad.sum())).astype(np.int32)
    keep = np.ones(len(col), bool)
    keep[order[bad]] = False
    k_rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=B))]).astype(np.int64)
    want = R.tables(k_rowptr, col[keep], val[keep], group, K, G)
    dev = torch.device(DEV)
    ops_in = [torch.from_numpy(a).to(dev) for a in (t_rowptr, t_bad, t_val, group.astype(np.int32), want[3])]
    r2 = torch.empty((K, G), dtype=torch.int64, device=dev)
    cnt = torch.empty((K, G), dtype=torch.int32, device=dev)
    tie = torch.empty(G, dtype=torch.int64, device=dev)
    nb = C.c_int64()
    assert _lib.lib().wgnn_rank_genes_groups_workspace(B, len(col), K, G, C.addressof(nb)) == 0
    ws = torch.empty(nb.value // 8 + 1, dtype=torch.int64, device=dev)
    rc = _lib.call(dev, "wgnn_rank_genes_groups", *map(_ptr, ops_in), B, K, G, _ptr(r2), G, _ptr(cnt), G, _ptr(tie), _ptr(ws),
                   nb.value, 0, _stream(dev))
    assert rc == 0
    _same((r2.cpu().numpy(), cnt.cpu().numpy(), tie.cpu().numpy(), want[3]), want)


def test_an_empty_batch_and_a_batch_without_entries():
    z64, z32 = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV)
    r2, cnt, tie, size = sda.rank_genes_groups(z64, z32, torch.zeros(0, device=DEV), z32, 3, 7)
    assert not r2.any() and not cnt.any() and not tie.any() and not size.any() and r2.shape == (3, 7)
    got = _run(np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), np.array([0, 0, 1, -1, 1]), 2, 3)
    _same(got, R.tables(np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), np.array([0, 0, 1, -1, 1]), 2, 3))
    assert got[0].tolist() == [[10] * 3, [10] * 3] and got[2].tolist() == [60] * 3      # four tied values: rank 2.5, 4^3 - 4


def test_wrapper_refusals():
    rp = torch.tensor([0, 1, 2], dtype=torch.int64, device=DEV)
    col = torch.zeros(2, dtype=torch.int32, device=DEV)
    val = torch.ones(2, device=DEV)
    group = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="n_groups"):
        sda.rank_genes_groups(rp, col, val, group, 4097, 3)
    with pytest.raises(ValueError, match="n_groups"):
        sda.rank_genes_groups(rp, col, val, group, 0, 3)
    with pytest.raises(ValueError, match="n_genes"):
        sda.rank_genes_groups(rp, col, val, group, 2, 0)
    with pytest.raises(ValueError, match="2\\^20"):
        sda.rank_genes_groups(torch.zeros(2 ** 20 + 2, dtype=torch.int32, device=DEV), col[:0], val[:0],
                              torch.zeros(2 ** 20 + 1, dtype=torch.int32, device=DEV), 2, 3)
    for bad in (dict(col=col.long()), dict(val=val.double()), dict(rp=rp.to(torch.int16)), dict(group=group.float()),
                dict(val=val[:1]), dict(group=group[:1])):
        a = {**dict(rp=rp, col=col, val=val, group=group), **bad}
        with pytest.raises(ValueError):
            sda.rank_genes_groups(a["rp"], a["col"], a["val"], a["group"], 2, 3)
    with pytest.raises(sda.WgnnError, match="out of range"):
        sda.rank_genes_groups(rp, col + 3, val, group, 2, 3)
    with pytest.raises(ValueError, match="tie_sum"):
        sda.rank_genes_groups(rp, col, val, group, 2, 3, out=(torch.zeros((2, 3), dtype=torch.int64, device=DEV),
                                                              torch.zeros((2, 3), dtype=torch.int32, device=DEV),
                                                              torch.zeros(4, dtype=torch.int64, device=DEV)))
    r2, cnt, tie, size = sda.rank_genes_groups(rp, col, val, group, 2, 3)              # and the next call runs
    assert r2.tolist() == [[6, 6, 6], [0, 0, 0]] and cnt.tolist() == [[2, 0, 0], [0, 0, 0]] and size.tolist() == [2, 0]
    assert tie.tolist() == [6, 6, 6]
