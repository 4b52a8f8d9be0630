"""``wgnn_pool_rows_accumulate`` / ``_count`` / ``_fill`` (``ops.pool_rows``) on the GPU: the cases of tests/pool_reference.py
against the numpy reference and - without a tolerance - against the existing kernels (``pair_rows`` for groups of two,
``align_rows(..., normalize="lognorm")`` for a group of one and for every group whose sums a float32 holds), every case at a unit
geometry that small shapes cross (4 cells per unit, slabs of 128 genes: 3 slabs over 300 genes, the last one partial) and at the
defaults, with an int32 and an int64 rowptr."""
import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

import pairs_reference as P
import pool_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEOMETRIES = [(4, 128), (0, 0)]                                      # (cells_per_unit, slab_genes); 0 = the kernel's default
CASES = [(which, thr, i64, geo) for which in ("groups", "all") for thr in R.THRESHOLDS for i64 in (False, True) for geo in GEOMETRIES]
NAMES = ("rowptr", "col", "val", "cnt", "total", "n_cells")


def _operands(m, i64=True):
    rowptr = torch.from_numpy(m.rowptr if i64 else m.rowptr.astype(np.int32)).to(DEV)
    return rowptr, torch.from_numpy(m.col).to(DEV), torch.from_numpy(m.cnt).to(DEV), torch.from_numpy(m.lib).to(DEV)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _pool(c, i64=True, geo=(4, 128), **kw):
    return ops.pool_rows(*_operands(c.m, i64), _dev(c.group), c.K, threshold=c.threshold, cells_per_unit=geo[0], slab_genes=geo[1],
                         n_genes=c.m.G, **kw)


def _same(got, want):
    for name, x, y in zip(NAMES, got, want):
        assert x.dtype == y.dtype and torch.equal(x, y), name


@pytest.fixture(scope="module")
def pooled():
    """``ops.pool_rows`` of every case, computed once."""
    return {key: _pool(R.case(key[1], key[0]), key[2], key[3]) for key in CASES}


@pytest.mark.parametrize("which,thr,i64,geo", CASES)
def test_pool_against_the_reference(pooled, which, thr, i64, geo):
    ref = R.case(thr, which).ref
    rowptr, col, val, cnt, total, n_cells = pooled[which, thr, i64, geo]
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
    assert cnt.dtype == total.dtype == n_cells.dtype == torch.int64
    np.testing.assert_array_equal(rowptr.cpu().numpy(), ref.rowptr)
    np.testing.assert_array_equal(col.cpu().numpy(), ref.col)
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref.cnt)
    np.testing.assert_array_equal(total.cpu().numpy(), ref.total)
    np.testing.assert_array_equal(n_cells.cpu().numpy(), ref.n_cells)
    got, want = val.cpu().numpy().view(np.int32).astype(np.int64), ref.val.view(np.int32).astype(np.int64)
    frag = R.fragile(ref.v64)
    assert frag.mean() <= R.FRAGILE_CAP
    np.testing.assert_array_equal(got[~frag], want[~frag])
    assert (np.abs(got - want)[frag] <= 1).all()


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_a_sum_above_2_24_is_taken_exactly(pooled, geo):
    """2^23 + 2^23 + 1 of one gene against a total at which float32(2^24 + 1) = 2^24 gives another float32 value."""
    ref = R.case(0.0).ref
    rowptr, col, val, cnt, total, _ = (t.cpu().numpy() for t in pooled["groups", 0.0, True, geo])
    row = slice(rowptr[R.GROUP_BIG], rowptr[R.GROUP_BIG + 1])
    at = int(np.flatnonzero(col[row] == R.BIG_GENE)[0])
    assert cnt[row][at] == 16_777_217 and total[R.GROUP_BIG] == R.big_total()
    exact = np.float32(R._value(float(R.BIG_COUNT), float(R.big_total()), R.SCALE))
    through_f32 = np.float32(R._value(2.0 ** 24, float(R.big_total()), R.SCALE))
    assert exact != through_f32 and val[row][at] == exact == ref.val[row][at]


@pytest.mark.parametrize("thr", R.THRESHOLDS)
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_groups_a_float32_holds_are_align_rows_on_the_summed_matrix(pooled, thr, geo):
    """No tolerance: the groups' summed counts as a dense float32 matrix (one more column, mapped to -1, holding the reads outside
    the bundle) through the existing log-normalising alignment."""
    c = R.case(thr)
    x, gmap = R.summed_dense(c.m, c.group, c.K)
    small = R.small_groups(c.m, c.group, c.K)
    assert small.sum() == c.K - 1
    w_rowptr, w_col, w_val = ops.align_rows(_dev(x[small]), _dev(gmap), c.m.G, thr, normalize="lognorm", scale=R.SCALE)
    rowptr, col, val = pooled["groups", thr, True, geo][:3]
    lens = (rowptr[1:] - rowptr[:-1])
    keep = torch.repeat_interleave(_dev(small), lens)
    assert torch.equal(lens[_dev(small)], w_rowptr[1:] - w_rowptr[:-1])
    assert torch.equal(col[keep], w_col) and torch.equal(val[keep], w_val)


@pytest.mark.parametrize("thr", R.THRESHOLDS)
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_groups_of_two_are_pair_rows_and_a_group_of_one_is_the_aligned_row(thr, geo):
    m = P.batch()
    rng = np.random.default_rng(4)
    a = rng.permutation(m.B)[:m.B // 2 * 2].astype(np.int32)
    a, b = a[::2].copy(), a[1::2].copy()
    group = np.full(m.B, -1, np.int32)
    group[a] = np.arange(len(a)); group[b] = np.arange(len(a))
    kw = dict(threshold=thr, cells_per_unit=geo[0], slab_genes=geo[1], n_genes=m.G)
    got = ops.pool_rows(*_operands(m), _dev(group), len(a), **kw)
    want = ops.pair_rows(*_operands(m), _dev(a), _dev(b), threshold=thr)
    for g, w in zip(got[:3], want):
        assert torch.equal(g, w)
    # every cell a group of its own: the bits of the cell's own lognorm-aligned row
    own = ops.pool_rows(*_operands(m), torch.arange(m.B, dtype=torch.int32, device=DEV), m.B, **kw)
    dense = np.zeros((m.B, m.G + 1), np.float32)
    for r in range(m.B):
        dense[r, m.col[m.rowptr[r]:m.rowptr[r + 1]]] = m.cnt[m.rowptr[r]:m.rowptr[r + 1]]
    dense[:, m.G] = m.rest
    gmap = _dev(np.concatenate([np.arange(m.G), [-1]]).astype(np.int32))
    want = ops.align_rows(_dev(dense), gmap, m.G, thr, normalize="lognorm", scale=R.SCALE)
    for g, w in zip(own[:3], want):
        assert torch.equal(g, w)
    assert torch.equal(own[4], _dev(m.lib)) and bool((own[5] == 1).all())


def test_launches_splits_chunks_and_permutations_give_the_same_bits(pooled):
    c = R.case(0.0)
    whole = pooled["groups", 0.0, True, (4, 128)]
    _same(_pool(c), whole)                                             # two launches
    _same(pooled["groups", 0.0, True, (0, 0)], whole)                  # another unit geometry
    _same(pooled["groups", 0.0, False, (4, 128)], whole)               # an int32 rowptr
    _same(_pool(c, max_bytes=1), whole)                                # one group per chunk
    _same(_pool(c, geo=(3, 7)), whole)                                 # 43 slabs, units of 3 cells
    # the group list split in two
    half = c.K // 2
    lo = ops.pool_rows(*_operands(c.m), _dev(np.where(c.group < half, c.group, -1).astype(np.int32)), half, cells_per_unit=4,
                       slab_genes=128, n_genes=c.m.G)
    hi = ops.pool_rows(*_operands(c.m), _dev(np.where(c.group >= half, c.group - half, -1).astype(np.int32)), c.K - half,
                       cells_per_unit=4, slab_genes=128, n_genes=c.m.G)
    for i in (1, 2, 3, 4, 5):
        assert torch.equal(torch.cat([lo[i], hi[i]]), whole[i]), NAMES[i]
    assert torch.equal(torch.cat([lo[0], hi[0][1:] + lo[0][-1]]), whole[0])
    # the cells permuted, group permuted alongside
    perm = np.random.default_rng(9).permutation(c.m.B)
    lens = np.diff(c.m.rowptr)
    entries = np.concatenate([np.arange(c.m.rowptr[r], c.m.rowptr[r + 1]) for r in perm])
    rowptr = _dev(np.concatenate([[0], np.cumsum(lens[perm])]).astype(np.int64))
    shuffled = ops.pool_rows(rowptr, _dev(c.m.col[entries]), _dev(c.m.cnt[entries]), _dev(c.m.lib[perm]), _dev(c.group[perm]), c.K,
                             cells_per_unit=4, slab_genes=128, n_genes=c.m.G)
    _same(shuffled, whole)
    # seed: the first half of the cells, then the second half on top, against all at once
    first = np.arange(c.m.B) < c.m.B // 2
    part = ops.pool_rows(*_operands(c.m), _dev(np.where(first, c.group, -1).astype(np.int32)), c.K, cells_per_unit=4, slab_genes=128,
                         n_genes=c.m.G)
    assert 0 < int(part[5].sum()) < int(whole[5].sum())
    for geo, max_bytes in (((4, 128), ops.POOL_CHUNK_BYTES), ((0, 0), 3 * 8 * c.m.G)):
        both = ops.pool_rows(*_operands(c.m), _dev(np.where(first, -1, c.group).astype(np.int32)), c.K, cells_per_unit=geo[0],
                             slab_genes=geo[1], n_genes=c.m.G, seed=(part[0], part[1], part[3], part[4], part[5]), max_bytes=max_bytes)
        _same(both, whole)
    # n_genes left to pool_rows: the largest gene id plus one
    _same(ops.pool_rows(*_operands(c.m), _dev(c.group), c.K, cells_per_unit=4, slab_genes=128), whole)


def test_nothing_is_written_outside_the_outputs():
    """The C entries on buffers with guard elements before and after every output and behind every accumulator row
    (``ld_acc > n_genes``)."""
    c = R.case(0.0)
    ref, G, K, pad = c.ref, c.m.G, c.K, 64
    rowptr, col, cnt, _ = _operands(c.m)
    group = _dev(c.group)
    key = torch.where(group < 0, K, group.long())
    members = torch.sort(key, stable=True)[1].to(torch.int32)
    group_ptr = torch.zeros(K + 1, dtype=torch.int64, device=DEV)
    group_ptr[1:] = torch.cumsum(torch.bincount(key, minlength=K + 1)[:K], 0)
    ptr, stream, dev = ops._ptr, ops._stream(torch.device(DEV)), torch.device(DEV)
    ld = G + 8
    status = torch.zeros(1 + 2 * pad, dtype=torch.int32, device=DEV)
    acc = torch.full((K + 2, ld), -7, dtype=torch.int64, device=DEV)         # a guard row before and one after
    acc[1:K + 1, :G] = 0
    for geo in GEOMETRIES:
        acc[1:K + 1, :G] = 0
        _lib.check(_lib.call(dev, "wgnn_pool_rows_accumulate", ptr(rowptr), ptr(col), ptr(cnt), c.m.B, int(col.shape[0]),
                             ptr(group_ptr), ptr(members), K, G, ptr(acc[1:]), ld, geo[0], geo[1], ptr(status[pad:]),
                             _lib.FLAG_ROWPTR_I64, stream), "accumulate")
        assert (acc[0] == -7).all() and (acc[K + 1] == -7).all() and (acc[:, G:] == -7).all()
        want = np.zeros((K, G), np.int64)
        want[np.repeat(np.arange(K), np.diff(ref.rowptr)), ref.col] = ref.cnt
        np.testing.assert_array_equal(acc[1:K + 1, :G].cpu().numpy(), want)
    # the kernel ADDS: a second pass over a pre-seeded accumulator doubles it
    _lib.check(_lib.call(dev, "wgnn_pool_rows_accumulate", ptr(rowptr), ptr(col), ptr(cnt), c.m.B, int(col.shape[0]),
                         ptr(group_ptr), ptr(members), K, G, ptr(acc[1:]), ld, 4, 128, ptr(status[pad:]),
                         _lib.FLAG_ROWPTR_I64, stream), "accumulate")
    np.testing.assert_array_equal(acc[1:K + 1, :G].cpu().numpy(), 2 * want)
    acc[1:K + 1, :G] = _dev(want)
    total = _dev(ref.total)
    kept = int(ref.rowptr[-1])
    head = (ptr(acc[1:]), ld, ptr(total), K, G, R.SCALE, 0.0)
    n_out = torch.full((K + 2 * pad,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.call(dev, "wgnn_pool_rows_count", *head, ptr(n_out[pad:]), ptr(status[pad:]), stream), "count")
    assert (n_out[:pad] == -7).all() and (n_out[K + pad:] == -7).all()
    np.testing.assert_array_equal(n_out[pad:K + pad].cpu().numpy(), np.diff(ref.rowptr))
    out_rowptr = _dev(ref.rowptr)
    out_col = torch.full((kept + 2 * pad,), -7, dtype=torch.int32, device=DEV)
    out_val = torch.full((kept + 2 * pad,), -7.0, dtype=torch.float32, device=DEV)
    out_cnt = torch.full((kept + 2 * pad,), -7, dtype=torch.int64, device=DEV)
    _lib.check(_lib.call(dev, "wgnn_pool_rows_fill", *head, ptr(out_rowptr), ptr(out_col[pad:]), ptr(out_val[pad:]),
                         ptr(out_cnt[pad:]), ptr(status[pad:]), stream), "fill")
    for buf in (out_col, out_val, out_cnt):
        assert (buf[:pad] == -7).all() and (buf[kept + pad:] == -7).all()
    np.testing.assert_array_equal(out_col[pad:kept + pad].cpu().numpy(), ref.col)
    np.testing.assert_array_equal(out_cnt[pad:kept + pad].cpu().numpy(), ref.cnt)
    assert not status.any() and (acc[:, G:] == -7).all()
    # out_cnt may be NULL
    out_col.fill_(-7)
    _lib.check(_lib.call(dev, "wgnn_pool_rows_fill", *head, ptr(out_rowptr), ptr(out_col[pad:]), ptr(out_val[pad:]), None,
                         ptr(status[pad:]), stream), "fill")
    np.testing.assert_array_equal(out_col[pad:kept + pad].cpu().numpy(), ref.col)
    # out_rowptr that leaves the last group one slot less: the slot is not written, the status word says so
    short = out_rowptr.clone()
    short[-1] -= 1
    out_col.fill_(-7)
    _lib.check(_lib.call(dev, "wgnn_pool_rows_fill", *head, ptr(short), ptr(out_col[pad:]), ptr(out_val[pad:]), ptr(out_cnt[pad:]),
                         ptr(status[pad:]), stream), "fill")
    assert int(status[pad]) == _lib.POOL_BAD_ROWPTR and int(out_col[kept + pad - 1]) == -7 and (out_col[kept + pad:] == -7).all()
    assert not status[:pad].any() and not status[pad + 1:].any()


def test_malformed_operands_raise_through_the_status_word():
    """Skip paths: nothing faults, the status word raises."""
    c = R.case(0.0)
    m = c.m
    rowptr, col, cnt, lib = _operands(m)
    group = _dev(c.group)
    kw = dict(cells_per_unit=4, slab_genes=128, n_genes=m.G)
    key = torch.where(group < 0, c.K, group.long())
    members = torch.sort(key, stable=True)[1].to(torch.int32)
    group_ptr = torch.zeros(c.K + 1, dtype=torch.int64, device=DEV)
    group_ptr[1:] = torch.cumsum(torch.bincount(key, minlength=c.K + 1)[:c.K], 0)
    total = _dev(c.ref.total)
    good = ops.pool_rows_grouped(rowptr, col, cnt, group_ptr, members, total, m.G, cells_per_unit=4, slab_genes=128)
    np.testing.assert_array_equal(good[3].cpu().numpy(), c.ref.cnt)
    for bad in (m.B, -1):                                             # a member out of range
        wrong = members.clone()
        wrong[5] = bad
        with pytest.raises(sda.WgnnError, match="outside \\[0, n_rows\\)"):
            ops.pool_rows_grouped(rowptr, col, cnt, group_ptr, wrong, total, m.G, cells_per_unit=4, slab_genes=128)
    beyond = rowptr.clone()                                           # a rowptr that points past col
    beyond[m.ROW_BIG_C + 1] += 5
    with pytest.raises(sda.WgnnError, match="rowptr points outside"):
        ops.pool_rows(beyond, col, cnt, lib, group, c.K, **kw)
    for at, value in ((3, 1), (c.K, m.B + 1), (0, -1)):               # a group_ptr that descends, runs past the members, starts below 0
        wrong = group_ptr.clone()
        wrong[at] = value
        with pytest.raises(sda.WgnnError, match="group_ptr is not ascending"):
            ops.pool_rows_grouped(rowptr, col, cnt, wrong, members, total, m.G, cells_per_unit=4, slab_genes=128)
    with pytest.raises(sda.WgnnError, match="gene id is outside"):    # a gene id at n_genes and beyond
        ops.pool_rows(rowptr, col, cnt, lib, group, c.K, cells_per_unit=4, slab_genes=128, n_genes=m.G - 1)
    negative = col.clone()
    negative[int(m.rowptr[P.ROW_65]) + 2] = -3
    with pytest.raises(sda.WgnnError, match="gene id is outside"):
        ops.pool_rows(rowptr, negative, cnt, lib, group, c.K, **kw)
    # argument errors
    for bad_kw in (dict(scale=0.0), dict(threshold=-1.0), dict(cells_per_unit=257), dict(slab_genes=16385), dict(max_bytes=0)):
        with pytest.raises(ValueError):
            ops.pool_rows(rowptr, col, cnt, lib, group, c.K, **{**kw, **bad_kw})
    with pytest.raises(ValueError, match="lib"):
        ops.pool_rows(rowptr, col, cnt, lib.int(), group, c.K, **kw)
    with pytest.raises(ValueError, match="group"):
        ops.pool_rows(rowptr, col, cnt, lib, group.long(), c.K, **kw)
    with pytest.raises(ValueError, match="out of range"):
        ops.pool_rows(rowptr, col, cnt, lib, group, c.K - 1, **kw)
    with pytest.raises(ValueError, match="seed"):
        ops.pool_rows(rowptr, col, cnt, lib, group, c.K, seed=(good[0][:-1], good[1], good[3], total, total), **kw)
    huge = lib.clone()
    huge[m.ROW_BIG_A] = 2 ** 53
    with pytest.raises(ValueError, match=f"group {R.GROUP_BIG} pools"):
        ops.pool_rows(rowptr, col, cnt, huge, group, c.K, **kw)
    none = ops.pool_rows(rowptr, col, cnt, lib, torch.full_like(group, -1), 2, **kw)          # every cell skipped
    assert none[0].tolist() == [0, 0, 0] and none[1].numel() == 0 and none[5].tolist() == [0, 0]
