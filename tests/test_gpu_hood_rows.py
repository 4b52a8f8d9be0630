"""``wgnn_hood_rows_count`` / ``wgnn_hood_rows_fill`` (``ops.hood_rows``) on the GPU: the cases of tests/hood_reference.py - 40
rows over 300 genes, units of 0 to 256 members - bit for bit against the numpy reference and against the existing kernels
(``align_rows(..., normalize="lognorm")`` for units of one, ``pair_rows`` for units of two, ``pool_rows_grouped`` for a
partition of the cells), at the default slab and at slabs of 128 genes (three over 300 genes, the last of 44), at threshold 0
(the counting walk's shortcut) and at a positive threshold, with an int32 and an int64 rowptr.  No tolerance anywhere: the
reference's values are decided (tests/test_hood_reference.py)."""
import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

import hood_reference as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLABS = (0, 128)
CASES = [(thr, slab) for thr in H.THRESHOLDS for slab in SLABS]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _operands(m, i64=True):
    return _dev(m.rowptr if i64 else m.rowptr.astype(np.int32)), _dev(m.col), _dev(m.cnt), _dev(m.lib)


def _hood(m, units, thr, slab=128, i64=True):
    ptr, members = H.lists(units)
    return ops.hood_rows(*_operands(m, i64), _dev(ptr), _dev(members), m.G, scale=H.SCALE, threshold=thr, slab_genes=slab)


def _same(got, want):
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and torch.equal(x, y)


@pytest.fixture(scope="module")
def pooled():
    """``ops.hood_rows`` of every case, computed once."""
    return {(thr, slab): _hood(H.batch(), H.units(), thr, slab) for thr, slab in CASES}


@pytest.mark.parametrize("thr,slab", CASES)
def test_hood_rows_against_the_reference(pooled, thr, slab):
    ref = H.case(thr).ref
    rowptr, col, val, cnt = pooled[thr, slab]
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32 and cnt.dtype == torch.int64
    np.testing.assert_array_equal(rowptr.cpu().numpy(), ref.rowptr)
    np.testing.assert_array_equal(col.cpu().numpy(), ref.col)
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref.cnt)
    np.testing.assert_array_equal(val.cpu().numpy().view(np.int32), ref.val.view(np.int32))
    row = slice(int(rowptr[H.UNIT_256]), int(rowptr[H.UNIT_256 + 1]))
    assert int(cnt[row][col[row] == H.BIG_GENE]) == 2 ** 31            # 256 x 2^23: the uint32 counter's limit, and c > 2^24


@pytest.mark.parametrize("thr,slab", CASES)
def test_units_of_one_are_the_cells_own_aligned_rows(thr, slab):
    """Every cell a unit of its own: the existing log-normalising alignment of the dense count matrix, one more column (mapped
    to -1) holding the reads outside the bundle."""
    m = H.batch()
    own = [[r] for r in range(m.B)]
    x, gmap = H.summed_dense(m, own)
    want = ops.align_rows(_dev(x), _dev(gmap), m.G, thr, normalize="lognorm", scale=H.SCALE)
    _same(_hood(m, own, thr, slab)[:3], want)


@pytest.mark.parametrize("thr,slab", CASES)
def test_units_of_two_are_pair_rows(thr, slab):
    m = H.batch()
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, m.B, 50), rng.integers(0, m.B, 50)
    a[:3], b[:3] = (H.ROW_ALL, H.ROW_EMPTY, 9), (H.ROW_BIG, H.ROW_EMPTY_READS, 9)                # and a cell paired with itself
    want = ops.pair_rows(*_operands(m), _dev(a.astype(np.int32)), _dev(b.astype(np.int32)), scale=H.SCALE, threshold=thr)
    _same(_hood(m, [[int(x), int(y)] for x, y in zip(a, b)], thr, slab)[:3], want)


@pytest.mark.parametrize("thr,slab", CASES)
def test_a_partition_of_the_cells_is_pool_rows(thr, slab):
    m = H.batch()
    K = 6
    group = np.random.default_rng(6).integers(0, K - 1, m.B)           # the last group holds no cell
    group[[H.ROW_BIG, H.ROW_BIG_ONE]] = 0
    order = np.argsort(group, kind="stable")
    group_ptr = np.concatenate([[0], np.cumsum(np.bincount(group, minlength=K))]).astype(np.int64)
    total = np.bincount(group, weights=m.lib, minlength=K).astype(np.int64)
    rowptr, col, cnt, _ = _operands(m)
    want = ops.pool_rows_grouped(rowptr, col, cnt, _dev(group_ptr), _dev(order.astype(np.int32)), _dev(total), m.G, H.SCALE, thr)
    got = _hood(m, [[int(r) for r in order[group_ptr[k]:group_ptr[k + 1]]] for k in range(K)], thr, slab)
    assert int(got[0][K] - got[0][K - 1]) == 0
    _same(got, want)


def test_launches_widths_slabs_splits_and_member_orders_give_the_same_bits(pooled):
    m, units = H.batch(), H.units()
    for thr in H.THRESHOLDS:
        whole = pooled[thr, 128]
        _same(_hood(m, units, thr), whole)                             # two launches
        _same(pooled[thr, 0], whole)                                   # one slab
        _same(_hood(m, units, thr, slab=7), whole)                     # 43 slabs
        _same(_hood(m, units, thr, i64=False), whole)                  # an int32 rowptr
        _same(_hood(m, units, thr, slab=0, i64=False), whole)
        # every unit's members in another order
        rng = np.random.default_rng(8)
        _same(_hood(m, [[u[i] for i in rng.permutation(len(u))] for u in units], thr), whole)
        # the units split at q0: hood_ptr + q0 next to the same members
        ptr, members = H.lists(units)
        for q0 in (0, H.UNIT_256, len(units)):
            parts = [ops.hood_rows(*_operands(m, i64), _dev(p), _dev(members), m.G, scale=H.SCALE, threshold=thr, slab_genes=128)
                     for i64, p in ((True, ptr[:q0 + 1]), (False, ptr[q0:]))]
            e0 = int(whole[0][q0])
            assert torch.equal(parts[0][0], whole[0][:q0 + 1]) and torch.equal(parts[1][0], whole[0][q0:] - e0)
            for i in (1, 2, 3):
                assert torch.equal(parts[0][i], whole[i][:e0]) and torch.equal(parts[1][i], whole[i][e0:])
    # the entries of every row in another order: rows need not be sorted
    rng = np.random.default_rng(9)
    order = np.concatenate([m.rowptr[r] + rng.permutation(m.rowptr[r + 1] - m.rowptr[r]) for r in range(m.B)]).astype(np.int64)
    ptr, members = H.lists(units)
    shuffled = ops.hood_rows(_dev(m.rowptr), _dev(m.col[order]), _dev(m.cnt[order]), _dev(m.lib), _dev(ptr), _dev(members), m.G,
                             slab_genes=128)
    _same(shuffled, pooled[0.0, 128])


def _entry_args(m, rowptr, col, cnt, lib, ptr, members, thr=0.0, slab=128):
    return (ops._ptr(rowptr), ops._ptr(col), ops._ptr(cnt), m.B, int(col.shape[0]), ops._ptr(lib), ops._ptr(ptr), ops._ptr(members),
            int(ptr.shape[0]) - 1, int(members.shape[0]), m.G, H.SCALE, thr, slab)


def test_nothing_is_written_outside_the_outputs():
    """The C entries on buffers with guard elements before and after every output; ``out_cnt`` may be NULL; an ``out_rowptr``
    that leaves the last unit one slot short sets the bit and writes nothing past the slot."""
    c = H.case(0.0)
    ref, pad = c.ref, 64
    n_units, kept = len(c.units), int(c.ref.rowptr[-1])
    dev, stream = torch.device(DEV), ops._stream(torch.device(DEV))
    operands = (*_operands(c.m), _dev(c.hood_ptr), _dev(c.members))    # held: the entries take addresses
    head = _entry_args(c.m, *operands)
    status = torch.zeros(1 + 2 * pad, dtype=torch.int32, device=DEV)
    n_out = torch.full((n_units + 2 * pad,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.call(dev, "wgnn_hood_rows_count", *head, ops._ptr(n_out[pad:]), ops._ptr(status[pad:]), _lib.FLAG_ROWPTR_I64,
                         stream), "count")
    assert (n_out[:pad] == -7).all() and (n_out[n_units + pad:] == -7).all()
    np.testing.assert_array_equal(n_out[pad:n_units + pad].cpu().numpy(), np.diff(ref.rowptr))
    out_rowptr = _dev(ref.rowptr)
    out_col = torch.full((kept + 2 * pad,), -7, dtype=torch.int32, device=DEV)
    out_val = torch.full((kept + 2 * pad,), -7.0, dtype=torch.float32, device=DEV)
    out_cnt = torch.full((kept + 2 * pad,), -7, dtype=torch.int64, device=DEV)
    fill = lambda ptr, cnt_buf: _lib.check(_lib.call(dev, "wgnn_hood_rows_fill", *head, ops._ptr(ptr), ops._ptr(out_col[pad:]),
                                                     ops._ptr(out_val[pad:]), cnt_buf, ops._ptr(status[pad:]), _lib.FLAG_ROWPTR_I64,
                                                     stream), "fill")
    fill(out_rowptr, ops._ptr(out_cnt[pad:]))
    for buf in (out_col, out_val, out_cnt):
        assert (buf[:pad] == -7).all() and (buf[kept + pad:] == -7).all()
    np.testing.assert_array_equal(out_col[pad:kept + pad].cpu().numpy(), ref.col)
    np.testing.assert_array_equal(out_cnt[pad:kept + pad].cpu().numpy(), ref.cnt)
    np.testing.assert_array_equal(out_val[pad:kept + pad].cpu().numpy().view(np.int32), ref.val.view(np.int32))
    assert not status.any()
    out_col.fill_(-7)
    fill(out_rowptr, None)                                             # out_cnt may be NULL
    np.testing.assert_array_equal(out_col[pad:kept + pad].cpu().numpy(), ref.col)
    assert not status.any()
    short = out_rowptr.clone()
    short[-1] -= 1
    out_col.fill_(-7)
    fill(short, ops._ptr(out_cnt[pad:]))
    assert int(status[pad]) == _lib.HOOD_BAD_ROWPTR and int(out_col[kept + pad - 1]) == -7 and (out_col[kept + pad:] == -7).all()
    np.testing.assert_array_equal(out_col[pad:kept + pad - 1].cpu().numpy(), ref.col[:-1])
    assert not status[:pad].any() and not status[pad + 1:].any()


def test_malformed_operands_set_exactly_their_bit_and_leave_the_other_units_intact():
    """Skip paths: nothing faults, the status word says what was skipped, every unit the operand does not touch is as before."""
    c = H.case(0.0)
    m, units = c.m, c.units
    n_units = len(units)
    rowptr, col, cnt, lib = _operands(m)
    ptr, members = _dev(c.hood_ptr), _dev(c.members)
    good = _hood(m, units, 0.0)
    kw = dict(scale=H.SCALE, threshold=0.0, slab_genes=128)

    def raw(rowptr=rowptr, col=col, ptr=ptr, members=members):
        """(status bits, out_rowptr, col, val, cnt) through the C entries, whatever the status word says."""
        dev, stream = torch.device(DEV), ops._stream(torch.device(DEV))
        head = _entry_args(m, rowptr, col, cnt, lib, ptr, members)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        n_out = torch.empty(n_units, dtype=torch.int32, device=DEV)
        _lib.check(_lib.call(dev, "wgnn_hood_rows_count", *head, ops._ptr(n_out), ops._ptr(status), _lib.FLAG_ROWPTR_I64, stream), "count")
        o_ptr = torch.zeros(n_units + 1, dtype=torch.int64, device=DEV)
        torch.cumsum(n_out, 0, dtype=torch.int64, out=o_ptr[1:])
        o_col = torch.empty(int(o_ptr[-1]), dtype=torch.int32, device=DEV)
        o_val = torch.empty(int(o_ptr[-1]), dtype=torch.float32, device=DEV)
        o_cnt = torch.empty(int(o_ptr[-1]), dtype=torch.int64, device=DEV)
        _lib.check(_lib.call(dev, "wgnn_hood_rows_fill", *head, ops._ptr(o_ptr), ops._ptr(o_col), ops._ptr(o_val), ops._ptr(o_cnt),
                             ops._ptr(status), _lib.FLAG_ROWPTR_I64, stream), "fill")
        return int(status), o_ptr, o_col, o_val, o_cnt

    def unit(got, q):
        a, b = int(got[1][q]), int(got[1][q + 1])
        return [t[a:b] for t in got[2:]]

    def intact(got, but):
        """Every unit outside ``but`` equals the good result."""
        for q in range(n_units):
            if q not in but:
                a, b = int(good[0][q]), int(good[0][q + 1])
                for x, y in zip(unit(got, q), (good[1][a:b], good[2][a:b], good[3][a:b])):
                    assert torch.equal(x, y), q

    def without(q, drop):
        """The reference's row of unit ``q`` with the members at the positions ``drop`` left out."""
        left = [r for i, r in enumerate(units[q]) if i not in drop]
        ref = H.hood_rows(m.rowptr, m.col, m.cnt, m.lib, *H.lists([left]), 0.0)
        return ref.col, ref.val, ref.cnt

    def equals(got_unit, want):
        for x, y in zip(got_unit, want):
            np.testing.assert_array_equal(x.cpu().numpy(), y)

    assert raw()[0] == 0
    Q = H.UNIT_RAGGED + 1                                              # the ragged unit of 9 members
    at = int(c.hood_ptr[Q]) + 4
    # a member outside [0, n_rows): that member is skipped, counts and library size
    for bad in (m.B, -1, 2 ** 31 - 1):
        wrong = members.clone()
        wrong[at] = bad
        got = raw(members=wrong)
        assert got[0] == _lib.HOOD_BAD_INDEX
        intact(got, {Q})
        equals(unit(got, Q), without(Q, {4}))
        with pytest.raises(sda.WgnnError, match="outside \\[0, n_rows\\)"):
            ops.hood_rows(rowptr, col, cnt, lib, ptr, wrong, m.G, **kw)
    # a row range outside [0, nnz]: the members that name the row are skipped
    victim = int(c.members[at])
    for edit in ((m.B, m.rowptr[-1] + 5), (victim, -1)):
        beyond = rowptr.clone()
        beyond[edit[0]] = int(edit[1])
        broken = m.B - 1 if edit[0] == m.B else victim                 # the row whose range left [0, nnz] ...
        if edit[0] == victim and victim > 0:
            broken = {victim - 1, victim}                              # ... or the two rows around a pointer below 0
        broken = broken if isinstance(broken, set) else {broken}
        got = raw(rowptr=beyond)
        assert got[0] == _lib.HOOD_BAD_ROWPTR
        touched = {q for q, u in enumerate(units) if broken & set(u)}
        intact(got, touched)
        for q in touched:
            equals(unit(got, q), without(q, {i for i, r in enumerate(units[q]) if r in broken}))
        with pytest.raises(sda.WgnnError, match="rowptr points outside"):
            ops.hood_rows(beyond, col, cnt, lib, ptr, members, m.G, **kw)
    # a hood_ptr range that descends or leaves [0, n_members]: the unit leaves the empty row
    for q, value in ((Q, int(c.hood_ptr[Q - 1]) - 1), (n_units, len(c.members) + 1), (0, -1)):
        wrong = ptr.clone()
        wrong[q] = value
        got = raw(ptr=wrong)
        assert got[0] == _lib.HOOD_BAD_ROWPTR
        bent = {u for u in (q - 1, q) if 0 <= u < n_units}             # the units on either side of the pointer
        empty = [u for u in bent if int(wrong[u]) < 0 or int(wrong[u + 1]) < int(wrong[u]) or int(wrong[u + 1]) > len(c.members)]
        assert empty and all(int(got[1][u + 1] - got[1][u]) == 0 for u in empty)
        intact(got, bent)
        with pytest.raises(sda.WgnnError, match="hood_ptr is not ascending"):
            ops.hood_rows(rowptr, col, cnt, lib, wrong, members, m.G, **kw)
    # gene ids outside [0, G): the entries are skipped
    for bad_id in (m.G, -3):
        wrong = col.clone()
        wrong[int(m.rowptr[H.ROW_65]) + 2] = bad_id
        got = raw(col=wrong)
        assert got[0] == _lib.HOOD_BAD_COL
        intact(got, {q for q, u in enumerate(units) if H.ROW_65 in u})
        lost = int(m.col[m.rowptr[H.ROW_65] + 2])                      # the unit of that row alone loses exactly this gene
        a, b = int(good[0][H.UNIT_ONE]), int(good[0][H.UNIT_ONE + 1])
        equals(unit(got, H.UNIT_ONE), [t[a:b][good[1][a:b] != lost].cpu().numpy() for t in good[1:]])
        with pytest.raises(sda.WgnnError, match="gene id is outside"):
            ops.hood_rows(rowptr, wrong, cnt, lib, ptr, members, m.G, **kw)
    # more than 256 members: the unit leaves the empty row
    long_ptr, long_members = H.lists(list(units) + [[H.ROW_ONE] * 257])
    n_units += 1
    got = raw(ptr=_dev(long_ptr), members=_dev(long_members))
    assert got[0] == _lib.HOOD_BAD_SIZE and int(got[1][-1] - got[1][-2]) == 0
    intact(got, {n_units - 1})
    with pytest.raises(sda.WgnnError, match="more than 256 members"):
        ops.hood_rows(rowptr, col, cnt, lib, _dev(long_ptr), _dev(long_members), m.G, **kw)
    # argument errors
    for bad_kw in (dict(scale=0.0), dict(threshold=-1.0), dict(slab_genes=16385), dict(slab_genes=-1)):
        with pytest.raises(ValueError):
            ops.hood_rows(rowptr, col, cnt, lib, ptr, members, m.G, **{**kw, **bad_kw})
    with pytest.raises(ValueError, match="lib"):
        ops.hood_rows(rowptr, col, cnt, lib.int(), ptr, members, m.G, **kw)
    with pytest.raises(ValueError, match="hood_ptr"):
        ops.hood_rows(rowptr, col, cnt, lib, ptr.int(), members, m.G, **kw)
    with pytest.raises(ValueError, match="members"):
        ops.hood_rows(rowptr, col, cnt, lib, ptr, members.long(), m.G, **kw)
    with pytest.raises(ValueError, match="n_genes"):
        ops.hood_rows(rowptr, col, cnt, lib, ptr, members, -1, **kw)
    none = ops.hood_rows(rowptr, col, cnt, lib, ptr[:1], members, m.G, **kw)             # no unit
    assert none[0].tolist() == [0] and all(t.numel() == 0 for t in none[1:])
    no_rows = ops.hood_rows(rowptr[:1], col[:0], cnt[:0], lib[:0], torch.zeros(3, dtype=torch.int64, device=DEV), members[:0], m.G, **kw)
    assert no_rows[0].tolist() == [0, 0, 0]                                              # no row, units without a member
