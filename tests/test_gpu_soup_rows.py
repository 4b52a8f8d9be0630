"""``wgnn_soup_rows_count`` / ``wgnn_soup_rows_fill`` (``ops.soup_rows``) on the GPU: the cases of tests/soup_reference.py against
the numpy reference and - without a tolerance - against the device's own ``align_rows(..., normalize="lognorm")`` on the
host-materialised contaminated count matrix, at the default slab and at slabs of 128 genes (three over 300 genes, the last of 44),
with an int32 and an int64 rowptr."""
import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

import soup_reference as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLABS = (0, 128)
PROFILES = ("uniform", "one", "rest", "wide")
CASES = [(name, thr, slab) for name in PROFILES for thr in S.THRESHOLDS for slab in SLABS]


def _dev(x):
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(DEV)


def _operands(m, i64=True, r0=0):
    rowptr = m.rowptr[r0:] if i64 else m.rowptr[r0:].astype(np.int32)
    return _dev(rowptr), _dev(m.col), _dev(m.cnt), _dev(m.lib[r0:]), _dev(m.n_add[r0:])


def _soup(c, slab=128, i64=True, **kw):
    kw = dict(dict(seed=S.CASE_SEED, scale=S.SCALE, threshold=c.threshold, slab_genes=slab, want_cnt=True), **kw)
    return ops.soup_rows(*_operands(c.m, i64), _dev(c.cdf), S.N_DRAWS, **kw)


@pytest.fixture(scope="module")
def merged():
    """``ops.soup_rows`` of every case, computed once."""
    return {key: _soup(S.case(key[0], key[1]), key[2]) for key in CASES}


@pytest.mark.parametrize("name,thr,slab", CASES)
def test_soup_rows_against_the_reference(merged, name, thr, slab):
    ref = S.case(name, thr).ref
    rowptr, col, val, mapped, cnt = merged[name, thr, slab]
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
    assert mapped.dtype == torch.int32 and cnt.dtype == torch.int64
    np.testing.assert_array_equal(np.diff(rowptr.cpu().numpy()), ref.n_out)
    np.testing.assert_array_equal(mapped.cpu().numpy(), ref.soup_mapped)
    np.testing.assert_array_equal(rowptr.cpu().numpy(), ref.rowptr)
    np.testing.assert_array_equal(col.cpu().numpy(), ref.col)
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref.cnt)
    got, want = val.cpu().numpy().view(np.int32).astype(np.int64), ref.val.view(np.int32).astype(np.int64)
    frag = S.fragile(ref.v64)
    assert frag.mean() <= S.FRAGILE_CAP
    np.testing.assert_array_equal(got[~frag], want[~frag])
    assert (np.abs(got - want)[frag] <= 1).all()


@pytest.mark.parametrize("name,thr,slab", CASES)
def test_soup_rows_are_align_rows_on_the_contaminated_matrix(merged, name, thr, slab):
    """No tolerance: the units' contaminated counts as a dense float32 matrix (one more column, mapped to -1, holding the reads
    outside the bundle and the soup reads of the rest bin) through the existing log-normalising alignment."""
    c = S.case(name, thr)
    x, gmap = S.contaminated_dense(c.m, c.m.n_add, c.cdf, S.N_DRAWS, seed=S.CASE_SEED)
    want = ops.align_rows(_dev(x), _dev(gmap), c.m.G, thr, normalize="lognorm", scale=S.SCALE)
    for g, w in zip(merged[name, thr, slab][:3], want):
        assert g.dtype == w.dtype and torch.equal(g, w)


def test_launches_slabs_splits_and_rowptr_widths_give_the_same_bits(merged):
    for name in ("uniform", "wide"):
        c = S.case(name, 0.0)
        whole = merged[name, 0.0, 128]
        same = lambda got: all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(got, whole))
        assert same(_soup(c))                                              # two launches
        assert same(merged[name, 0.0, 0])                                  # one slab
        assert same(_soup(c, slab=7))                                      # 43 slabs
        assert same(_soup(c, i64=False))                                   # an int32 rowptr
        # split by cells: rowptr + r0 next to the same col / cnt, row0 = r0
        r0 = 5
        q0 = r0 * S.N_DRAWS
        for i64 in (True, False):
            tail = ops.soup_rows(*_operands(c.m, i64, r0), _dev(c.cdf), S.N_DRAWS, row0=r0, seed=S.CASE_SEED, scale=S.SCALE,
                                 threshold=0.0, slab_genes=128, want_cnt=True)
            e0 = int(whole[0][q0])
            assert torch.equal(tail[0], whole[0][q0:] - e0) and torch.equal(tail[3], whole[3][q0:])
            for i in (1, 2, 4):
                assert torch.equal(tail[i], whole[i][e0:])
        # split by draws: draw d alone, draw0 = d
        ptr = whole[0].cpu().numpy()
        for d in range(S.N_DRAWS):
            one = ops.soup_rows(*_operands(c.m), _dev(c.cdf), 1, draw0=d, seed=S.CASE_SEED, scale=S.SCALE, threshold=0.0,
                                slab_genes=128, want_cnt=True)
            units = np.arange(c.m.B) * S.N_DRAWS + d
            entries = _dev(np.concatenate([np.arange(ptr[q], ptr[q + 1]) for q in units]).astype(np.int64))
            assert torch.equal(one[0][1:] - one[0][:-1], (whole[0][1:] - whole[0][:-1])[_dev(units)])
            assert torch.equal(one[3], whole[3][_dev(units)])
            for i in (1, 2, 4):
                assert torch.equal(one[i], whole[i][entries])


def _entry_args(c, rowptr, col, cnt, lib, n_add, cdf, slab=128):
    return (ops._ptr(rowptr), ops._ptr(col), ops._ptr(cnt), c.m.B, int(col.shape[0]), ops._ptr(lib), ops._ptr(n_add), ops._ptr(cdf),
            c.m.G, S.N_DRAWS, 0, 0, S.CASE_SEED, S.SCALE, 0.0, slab)


def test_nothing_is_written_outside_the_outputs():
    """The C entries on buffers with guard elements before and after every output; ``soup_mapped`` and ``out_cnt`` may be NULL;
    an ``out_rowptr`` that leaves the last unit one slot short sets the bit and writes nothing past the slot."""
    c = S.case("wide", 0.0)
    ref, pad = c.ref, 64
    units, kept = c.m.B * S.N_DRAWS, int(c.ref.rowptr[-1])
    dev, stream = torch.device(DEV), ops._stream(torch.device(DEV))
    operands = (*_operands(c.m), _dev(c.cdf))
    head = _entry_args(c, *operands)
    status = torch.zeros(1 + 2 * pad, dtype=torch.int32, device=DEV)
    n_out = torch.full((units + 2 * pad,), -7, dtype=torch.int32, device=DEV)
    mapped = torch.full((units + 2 * pad,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.call(dev, "wgnn_soup_rows_count", *head, ops._ptr(n_out[pad:]), ops._ptr(mapped[pad:]), ops._ptr(status[pad:]),
                         _lib.FLAG_ROWPTR_I64, stream), "count")
    for buf, want in ((n_out, ref.n_out), (mapped, ref.soup_mapped)):
        assert (buf[:pad] == -7).all() and (buf[units + pad:] == -7).all()
        np.testing.assert_array_equal(buf[pad:units + pad].cpu().numpy(), want)
    n_out.fill_(-7)
    _lib.check(_lib.call(dev, "wgnn_soup_rows_count", *head, ops._ptr(n_out[pad:]), None, ops._ptr(status[pad:]),
                         _lib.FLAG_ROWPTR_I64, stream), "count")
    np.testing.assert_array_equal(n_out[pad:units + pad].cpu().numpy(), ref.n_out)
    out_rowptr = _dev(ref.rowptr)
    out_col = torch.full((kept + 2 * pad,), -7, dtype=torch.int32, device=DEV)
    out_val = torch.full((kept + 2 * pad,), -7.0, dtype=torch.float32, device=DEV)
    out_cnt = torch.full((kept + 2 * pad,), -7, dtype=torch.int64, device=DEV)
    fill = lambda ptr, cnt_buf: _lib.check(_lib.call(dev, "wgnn_soup_rows_fill", *head, ops._ptr(ptr), ops._ptr(out_col[pad:]),
                                                     ops._ptr(out_val[pad:]), cnt_buf, ops._ptr(status[pad:]), _lib.FLAG_ROWPTR_I64,
                                                     stream), "fill")
    fill(out_rowptr, ops._ptr(out_cnt[pad:]))
    for buf in (out_col, out_val, out_cnt):
        assert (buf[:pad] == -7).all() and (buf[kept + pad:] == -7).all()
    np.testing.assert_array_equal(out_col[pad:kept + pad].cpu().numpy(), ref.col)
    np.testing.assert_array_equal(out_cnt[pad:kept + pad].cpu().numpy(), ref.cnt)
    assert not status.any()
    out_col.fill_(-7)
    fill(out_rowptr, None)                                             # out_cnt may be NULL
    np.testing.assert_array_equal(out_col[pad:kept + pad].cpu().numpy(), ref.col)
    assert not status.any()
    short = out_rowptr.clone()
    short[-1] -= 1
    out_col.fill_(-7)
    fill(short, ops._ptr(out_cnt[pad:]))
    assert int(status[pad]) == _lib.SOUP_BAD_ROWPTR and int(out_col[kept + pad - 1]) == -7 and (out_col[kept + pad:] == -7).all()
    np.testing.assert_array_equal(out_col[pad:kept + pad - 1].cpu().numpy(), ref.col[:-1])
    assert not status[:pad].any() and not status[pad + 1:].any()


def test_malformed_operands_set_their_bit_and_leave_the_other_units_intact():
    """Skip paths: nothing faults, the status word says what was skipped, every unit the operand does not touch is as before."""
    c = S.case("uniform", 0.0)
    m, D = c.m, S.N_DRAWS
    rowptr, col, cnt, lib, n_add = _operands(m)
    cdf = _dev(c.cdf)
    good = _soup(c)
    kw = dict(seed=S.CASE_SEED, scale=S.SCALE, threshold=0.0, slab_genes=128)

    def raw(rowptr=rowptr, col=col, cnt=cnt, lib=lib, n_add=n_add):
        """(status bits, out_rowptr, soup_mapped, col, val) through the C entries, whatever the status word says."""
        dev, stream = torch.device(DEV), ops._stream(torch.device(DEV))
        head = _entry_args(c, rowptr, col, cnt, lib, n_add, cdf)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        n_out = torch.empty(m.B * D, dtype=torch.int32, device=DEV)
        mapped = torch.empty(m.B * D, dtype=torch.int32, device=DEV)
        _lib.check(_lib.call(dev, "wgnn_soup_rows_count", *head, ops._ptr(n_out), ops._ptr(mapped), ops._ptr(status),
                             _lib.FLAG_ROWPTR_I64, stream), "count")
        ptr = torch.zeros(m.B * D + 1, dtype=torch.int64, device=DEV)
        torch.cumsum(n_out, 0, dtype=torch.int64, out=ptr[1:])
        o_col = torch.empty(int(ptr[-1]), dtype=torch.int32, device=DEV)
        o_val = torch.empty(int(ptr[-1]), dtype=torch.float32, device=DEV)
        _lib.check(_lib.call(dev, "wgnn_soup_rows_fill", *head, ops._ptr(ptr), ops._ptr(o_col), ops._ptr(o_val), None, ops._ptr(status),
                             _lib.FLAG_ROWPTR_I64, stream), "fill")
        return int(status), ptr, mapped, o_col, o_val

    def intact(got, but_row):
        """Every unit of every row but ``but_row`` equals the good result."""
        _, ptr, mapped, o_col, o_val = got
        for r in range(m.B):
            if r == but_row:
                continue
            for q in range(r * D, (r + 1) * D):
                a, b, a0, b0 = int(ptr[q]), int(ptr[q + 1]), int(good[0][q]), int(good[0][q + 1])
                assert b - a == b0 - a0 and torch.equal(o_col[a:b], good[1][a0:b0]) and torch.equal(o_val[a:b], good[2][a0:b0]), r
                assert int(mapped[q]) == int(good[3][q])

    assert raw()[0] == 0
    # a row range past col: the unit leaves the empty row
    beyond = rowptr.clone()
    beyond[-1] += 5
    got = raw(rowptr=beyond)
    last = m.B - 1
    assert got[0] == _lib.SOUP_BAD_ROWPTR and int(got[1][-1] - got[1][last * D]) == 0
    intact(got, last)
    with pytest.raises(sda.WgnnError, match="rowptr points outside"):
        ops.soup_rows(beyond, col, cnt, lib, n_add, cdf, D, **kw)
    # gene ids outside [0, G): the entries are skipped
    for bad_id in (m.G, -3):
        wrong = col.clone()
        wrong[int(m.rowptr[S.ROW_65]) + 2] = bad_id
        got = raw(col=wrong)
        assert got[0] == _lib.SOUP_BAD_COL
        intact(got, S.ROW_65)
        q = S.ROW_65 * D
        assert int(got[1][q + 1] - got[1][q]) in (int(good[0][q + 1] - good[0][q]), int(good[0][q + 1] - good[0][q]) - 1)
        with pytest.raises(sda.WgnnError, match="gene id is outside"):
            ops.soup_rows(rowptr, wrong, cnt, lib, n_add, cdf, D, **kw)
    # an n_add out of range: the unit is treated as 0 reads
    clean = S.soup_rows(m, np.zeros(m.B, np.int64), c.cdf, D, 0.0, seed=S.CASE_SEED)
    for bad_add in (-1, 2 ** 23 + 1):
        wrong = n_add.clone()
        wrong[S.ROW_DEEP_B] = bad_add
        got = raw(n_add=wrong)
        assert got[0] == _lib.SOUP_BAD_ADD
        intact(got, S.ROW_DEEP_B)
        q = S.ROW_DEEP_B * D
        a, b = int(got[1][q]), int(got[1][q + 1])
        np.testing.assert_array_equal(got[3][a:b].cpu().numpy(), clean.col[clean.rowptr[q]:clean.rowptr[q + 1]])
        assert int(got[2][q]) == 0
        with pytest.raises(sda.WgnnError, match="n_add is outside"):
            ops.soup_rows(rowptr, col, cnt, lib, wrong, cdf, D, **kw)
    # a cdf that is not ascending: unspecified draws, no fault, no bit
    jumbled = cdf.clone()
    jumbled[1:-1] = jumbled[1:-1].flip(0)
    out = ops.soup_rows(rowptr, col, cnt, lib, n_add, jumbled, D, **kw)
    assert int(out[1].min()) >= 0 and int(out[1].max()) < m.G
    # argument errors
    for bad_kw in (dict(scale=0.0), dict(threshold=-1.0), dict(slab_genes=16385), dict(row0=-1), dict(draw0=-1)):
        with pytest.raises(ValueError):
            ops.soup_rows(rowptr, col, cnt, lib, n_add, cdf, D, **{**kw, **bad_kw})
    with pytest.raises(ValueError, match="n_draws"):
        ops.soup_rows(rowptr, col, cnt, lib, n_add, cdf, 0, **kw)
    with pytest.raises(ValueError, match="lib"):
        ops.soup_rows(rowptr, col, cnt, lib.int(), n_add, cdf, D, **kw)
    with pytest.raises(ValueError, match="n_add"):
        ops.soup_rows(rowptr, col, cnt, lib, n_add[:-1], cdf, D, **kw)
    with pytest.raises(ValueError, match="cdf"):
        ops.soup_rows(rowptr, col, cnt, lib, n_add, cdf.double(), D, **kw)
    with pytest.raises(ValueError, match="total weight"):
        ops.soup_rows(rowptr, col, cnt, lib, n_add, torch.zeros_like(cdf), D, **kw)
    none = ops.soup_rows(rowptr[:1], col, cnt, lib[:0], n_add[:0], cdf, D, **kw)          # no cell
    assert none[0].tolist() == [0] and none[1].numel() == 0 and none[3].numel() == 0
