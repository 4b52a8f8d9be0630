"""``wgnn_pair_rows_count`` / ``wgnn_pair_rows_fill`` (``ops.pair_rows``) on the GPU: every ordered pair of the case batch of
tests/pairs_reference.py against the numpy reference and - the primary oracle, without a tolerance - against the existing
``align_rows(..., normalize="lognorm")`` on the host-summed count matrix."""
import ctypes as C

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

import pairs_reference as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(0.0, False), (0.0, True), (1.5, False), (1.5, True)]          # (threshold, int64 rowptr)


def _operands(m, i64=True):
    rowptr = torch.from_numpy(m.rowptr if i64 else m.rowptr.astype(np.int32)).to(DEV)
    return rowptr, torch.from_numpy(m.col).to(DEV), torch.from_numpy(m.cnt).to(DEV), torch.from_numpy(m.lib).to(DEV)


def _pairs(c):
    return torch.from_numpy(c.a).to(DEV), torch.from_numpy(c.b).to(DEV)


@pytest.fixture(scope="module")
def merged():
    """``ops.pair_rows`` of every case, computed once."""
    out = {}
    for thr, i64 in CASES:
        c = P.case(thr)
        out[thr, i64] = ops.pair_rows(*_operands(c.m, i64), *_pairs(c), threshold=thr)
    return out


@pytest.mark.parametrize("thr,i64", CASES)
def test_pairs_against_the_reference(merged, thr, i64):
    c = P.case(thr)
    rowptr, col, val = merged[thr, i64]
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
    np.testing.assert_array_equal(rowptr.cpu().numpy(), c.rowptr)
    np.testing.assert_array_equal(col.cpu().numpy(), c.col)
    got, want = val.cpu().numpy().view(np.int32).astype(np.int64), c.val.view(np.int32).astype(np.int64)
    frag = P.fragile(c.v64)
    np.testing.assert_array_equal(got[~frag], want[~frag])
    assert (np.abs(got - want)[frag] <= 1).all()


@pytest.mark.parametrize("thr,i64", CASES)
def test_pairs_are_align_rows_on_the_summed_matrix(merged, thr, i64):
    """No tolerance: the summed counts as a dense matrix (one more column, mapped to -1, holding the reads outside the bundle)
    through the existing log-normalising alignment."""
    c = P.case(thr)
    x, gmap = P.summed_dense(c.m.rowptr, c.m.col, c.m.cnt, c.m.lib, c.a, c.b, c.m.G)
    want = ops.align_rows(torch.from_numpy(x).to(DEV), torch.from_numpy(gmap).to(DEV), c.m.G, thr, normalize="lognorm", scale=P.SCALE)
    for got, ref in zip(merged[thr, i64], want):
        assert torch.equal(got, ref)


@pytest.mark.parametrize("thr", P.THRESHOLDS)
def test_self_pair_carries_the_bits_of_the_row_itself(merged, thr):
    m = P.batch()
    same = torch.arange(m.B, dtype=torch.int32, device=DEV)
    got = ops.pair_rows(*_operands(m), same, same, threshold=thr)
    dense = np.zeros((m.B, m.G + 1), np.float32)
    for r in range(m.B):
        dense[r, m.col[m.rowptr[r]:m.rowptr[r + 1]]] = m.cnt[m.rowptr[r]:m.rowptr[r + 1]]
    dense[:, m.G] = m.rest
    gmap = torch.from_numpy(np.concatenate([np.arange(m.G), [-1]]).astype(np.int32)).to(DEV)
    want = ops.align_rows(torch.from_numpy(dense).to(DEV), gmap, m.G, thr, normalize="lognorm", scale=P.SCALE)
    for g, w in zip(got, want):
        assert torch.equal(g, w)                                      # 2c / 2T == c / T exactly


def test_two_launches_and_a_split_pair_list_give_the_same_bits(merged):
    c = P.case(1.5)
    ops_in, (a, b) = _operands(c.m), _pairs(c)
    again = ops.pair_rows(*ops_in, a, b, threshold=1.5)
    for x, y in zip(again, merged[1.5, True]):
        assert torch.equal(x, y)
    n = a.shape[0]
    cuts = [0, n // 3 + 1, 2 * n // 3 + 2, n]
    parts = [ops.pair_rows(*ops_in, a[s:e], b[s:e], threshold=1.5) for s, e in zip(cuts, cuts[1:])]
    assert torch.equal(torch.cat([p[1] for p in parts]), again[1]) and torch.equal(torch.cat([p[2] for p in parts]), again[2])
    lens = torch.cat([p[0][1:] - p[0][:-1] for p in parts])
    assert torch.equal(lens, again[0][1:] - again[0][:-1])


def test_nothing_is_written_outside_the_outputs():
    """The C entries on buffers with guard elements before and after every output."""
    c = P.case(0.0)
    rowptr, col, cnt, lib = _operands(c.m)
    a, b = _pairs(c)
    n, total, pad = int(a.shape[0]), int(c.rowptr[-1]), 64
    ptr, stream = ops._ptr, ops._stream(torch.device(DEV))
    status = torch.zeros(1 + 2 * pad, dtype=torch.int32, device=DEV)
    n_out = torch.full((n + 2 * pad,), -7, dtype=torch.int32, device=DEV)
    head = (ptr(rowptr), ptr(col), ptr(cnt), c.m.B, int(col.shape[0]), ptr(lib), ptr(a), ptr(b), n, P.SCALE, 0.0)
    _lib.check(_lib.call(torch.device(DEV), "wgnn_pair_rows_count", *head, ptr(n_out[pad:]), ptr(status[pad:]),
                         _lib.FLAG_ROWPTR_I64, stream), "count")
    assert (n_out[:pad] == -7).all() and (n_out[n + pad:] == -7).all()
    np.testing.assert_array_equal(n_out[pad:n + pad].cpu().numpy(), np.diff(c.rowptr))
    out_rowptr = torch.from_numpy(c.rowptr).to(DEV)
    out_col = torch.full((total + 2 * pad,), -7, dtype=torch.int32, device=DEV)
    out_val = torch.full((total + 2 * pad,), -7.0, dtype=torch.float32, device=DEV)
    _lib.check(_lib.call(torch.device(DEV), "wgnn_pair_rows_fill", *head, ptr(out_rowptr), ptr(out_col[pad:]), ptr(out_val[pad:]),
                         ptr(status[pad:]), _lib.FLAG_ROWPTR_I64, stream), "fill")
    for buf in (out_col, out_val):
        assert (buf[:pad] == -7).all() and (buf[total + pad:] == -7).all()
    np.testing.assert_array_equal(out_col[pad:total + pad].cpu().numpy(), c.col)
    assert not status.any()
    # out_rowptr that leaves the last pair one slot less: the slot is not written, the status word says so
    short = out_rowptr.clone()
    short[-1] -= 1
    out_col.fill_(-7)
    _lib.check(_lib.call(torch.device(DEV), "wgnn_pair_rows_fill", *head, ptr(short), ptr(out_col[pad:]), ptr(out_val[pad:]),
                         ptr(status[pad:]), _lib.FLAG_ROWPTR_I64, stream), "fill")
    assert int(status[pad]) == _lib.PAIR_BAD_ROWPTR and int(out_col[total + pad - 1]) == -7 and (out_col[total + pad:] == -7).all()


def test_malformed_operands_raise_through_the_status_word():
    m = P.batch()
    rowptr, col, cnt, lib = _operands(m)
    a = torch.tensor([P.ROW_64, P.ROW_ONE], dtype=torch.int32, device=DEV)
    for bad in (m.B, -1):                                             # a partner out of range
        with pytest.raises(sda.WgnnError, match="outside \\[0, n_rows\\)"):
            ops.pair_rows(rowptr, col, cnt, lib, a, torch.tensor([P.ROW_65, bad], dtype=torch.int32, device=DEV))
    swapped = col.clone()                                             # an unsorted row: two neighbours of the 64-gene row swapped
    s = int(m.rowptr[P.ROW_64]) + 10
    swapped[s], swapped[s + 1] = col[s + 1], col[s]
    b = torch.tensor([P.ROW_65, P.ROW_130], dtype=torch.int32, device=DEV)
    with pytest.raises(sda.WgnnError, match="not strictly ascending"):
        ops.pair_rows(rowptr, swapped, cnt, lib, a, b)
    twice = col.clone()                                               # a gene listed twice
    twice[s + 1] = col[s]
    with pytest.raises(sda.WgnnError, match="not strictly ascending"):
        ops.pair_rows(rowptr, twice, cnt, lib, a, b)
    beyond = rowptr.clone()                                           # a rowptr that points past col
    beyond[-1] += 5
    last = torch.tensor([m.B - 1], dtype=torch.int32, device=DEV)
    with pytest.raises(sda.WgnnError, match="rowptr points outside"):
        ops.pair_rows(beyond, col, cnt, lib, last, last)
    fixed = ops.csr_rows_ascending(rowptr, swapped, cnt)              # the helper sorts what the kernel refuses
    assert torch.equal(fixed[1], col)
    for bad_kw in (dict(scale=0.0), dict(threshold=-1.0)):
        with pytest.raises(ValueError):
            ops.pair_rows(rowptr, col, cnt, lib, a, b, **bad_kw)
    with pytest.raises(ValueError, match="lib"):
        ops.pair_rows(rowptr, col, cnt, lib.int(), a, b)
    empty = ops.pair_rows(rowptr, col, cnt, lib, a[:0], b[:0])
    assert empty[0].tolist() == [0] and empty[1].numel() == 0
