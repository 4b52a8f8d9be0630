"""The operand layer of the resident row ops (``ops._csr_operand``, ``_group_operand``, ``_group_major``, ``_view_2d``, ``_ld``):
plain functions on tensors, checked here on CPU tensors.  The device work behind them is covered by the ops' own GPU tests."""
import pytest
import torch

from scdeepsort_amd import _lib, ops
from scdeepsort_amd._lib import WgnnError

I32, I64, F32 = torch.int32, torch.int64, torch.float32


def _csr(rowptr_dtype=I32):
    return torch.tensor([0, 2, 3, 5], dtype=rowptr_dtype), torch.tensor([0, 3, 1, 2, 5], dtype=I32), torch.arange(5, dtype=F32)


@pytest.mark.parametrize("exc", [WgnnError, ValueError])
def test_csr_operand_refuses_wrong_dtypes_and_shapes_in_the_ops_class(exc):
    rowptr, col, val = _csr()
    bad = {"rowptr float": (rowptr.float(), col, val), "rowptr int16": (rowptr.short(), col, val),
           "col int64": (rowptr, col.long(), val), "val float64": (rowptr, col, val.double()), "val int": (rowptr, col, col)}
    for what, triple in bad.items():
        with pytest.raises(exc, match="some_op takes rowptr int32 / int64, col int32, scores float32"):
            ops._csr_operand("some_op", exc, *triple, "scores")
            pytest.fail(what)
    malformed = {"col 2-D": (rowptr, col.reshape(1, 5), val.reshape(1, 5)), "lengths": (rowptr, col, val[:4]),
                 "rowptr empty": (rowptr[:0], col, val), "rowptr 2-D": (rowptr.reshape(1, 4), col, val)}
    for what, triple in malformed.items():
        with pytest.raises(exc, match="malformed CSR: rowptr .*, col .*, scores .*; col has 5 entries, scores [45]"):
            ops._csr_operand("some_op", exc, *triple, "scores")
            pytest.fail(what)


def test_csr_operand_returns_contiguous_tensors_sizes_and_the_rowptr_flag():
    rowptr, col, val = _csr()
    out = ops._csr_operand("some_op", ValueError, rowptr, col, val, "val")
    assert out[0] is rowptr and out[1] is col and out[2] is val and out[3:] == (3, 5, 0)
    assert ops._csr_operand("some_op", ValueError, *_csr(I64), "val")[3:] == (3, 5, _lib.FLAG_ROWPTR_I64)
    strided = torch.stack([col, col + 7], 1)[:, 0]
    assert not strided.is_contiguous()
    got = ops._csr_operand("some_op", ValueError, rowptr, strided, val, "val")[1]
    assert got.is_contiguous() and torch.equal(got, col)
    empty = ops._csr_operand("some_op", ValueError, torch.zeros(1, dtype=I32), col[:0], val[:0], "val")
    assert empty[3:] == (0, 0, 0)


@pytest.mark.parametrize("exc", [WgnnError, ValueError])
def test_group_operand_checks_shape_dtype_and_range(exc):
    group = torch.tensor([0, -1, 1, 2], dtype=I32)
    assert ops._group_operand("some_op", exc, group, 4, 3, True) is group
    assert ops._group_operand("some_op", exc, group.long(), 4, 3, True).dtype == I64
    for bad in (group[:3], group.reshape(2, 2), group.float()):
        with pytest.raises(exc, match=r"some_op: group must hold one id per cell \(\[4\]\), int32 / int64, got torch"):
            ops._group_operand("some_op", exc, bad, 4, 3, True)
    with pytest.raises(exc, match=r"other_op: group must be int32 \[4\], got torch.int64 \(4,\)"):
        ops._group_operand("some_op", exc, group.long(), 4, 3, True, dtypes=(I32,), says="other_op: group must be int32 [4]")
    for value in (-2, 3):
        off = group.clone()
        off[1] = value
        with pytest.raises(exc, match=r"some_op: group id out of range \[-1, 3\)"):
            ops._group_operand("some_op", exc, off, 4, 3, True)
        assert ops._group_operand("some_op", exc, off, 4, 3, False) is off          # without check: let through
    none = torch.zeros(0, dtype=I32)
    assert ops._group_operand("some_op", exc, none, 0, 3, True) is none                # an empty batch has no range to check


def _group_major_by_loop(group, K):
    order = [i for k in range(K) for i, g in enumerate(group) if g == k] + [i for i, g in enumerate(group) if not 0 <= g < K]
    seg_ptr = [sum(1 for g in group if 0 <= g < k) for k in range(K + 1)]
    return order, seg_ptr


@pytest.mark.parametrize("dtype", [I32, I64])
@pytest.mark.parametrize("group,K", [([2, -1, 0, 2, 5, 0], 3), ([0, 0, 0], 1), ([3, 0, 3, 0, 1], 4), ([], 2), ([-1, 7], 2)])
def test_group_major_is_the_stable_group_order_of_a_plain_loop(group, K, dtype):
    order, seg_ptr = ops._group_major(torch.tensor(group, dtype=dtype), K)
    assert order.dtype == I32 and tuple(order.shape) == (len(group),)
    assert seg_ptr.dtype == I64 and tuple(seg_ptr.shape) == (K + 1,) and seg_ptr.is_contiguous()
    want_order, want_ptr = _group_major_by_loop(group, K)
    assert seg_ptr.tolist() == want_ptr and order.tolist() == want_order


def test_group_major_on_the_issue_example():
    order, seg_ptr = ops._group_major(torch.tensor([2, -1, 0, 2, 5, 0], dtype=I32), 3)
    assert seg_ptr.tolist() == [0, 2, 2, 4] and order[:4].tolist() == [2, 5, 0, 3]
    assert sorted(order[4:].tolist()) == [1, 4]                                        # the ids -1 and 5 sort last
    order, seg_ptr = ops._group_major(torch.tensor([3, 0, 3, 0, 1], dtype=I32), 4)     # group 2 is empty, in the middle
    assert seg_ptr.tolist() == [0, 2, 3, 3, 5]


def test_view_2d_and_ld_take_row_strided_views():
    one = torch.zeros(1, 8, dtype=I64)[:, :3]
    assert ops._view_2d("some_op", ValueError, "out's sum", one, I64, 1, 3) is one
    assert ops._ld(one, 1, 3) == 3                                                     # a single row's stride says nothing
    four = torch.zeros(4, 8, dtype=I64)[:, :3]
    assert ops._view_2d("some_op", ValueError, "out's sum", four, I64, 4, 3) is four
    assert ops._ld(four, 4, 3) == 8
    dense = torch.zeros(4, 3, dtype=I64)
    assert ops._ld(ops._view_2d("some_op", WgnnError, "out's sum", dense, I64, 4, 3), 4, 3) == 3
    assert ops._ld(torch.zeros(0, 3, dtype=I64), 0, 3) == 3


@pytest.mark.parametrize("exc", [WgnnError, ValueError])
def test_view_2d_refuses_what_is_not_row_strided(exc):
    message = r"some_op: out's sum must be int64 \[4, 3\] with unit column stride and a row stride >= 3"
    bad = {"transposed": torch.zeros(3, 4, dtype=I64).t(), "dtype": torch.zeros(4, 3, dtype=I32),
           "rows": torch.zeros(5, 3, dtype=I64), "cols": torch.zeros(4, 5, dtype=I64), "1-D": torch.zeros(12, dtype=I64),
           "column stride": torch.zeros(4, 6, dtype=I64)[:, ::2], "no tensor": (1, 2)}
    for what, t in bad.items():
        with pytest.raises(exc, match=message):
            ops._view_2d("some_op", exc, "out's sum", t, I64, 4, 3)
            pytest.fail(what)


def test_view_2d_at_least_cols():
    wide = torch.zeros(4, 5, dtype=I32)
    assert ops._view_2d("some_op", ValueError, "out's present", wide, I32, 4, 3, at_least_cols=True) is wide
    assert ops._ld(wide, 4, 3) == 5
    with pytest.raises(ValueError, match=r"some_op: out's present must be int32 \[4, >= 3\] with unit column stride"):
        ops._view_2d("some_op", ValueError, "out's present", torch.zeros(4, 2, dtype=I32), I32, 4, 3, at_least_cols=True)
    with pytest.raises(WgnnError, match=r"^votes must be int32 \[4, 3\] with unit column stride and a row stride >= 3"):
        ops._view_2d(None, WgnnError, "votes", wide, I32, 4, 3)
