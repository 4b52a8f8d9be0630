"""``wgnn_rank_sets_rows`` on the GPU: ``rank2_sum`` and ``present`` EXACTLY those of the ``rankdata`` reference of
tests/signatures_reference.py - tie-heavy rows of every length around the wave and vector widths, 1 / 13 / 64 sets with the
bits above ``n_sets`` set, an empty set and the whole vocabulary, both rowptr widths, the cap biting and not biting; guard rows
and columns, determinism, splitting by cells and by sets; the key order on negative values, signed zeros and a NaN; a permuted
gene order.

The kernel has two limits, each crossed here on a 20 000-gene vocabulary: it stages 16 384 keys of a row in LDS (rows of
16 384, 16 385 and 17 000 entries - the tail is read from global memory), and it holds 512 member entries between two rankings
(rows with 512, 513, 1 025 and 17 000 members - a row with more runs in passes)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import ops

import signatures_reference as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 300


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def words(member):
    return t(S.pack(member).view(np.int64))


def _csr(indptr, indices, data, i64=False):
    return t(indptr.astype(np.int64 if i64 else np.int32)), t(indices.astype(np.int32)), t(data.astype(np.float32))


@lru_cache(maxsize=None)
def _case(max_rank):
    """The rows of S.case_rows, 64 sets, and the reference's integer tables - computed once per max_rank, never modified."""
    rows = S.case_rows(G)
    member = S.membership(G, 64)
    r2, present, _ = S.rank_sets(*rows, G, member, max_rank)
    return rows, member, r2, present


def _same(got, r2, present):
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32
    np.testing.assert_array_equal(got[0].cpu().numpy(), r2)
    np.testing.assert_array_equal(got[1].cpu().numpy(), present)


@pytest.mark.parametrize("max_rank", [40, 1000])                   # the cap bites / never bites (2 * 300 + 1 < 2 * 1001)
@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("n_sets", [1, 13, 64])
def test_op_equals_the_reference(n_sets, i64, max_rank):
    rows, member, r2, present = _case(max_rank)
    lens = np.diff(rows[0])
    assert {0, 1, 2, 63, 64, 65, 127, 129}.issubset(lens.tolist()) and {1, 2, 3}.issubset((lens % 4).tolist())
    assert (r2 < _case(1000)[2]).any() == (max_rank == 40)         # the cap bites at 40 only: R2 <= 2 * 300 + 1 < 2 * 1001
    assert present[S.ALL_MEMBERS, 0] == S.N_CORE and not present[:, S.EMPTY_SET].any()
    assert np.array_equal(present[:, S.WHOLE_SET], lens)
    w = words(member)                                              # all 64 bits in use: those at or above n_sets are ignored
    B = len(lens)
    # guard rows and columns around both outputs, ld > n_sets
    sum_buf = torch.full((B + 2, n_sets + 3), -7, dtype=torch.int64, device=DEV)
    cnt_buf = torch.full((B + 2, n_sets + 3), -7, dtype=torch.int32, device=DEV)
    got = ops.rank_sets_rows(*_csr(*rows, i64), w, n_sets, max_rank, G, out=(sum_buf[1:B + 1, 1:], cnt_buf[1:B + 1, 1:]))
    _same(got, r2[:, :n_sets], present[:, :n_sets])
    for buf in (sum_buf, cnt_buf):
        assert (buf[0] == -7).all() and (buf[-1] == -7).all() and (buf[:, 0] == -7).all() and (buf[:, n_sets + 1:] == -7).all()
        assert torch.equal(buf[1:B + 1, 1:n_sets + 1], got[0] if buf is sum_buf else got[1])
    # two launches are bit-identical, and so is a freshly allocated output
    again = ops.rank_sets_rows(*_csr(*rows, i64), w, n_sets, max_rank, G)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def test_split_by_cells_and_by_sets_equals_the_whole():
    rows, member, r2, present = _case(40)
    rp, col, val = _csr(*rows)
    B = rp.shape[0] - 1
    for r0, r1 in ((0, 5), (5, 6), (6, B)):                        # a slice of rowptr that does not start at 0
        _same(ops.rank_sets_rows(rp[r0:r1 + 1], col, val, words(member), 64, 40, G), r2[r0:r1], present[r0:r1])
    for p0, p1 in ((0, 13), (13, 14), (14, 64)):
        _same(ops.rank_sets_rows(rp, col, val, words(member[p0:p1]), p1 - p0, 40, G), r2[:, p0:p1], present[:, p0:p1])


def test_permuted_gene_order_gives_the_same_sums():
    rows, member, r2, present = _case(40)
    indptr, indices, data = rows
    rng = np.random.default_rng(5)
    order = np.concatenate([indptr[r] + rng.permutation(indptr[r + 1] - indptr[r]) for r in range(len(indptr) - 1)]).astype(np.int64)
    assert not np.array_equal(order, np.arange(len(order)))
    _same(ops.rank_sets_rows(*_csr(indptr, indices[order], data[order]), words(member), 64, 40, G), r2, present)


def test_key_order_on_negative_values_signed_zeros_and_a_nan():
    rng = np.random.default_rng(2)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 0.0, -0.0, -1.5, -1.5, 2.0, 1e-40, -1e-40], np.float32)
    data = np.concatenate([special, rng.standard_normal(70).astype(np.float32), S.VALUES])
    data = data[rng.permutation(len(data))]
    n = len(data)
    indptr, indices = np.array([0, n], np.int64), rng.permutation(G)[:n].astype(np.int32)
    member = S.membership(G, 13)
    for max_rank in (20, 1000):
        r2, present, _ = S.rank_sets(indptr, indices, data, G, member, max_rank, by_key=True)
        c2, cp = S.count_form(indptr, indices, data, member, max_rank)
        assert np.array_equal(r2, c2) and np.array_equal(present, cp)
        _same(ops.rank_sets_rows(*_csr(indptr, indices, data), words(member), 13, max_rank, G), r2, present)


def test_a_gene_id_out_of_range_belongs_to_no_set_and_is_never_an_index():
    rows, member, _, _ = _case(40)
    indptr, indices, data = (a.copy() for a in rows)
    at = [int(indptr[7]), int(indptr[7]) + 3, int(indptr[-1]) - 1]                     # entries of the rows of 129 and 300 genes
    indices[at] = [-1, G, 2 ** 31 - 1]
    wide = np.concatenate([member, np.zeros((64, 3), bool)], axis=1)                   # three more genes, in no set
    moved = indices.astype(np.int64)
    moved[at] = [G, G + 1, G + 2]
    r2, present = S.count_form(indptr, moved, data, wide, 40)
    assert present[7, S.WHOLE_SET] == 127
    _same(ops.rank_sets_rows(*_csr(indptr, indices, data), words(member), 64, 40, G, check_cols=False), r2, present)
    with pytest.raises(sda.WgnnError, match="out of range"):
        ops.rank_sets_rows(*_csr(indptr, indices, data), words(member), 64, 40, G)


BIG_G = 20000
BIG_LENGTHS = (17000, 0, 16384, 16385, 512, 513, 1025, 3)


@pytest.mark.parametrize("i64", [False, True])
def test_rows_beyond_the_staged_keys_and_beyond_the_stash(i64):
    rows = S.case_rows(BIG_G, BIG_LENGTHS, seed=4)
    rng = np.random.default_rng(6)
    member = np.stack([np.ones(BIG_G, bool), rng.random(BIG_G) < 0.125, np.arange(BIG_G) < 600, rng.random(BIG_G) < 0.5])
    w = words(member)
    for max_rank in (1500, 2 ** 30):                               # ranks capped at 1 501 / never
        r2, present, _ = S.rank_sets(*rows, BIG_G, member, max_rank)
        assert present[0].tolist()[0] == 17000 and present[0, 3] > 512 * 8             # many passes, every wave with several groups
        assert present[4:7, 0].tolist() == [512, 513, 1025]
        _same(ops.rank_sets_rows(*_csr(*rows, i64), w, 4, max_rank, BIG_G), r2, present)


def test_ops_argument_errors():
    rp = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    col, val = torch.zeros(1, dtype=torch.int32, device=DEV), torch.ones(1, device=DEV)
    member = torch.ones(3, dtype=torch.int64, device=DEV)
    r2, present = ops.rank_sets_rows(rp, col, val, member, 2, 10, 3)
    assert r2.tolist() == [[2, 0]] and present.tolist() == [[1, 0]]
    empty = ops.rank_sets_rows(rp[:1], col[:0], val[:0], member, 2, 10, 3)
    assert empty[0].shape == (0, 2) and empty[1].shape == (0, 2)
    base = dict(rowptr=rp, col=col, val=val, member=member, n_sets=2, max_rank=10, n_genes=3)
    for kw in (dict(n_sets=0), dict(n_sets=65), dict(max_rank=0), dict(max_rank=2 ** 30 + 1), dict(n_genes=0),
               dict(member=member.int()), dict(member=member[:2]), dict(val=val.double()), dict(col=col.long()),
               dict(val=torch.ones(2, device=DEV)), dict(out=(torch.zeros((1, 1), dtype=torch.int64, device=DEV), present)),
               dict(out=(r2, present.long())), dict(out=(torch.zeros((2, 2), dtype=torch.int64, device=DEV), present))):
        with pytest.raises(ValueError):
            ops.rank_sets_rows(**{**base, **kw})
