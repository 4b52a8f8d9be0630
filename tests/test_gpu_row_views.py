"""The two host-side rules the resident row ops share, on the GPU: a SINGLE row written through a strided view (its leading
dimension is the width, whatever stride the view reports) and an EMPTY batch through the gene-major reorder.  Tiny tables; each
result is compared, bit for bit, with the same call on contiguous tensors, and every element around a view stays as it was."""
import pytest
import torch

from scdeepsort_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G, H, C = 12, 8, 3
SENTINEL = -7


def _model():
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).to(DEV)
    return rnd(G, H), torch.rand(G + 2, generator=gen).to(DEV), rnd(H), (rnd(C, H), rnd(C))


def _one_cell(counts=False):
    """one cell that lists 7 of the G genes: ``(rowptr, col, raw)``"""
    col = torch.tensor([9, 0, 4, 11, 2, 7, 5], dtype=torch.int32, device=DEV)
    raw = torch.tensor([3., 1., 2., 5., 1., 4., 2.] if counts else [.5, 1.25, 2., .75, 3.5, 1., 2.25], device=DEV)
    return torch.tensor([0, 7], dtype=torch.int32, device=DEV), col, raw


def _window(width, wide, dtype, at=1):
    """``(buffer [1, wide] full of the sentinel, its view [1, width] that starts at column ``at``)``"""
    buf = torch.full((1, wide), SENTINEL, dtype=dtype, device=DEV)
    view = buf[:, at:at + width]
    assert tuple(view.shape) == (1, width) and view.stride(0) == wide > width
    return buf, view


def _untouched_around(buf, view_width, at=1):
    return bool((buf[:, :at] == SENTINEL).all()) and bool((buf[:, at + view_width:] == SENTINEL).all())


def test_a_single_row_is_written_through_a_strided_view():
    table, alpha, bias, head = _model()
    # rank_sets_rows: B = 1, three sets, both outputs views into [1, 8]
    rowptr, col, val = _one_cell()
    member = torch.tensor([1, 3, 4, 0, 7, 2, 0, 5, 0, 6, 1, 2], dtype=torch.int64, device=DEV)
    want = ops.rank_sets_rows(rowptr, col, val, member, 3, 5, G)
    sum_buf, sum_view = _window(3, 8, torch.int64)
    cnt_buf, cnt_view = _window(3, 8, torch.int32)
    got = ops.rank_sets_rows(rowptr, col, val, member, 3, 5, G, out=(sum_view, cnt_view))
    assert bool(want[1].any()) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(sum_buf[:, 1:4], want[0]) and torch.equal(cnt_buf[:, 1:4], want[1])
    assert _untouched_around(sum_buf, 3) and _untouched_around(cnt_buf, 3)

    # rank_genes_groups: K = 1, G = 5, rank2_sum and count views into [1, 8]
    rp3 = torch.tensor([0, 2, 5, 6], dtype=torch.int32, device=DEV)
    col3 = torch.tensor([0, 3, 1, 3, 4, 3], dtype=torch.int32, device=DEV)
    val3 = torch.tensor([1., 2., 1., 2., 3., .5], device=DEV)
    group = torch.tensor([0, -1, 0], dtype=torch.int32, device=DEV)
    want = ops.rank_genes_groups(rp3, col3, val3, group, 1, 5)
    r2_buf, r2_view = _window(5, 8, torch.int64)
    n_buf, n_view = _window(5, 8, torch.int32)
    tie = torch.full((5,), SENTINEL, dtype=torch.int64, device=DEV)
    got = ops.rank_genes_groups(rp3, col3, val3, group, 1, 5, out=(r2_view, n_view, tie))
    assert want[1].tolist() == [[1, 0, 0, 2, 0]] and want[3].tolist() == [2]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(r2_buf[:, 1:6], want[0]) and torch.equal(n_buf[:, 1:6], want[1])
    assert _untouched_around(r2_buf, 5) and _untouched_around(n_buf, 5)

    # predict_rows_dropout with a head: B = 1, votes a view into [1, C + 4]
    kw = dict(head=head, n_draws=6, keep=0.6, seed=3, want_draws=True)
    want = ops.predict_rows_dropout(rowptr, col, val, table, alpha, bias, **kw)
    votes_buf, votes_view = _window(C, C + 4, torch.int32, at=2)
    rest = (torch.empty(1, dtype=torch.int32, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV),
            torch.empty(1, dtype=torch.float64, device=DEV))
    got = ops.predict_rows_dropout(rowptr, col, val, table, alpha, bias, out=(votes_view, *rest), **kw)
    assert int(want[0].sum()) + int(want[1][0]) == 6                                   # every draw voted, or was unsure
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(votes_buf[:, 2:2 + C], want[0]) and _untouched_around(votes_buf, C, at=2)

    # predict_rows_panels in counts mode: B = 1, lib a view into [1, P + 4]
    P = 3
    rowptr, col, cnt = _one_cell(counts=True)
    inside = torch.stack([(cnt * ((member[col.long()] >> p) & 1)).sum() for p in range(P)]).to(torch.int64)
    lib_buf, lib_view = _window(P, P + 4, torch.int64, at=2)
    lib_view.copy_((inside + torch.tensor([0, 4, 9], device=DEV)).reshape(1, P))
    kw = dict(head=head, want_logits=True, want_entries=True)
    want = ops.predict_rows_panels(rowptr, col, cnt, table, alpha, bias, member, P, lib=lib_view.contiguous(), **kw)
    got = ops.predict_rows_panels(rowptr, col, cnt, table, alpha, bias, member, P, lib=lib_view, **kw)
    assert want[3].tolist() == [[int(((member[col.long()] >> p) & 1).sum()) for p in range(P)]] and bool(want[3].all())
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert _untouched_around(lib_buf, P, at=2)                                         # lib is only read


def test_an_empty_batch_writes_every_element_of_the_tables():
    K, n_genes = 2, 4
    rowptr = torch.zeros(1, dtype=torch.int32, device=DEV)
    col, val = torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, device=DEV)
    group = torch.zeros(0, dtype=torch.int32, device=DEV)
    full = lambda shape, dtype: torch.full(shape, SENTINEL, dtype=dtype, device=DEV)
    out = (full((K, n_genes), torch.float64), full((K, n_genes), torch.int32))
    total, count = ops.group_gene_reduce(rowptr, col, val, group, K, n_genes, out=out)
    assert total is out[0] and count is out[1]
    assert bool((total == 0).all()) and bool((count == 0).all())
    total, count = ops.group_gene_reduce(rowptr, col, val, group, K, n_genes)
    assert tuple(total.shape) == (K, n_genes) and bool((total == 0).all()) and bool((count == 0).all())

    out = (full((K, n_genes), torch.int64), full((K, n_genes), torch.int32), full((n_genes,), torch.int64))
    rank2_sum, n, tie_sum, group_size = ops.rank_genes_groups(rowptr, col, val, group, K, n_genes, out=out)
    assert rank2_sum is out[0] and n is out[1] and tie_sum is out[2]
    assert bool((rank2_sum == 0).all()) and bool((n == 0).all()) and bool((tie_sum == 0).all())
    assert group_size.dtype == torch.int64 and group_size.tolist() == [0, 0]
