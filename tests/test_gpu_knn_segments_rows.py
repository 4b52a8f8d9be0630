"""``ops.knn_segments`` (``wgnn_knn_segments``) on the GPU against the fp64 restatement (tests/bbknn_reference.py): bit for bit on
the lattice fixture, whose float32 distances are exact - the blocked and the merged lists, ties by row id within and across
segments - and on real-valued rows up to the near-ties the error bound leaves open; the split, the chunking and the launch
change no bit; a malformed ``order`` is skipped and reported."""
import numpy as np
import pytest
import torch

from scdeepsort_amd import _lib, ops

import bbknn_reference as BR
import knn_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(x, group, S, k, **kw):
    out = ops.knn_segments(torch.tensor(x, device=DEV), torch.tensor(np.asarray(group), device=DEV), S, k, **kw)
    n = x.shape[0]
    assert isinstance(out, ops.SegmentLists) and out.idx.shape == out.d2.shape == (n, S, k)
    assert out.merged_idx.shape == out.merged_d2.shape == (n, S * k)
    assert out.idx.dtype == out.merged_idx.dtype == torch.int32 and out.d2.dtype == out.merged_d2.dtype == torch.float32
    return tuple(t.cpu().numpy() for t in out)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_exact(got, want):
    """the kernel's four tables equal the reference's: the indices, and the float32 bits of the (exact) distances"""
    for g, w in zip(got, want):
        if g.dtype == np.float32:
            np.testing.assert_array_equal(_bits(g), _bits(w.astype(np.float32)))
        else:
            np.testing.assert_array_equal(g, w)


def _assert_same(got, first):
    for g, w in zip(got, first):
        np.testing.assert_array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)


@pytest.mark.parametrize("D", R.LATTICE_DIMS)
@pytest.mark.parametrize("S,k", [(1, 15), (3, 3), (4, 16), (64, 1)])
def test_lattice_is_bit_exact_for_every_split(D, S, k):
    x = R.lattice(D)
    group, *want = BR.reference("lattice", S, k, D)
    for n_splits in (0, 1, 2, 7):
        _assert_exact(_run(x, group, S, k, n_splits=n_splits), want)


@pytest.mark.parametrize("k", [1, 15, 64])
def test_one_group_is_knn_rows_bit_for_bit(k):
    x = R.real(300, 200, 0)
    idx, d2, m_idx, m_d2 = _run(x, np.zeros(300, np.int64), 1, k)
    plain = ops.knn_rows(torch.tensor(x, device=DEV), k)
    for mine in ((idx[:, 0], d2[:, 0]), (m_idx, m_d2)):
        np.testing.assert_array_equal(mine[0], plain[0].cpu().numpy())
        np.testing.assert_array_equal(_bits(mine[1]), _bits(plain[1].cpu().numpy()))


@pytest.mark.parametrize("k", [4, 12])
def test_uneven_segments_their_tails_and_the_staging_overflow(k):
    """Segments of 1, 0, 63, 64 and 69 cells with interleaved labels: a tile that ends with its segment while the next one's rows
    follow in ``order``, the empty and the one-cell segment, and - every candidate of a segment's first tile beats the empty
    lists - more survivors per query than the staging list holds."""
    x = R.lattice(36)
    S = len(BR.UNEVEN_SIZES)
    group, *want = BR.reference("uneven", S, k, 36)
    for n_splits in (0, 1, 3):
        _assert_exact(_run(x, group, S, k, n_splits=n_splits), want)


def _raw(x, order, seg_ptr, S, k, q_first, n_q, n_splits, idx, d2, merged, status):
    """``wgnn_knn_segments`` itself on device tensors; ``idx`` / ``d2`` / ``merged`` are row-strided views."""
    n = x.shape[0]
    ws, ws_bytes = ops._workspace(x.device, "wgnn_knn_segments_workspace_bytes", n_q, n, S, k, n_splits)
    m_idx, m_d2 = merged if merged is not None else (None, None)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    _lib.run(x.device, "wgnn_knn_segments", x.data_ptr(), x.stride(0), n, x.shape[1], order.data_ptr(), seg_ptr.data_ptr(), S, k,
             q_first, n_q, n_splits, idx.data_ptr(), d2.data_ptr(), idx.stride(0), ptr(m_idx), ptr(m_d2),
             0 if m_idx is None else m_idx.stride(0), status.data_ptr(), ws.data_ptr(), ws_bytes, 0, None)
    torch.cuda.synchronize()


def test_wider_strides_guards_and_a_query_sub_range():
    x = R.lattice(36)
    N, S, k = x.shape[0], 3, 3
    group, *want = BR.reference("lattice", S, k, 36)
    wide = torch.full((N + 2, 36 + 12), 777.0, device=DEV)
    wide[1:N + 1, 4:40] = torch.tensor(x, device=DEV)
    rows = wide[1:N + 1, 4:40]                           # ld 48 > D, the base 16 bytes into a row
    # through the op: the view is taken as it is
    got = ops.knn_segments(rows, torch.tensor(group, device=DEV), S, k)
    _assert_exact(tuple(t.cpu().numpy() for t in got), want)
    # through the entry: outputs inside wider tables, a query sub-range that starts and ends inside a tile
    order, seg_ptr = ops._group_major(torch.tensor(group, device=DEV), S)
    q_first, n_q = 37, 101
    for n_splits in (1, 3):
        tables = [torch.full((n_q + 2, S * k + 3), -7, dtype=dt, device=DEV) for dt in (torch.int32, torch.float32) * 2]
        views = [t[1:n_q + 1, 1:S * k + 1] for t in tables]
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        _raw(rows, order, seg_ptr, S, k, q_first, n_q, n_splits, views[0], views[1], (views[2], views[3]), status)
        assert int(status) == 0
        cut = slice(q_first, q_first + n_q)
        _assert_exact((views[0].cpu().numpy().reshape(n_q, S, k), views[1].cpu().numpy().reshape(n_q, S, k), views[2].cpu().numpy(),
                       views[3].cpu().numpy()), tuple(w[cut] for w in want))
        for t in tables:                                 # guard rows and columns are untouched
            assert (t[0] == -7).all() and (t[-1] == -7).all() and (t[:, 0] == -7).all() and (t[:, S * k + 1:] == -7).all()
    # without the merged list: the blocked one alone
    idx = torch.full((N, S * k), -7, dtype=torch.int32, device=DEV)
    d2 = torch.full((N, S * k), -7.0, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _raw(rows, order, seg_ptr, S, k, 0, N, 0, idx, d2, None, status)
    _assert_exact((idx.cpu().numpy().reshape(N, S, k), d2.cpu().numpy().reshape(N, S, k)), want[:2])
    assert (wide[0] == 777).all() and (wide[:, :4] == 777).all() and (wide[:, 40:] == 777).all()


@pytest.mark.parametrize("case", R.REAL_CASES)
def test_real_rows_agree_up_to_near_ties(case, monkeypatch):
    x = R.real(*case)
    N, D = x.shape
    S, k = 4, 3
    group, want_idx, _, _, _ = BR.reference("real", S, k, *case)
    near = BR.near_ties(x, group, S, k)
    idx, d2, m_idx, m_d2 = first = _run(x, group, S, k)
    differs = idx != want_idx
    print(f"{case}: {int(differs.sum())} positions differ from the reference, {int(near.sum())} of {near.size} are near-ties")
    assert near.mean() <= 0.01                                                    # what may be excused at all
    assert not (differs & ~near).any()
    # every distance is within gamma * d of the fp64 distance of the pair it names; a block ascends, lists its own segment and
    # never the query
    exact = R.sq_distances(x, x)[np.arange(N)[:, None, None], idx]
    err = np.abs(d2.astype(np.float64) - exact)
    print(f"{case}: largest |d2 - exact| / exact = {(err / exact).max():.3e}, gamma = {R.gamma(D):.3e}")
    assert (err <= R.gamma(D) * exact).all()
    assert (np.diff(d2, axis=2) >= 0).all() and (idx >= 0).all() and (idx != np.arange(N)[:, None, None]).all()
    assert (group[idx] == np.arange(S)[None, :, None]).all()
    # the merged list is the kernel's own blocked lists under (d2, id)
    _assert_exact((m_idx, m_d2), BR.merge(idx.astype(np.int64), d2))
    # the bits of knn_rows for the pairs both list
    p_idx, p_d2 = (t.cpu().numpy() for t in ops.knn_rows(torch.tensor(x, device=DEV), 15))
    plain = {(i, int(j)): b for i in range(N) for j, b in zip(p_idx[i], _bits(p_d2)[i])}
    both = [(i, int(j), b) for i in range(N) for j, b in zip(m_idx[i], _bits(m_d2)[i]) if (i, int(j)) in plain]
    assert len(both) > N and all(plain[(i, j)] == b for i, j, b in both)
    # a second launch, every split and any query chunking: the same bits
    for kw in (dict(), dict(n_splits=1), dict(n_splits=3), dict(n_splits=16), dict(n_splits=64)):
        _assert_same(_run(x, group, S, k, **kw), first)
    monkeypatch.setattr(ops, "KNN_WORKSPACE_BYTES", 8 * k * S * 50)               # partial lists of 50 queries' units: 4+ chunks
    for kw in (dict(n_splits=1), dict(n_splits=3)):
        _assert_same(_run(x, group, S, k, **kw), first)


def test_a_nan_row_is_listed_nowhere_and_lists_nothing():
    x = R.lattice(36).copy()
    x[33, 5] = np.nan
    N, S, k = x.shape[0], 3, 3
    group = np.arange(N) % S
    keep = np.delete(np.arange(N), 33)
    want = BR.segments(x[keep], group[keep], S, k)                                # the other lists: the reference without that row
    for n_splits in (1, 2):
        got = _run(x, group, S, k, n_splits=n_splits)
        for t in (got[0], got[2]):
            assert not (t == 33).any() and (t[33] == -1).all()
        assert np.isposinf(got[1][33]).all() and np.isposinf(got[3][33]).all()
        _assert_exact(tuple(t[keep] for t in got), (keep[want[0]], want[1], keep[want[2]], want[3]))


def test_tiny_batches_and_empty_ones():
    x = R.tiny()
    group = np.arange(R.TINY_N) % 2
    idx, d2, m_idx, m_d2 = _run(x, group, 2, 8)                                   # 5 cells a group: 4 or 5 neighbours, then the tail
    n_listed = (idx >= 0).sum(axis=2)
    assert (n_listed == np.where(group[:, None] == np.arange(2)[None, :], 4, 5)).all()
    assert (np.isposinf(d2) == (idx < 0)).all() and ((m_idx >= 0).sum(axis=1) == 9).all() and (m_idx[:, 9:] == -1).all()
    want = BR.segments(x, group, 2, 8)
    assert not ((idx != want[0]) & ~BR.near_ties(x, group, 2, 8)).any()
    one = _run(x[:1], np.zeros(1, np.int64), 1, 3)                                # a single cell has no neighbour
    assert (one[0] == -1).all() and np.isposinf(one[1]).all() and (one[2] == -1).all() and np.isposinf(one[3]).all()
    none = ops.knn_segments(torch.zeros((0, 8), device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), 2, 3)
    assert none.idx.shape == (0, 2, 3) and none.merged_d2.shape == (0, 6)


def test_a_malformed_order_is_skipped_and_reported():
    """One id out of range and one listed twice, through the entry itself: the call returns, the status bit is set, and every
    slot holds -1 or a row id.  The kernel tests every id before it forms an address: this reads a refusal."""
    x = R.lattice(20)
    N, S, k = x.shape[0], 3, 3
    group = np.arange(N) % S
    rows = torch.tensor(x, device=DEV)
    order, seg_ptr = ops._group_major(torch.tensor(group, device=DEV), S)
    lost_a, lost_b, twice = int(order[10]), int(order[100]), int(order[101])
    order[10] = N + 5                                                             # outside [0, n_rows): row lost_a is no candidate
    order[100] = twice                                                            # row lost_b gives way to a second `twice`
    seg_ptr[S] = N + 1000                                                         # and the last bound points past `order`: clamped
    tables = [torch.full((N + 2, S * k + 2), -7, dtype=dt, device=DEV) for dt in (torch.int32, torch.float32) * 2]
    views = [t[1:N + 1, 1:S * k + 1] for t in tables]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _raw(rows, order, seg_ptr, S, k, 0, N, 2, views[0], views[1], (views[2], views[3]), status)
    assert int(status) == _lib.KNN_SEGMENTS_BAD_ORDER
    for t in (views[0], views[2]):
        t = t.cpu().numpy()
        assert ((t >= -1) & (t < N)).all() and not (t == lost_a).any() and not (t == lost_b).any()
    for t in tables:
        assert (t[0] == -7).all() and (t[-1] == -7).all() and (t[:, 0] == -7).all() and (t[:, S * k + 1:] == -7).all()
    # the lists of the rows that neither a lost row nor the double would have entered are the reference's
    _, want_idx, _, _, _ = BR.reference("lattice", S, k, 20)
    clean = ~np.isin(want_idx, (lost_a, lost_b, twice)).any(axis=(1, 2))
    assert clean.sum() > N // 2
    np.testing.assert_array_equal(views[0].cpu().numpy().reshape(N, S, k)[clean], want_idx[clean])
    with pytest.raises(ops.WgnnError, match="order names a row"):
        ops._check_status("knn_segments", int(status), ops._KNN_SEGMENTS_STATUS)


def test_argument_errors():
    x = torch.zeros((20, 8), device=DEV)
    g = torch.zeros(20, dtype=torch.int64, device=DEV)
    for kw in (dict(n_groups=0, k=3), dict(n_groups=65, k=1), dict(n_groups=2, k=0), dict(n_groups=1, k=65), dict(n_groups=5, k=13),
               dict(n_groups=64, k=2), dict(n_groups=2, k=3, n_splits=65), dict(n_groups=2, k=3, n_splits=-1)):
        with pytest.raises(ValueError):
            ops.knn_segments(x, g, **kw)
    for bad in (g[:19], g.float(), g.view(4, 5), g - 1, g + 2, torch.where(torch.arange(20, device=DEV) == 7, 2, 0)):
        with pytest.raises(ValueError, match="group"):
            ops.knn_segments(x, bad, 2, 3)
    with pytest.raises(ValueError, match="D = 1028"):
        ops.knn_segments(torch.zeros((4, 1028), device=DEV), g[:4], 1, 2)
    with pytest.raises(ValueError, match="float32"):
        ops.knn_segments(x.double(), g, 1, 2)
    # an empty group is allowed; int32 ids too; a width that is no multiple of 4 is zero-padded
    odd = torch.from_numpy(R.real(300, 20, 0)[:, :7].copy()).to(DEV)
    ids = torch.from_numpy(BR.random_groups(300, 4, 0)).to(DEV) * 2               # groups 1, 3, 5 and 7 hold no row
    a, b = ops.knn_segments(odd, ids.to(torch.int32), 8, 5), ops.knn_segments(torch.nn.functional.pad(odd, (0, 1)), ids, 8, 5)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and (a.idx[:, 1::2] == -1).all() and (a.idx[:, 0::2] >= 0).all()
