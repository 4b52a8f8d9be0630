"""``ops.silhouette_rows`` on the GPU against its numpy restatement (tests/silhouette_reference.py): bit for bit wherever the float32
squared distances are exact (the lattice, ``blobs``) - everything then rests on ``sqrtf`` being correctly rounded and on the order
of the fp64 additions - and within the stated bound of the plain fp64 silhouette on real-valued rows; neither ``n_splits`` nor a
second launch changes a bit."""
import numpy as np
import pytest
import torch

from scdeepsort_amd import ops

import kmeans_reference as M
import knn_reference as R
import silhouette_reference as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _dev(x):
    return torch.tensor(np.asarray(x), device=DEV)


def _host(out):
    return tuple(t.cpu().numpy() for t in out)


def _assert_bits(got, want):
    """``a``, ``b``, ``score`` bit for bit (every NaN is the same to this test), ``nearest`` and ``size`` exactly."""
    for name, g, w in zip(("a", "b", "score"), got[:3], want[:3]):
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=name)
        np.testing.assert_array_equal(_bits(g)[~np.isnan(g)], _bits(w)[~np.isnan(w)], err_msg=name)
    np.testing.assert_array_equal(got[3], want[3])
    np.testing.assert_array_equal(got[4], want[4])


def _same(a, b):
    return all(torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u, v.view(torch.int64) if v.dtype == torch.float64 else v)
               for u, v in zip(a, b))


@pytest.mark.parametrize("D", R.LATTICE_DIMS)
def test_the_lattice_is_bit_exact_for_every_split_and_operand_form(D):
    x, g, K = R.lattice(D), S.lattice_groups(), 7
    want = S.reference("lattice", D)
    assert want[4].tolist()[:3] == [100, 0, 1] and want[4].sum() == 190
    first = ops.silhouette_rows(_dev(x), _dev(g), K)
    assert [t.dtype for t in first] == [torch.float64] * 3 + [torch.int32, torch.int64]
    _assert_bits(_host(first), want)
    for n_splits in (1, 2, 5):                                           # 7 groups in 1, 2 and 5 ranges, and the call again
        assert _same(ops.silhouette_rows(_dev(x), _dev(g), K, n_splits=n_splits), first), n_splits
    assert _same(ops.silhouette_rows(_dev(x), _dev(g.astype(np.int32)), K), first)
    wide = torch.full((R.LATTICE_N + 2, D + 12), 777.0, device=DEV)      # a strided view between guard columns and rows
    wide[1:-1, 4:4 + D] = _dev(x)
    assert _same(ops.silhouette_rows(wide[1:-1, 4:4 + D], _dev(g), K), first)
    assert (wide[0] == 777).all() and (wide[-1] == 777).all() and (wide[:, :4] == 777).all() and (wide[:, 4 + D:] == 777).all()
    assert torch.equal(wide[1:-1, 4:4 + D], _dev(x))


@pytest.mark.parametrize("D", M.BLOB_DIMS)
def test_blobs_with_the_reference_kmeans_labels_are_bit_exact(D):
    x, label = M.blobs(D), M.reference("blobs", 5, 0, D)["label"]
    got = ops.silhouette_rows(_dev(x), _dev(label), 5)
    _assert_bits(_host(got), S.reference("blobs", D))
    assert _same(ops.silhouette_rows(_dev(x), _dev(label), 5, n_splits=5), got)


def test_many_small_groups_over_every_split_count():
    """600 groups for 197 cells - most empty, the others of one to three cells: the plan kernel walks several groups per thread
    and deals them to as many as 64 splits."""
    x, K = R.lattice(36), 600
    g = np.random.default_rng(7).integers(0, K, R.LATTICE_N)
    g[[4, 90]] = -1
    want = S.silhouette(x, g, K)
    assert (want[4] == 0).sum() > 400 and (want[4] == 1).sum() > 50 and want[4].max() >= 2
    first = ops.silhouette_rows(_dev(x), _dev(g), K, n_splits=1)
    _assert_bits(_host(first), want)
    for n_splits in (0, 3, 64):
        assert _same(ops.silhouette_rows(_dev(x), _dev(g), K, n_splits=n_splits), first), n_splits
    top = np.full(R.LATTICE_N, 4095)                                     # the last id of the most groups there can be
    top[::2] = 17
    for n_splits in (0, 64):                                             # 64 splits for four candidate tiles: most get no group
        _assert_bits(_host(ops.silhouette_rows(_dev(x), _dev(top), 4096, n_splits=n_splits)), S.silhouette(x, top, 4096))


def _real_cases():
    big = np.array(S.real_groups(300))
    big[big != 0] = 1                                                    # one group of ~ 240 cells: four candidate tiles
    assert 192 < (big == 1).sum() <= 256
    return (("overlap-20", M.overlap(300, 20, 0), S.real_groups(300), 4), ("overlap-200", M.overlap(300, 200, 0), S.real_groups(300), 4),
            ("overlap-200-big-group", M.overlap(300, 200, 0), big, 2), ("overlap-197-columns", M.overlap(300, 200, 0)[:, :197].copy(),
                                                                           S.real_groups(300), 4))


@pytest.mark.parametrize("case", _real_cases(), ids=lambda c: c[0])
def test_real_rows_are_within_the_bound_of_plain_fp64(case):
    _, x, g, K = case
    D, on = x.shape[1], S.participants(x, g, K)
    first = ops.silhouette_rows(_dev(x), _dev(g), K)
    a, b, s, nearest, size = _host(first)
    pa, pb, ps, pn, psize = S.plain(x, g, K)
    np.testing.assert_array_equal(size, psize)
    assert np.isnan(s[~on]).all() and np.isnan(a[~on]).all() and np.isnan(b[~on]).all() and (nearest[~on] == -1).all()
    worst = np.abs(s[on] - ps[on]).max()
    print(case[0], "worst deviation of score from plain fp64", worst, "bound", S.bound(D))
    assert worst <= S.bound(D)
    e = S.bound(D)
    assert (np.abs(a[on] - pa[on]) <= e * pa[on]).all() and (np.abs(b[on] - pb[on]) <= e * pb[on]).all()
    free = S.two_lowest_gap(x, g, K) > S.bound(D)                         # the two lowest means are apart: no near-tie
    assert (on & ~free).sum() <= 0.02 * on.sum()
    np.testing.assert_array_equal(nearest[on & free], pn[on & free])
    for n_splits in (1, 2, 5):
        assert _same(ops.silhouette_rows(_dev(x), _dev(g), K, n_splits=n_splits), first), n_splits
    # the restatement itself: its d2 is the fp64 distance rounded once, the kernel's a chain - equal wherever no chain rounds twice
    ra, rb, rs, rn, _ = S.silhouette(x, g, K)
    assert np.abs(s[on] - rs[on]).max() <= S.bound(D)


def test_rows_and_groups_that_take_no_part():
    x, g, K = np.array(R.lattice(20)), np.array(S.lattice_groups()), 7
    x[3, 5], x[9, 0] = np.nan, np.inf                                    # a NaN row and an inf row
    g[11] = 9                                                            # an id outside [0, K)
    got = _host(ops.silhouette_rows(_dev(x), _dev(g), K))
    _assert_bits(got, S.silhouette(x, g, K))
    out = [3, 9, 11]
    assert np.isnan(got[0][out]).all() and np.isnan(got[1][out]).all() and np.isnan(got[2][out]).all() and (got[3][out] == -1).all()
    # all participating cells in one group: b = +inf, nearest = -1, score = NaN
    one = np.where(S.lattice_groups() >= 0, 3, -1)
    a, b, s, nearest, size = _host(ops.silhouette_rows(_dev(R.lattice(20)), _dev(one), K))
    on = one >= 0
    assert np.isinf(b[on]).all() and (b[on] > 0).all() and (nearest == -1).all() and np.isnan(s).all() and (a[on] > 0).all()
    assert np.isnan(a[~on]).all() and size.tolist() == [0, 0, 0, 190, 0, 0, 0]
    _assert_bits((a, b, s, nearest, size), S.silhouette(R.lattice(20), one, K))
    # nobody takes part
    a, b, s, nearest, size = _host(ops.silhouette_rows(_dev(R.lattice(20)), _dev(np.full(197, -1)), K))
    assert np.isnan(a).all() and np.isnan(b).all() and np.isnan(s).all() and (nearest == -1).all() and (size == 0).all()


def test_tiny_batches_and_argument_errors():
    one = ops.silhouette_rows(torch.ones((1, 8), device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), 2)
    a, b, s, nearest, size = _host(one)
    assert a.tolist() == [0.0] and np.isinf(b).all() and np.isnan(s).all() and nearest.tolist() == [-1] and size.tolist() == [1, 0]
    none = ops.silhouette_rows(torch.ones((0, 8), device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), 2)
    assert [tuple(t.shape) for t in none] == [(0,)] * 4 + [(2,)] and none[4].tolist() == [0, 0]
    # two cells, two groups: a = 0 (singletons), b = the distance, score 0
    two = torch.tensor([[0.0] * 8, [3.0, 4.0] + [0.0] * 6], device=DEV)
    a, b, s, nearest, _ = _host(ops.silhouette_rows(two, torch.tensor([0, 1], device=DEV), 2))
    assert a.tolist() == [0, 0] and b.tolist() == [5, 5] and s.tolist() == [0, 0] and nearest.tolist() == [1, 0]
    # a width that is no multiple of 4 is zero-padded: no bit changes
    odd = M.overlap(300, 20, 0)[:, :7].copy()
    g = _dev(S.real_groups(300))
    assert _same(ops.silhouette_rows(_dev(odd), g, 4), ops.silhouette_rows(torch.nn.functional.pad(_dev(odd), (0, 1)), g, 4))
    x = _dev(M.blobs(20))
    ids = torch.zeros(197, dtype=torch.int64, device=DEV)
    for kw in (dict(n_groups=0), dict(n_groups=4097), dict(n_groups=3, n_splits=-1), dict(n_groups=3, n_splits=65)):
        with pytest.raises(ValueError):
            ops.silhouette_rows(x, ids, **kw)
    with pytest.raises(ValueError, match="float32"):
        ops.silhouette_rows(x.double(), ids, 3)
    with pytest.raises(ValueError, match="D = 1028"):
        ops.silhouette_rows(torch.zeros((8, 1028), device=DEV), ids[:8], 2)
    with pytest.raises(ValueError, match="one id per cell"):
        ops.silhouette_rows(x, ids[:5], 3)
    with pytest.raises(ValueError, match="one id per cell"):
        ops.silhouette_rows(x, ids.float(), 3)
