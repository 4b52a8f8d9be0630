"""``ops.knn_rows`` (``wgnn_knn_rows``) on the GPU against the fp64 brute-force reference (tests/knn_reference.py): bit for bit on
the lattice fixture, whose float32 distances are exact, and on real-valued rows up to the near-ties the error bound leaves
open; the split, the chunking and the launch change no bit."""
import numpy as np
import pytest
import torch

from scdeepsort_amd import ops

import knn_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(x, k, **kw):
    idx, d2 = ops.knn_rows(torch.tensor(x, device=DEV), k, **kw)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape
    return idx.cpu().numpy(), d2.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_exact(got, want):
    """the kernel's lists equal the reference's: the indices, and the float32 bits of the (exact) distances"""
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1].astype(np.float32)))


@pytest.mark.parametrize("D", R.LATTICE_DIMS)
@pytest.mark.parametrize("k", [1, 15, 64])
def test_lattice_is_bit_exact_for_every_split(D, k):
    x = R.lattice(D)
    want = R.reference("lattice", k, D)
    for n_splits in (0, 1, 3, 7):
        _assert_exact(_run(x, k, n_splits=n_splits), want)


def test_lattice_with_a_wider_row_stride_and_guards():
    x = R.lattice(36)
    N, k = x.shape[0], 15
    wide = torch.full((N + 2, 36 + 12), 777.0, device=DEV)
    wide[1:N + 1, 4:40] = torch.tensor(x, device=DEV)
    rows = wide[1:N + 1, 4:40]                           # ld 48 > D, the base 16 bytes into a row
    idx = torch.full((N + 2, k + 3), -7, dtype=torch.int32, device=DEV)
    d2 = torch.full((N + 2, k + 3), -7.0, device=DEV)
    for n_splits in (1, 3):
        out = ops.knn_rows(rows, k, n_splits=n_splits, out=(idx[1:N + 1, 1:k + 1], d2[1:N + 1, 1:k + 1]))
        _assert_exact((out[0].cpu().numpy(), out[1].cpu().numpy()), R.reference("lattice", k, 36))
        for t in (idx, d2):                              # guard rows and columns are untouched
            assert (t[0] == -7).all() and (t[-1] == -7).all() and (t[:, 0] == -7).all() and (t[:, k + 1:] == -7).all()
    assert (wide[0] == 777).all() and (wide[:, :4] == 777).all()


def test_lattice_queries_as_a_sub_range_without_self_and_as_strangers():
    x = R.lattice(20)
    dev_x = torch.tensor(x, device=DEV)
    k = 15
    # a sub-range of the rows as queries: query i is candidate 60 + i
    want = R.knn(x, k, queries=x[60:190], self_offset=60)
    for n_splits in (0, 3):
        got = ops.knn_rows(dev_x, k, queries=dev_x[60:190], self_offset=60, n_splits=n_splits)
        _assert_exact((got[0].cpu().numpy(), got[1].cpu().numpy()), want)
    # nothing left out: the cell itself comes first at distance 0 - unless a duplicate with a lower index does
    idx, d2 = _run(x, k, exclude_self=False)
    _assert_exact((idx, d2), R.knn(x, k, self_offset=None))
    first = np.arange(x.shape[0]); first[[50, 120]] = 7; first[121] = 8
    assert (d2[:, 0] == 0).all() and (idx[:, 0] == first).all()
    # queries that are no candidates
    q = (np.random.default_rng(9).integers(-32, 33, size=(70, 20)) / 8.0).astype(np.float32)
    got = ops.knn_rows(dev_x, k, queries=torch.from_numpy(q).to(DEV), exclude_self=False)
    _assert_exact((got[0].cpu().numpy(), got[1].cpu().numpy()), R.knn(x, k, queries=q, self_offset=None))


@pytest.mark.parametrize("case", R.REAL_CASES)
def test_real_rows_agree_up_to_near_ties(case, monkeypatch):
    x = R.real(*case)
    N, D = x.shape
    k = 15
    want_idx, _ = R.reference("real", k, *case)
    near = R.near_ties(x, k)
    idx, d2 = _run(x, k)
    differs = idx != want_idx
    print(f"{case}: {int(differs.sum())} positions differ from the reference, {int(near.sum())} near-ties")
    assert not (differs & ~near).any()
    # every distance is within gamma * d of the fp64 distance of the pair it names, and a row ascends
    exact = R.sq_distances(x, x)[np.arange(N)[:, None], idx]
    err = np.abs(d2.astype(np.float64) - exact)
    print(f"{case}: largest |d2 - exact| / exact = {(err / exact).max():.3e}, gamma = {R.gamma(D):.3e}")
    assert (err <= R.gamma(D) * exact).all()
    assert (np.diff(d2, axis=1) >= 0).all() and (idx >= 0).all() and (idx != np.arange(N)[:, None]).all()
    # d2(i, j) and d2(j, i) carry the same bits wherever both are listed
    at = {(i, int(j)): _bits(d2)[i, c] for i in range(N) for c, j in enumerate(idx[i])}
    both = [(p, q) for (p, q) in at if (q, p) in at]
    assert len(both) > N and all(at[(p, q)] == at[(q, p)] for p, q in both)
    # a second launch, every split and any query chunking: the same bits
    for kw in (dict(), dict(n_splits=1), dict(n_splits=3), dict(n_splits=7), dict(n_splits=64)):
        again = _run(x, k, **kw)
        np.testing.assert_array_equal(again[0], idx); np.testing.assert_array_equal(_bits(again[1]), _bits(d2))
    monkeypatch.setattr(ops, "KNN_WORKSPACE_BYTES", 8 * k * 100)          # partial lists of 100 (query, split) pairs: 8+ chunks
    for kw in (dict(), dict(n_splits=3)):
        again = _run(x, k, **kw)
        np.testing.assert_array_equal(again[0], idx); np.testing.assert_array_equal(_bits(again[1]), _bits(d2))


def test_tiny_batch_leaves_a_tail():
    x = R.tiny()
    for n_splits in (0, 2):
        idx, d2 = _run(x, R.TINY_K, n_splits=n_splits)
        differs = idx != R.reference("tiny", R.TINY_K)[0]
        assert not (differs & ~R.near_ties(x, R.TINY_K)).any()                    # nine neighbours each, then the tail
        assert (idx[:, R.TINY_N - 1:] == -1).all() and np.isposinf(d2[:, R.TINY_N - 1:]).all()
        assert np.isfinite(d2[:, :R.TINY_N - 1]).all()
    one = _run(x[:1], 3)                                                          # a single cell has no neighbour
    assert (one[0] == -1).all() and np.isposinf(one[1]).all()
    none = ops.knn_rows(torch.zeros((0, 8), device=DEV), 3)
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3)


def test_a_nan_row_is_listed_nowhere():
    x = R.lattice(36).copy()
    x[33, 5] = np.nan
    k = 15
    for n_splits in (1, 3):
        idx, d2 = _run(x, k, n_splits=n_splits)
        assert not (idx == 33).any() and (idx[33] == -1).all() and np.isposinf(d2[33]).all()
        keep = np.delete(np.arange(x.shape[0]), 33)
        want_idx, want_d2 = R.knn(x[keep], k)                                     # the other lists: the reference without that row
        _assert_exact((idx[keep], d2[keep]), (keep[want_idx], want_d2))


def test_argument_errors():
    x = torch.zeros((20, 8), device=DEV)
    for kw in (dict(k=0), dict(k=65), dict(k=3, n_splits=65), dict(k=3, n_splits=-1), dict(k=3, self_offset=1),
               dict(k=3, queries=torch.zeros((4, 12), device=DEV)), dict(k=3, queries=x[:5], self_offset=16),
               dict(k=3, out=(torch.zeros((20, 3), dtype=torch.int64, device=DEV), torch.zeros((20, 3), device=DEV)))):
        with pytest.raises(ValueError):
            ops.knn_rows(x, **kw)
    with pytest.raises(ValueError, match="D = 1028"):
        ops.knn_rows(torch.zeros((4, 1028), device=DEV), 2)
    with pytest.raises(ValueError, match="float32"):
        ops.knn_rows(x.double(), 2)
    # a width that is no multiple of 4 is zero-padded: the same lists as the padded rows give
    odd = torch.from_numpy(R.real(300, 20, 0)[:, :7].copy()).to(DEV)
    a, b = ops.knn_rows(odd, 5), ops.knn_rows(torch.nn.functional.pad(odd, (0, 1)), 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
