"""``ops.fuzzy_graph`` and ``ops.layout_graph`` on the GPU against the numpy restatement (tests/umap_reference.py).

Fuzzy rows: ``rho`` is EQUAL; a membership is within 2^-24 absolute - the device's float64 ``exp`` and numpy's differ in the last
bit, which moves ``p`` by about k 2^-52, ``sigma`` by ``dp / sum((x/s) e^(-x/s))`` relative and a membership by at most ``dp``, so
the two agree to about 1e-14 before the cast to float32 and within one float32 ulp (at most 2^-24 below 1) after it; ``sigma``,
whose conditioning is unbounded, is checked through its defining residual ``|p(sigma) - log2(k + 1)|`` where it is the bisection's,
and is EQUAL where it is the floor or the bisection ran away to 2^64; rows whose memberships are exactly 1 or 0 are EQUAL.  The
union's weights are EQUAL to numpy's from the device's own memberships.  The layout with ``b = 1`` is +, -, x, / in float32 and
EQUAL after every number of epochs; with ``b = 0.895`` one epoch is EQUAL but for the float64 ``pow``'s last bit straddling a
float32 rounding boundary (about 2^-29 per term): at most 0.1 % of the vertices, each within 2 float32 ulp at the magnitude
``max(|y|, 4 alpha)``.  The C entries expose no block size and no lanes-per-vertex choice, so there is no geometry to vary."""
import numpy as np
import pytest
import torch

from scdeepsort_amd import _lib, ops
from scdeepsort_amd.graph import _ptr, _stream

import umap_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


def _dev(x, dtype=None):
    return torch.tensor(np.asarray(x), device=DEV, dtype=dtype)


def _graph(rowptr, col, w):
    return _dev(rowptr, torch.int64), _dev(col, torch.int32), _dev(w, torch.float32)


def _check_fuzzy(idx, d2, got):
    n, k = idx.shape
    want = R.fuzzy_rows(idx, d2)
    rho, sigma, member = got.rho.cpu().numpy(), got.sigma.cpu().numpy(), got.member.cpu().numpy()
    assert (rho.dtype, sigma.dtype, member.dtype, member.shape) == (np.float64, np.float64, F, (n, k))
    np.testing.assert_array_equal(rho, want.rho)
    assert np.abs(member.astype(np.float64) - want.member).max(initial=0.0) <= 2.0 ** -24
    listed = (idx >= 0) & np.isfinite(d2)
    assert (member[~listed] == 0).all()
    np.testing.assert_array_equal(member[want.constant], want.member[want.constant])
    exact = want.floored | (want.sigma >= 2.0 ** 60) | ~listed.any(1)
    np.testing.assert_array_equal(sigma[exact], want.sigma[exact])
    free = ~exact & ~want.constant
    assert R.fuzzy_residual(idx, d2, rho, sigma)[free].max(initial=0.0) <= 1e-9
    # the union: the structure is snn_graph's, the weights numpy's from the device's own memberships, and symmetric
    rowptr, col, _ = R.snn_graph(idx, "unit")
    np.testing.assert_array_equal(got.rowptr.cpu().numpy(), rowptr)
    np.testing.assert_array_equal(got.col.cpu().numpy(), col)
    w = got.w.cpu().numpy()
    assert w.dtype == F
    np.testing.assert_array_equal(w, R.fuzzy_union(idx, member, rowptr, col))
    row = np.repeat(np.arange(n), np.diff(rowptr))
    back = {(int(r), int(c)): v for r, c, v in zip(row, col, w)}
    assert all(back[(c, r)] == v for (r, c), v in back.items())
    return want


@pytest.mark.parametrize("k", [1, 3, 15, 64])
def test_fuzzy_graph(k):
    idx, d2 = R.ragged_lists(70, k)
    want = _check_fuzzy(idx, d2, ops.fuzzy_graph(_dev(idx), _dev(d2)))
    if k >= 3:                                                          # the fixture holds the cases it says it holds
        assert want.constant[5] and want.floored[5] and (d2[0, :3] == 0).all() and (idx[9, 1:] == -1).all() and (idx[11] == -1).all()
        assert (~want.floored & ~want.constant).sum() >= 50
    first = ops.fuzzy_graph(_dev(idx), _dev(d2))
    # int32 lists, and both operands as views into wider rows
    wide_idx = torch.full((70, k + 3), 7, dtype=torch.int32, device=DEV)
    wide_d2 = torch.full((70, k + 5), 0.25, dtype=torch.float32, device=DEV)
    wide_idx[:, :k], wide_d2[:, :k] = _dev(idx, torch.int32), _dev(d2)
    for other in (ops.fuzzy_graph(_dev(idx, torch.int32), _dev(d2)), ops.fuzzy_graph(wide_idx[:, :k], wide_d2[:, :k])):
        assert all(torch.equal(a, b) for a, b in zip(first, other))


def test_fuzzy_graph_of_one_cell_and_argument_errors():
    for k in (1, 5):
        idx, d2 = np.full((1, k), -1, np.int64), np.full((1, k), np.inf, F)
        out = ops.fuzzy_graph(_dev(idx), _dev(d2))
        _check_fuzzy(idx, d2, out)
        assert out.rowptr.tolist() == [0, 0] and out.w.numel() == 0 and out.sigma.tolist() == [0.0]
    idx, d2 = R.ragged_lists(70, 3)
    for bad_idx, bad_d2 in ((_dev(idx).float(), _dev(d2)), (_dev(idx), _dev(d2).double()), (_dev(idx), _dev(d2)[:, :2]),
                            (_dev(idx)[:69], _dev(d2)), (_dev(np.zeros((4, 65), np.int64)), _dev(np.zeros((4, 65), F))),
                            (_dev(idx), -_dev(d2).clamp(max=9.0) - 1.0), (_dev(np.where(idx == 3, 70, idx)), _dev(d2)),
                            (_dev(np.where(idx == 3, -2, idx)), _dev(d2)), (_dev(idx).T.contiguous().T, _dev(d2))):
        with pytest.raises(ValueError):
            ops.fuzzy_graph(bad_idx, bad_d2)


# ---------------------------------------------------------------------------------------------------------------------------
def isolated_graph():
    """Two triangles sharing a vertex, and vertex 5 without an edge."""
    return R.csr_of(7, [(0, 1), (1, 2), (0, 2), (2, 3), (3, 4), (2, 4), (4, 6)], [1.0, 0.75, 0.5, 1.0, 0.25, 0.8125, 0.0625])


GRAPHS = {}


def graph(name):
    if name not in GRAPHS:
        GRAPHS[name] = {"small": lambda: R.blob_graph(40, 4, seed=2)[:3], "star": lambda: R.star_graph(300),
                        "isolated": isolated_graph, "one": lambda: (np.zeros(2, np.int64), np.zeros(0, np.int32), np.zeros(0, F)),
                        "full": lambda: R.blob_graph(200, 6, seed=4)[:3], "large": lambda: R.blob_graph(2000, 15, seed=5)[:3]}[name]()
    return GRAPHS[name]


@pytest.mark.parametrize("name", ["small", "star", "isolated", "one"])
def test_twenty_epochs_are_the_restatement_bit_for_bit(name):
    rowptr, col, w = graph(name)
    n = len(rowptr) - 1
    if name == "star":
        assert rowptr[1] - rowptr[0] == 300 > 16 * ops.LAYOUT_LANES
    for kw in (dict(a=1.0, b=1.0, seed=0), dict(a=1.577, b=1.0, seed=9, n_neg=2, gamma=0.5, lr=0.7)):
        want = R.layout_graph(rowptr, col, w, "hash", n_epochs=20, **kw)
        got = ops.layout_graph(*_graph(rowptr, col, w), "hash", n_epochs=20, **kw)
        assert got.y.dtype == torch.float32 and tuple(got.y.shape) == (n, 2)
        np.testing.assert_array_equal(got.y.cpu().numpy(), want.y)
        assert (got.n_epochs, got.n_fired) == (20, want.n_fired) and type(got.n_fired) is int
        again = ops.layout_graph(*_graph(rowptr, col, w), "hash", n_epochs=20, **kw)
        assert torch.equal(again.y, got.y) and again.n_fired == got.n_fired
        start = R.layout_init(n, kw["seed"])
        if name == "one":
            np.testing.assert_array_equal(want.y, start)
        else:
            assert want.n_fired > 0 and not np.array_equal(want.y, start)
        if name == "isolated":
            np.testing.assert_array_equal(got.y.cpu().numpy()[5], start[5])                # no edge: the position is kept


@pytest.mark.parametrize("a", [1.0, 1.577])
def test_a_full_run_with_b_equal_to_one(a):
    rowptr, col, w = graph("full")
    init = (R.layout_init(200, 11) * F(0.5)).astype(F)
    for seed, n_neg, start in ((0, 5, "hash"), (3, 5, "hash"), (0, 0, "hash"), (3, 0, init)):
        want = R.layout_graph(rowptr, col, w, start, n_epochs=50, a=a, b=1.0, n_neg=n_neg, seed=seed)
        got = ops.layout_graph(*_graph(rowptr, col, w), start if isinstance(start, str) else _dev(start), n_epochs=50, a=a, b=1.0,
                               n_neg=n_neg, seed=seed)
        np.testing.assert_array_equal(got.y.cpu().numpy(), want.y)
        assert got.n_fired == want.n_fired > 0 and np.isfinite(want.y).all()


def _one_epoch(graph_dev, n, nnz, wmax, y, epoch, n_epochs, a, b, gamma, alpha, n_neg, seed):
    out = torch.empty_like(y)
    dev = y.device
    _lib.run(dev, "wgnn_layout_epoch", _ptr(graph_dev[0]), _ptr(graph_dev[1]), _ptr(graph_dev[2]), n, nnz, wmax, _ptr(y), _ptr(out),
             epoch, n_epochs, a, b, gamma, alpha, n_neg, seed, None, 0, _stream(dev))
    return out


def test_one_epoch_with_a_fractional_b():
    rowptr, col, w = graph("large")
    n, nnz = len(rowptr) - 1, len(col)
    on_device = _graph(rowptr, col, w)
    wmax = float(w.max())
    spread = R.layout_graph(rowptr, col, w, "hash", n_epochs=6, b=1.0).y
    for y, epoch, alpha in ((R.layout_init(n, 0), 0, 1.0), ((R.layout_init(n, 1) * F(0.1)).astype(F), 37, 0.815), (spread, 199, 0.005)):
        want, _ = R.layout_epoch(rowptr, col, w, wmax, y, epoch, 200, 1.577, 0.895, 1.0, alpha, 5, 2)
        got = _one_epoch(on_device, n, nnz, wmax, _dev(y), epoch, 200, 1.577, 0.895, 1.0, alpha, 5, 2).cpu().numpy()
        assert np.isfinite(want).all() and not np.array_equal(want, y)
        differs = (got != want).any(axis=1)
        room = 2.0 * np.spacing(np.maximum(np.abs(want), F(4.0 * alpha)).astype(F)).astype(np.float64)
        print(f"epoch {epoch}: {int(differs.sum())} of {n} vertices differ, largest difference "
              f"{np.abs(got.astype(np.float64) - want).max():.3g}")
        assert differs.sum() <= n // 1000 and (np.abs(got.astype(np.float64) - want) <= room).all()


def test_layout_argument_errors():
    rowptr, col, w = _graph(*graph("small"))
    n = int(rowptr.shape[0]) - 1
    good = _dev(R.layout_init(n, 1))
    nan_w, neg_w, nan_y = w.clone(), w.clone(), good.clone()
    nan_w[3], neg_w[0], nan_y[1, 1] = float("nan"), -0.5, float("inf")
    for args, kw in (((rowptr, col, w, "pca"), {}), ((rowptr, col, w, "hash"), dict(n_epochs=0)),
                     ((rowptr, col, w, "hash"), dict(n_epochs=10001)), ((rowptr, col, w, "hash"), dict(n_neg=-1)),
                     ((rowptr, col, w, "hash"), dict(n_neg=65)), ((rowptr, col, w, "hash"), dict(seed=-1)),
                     ((rowptr, col, w, "hash"), dict(seed=2 ** 32)), ((rowptr, col, w, "hash"), dict(a=0.0)),
                     ((rowptr, col, w, "hash"), dict(b=float("nan"))), ((rowptr, col, w, "hash"), dict(lr=0.0)),
                     ((rowptr, col, w, "hash"), dict(gamma=-1.0)), ((rowptr, col, w, good[:-1]), {}),
                     ((rowptr, col, w, good.double()), {}), ((rowptr, col, w, nan_y), {}), ((rowptr, col, nan_w, good), {}),
                     ((rowptr, col, neg_w, good), {}), ((rowptr.to(torch.int32), col, w, good), {}),
                     ((rowptr, col.long(), w, good), {}), ((rowptr, col, w.double(), good), {}), ((rowptr, col[:-1], w, good), {}),
                     ((rowptr[:-1], col, w, good[:-1]), {})):
        with pytest.raises(ValueError):
            ops.layout_graph(*args, **kw)
    # an array start is copied, never written; all-zero weights fire nothing
    out = ops.layout_graph(rowptr, col, w, good, n_epochs=3)
    assert not torch.equal(out.y, good) and np.array_equal(good.cpu().numpy(), R.layout_init(n, 1))
    still = ops.layout_graph(rowptr, col, torch.zeros_like(w), "hash", n_epochs=3, seed=4)
    np.testing.assert_array_equal(still.y.cpu().numpy(), R.layout_init(n, 4))
    assert still.n_fired == 0
