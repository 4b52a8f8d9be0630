"""``wgnn_geodesic_round`` / ``ops.geodesic_rows`` / ``ops.distance_graph`` / ``ops.group_edges`` on the GPU against the numpy
restatement (tests/geodesic_reference.py) with NO tolerance: single launches on states from the middle of its runs, whole runs on
every fixture, every grid and read-back period, the ``max_rounds`` cut, and the status bits of a malformed graph."""
import functools

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops
from scdeepsort_amd.graph import _ptr, _stream

import geodesic_reference as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F = np.float32


def _on_device(rowptr, col, length):
    return (torch.from_numpy(np.asarray(rowptr, np.int64)).to(DEV), torch.from_numpy(np.asarray(col, np.int32)).to(DEV),
            torch.from_numpy(np.asarray(length, F)).to(DEV))


@functools.lru_cache(maxsize=None)
def _fixture(name):
    """``(rowptr, col, length, roots)`` on the host, computed once."""
    if name in G.HAND:
        return G.hand(name)
    if name == "star":
        return G.star()
    if name == "duplicates":
        return G.distance_graph(*G.duplicates()) + (0,)
    if name == "arc":
        return G.distance_graph(*G.arc()[1:]) + (0,)
    B, D, k = {"gauss600": (600, 8, 10), "gauss300": (300, 3, 5), "gauss1000": (1000, 16, 15)}[name]
    return G.distance_graph(*G.gaussian(B, D, k, seed=B)) + ([0, B // 2],)


@functools.lru_cache(maxsize=None)
def _reference(name, max_rounds=None):
    rowptr, col, length, roots = _fixture(name)
    states = []
    return G.geodesic_rows(rowptr, col, length, roots, max_rounds=max_rounds, states=states), states


FIXTURES = ("detour", "ties", "rounding", "chain", "chain2", "square", "edgeless", "star", "duplicates", "gauss600", "gauss300", "gauss1000", "arc")


def _same(out, want):
    np.testing.assert_array_equal(out.dist.cpu().numpy().view(np.uint32), want.dist.view(np.uint32))
    np.testing.assert_array_equal(out.pred.cpu().numpy(), want.pred)
    assert out.dist.dtype == torch.float32 and out.pred.dtype == torch.int32
    assert (out.rounds, out.converged, out.reached) == (want.rounds, want.converged, want.reached)


def _launch(graph, dist, pred, grid_blocks=0):
    """One ``wgnn_geodesic_round`` on the host state: ``(dist', pred', changed, status)``."""
    rowptr, col, length = _on_device(*graph)
    d_in, p_in = torch.from_numpy(np.asarray(dist, F)).to(DEV), torch.from_numpy(np.asarray(pred, np.int32)).to(DEV)
    d_out, p_out = torch.full_like(d_in, -7.0), torch.full_like(p_in, -7)
    slots = torch.zeros(2, dtype=torch.int64, device=DEV)
    _lib.run(DEV, "wgnn_geodesic_round", _ptr(rowptr), _ptr(col), _ptr(length), len(dist), int(col.shape[0]), _ptr(d_in), _ptr(p_in),
             _ptr(d_out), _ptr(p_out), slots.data_ptr(), slots.data_ptr() + 8, grid_blocks, 0, _stream(DEV))
    changed, status = slots.tolist()
    np.testing.assert_array_equal(d_in.cpu().numpy().view(np.uint32), np.asarray(dist, F).view(np.uint32))      # the input is read only
    return d_out.cpu().numpy(), p_out.cpu().numpy(), changed, status


@pytest.mark.parametrize("name, after", [("detour", 1), ("detour", 2), ("ties", 2), ("arc", 37), ("star", 1)])
def test_a_single_launch_from_the_middle_of_a_run(name, after):
    """The state after ``after`` rounds of the restatement, one launch, the restatement's next state - and its changed count."""
    rowptr, col, length, _ = _fixture(name)
    _, states = _reference(name)
    (dist, pred, _), (want_d, want_p, want_changed) = states[after - 1], states[after]
    assert want_changed > 0
    for grid_blocks in (0, 1, 7):
        got_d, got_p, changed, status = _launch((rowptr, col, length), dist, pred, grid_blocks)
        np.testing.assert_array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
        np.testing.assert_array_equal(got_p, want_p)
        assert (changed, status) == (want_changed, 0)
    # at the fixed point a round is the identity
    fin_d, fin_p, _ = states[-1]
    got_d, got_p, changed, status = _launch((rowptr, col, length), fin_d, fin_p)
    np.testing.assert_array_equal(got_d.view(np.uint32), fin_d.view(np.uint32))
    np.testing.assert_array_equal(got_p, fin_p)
    assert (changed, status) == (0, 0)


@pytest.mark.parametrize("name", FIXTURES)
def test_whole_runs_equal_the_restatement(name):
    rowptr, col, length, roots = _fixture(name)
    want, _ = _reference(name)
    graph = _on_device(rowptr, col, length)
    out = ops.geodesic_rows(*graph, roots)
    assert isinstance(out, ops.GeodesicRows)
    _same(out, want)
    _same(ops.geodesic_rows(*graph, roots), want)                       # two calls, the same bits


def test_roots_in_every_form():
    rowptr, col, length, _ = _fixture("gauss300")
    graph = _on_device(rowptr, col, length)
    want = G.geodesic_rows(rowptr, col, length, [7, 150, 299])
    for roots in ([7, 150, 299], (299, 7, 150, 7), np.array([150, 7, 299], np.int32), torch.tensor([299, 150, 7], device=DEV),
                  torch.tensor([7, 150, 299], dtype=torch.int32, device=DEV)):
        _same(ops.geodesic_rows(*graph, roots), want)
    one = G.geodesic_rows(rowptr, col, length, 5)
    for roots in (5, np.int64(5), [5], torch.tensor(5, device=DEV)):
        _same(ops.geodesic_rows(*graph, roots), one)
    for bad in ([], -1, 300, [0, 300], [0.5], "0", np.zeros((2, 2), np.int64), torch.tensor([1.0], device=DEV),
                torch.zeros(0, dtype=torch.int64, device=DEV), torch.tensor([300], device=DEV)):
        with pytest.raises(ValueError):
            ops.geodesic_rows(*graph, bad)
    with pytest.raises(sda.WgnnError, match="GPU only"):                 # a tensor of roots lives on the device, as every operand
        ops.geodesic_rows(*graph, torch.tensor([7]))
    for kw in (dict(max_rounds=-1), dict(check_every=0), dict(grid_blocks=-1), dict(grid_blocks=8193)):
        with pytest.raises(ValueError):
            ops.geodesic_rows(*graph, 0, **kw)
    with pytest.raises(ValueError):
        ops.geodesic_rows(graph[0], graph[1], graph[2].double(), 0)
    with pytest.raises(ValueError):
        ops.geodesic_rows(graph[0].int(), graph[1], graph[2], 0)


@pytest.mark.parametrize("name", ["arc", "star", "chain2"])
def test_grid_and_read_back_period_change_no_bit(name):
    rowptr, col, length, roots = _fixture(name)
    want, _ = _reference(name)
    graph = _on_device(rowptr, col, length)
    for grid_blocks in (1, 7, 0):
        for check_every in (1, 8, 64):
            _same(ops.geodesic_rows(*graph, roots, check_every=check_every, grid_blocks=grid_blocks), want)


def test_the_max_rounds_cut_is_exact():
    rowptr, col, length, roots = _fixture("chain")
    graph = _on_device(rowptr, col, length)
    for max_rounds in (100, 299, 300, 0, 1):                            # 100 = 12 x 8 + 4 and 299 = 37 x 8 + 3: the last batch is cut
        want, _ = _reference("chain", max_rounds)
        for check_every in (1, 8, 64):
            _same(ops.geodesic_rows(*graph, roots, max_rounds=max_rounds, check_every=check_every), want)
    cut, _ = _reference("chain", 100)
    assert (cut.reached, cut.converged, cut.rounds) == (101, False, 100)
    rowptr, col, length, roots = _fixture("arc")
    want, _ = _reference("arc", 20)
    assert not want.converged
    _same(ops.geodesic_rows(*_on_device(rowptr, col, length), roots, max_rounds=20), want)


def test_a_malformed_graph_raises_from_the_status_word():
    rowptr, col, length, _ = _fixture("gauss300")
    assert rowptr[11] - rowptr[10] >= 2

    def raises(word, rowptr=rowptr, col=col, length=length):
        with pytest.raises(sda.WgnnError, match=word):
            ops.geodesic_rows(*_on_device(rowptr, col, length), 0)

    swapped = col.copy()
    swapped[[rowptr[10], rowptr[10] + 1]] = swapped[[rowptr[10] + 1, rowptr[10]]]
    raises("not strictly ascending", col=swapped)
    twice = col.copy()
    twice[rowptr[10] + 1] = twice[rowptr[10]]
    raises("not strictly ascending", col=twice)
    for bad in (300, -1, 2 ** 31 - 1):
        out = col.copy()
        out[rowptr[20 + 1] - 1 if bad > 0 else rowptr[20]] = bad       # the row stays ascending
        raises(r"column is outside \[0, n\)", col=out)
    for bad in (-0.5, np.nan, np.inf, -np.inf):
        out = length.copy()
        out[17] = bad
        raises("negative, infinite or NaN", length=out)
    for at, bad in ((40, rowptr[41] + 1), (40, -3), (0, 1), (300, len(col) + 5), (300, len(col) - 1), (40, len(col) + 100)):
        out = rowptr.copy()
        out[at] = bad
        raises("rowptr does not ascend", rowptr=out)
    # ... and a single launch on such a graph writes a whole state all the same: nothing is read or written out of bounds
    out = col.copy()
    out[5] = 10 ** 6
    states = []
    G.geodesic_rows(rowptr, col, length, 0, states=states)
    got_d, got_p, changed, status = _launch((rowptr, out, length), states[1][0], states[1][1])
    assert status & _lib.GEODESIC_BAD_COL and np.isfinite(got_d).sum() >= np.isfinite(states[1][0]).sum() and (got_p >= -1).all()


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_distance_graph_equals_the_restatement(dtype):
    for idx, d2 in (G.gaussian(300, 3, 5, seed=300), G.duplicates(), G.arc()[1:]):
        want = G.distance_graph(idx, d2)
        out = ops.distance_graph(torch.from_numpy(idx).to(DEV, dtype), torch.from_numpy(d2).to(DEV))
        assert isinstance(out, ops.DistanceGraph) and (out.rowptr.dtype, out.col.dtype, out.length.dtype) == (torch.int64, torch.int32, torch.float32)
        np.testing.assert_array_equal(out.rowptr.cpu().numpy(), want[0])
        np.testing.assert_array_equal(out.col.cpu().numpy(), want[1])
        np.testing.assert_array_equal(out.length.cpu().numpy().view(np.uint32), want[2].view(np.uint32))
        snn = ops.snn_graph(torch.from_numpy(idx).to(DEV, dtype), "unit")          # snn_graph's structure exactly
        assert torch.equal(out.rowptr, snn.rowptr) and torch.equal(out.col, snn.col)


def test_distance_graph_roots_are_correctly_rounded():
    """float32 values around every kind of rounding case: the device's ``length`` has the bits of ``np.sqrt`` in float32."""
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.uniform(0, 4, 6000), 10.0 ** rng.uniform(-30, 30, 6000), [0.0, 1.0, 2.0, 3.0, 1e-40, 3e38],
                           np.arange(1, 4001) ** 2.0, (np.arange(1, 3995) ** 2.0) + 1]).astype(F)
    n = len(vals)
    assert n == 20000
    idx = np.stack([(np.arange(n) + 1) % n], axis=1)                    # a ring: cell i lists i + 1 at the squared distance vals[i]
    out = ops.distance_graph(torch.from_numpy(idx).to(DEV), torch.from_numpy(vals[:, None]).to(DEV))
    rowptr, col, length = (t.cpu().numpy() for t in out)
    assert (np.diff(rowptr) == 2).all()
    row = np.repeat(np.arange(n), 2)
    want = np.sqrt(np.where(col == (row + 1) % n, vals[row], vals[col]))
    np.testing.assert_array_equal(length.view(np.uint32), want.view(np.uint32))


def test_distance_graph_argument_errors():
    idx, d2 = G.gaussian(300, 3, 5, seed=300)
    ti, td = torch.from_numpy(idx).to(DEV), torch.from_numpy(d2).to(DEV)
    for bad in (-1.0, float("nan"), float("inf")):
        broken = td.clone()
        broken[3, 2] = bad
        with pytest.raises(ValueError, match="negative, NaN or infinite"):
            ops.distance_graph(ti, broken)
    short_i, short_d = ti.clone(), td.clone()                           # a list that is short: -1 / +inf is no error
    short_i[3, 4], short_d[3, 4] = -1, float("inf")
    assert ops.distance_graph(short_i, short_d).col.shape[0] > 0
    out_of_range = ti.clone()
    out_of_range[0, 0] = 300
    for args in ((out_of_range, td), (ti.float(), td), (ti, td.double()), (ti[:, :3], td), (ti[0], td[0]),
                 (torch.zeros((3, 65), dtype=torch.int64, device=DEV), torch.zeros((3, 65), device=DEV))):
        with pytest.raises(ValueError):
            ops.distance_graph(*args)


def test_group_edges_equal_the_numpy_tables():
    s, idx, _ = G.arc()
    rng = np.random.default_rng(2)
    for K, group in ((4, np.floor(4 * s).astype(np.int64)), (7, rng.integers(-1, 7, 800)), (3, np.full(800, -1)), (4096, rng.integers(0, 4096, 800))):
        want = G.group_edges(idx, group, K)
        for dtype in (torch.int32, torch.int64):
            out = ops.group_edges(torch.from_numpy(idx).to(DEV, dtype), torch.from_numpy(group).to(DEV, dtype), K)
            assert isinstance(out, ops.GroupEdges) and out.edges.dtype == out.size.dtype == torch.int64
            assert tuple(out.edges.shape) == (K, K) and tuple(out.size.shape) == (K,)
            np.testing.assert_array_equal(out.edges.cpu().numpy(), want[0])
            np.testing.assert_array_equal(out.size.cpu().numpy(), want[1])
    short = idx.copy()
    short[::5, -2:] = -1                                                # short lists
    group = rng.integers(-1, 5, 800)
    out = ops.group_edges(torch.from_numpy(short).to(DEV), torch.from_numpy(group).to(DEV), 5)
    np.testing.assert_array_equal(out.edges.cpu().numpy(), G.group_edges(short, group, 5)[0])
    ti, tg = torch.from_numpy(idx).to(DEV), torch.from_numpy(group).to(DEV)
    for args in ((ti, tg, 0), (ti, tg, 4097), (ti, tg, 4), (ti, tg[:-1], 5), (ti, tg.float(), 5), (ti.float(), tg, 5),
                 (torch.where(ti == 0, 800, ti), tg, 5), (ti, torch.where(tg == 0, -2, tg), 5)):
        with pytest.raises(ValueError):
            ops.group_edges(*args)
