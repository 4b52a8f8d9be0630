"""``ops.leiden_graph`` and the three ``wgnn_leiden_*`` kernels on the GPU against the numpy restatement (tests/leiden_reference.py):
single launches on states taken from the middle of the restatement's runs, and whole runs whose every level's labels, refined
labels, counts, ``qnum_trace`` and clusters are EQUAL - integers leave no tolerance - on the graphs where Louvain leaves a
disconnected community, where the refinement falls back, on kNN graphs, on the three routes of the sweep kernel and where the
gains need all 64 bits; the launch geometry changes no bit, and ``louvain_graph`` is what it was."""
import numpy as np
import pytest
import torch

from scdeepsort_amd import WgnnError, _lib, ops
from scdeepsort_amd.graph import _ptr, _stream

import leiden_reference as L
import louvain_reference as R
from test_gpu_louvain_rows import NEEDS_64_BITS, dense_coarse_graph
from test_leiden_reference import fallback_graph, g14, g30
from test_louvain_reference import csr_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x, dtype=None):
    return torch.tensor(np.asarray(x), device=DEV, dtype=dtype)


def _graph(rowptr, col, w):
    return _dev(rowptr, torch.int64), _dev(col, torch.int32), _dev(w, torch.int32)


def _same(got, want):
    np.testing.assert_array_equal(got.cluster.cpu().numpy(), want.cluster)
    assert got.cluster.dtype == torch.int64
    assert len(got.level_labels) == len(want.level_labels) and len(got.refined_labels) == len(want.refined_labels)
    for mine, theirs in zip(got.level_labels + got.refined_labels, want.level_labels + want.refined_labels):
        np.testing.assert_array_equal(mine.cpu().numpy(), theirs)
    assert got.levels == want.levels and got.qnum_trace == want.qnum_trace and all(type(q) is int for q in got.qnum_trace)
    assert (got.modularity, got.resolution, got.M, got.converged) == (want.modularity, want.resolution, want.M, want.converged)


def _identical(a, b):
    assert torch.equal(a.cluster, b.cluster)
    assert all(torch.equal(x, y) for x, y in zip(a.level_labels + a.refined_labels, b.level_labels + b.refined_labels))
    assert (a.levels, a.qnum_trace, a.modularity, a.converged) == (b.levels, b.qnum_trace, b.modularity, b.converged)


def _single_launches(level, sweep, M, frac, wave_rows=128, block_rows=2048):
    """The three kernels, one launch each, on what the restatement's sweep read: what they leave is what it left."""
    dev, stream = torch.device(DEV), _stream(torch.device(DEV))
    rowptr, col, w = _graph(level["rowptr"], level["col"], level["w"])
    n, nnz = len(level["deg"]), len(level["col"])
    P, ref, size = (_dev(sweep[name], torch.int32) for name in ("P", "ref", "size_r"))
    deg, totP, tot = _dev(level["deg"], torch.int64), _dev(sweep["totP"], torch.int64), _dev(sweep["tot_r"], torch.int64)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    ext, kinP = torch.full((n,), -7, dtype=torch.int64, device=dev), torch.full((n,), -7, dtype=torch.int64, device=dev)
    _lib.run(dev, "wgnn_leiden_boundary", _ptr(rowptr), _ptr(col), _ptr(w), n, nnz, _ptr(P), _ptr(ref), _ptr(ext), _ptr(kinP),
             _ptr(stats), 0, stream)
    np.testing.assert_array_equal(ext.cpu().numpy(), sweep["ext"])
    np.testing.assert_array_equal(kinP.cpu().numpy(), sweep["kinP"])
    again = torch.full((n,), -7, dtype=torch.int64, device=dev)
    _lib.run(dev, "wgnn_leiden_boundary", _ptr(rowptr), _ptr(col), _ptr(w), n, nnz, _ptr(P), _ptr(ref), _ptr(again), None,
             _ptr(stats), 0, stream)                                                          # kinP not wanted
    assert torch.equal(again, ext)
    lens = np.diff(level["rowptr"])
    heavy = _dev(np.flatnonzero(lens > wave_rows), torch.int32)
    n_scratch = int((lens > block_rows).sum())
    ws = torch.zeros(max(n * n_scratch, 1), dtype=torch.int32, device=dev)
    prop, gain = torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n,), -7, dtype=torch.int64, device=dev)
    _lib.run(dev, "wgnn_leiden_refine_sweep", _ptr(rowptr), _ptr(col), _ptr(w), n, nnz, _ptr(P), _ptr(ref), _ptr(deg), _ptr(totP),
             _ptr(tot), _ptr(size), _ptr(ext), _ptr(kinP), M * frac.denominator, frac.numerator, sweep["r"],
             _ptr(heavy) if len(heavy) else None, len(heavy), wave_rows, block_rows, _ptr(prop), _ptr(gain), _ptr(stats),
             _ptr(ws) if n_scratch else None, n * n_scratch * 4, n_scratch, 0, stream)
    np.testing.assert_array_equal(prop.cpu().numpy(), sweep["prop"])
    np.testing.assert_array_equal(gain.cpu().numpy(), sweep["gain"])
    assert not ws.any()                                                                       # the scratch is zero again
    nxt = torch.full((n,), -7, dtype=torch.int32, device=dev)
    stats[0] = 99
    _lib.run(dev, "wgnn_leiden_accept", _ptr(ref), _ptr(prop), n, _ptr(nxt), _ptr(gain), _ptr(stats), 0, stream)
    np.testing.assert_array_equal(nxt.cpu().numpy(), sweep["next"])
    np.testing.assert_array_equal(gain.cpu().numpy(), sweep["kept"])
    assert stats.tolist() == [int((sweep["next"] != sweep["ref"]).sum()), 0, 0, 0]


@pytest.mark.parametrize("name", ["g30", "fallback"])
def test_single_launches_on_states_from_the_restatement(name):
    graph = {"g30": g30, "fallback": fallback_graph}[name]()
    states = []
    out = L.leiden_graph(*graph, resolution=0.5, states=states)
    first = states[0]["sweeps"]
    assert (first[0]["size_r"] == 1).all() and first[1]["size_r"].max() > 1 and (first[1]["ref"] != np.arange(30)).any()
    assert any((s["prop"] != s["next"]).any() for level in states for s in level["sweeps"])  # a refused proposal is among them
    for level in states:
        for sweep in level["sweeps"]:
            _single_launches(level, sweep, out.M, out.resolution)
    for sweep in first[:2]:                                             # ... and through the workgroup table and the scratch
        _single_launches(states[0], sweep, out.M, out.resolution, wave_rows=2, block_rows=2048)
        _single_launches(states[0], sweep, out.M, out.resolution, wave_rows=1, block_rows=3)


@pytest.mark.parametrize("name,resolution", [("g14", 0.5), ("g30", 0.5), ("fallback", 0.5), ("g30", 1), ("g30", 2), ("fallback", 1)])
def test_the_committed_graphs(name, resolution):
    graph = {"g14": g14, "g30": g30, "fallback": fallback_graph}[name]()
    want = L.leiden_graph(*graph, resolution=resolution)
    out = ops.leiden_graph(*_graph(*graph), resolution=resolution)
    _same(out, want)
    assert L.disconnected(graph[0], graph[1], out.cluster.cpu().numpy()) == 0
    if (name, resolution) == ("g14", 0.5):
        assert out.levels[-1]["split"] == 1 and out.qnum_trace[-1] == 7086 and len(out.level_labels) == len(out.levels) + 1
    if (name, resolution) == ("g30", 0.5):
        assert out.qnum_trace[-1] == 116238 and len(out.levels) == 4
    if (name, resolution) == ("fallback", 0.5):
        assert [level["refine_fallback_moves"] for level in out.levels] == [0, 1, 0, 0]


def test_louvain_graph_is_what_it_was():
    graph = g30()
    want = R.louvain_graph(*graph, resolution=0.5)
    out = ops.louvain_graph(*_graph(*graph), resolution=0.5)
    np.testing.assert_array_equal(out.cluster.cpu().numpy(), want.cluster)
    for mine, theirs in zip(out.level_labels, want.level_labels):
        np.testing.assert_array_equal(mine.cpu().numpy(), theirs)
    assert (out.levels, out.qnum_trace, out.modularity) == (want.levels, want.qnum_trace, want.modularity)
    assert out.modularity == 0.5891987513007284 and L.disconnected(graph[0], graph[1], out.cluster.cpu().numpy()) == 1


@pytest.mark.parametrize("weights", ["snn", "unit"])
@pytest.mark.parametrize("B,D,n_blobs,k", [(64, 4, 3, 5), (300, 6, 5, 6)])
def test_knn_graphs(B, D, n_blobs, k, weights):
    graph = R.snn_graph(R.knn_lists(R.blobs(B, D, n_blobs, 2.0, seed=0), k), weights)
    on_device = _graph(*graph)
    for resolution in (0.5, 1, 2):
        _same(ops.leiden_graph(*on_device, resolution=resolution), L.leiden_graph(*graph, resolution=resolution))
    stopped = ops.leiden_graph(*on_device, max_sweeps=2)
    assert not stopped.converged
    _same(stopped, L.leiden_graph(*graph, max_sweeps=2))


def star_graph(n_leaves, seed=0):
    """A hub (the highest id, so that sweep 0 of the refinement lets it look at every leaf) with ``n_leaves`` leaves of weight 1 to
    5, a few edges among the leaves, and a clique of six tied to the hub by three light edges: another community of P, whose
    entries the hub's long row has to skip."""
    rng = np.random.default_rng(seed)
    hub = n_leaves + 6
    edges = {(i, hub): int(rng.integers(1, 6)) for i in range(n_leaves)}
    for _ in range(n_leaves // 10):
        a, b = sorted(rng.choice(n_leaves, 2, replace=False).tolist())
        edges[(a, b)] = 1
    clique = list(range(n_leaves, n_leaves + 6))
    edges.update({(a, b): 40 for x, a in enumerate(clique) for b in clique[x + 1:]})
    edges.update({(a, hub): 1 for a in clique[:3]})
    return csr_of(hub + 1, list(edges), list(edges.values())), hub


@pytest.mark.parametrize("n_leaves,at_least,route", [(130, 130, "workgroup"), (2500, 2100, "scratch")])
def test_a_long_row_inside_one_community(n_leaves, at_least, route):
    """The hub has 130 (all of its leaves) and 2 166 (of 2 500 leaves) entries inside its own community of P."""
    graph, hub = star_graph(n_leaves)
    states = []
    want = L.leiden_graph(*graph, states=states)
    first = states[0]["sweeps"][0]
    inside = graph[1][graph[0][hub]:graph[0][hub + 1]]
    inside = inside[first["P"][inside] == first["P"][hub]]
    assert len(inside) >= at_least > (ops.LOUVAIN_BLOCK_ROWS if route == "scratch" else ops.LOUVAIN_WAVE_ROWS)
    assert len(inside) < graph[0][hub + 1] - graph[0][hub] and first["prop"][hub] != hub     # the hub moves, past foreign entries
    on_device = _graph(*graph)
    out = ops.leiden_graph(*on_device)
    _same(out, want)
    for knobs in (dict(scratch_blocks=1), dict(wave_rows=2, block_rows=3, scratch_blocks=7), dict(wave_rows=0, block_rows=2048)):
        _identical(ops.leiden_graph(*on_device, **knobs), out)
    for sweep in states[0]["sweeps"][:2]:
        _single_launches(states[0], sweep, want.M, want.resolution)


@pytest.mark.parametrize("inside", [1, 2])
def test_dense_coarse_level(inside):
    graph = dense_coarse_graph(inside)
    on_device = _graph(*graph)
    out = ops.leiden_graph(*on_device)
    _same(out, L.leiden_graph(*graph))
    for knobs in (dict(wave_rows=16), dict(wave_rows=16, block_rows=20), dict(wave_rows=0, block_rows=0, scratch_blocks=3)):
        _identical(ops.leiden_graph(*on_device, **knobs), out)


@pytest.mark.parametrize("x,y,p,q,diff", NEEDS_64_BITS)
def test_gains_need_all_64_bits(x, y, p, q, diff):
    graph = csr_of(5, [(4, 0), (4, 2), (0, 1), (2, 3)], [x, y, p, q])
    _same(ops.leiden_graph(*_graph(*graph)), L.leiden_graph(*graph))


def test_scaled_weights_keep_64_bit_products_exact():
    """The 300-cell kNN graph with every weight multiplied by the largest odd factors under the guard: the two well-connectedness
    products and the scores pass 2^53."""
    rowptr, col, w = R.snn_graph(R.knn_lists(R.blobs(300, 6, 5, 2.0, seed=0), 6))
    for factor, resolution in ((100003, 1), (70001, 0.5)):
        scaled = w.astype(np.int64) * factor
        want = L.leiden_graph(rowptr, col, scaled, resolution=resolution)
        assert 2 ** 59 < want.M * want.M * max(want.resolution.numerator, want.resolution.denominator) < 2 ** 62
        _same(ops.leiden_graph(*_graph(rowptr, col, scaled), resolution=resolution), want)


def test_two_calls_and_every_launch_geometry_give_the_same_bits():
    graph = _graph(*fallback_graph())
    first = ops.leiden_graph(*graph, resolution=0.5)
    _identical(ops.leiden_graph(*graph, resolution=0.5), first)
    for knobs in (dict(wave_rows=0), dict(block_rows=0), dict(scratch_blocks=1), dict(wave_rows=0, block_rows=0, scratch_blocks=1),
                  dict(wave_rows=3, block_rows=6), dict(wave_rows=0, block_rows=0, scratch_blocks=256)):
        _identical(ops.leiden_graph(*graph, resolution=0.5, **knobs), first)


def test_a_malformed_partition_is_a_status_bit():
    """Ids outside [0, n) and a founder in another community: skipped and reported, by the boundary kernel and by the sweep."""
    states = []
    out = L.leiden_graph(*g30(), resolution=0.5, states=states)
    level, sweep = states[0], states[0]["sweeps"][1]
    dev, stream = torch.device(DEV), _stream(torch.device(DEV))
    rowptr, col, w = _graph(level["rowptr"], level["col"], level["w"])
    n, nnz = 30, len(level["col"])
    deg, totP, tot = _dev(level["deg"], torch.int64), _dev(sweep["totP"], torch.int64), _dev(sweep["tot_r"], torch.int64)
    size, ext, kinP = _dev(sweep["size_r"], torch.int32), _dev(sweep["ext"], torch.int64), _dev(sweep["kinP"], torch.int64)
    other = int(np.flatnonzero(sweep["P"] != sweep["P"][0])[0])
    for what, v, value in (("ref", 3, 30), ("ref", 3, -1), ("P", 5, 2 ** 31 - 1), ("ref", 0, other)):
        bad = {name: sweep[name].copy() for name in ("P", "ref")}
        bad[what][v] = value
        P, ref = _dev(bad["P"], torch.int32), _dev(bad["ref"], torch.int32)
        stats = torch.zeros(4, dtype=torch.int64, device=dev)
        out_ext = torch.zeros(n, dtype=torch.int64, device=dev)
        _lib.run(dev, "wgnn_leiden_boundary", _ptr(rowptr), _ptr(col), _ptr(w), n, nnz, _ptr(P), _ptr(ref), _ptr(out_ext), None,
                 _ptr(stats), 0, stream)
        assert stats.tolist() == [0, 0, 0, _lib.LEIDEN_BAD_PARTITION], (what, v, value)
        stats.zero_()
        prop, gain = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
        _lib.run(dev, "wgnn_leiden_refine_sweep", _ptr(rowptr), _ptr(col), _ptr(w), n, nnz, _ptr(P), _ptr(ref), _ptr(deg), _ptr(totP),
                 _ptr(tot), _ptr(size), _ptr(ext), _ptr(kinP), out.M * 2, 1, 1, None, 0, 128, 2048, _ptr(prop), _ptr(gain), _ptr(stats),
                 None, 0, 0, 0, stream)
        assert int(stats[3]) == _lib.LEIDEN_BAD_PARTITION and int(prop[v]) == int(ref[v]) and int(gain[v]) == 0
        nxt = torch.zeros(n, dtype=torch.int32, device=dev)
        _lib.run(dev, "wgnn_leiden_accept", _ptr(ref), _ptr(prop), n, _ptr(nxt), _ptr(gain), _ptr(stats), 0, stream)
        assert int(nxt[v]) == int(ref[v])


def test_guard_and_refusals():
    for resolution, W in ((1, 2 ** 30), (2, 2 ** 30 - 1)):
        with pytest.raises(ValueError, match="2\\^62"):
            ops.leiden_graph(*_graph(*csr_of(2, [(0, 1)], [W])), resolution=resolution)
    _same(ops.leiden_graph(*_graph(*csr_of(2, [(0, 1)], [2 ** 30 - 1]))), L.leiden_graph(*csr_of(2, [(0, 1)], [2 ** 30 - 1])))
    rowptr, col, w = _graph(*csr_of(6, [(0, 1), (0, 2), (1, 2), (4, 5)]))
    for bad in (dict(resolution=0), dict(resolution=-1), dict(max_sweeps=0), dict(wave_rows=129), dict(block_rows=2049),
                dict(scratch_blocks=0)):
        with pytest.raises(ValueError):
            ops.leiden_graph(rowptr, col, w, **bad)
    with pytest.raises(ValueError):
        ops.leiden_graph(rowptr.to(torch.int32), col, w)
    with pytest.raises(ValueError, match="self loop"):
        ops.leiden_graph(*_graph([0, 2, 3], [0, 1, 0], [1, 1, 1]))
    swapped = col.clone()
    swapped[0], swapped[1] = col[1], col[0]
    with pytest.raises(WgnnError, match="ascending"):
        ops.leiden_graph(rowptr, swapped, w)
    far = col.clone()
    far[-1] = 6
    with pytest.raises(WgnnError, match="outside"):
        ops.leiden_graph(rowptr, far, w)
    empty = ops.leiden_graph(torch.zeros(5, dtype=torch.int64, device=DEV), col[:0], w[:0])
    assert empty.cluster.tolist() == [-1] * 4 and empty.M == 0 and empty.qnum_trace == [0] and empty.levels[0]["split"] == 0
    assert ops.leiden_graph(rowptr, col, w).cluster.tolist() == [0, 0, 0, -1, 1, 1]
