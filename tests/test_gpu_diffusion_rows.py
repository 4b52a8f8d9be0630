"""The ``wgnn_diffusion_*`` / ``wgnn_lanczos_*`` / ``wgnn_basis_combine`` kernels and ``ops.diffusion_operator`` / ``lanczos_graph`` /
``basis_combine`` / ``diffusion_distance`` / ``graph_components`` on the GPU against the numpy restatement
(tests/diffusion_reference.py) with NO tolerance: single launches of every kernel on every grid, the dots and updates at the
sizes around a chunk, whole runs basis vector by basis vector, the clip, the breakdown, the inert step behind it, and the status
bits of a malformed graph."""
import functools

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops
from scdeepsort_amd.graph import _ptr, _stream

import diffusion_reference as R
from umap_reference import blob_graph, star_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GRIDS = (1, 7, 0)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(DEV)


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want):
    np.testing.assert_array_equal(_bits(got), _bits(want))


@functools.lru_cache(maxsize=None)
def _graph(name):
    """``(rowptr, col, w)`` on the host."""
    if name == "hand":
        return R.hand_graph()
    if name == "star":
        return star_graph(300)
    if name == "two_parts":
        return tuple(R.two_parts()[:3])
    return tuple(blob_graph(200, 8, seed=4)[:3])


@functools.lru_cache(maxsize=None)
def _operator(name):
    return R.diffusion_operator(*_graph(name))


@functools.lru_cache(maxsize=None)
def _run(name, n_steps=32, seed=0):
    rowptr, col, _ = _graph(name)
    op = _operator(name)
    mask, _ = R.largest_component(rowptr, col)
    return mask, R.lanczos_graph(rowptr, col, op.t, op.z, mask, n_steps, seed)


def _on_device(name):
    rowptr, col, w = _graph(name)
    return _dev(rowptr, np.int64), _dev(col, np.int32), _dev(w, np.float32)


GRAPHS = ("hand", "star", "knn200")


@pytest.mark.parametrize("name", GRAPHS)
def test_single_launches_of_the_operator_kernels(name):
    rowptr, col, w = _on_device(name)
    want = _operator(name)
    n, nnz = rowptr.shape[0] - 1, col.shape[0]
    graph = (_ptr(rowptr), _ptr(col), _ptr(w), n, nnz)
    q_in, z_in = _dev(want.q, np.float64), _dev(want.z, np.float64)     # named: a pointer does not keep its tensor alive
    for grid in GRIDS:
        q, z = torch.full((n,), -7.0, dtype=torch.float64, device=DEV), torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
        t = torch.full((nnz,), -7.0, dtype=torch.float64, device=DEV)
        status = torch.zeros(1, dtype=torch.int64, device=DEV)
        _lib.run(DEV, "wgnn_diffusion_degree", *graph, None, _ptr(q), _ptr(status), grid, 0, _stream(DEV))
        _same(q, want.q)
        _lib.run(DEV, "wgnn_diffusion_degree", *graph, _ptr(q_in), _ptr(z), _ptr(status), grid, 0, _stream(DEV))
        _same(z, want.z)
        _lib.run(DEV, "wgnn_diffusion_weights", *graph, _ptr(q_in), _ptr(z_in), _ptr(t), _ptr(status), grid, 0, _stream(DEV))
        _same(t, want.t)
        assert int(status) == 0
    out = ops.diffusion_operator(rowptr, col, w)
    assert isinstance(out, ops.DiffusionOperator) and out.t.dtype == out.q.dtype == out.z.dtype == torch.float64
    _same(out.t, want.t); _same(out.q, want.q); _same(out.z, want.z)
    row = np.repeat(np.arange(n), np.diff(_graph(name)[0]))
    back = {(int(c), int(r)): v for r, c, v in zip(row, _graph(name)[1], _bits(out.t))}
    assert all(back[(int(r), int(c))] == v for r, c, v in zip(row, _graph(name)[1], _bits(out.t)))      # t_ij and t_ji: the same bits
    if name == "hand":
        assert float(out.q[7]) == 0 and float(out.z[7]) == 0 and (out.t[w == 0] == 0).all()


@pytest.mark.parametrize("name", GRAPHS)
def test_a_single_apply(name):
    rowptr, col, _ = _on_device(name)
    n, nnz = rowptr.shape[0] - 1, col.shape[0]
    t = _operator(name).t
    x = np.random.default_rng(3).normal(size=n)
    want = R.apply(_graph(name)[0], _graph(name)[1], t, x)
    td, xd = _dev(t, np.float64), _dev(x, np.float64)
    words = torch.zeros(2, dtype=torch.int64, device=DEV)
    for grid in GRIDS:
        y = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
        _lib.run(DEV, "wgnn_lanczos_apply", _ptr(rowptr), _ptr(col), _ptr(td), n, nnz, _ptr(xd), _ptr(y), words.data_ptr(),
                 words.data_ptr() + 8, grid, 0, _stream(DEV))
        _same(y, want)
    _same(xd, x)
    words[0] = 5                                                        # halted: the launch is inert
    y = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    _lib.run(DEV, "wgnn_lanczos_apply", _ptr(rowptr), _ptr(col), _ptr(td), n, nnz, _ptr(xd), _ptr(y), words.data_ptr(),
             words.data_ptr() + 8, 0, 0, _stream(DEV))
    assert (y == -7.0).all() and words.tolist() == [5, 0]


def _dots(V, w, c, keep, halt, tag, ws, grid, flags=0):
    n = w.shape[0]
    _lib.run(DEV, "wgnn_lanczos_dots", None if V is None else _ptr(V), n, 1 if V is None else V.shape[0], _ptr(w), n, _ptr(c),
             None if keep is None else _ptr(keep), halt, tag, _ptr(ws), ws.numel() * 8, grid, flags, _stream(DEV))


@pytest.mark.parametrize("B", [1, 255, 256, 257, 1000])
def test_dots_update_norm_and_scale_around_a_chunk(B):
    rng = np.random.default_rng(B)
    for n_rows in (1, 2, 129):
        V, w = rng.normal(size=(n_rows, B)), rng.normal(size=B)
        want_c = R.dots(V, w)
        want_w = R.update(V, want_c, w)
        want_norm = R.norm(w)
        Vd, wd = _dev(V, np.float64), _dev(w, np.float64)
        ws = torch.empty(int(_lib.lib().wgnn_lanczos_dots_workspace_bytes(B, n_rows)) // 8, dtype=torch.float64, device=DEV)
        assert ws.numel() == -(-B // 256) * n_rows
        halt = torch.zeros(1, dtype=torch.int64, device=DEV)
        for grid in GRIDS:
            c, keep = torch.full((n_rows,), -7.0, dtype=torch.float64, device=DEV), torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
            _dots(Vd, wd, c, keep, halt.data_ptr(), 1, ws, grid)
            _same(c, want_c); _same(keep, want_c[-1:])
            nrm = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
            _dots(None, wd, nrm, keep, halt.data_ptr(), 3, ws, grid, _lib.LANCZOS_NORM)
            _same(nrm, [want_norm]); _same(keep, [want_norm])
            assert int(halt) == 0                                       # far above 2^-26
            upd = wd.clone()
            _lib.run(DEV, "wgnn_lanczos_update", _ptr(Vd), B, n_rows, _ptr(c), _ptr(upd), B, halt.data_ptr(), grid, 0, _stream(DEV))
            _same(upd, want_w)
            v = torch.full((B,), -7.0, dtype=torch.float64, device=DEV)
            _lib.run(DEV, "wgnn_lanczos_scale", _ptr(wd), _ptr(nrm), _ptr(v), B, halt.data_ptr(), grid, 0, _stream(DEV))
            _same(v, w / want_norm)
        _same(Vd, V); _same(wd, w)                                      # the inputs are read only


def test_a_small_norm_sets_the_halt_word_and_later_launches_are_inert():
    B = 300
    w = np.full(B, 2.0 ** -40)
    wd = _dev(w, np.float64)
    ws = torch.empty(2, dtype=torch.float64, device=DEV)
    halt = torch.zeros(1, dtype=torch.int64, device=DEV)
    nrm = torch.zeros(1, dtype=torch.float64, device=DEV)
    _dots(None, wd, nrm, None, halt.data_ptr(), 9, ws, 0, _lib.LANCZOS_NORM)
    _same(nrm, [R.norm(w)])
    assert int(halt) == 9 and float(nrm) <= ops.LANCZOS_BREAKDOWN
    big = _dev(np.ones(B), np.float64)
    _dots(None, big, nrm, None, halt.data_ptr(), 11, ws, 0, _lib.LANCZOS_NORM)
    _same(nrm, [R.norm(w)])                                             # inert: neither the norm nor the word is written again
    assert int(halt) == 9
    V = _dev(np.ones((2, B)), np.float64)
    c, upd, v = torch.full((2,), -7.0, dtype=torch.float64, device=DEV), wd.clone(), torch.full((B,), -7.0, dtype=torch.float64, device=DEV)
    _dots(V, wd, c, None, halt.data_ptr(), 1, torch.empty(4, dtype=torch.float64, device=DEV), 0)
    ones = _dev([1.0, 1.0], np.float64)
    _lib.run(DEV, "wgnn_lanczos_update", _ptr(V), B, 2, _ptr(ones), _ptr(upd), B, halt.data_ptr(), 0, 0, _stream(DEV))
    _lib.run(DEV, "wgnn_lanczos_scale", _ptr(wd), _ptr(nrm), _ptr(v), B, halt.data_ptr(), 0, 0, _stream(DEV))
    assert (c == -7.0).all() and (v == -7.0).all()
    _same(upd, w)


def test_the_start_vectors():
    z = np.random.default_rng(0).uniform(0.1, 1.0, 700)
    mask = np.random.default_rng(1).uniform(size=700) < 0.8
    for seed in (0, 1, 2 ** 32 - 1):
        w0, w1 = torch.empty(700, dtype=torch.float64, device=DEV), torch.empty(700, dtype=torch.float64, device=DEV)
        zd, md = _dev(z, np.float64), _dev(mask, np.uint8)
        _lib.run(DEV, "wgnn_lanczos_init", _ptr(zd), _ptr(md), 700, seed, _ptr(w0), _ptr(w1), 0, _stream(DEV))
        want0, want1 = R.lanczos_init(z, mask, seed)
        _same(w0, want0); _same(w1, want1)
        assert (w1[_dev(~mask, bool)] == 0).all() and float(w1.min()) >= -1 and float(w1.max()) < 1


def _same_run(out, want):
    assert isinstance(out, ops.LanczosRows)
    assert (out.n_run, out.breakdown, out.n_cells) == (want.n_run, want.breakdown, want.n_cells)
    _same(out.alpha, want.alpha); _same(out.beta, want.beta)
    assert tuple(out.V.shape) == want.V.shape
    for j in range(want.V.shape[0]):
        np.testing.assert_array_equal(_bits(out.V[j]), _bits(want.V[j]), err_msg=f"basis vector {j}")


@pytest.mark.parametrize("name", ["knn200", "two_parts"])
def test_whole_runs_equal_the_restatement(name):
    rowptr, col, _ = _on_device(name)
    mask, want = _run(name)
    op = _operator(name)
    assert want.n_run == 32 and not want.breakdown
    t, z, m = _dev(op.t, np.float64), _dev(op.z, np.float64), _dev(mask, bool)
    out = ops.lanczos_graph(rowptr, col, t, z, m, n_steps=32)
    _same_run(out, want)
    _same_run(ops.lanczos_graph(rowptr, col, t, z, m, n_steps=32), want)              # two calls, the same bits
    _same_run(ops.lanczos_graph(rowptr, col, t, z, m, n_steps=32, check_every=1, grid_blocks=1), want)
    _same_run(ops.lanczos_graph(rowptr, col, t, z, m, n_steps=32, check_every=5, grid_blocks=7), want)
    if name == "two_parts":
        assert 0 < mask.sum() < len(mask) and (out.V[:, _dev(~mask, bool)] == 0).all()      # masked rows stay exactly zero
        assert mask.sum() == 80 and not mask[0]                         # the larger part, which is not the one with cell 0
    other = R.lanczos_graph(_graph(name)[0], _graph(name)[1], op.t, op.z, mask, 8, seed=5)
    _same_run(ops.lanczos_graph(rowptr, col, t, z, m, n_steps=8, seed=5), other)
    assert not np.array_equal(other.V[1], want.V[1])


def test_the_clip_on_a_path_and_the_breakdown_on_a_complete_graph():
    for graph, n_steps, n_run in ((R.path_graph(5), 32, 4), (R.complete_graph(8), 7, 1), (R.complete_graph(8), 32, 1)):
        rowptr, col, w = graph
        n = len(rowptr) - 1
        op = R.diffusion_operator(rowptr, col, w)
        want = R.lanczos_graph(rowptr, col, op.t, op.z, np.ones(n, bool), n_steps)
        assert want.n_run == n_run and want.breakdown and want.V.shape[0] == min(n_steps, n - 1) + 1
        for check_every in (1, 16):
            out = ops.lanczos_graph(_dev(rowptr, np.int64), _dev(col, np.int32), _dev(op.t, np.float64), _dev(op.z, np.float64),
                                    torch.ones(n, dtype=torch.bool, device=DEV), n_steps=n_steps, check_every=check_every)
            _same_run(out, want)                                        # the steps enqueued behind the breakdown wrote nothing
    # one cell, and none
    rowptr, col, w = R.hand_graph()
    op = R.diffusion_operator(rowptr, col, w)
    args = (_dev(rowptr, np.int64), _dev(col, np.int32), _dev(op.t, np.float64), _dev(op.z, np.float64))
    for cells in ([3], [7], []):
        mask = np.zeros(12, bool)
        mask[cells] = True
        _same_run(ops.lanczos_graph(*args, _dev(mask, bool), n_steps=4), R.lanczos_graph(rowptr, col, op.t, op.z, mask, 4))


def test_ritz_vectors_and_distances_equal_the_restatement():
    rowptr, col, w = _graph("knn200")
    want = R.diffmap(rowptr, col, w, n_comps=9, n_steps=32)
    _, run = _run("knn200")
    theta, S, _ = ops.lanczos_ritz(run.alpha, run.beta, run.n_run)
    V = _dev(run.V, np.float64)
    for n_cols in (8, 1, 0, 32):
        Y = ops.basis_combine(V, S[:, :n_cols])
        _same(Y, R.basis_combine(run.V, S[:, :n_cols]))
    Y = ops.basis_combine(V, torch.from_numpy(S[:, :8].copy()).to(DEV))
    _same(Y, want.Y)
    first = Y[:, 1:].abs().argmax(dim=0)
    assert (Y[first, torch.arange(1, 9, device=DEV)] > 0).all()
    g = R.diffusion_weights(want.eigenvalues)
    for roots in (0, [5, 150], torch.tensor([199, 0, 7], device=DEV)):
        for n_dcs in (2, 9):
            r = roots.cpu().numpy() if isinstance(roots, torch.Tensor) else roots
            d = ops.diffusion_distance(Y[:, :n_dcs].contiguous(), g[:n_dcs], roots)
            _same(d, R.diffusion_distance(want.Y[:, :n_dcs], g[:n_dcs], r))
    _same(ops.diffusion_distance(Y, g, 0), R.diffusion_distance(want.Y, g, 0))          # a wider Y than n_dcs is a view
    holed = Y.clone()
    holed[17] = float("nan")
    d = ops.diffusion_distance(holed, g, [0, 3])
    assert torch.isnan(d[17]) and int(torch.isnan(d).sum()) == 1
    for bad in (dict(Y=Y.float()), dict(g=g[:1]), dict(g=np.zeros(10)), dict(roots=200), dict(roots=[])):
        with pytest.raises(ValueError):
            ops.diffusion_distance(**{**dict(Y=Y, g=g, roots=0), **bad})
    with pytest.raises(ValueError):
        ops.basis_combine(V, np.zeros((33, 2)))
    with pytest.raises(ValueError):
        ops.basis_combine(V[:5], np.zeros((4, 64)))


@pytest.mark.parametrize("name", ["hand", "two_parts", "knn200"])
def test_graph_components(name):
    rowptr, col, _ = _on_device(name)
    out = ops.graph_components(rowptr, col)
    assert out.dtype == torch.int64
    np.testing.assert_array_equal(out.cpu().numpy(), R.components(*_graph(name)[:2]))
    if name == "hand":
        assert out.tolist() == [0] * 7 + [7] + [0] * 4
    bad = col.clone()
    bad[0] = rowptr.shape[0] - 1
    with pytest.raises(ValueError):
        ops.graph_components(rowptr, bad)
    with pytest.raises(ValueError):
        ops.graph_components(rowptr[:-1], col)


def test_a_malformed_graph_raises_from_the_status_word():
    rowptr, col, w = _graph("knn200")
    t, z = _operator("knn200").t, _operator("knn200").z
    n = len(rowptr) - 1
    assert rowptr[11] - rowptr[10] >= 2

    def raises(word, rowptr=rowptr, col=col, w=w, t=t):
        with pytest.raises(sda.WgnnError, match=word):
            ops.diffusion_operator(_dev(rowptr, np.int64), _dev(col, np.int32), _dev(w, np.float32))
        with pytest.raises(sda.WgnnError, match=word):
            ops.lanczos_graph(_dev(rowptr, np.int64), _dev(col, np.int32), _dev(t, np.float64), _dev(z, np.float64),
                              torch.ones(n, dtype=torch.bool, device=DEV), n_steps=2)

    swapped = col.copy()
    swapped[[rowptr[10], rowptr[10] + 1]] = swapped[[rowptr[10] + 1, rowptr[10]]]
    raises("not strictly ascending", col=swapped)
    for bad in (n, -1, 2 ** 31 - 1):
        out = col.copy()
        out[rowptr[20 + 1] - 1 if bad > 0 else rowptr[20]] = bad        # the row stays ascending
        raises(r"column is outside \[0, n\)", col=out)
    for bad in (-0.5, np.nan, np.inf, -np.inf):
        out_w, out_t = w.copy(), t.copy()
        out_w[17] = out_t[17] = bad
        raises("negative, infinite or NaN", w=out_w, t=out_t)
    for at, bad in ((40, rowptr[41] + 1), (40, -3), (0, 1), (n, len(col) + 5), (n, len(col) - 1), (40, len(col) + 100)):
        out = rowptr.copy()
        out[at] = bad
        raises("rowptr does not ascend", rowptr=out)
    # ... and a single launch on such a graph writes every row all the same: nothing is read or written out of bounds
    out = col.copy()
    out[5] = 10 ** 6
    y = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    words = torch.zeros(2, dtype=torch.int64, device=DEV)
    held = (_dev(rowptr, np.int64), _dev(out, np.int32), _dev(t, np.float64), _dev(z, np.float64))
    _lib.run(DEV, "wgnn_lanczos_apply", _ptr(held[0]), _ptr(held[1]), _ptr(held[2]), n, len(col), _ptr(held[3]), _ptr(y),
             words.data_ptr(), words.data_ptr() + 8, 0, 0, _stream(DEV))
    halted, status = words.tolist()                                    # the entry behind it is now out of order as well
    assert halted == 0 and status == _lib.DIFFUSION_BAD_COL | _lib.DIFFUSION_UNSORTED
    assert bool(torch.isfinite(y).all()) and not (y == -7.0).any()


def test_argument_errors(monkeypatch):
    rowptr, col, w = _on_device("knn200")
    op = _operator("knn200")
    t, z = _dev(op.t, np.float64), _dev(op.z, np.float64)
    mask = torch.ones(200, dtype=torch.bool, device=DEV)
    for bad in (dict(n_steps=0), dict(n_steps=1025), dict(seed=-1), dict(seed=2 ** 32), dict(check_every=0), dict(grid_blocks=-1),
                dict(grid_blocks=8193), dict(mask=mask[:-1]), dict(mask=mask.int()), dict(z=z.float()), dict(t=t.float())):
        with pytest.raises(ValueError):
            ops.lanczos_graph(**{**dict(rowptr=rowptr, col=col, t=t, z=z, mask=mask, n_steps=4), **bad})
    monkeypatch.setattr(ops, "LANCZOS_BASIS_BYTES", 5 * 200 * 8 - 1)
    with pytest.raises(ValueError, match="LANCZOS_BASIS_BYTES"):
        ops.lanczos_graph(rowptr, col, t, z, mask, n_steps=4)
    assert ops.lanczos_graph(rowptr, col, t, z, mask, n_steps=3).n_run == 3
    for bad in (dict(w=w.double()), dict(rowptr=rowptr.int()), dict(grid_blocks=8193)):
        with pytest.raises(ValueError):
            ops.diffusion_operator(**{**dict(rowptr=rowptr, col=col, w=w), **bad})
