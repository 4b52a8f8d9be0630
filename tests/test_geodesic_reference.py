"""The numpy restatement of the geodesic rounds and the PAGA tables (tests/geodesic_reference.py) against hand-computed graphs, a
float32 heap Dijkstra, scipy's float64 Dijkstra and exact rationals - and the host tables (``tables.Pseudotime`` /
``tables.Abstraction``) on its results.  No GPU: tests/test_gpu_geodesic_rows.py holds the device to the same restatement with no
tolerance."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import dijkstra
from scipy.stats import spearmanr

import geodesic_reference as G
from scdeepsort_amd import tables

F = np.float32
inf = np.inf


def _run(name, **kw):
    rowptr, col, length, roots = G.hand(name)
    return G.geodesic_rows(rowptr, col, length, roots, **kw), (rowptr, col, length, roots)


def _scipy(rowptr, col, length, roots):
    """scipy's float64 Dijkstra on the same float32 lengths: ``(dist, pred)`` to the nearest root."""
    n = len(rowptr) - 1
    m = sp.csr_matrix((np.asarray(length, np.float64), col, rowptr), shape=(n, n))
    d, p, _ = dijkstra(m, directed=True, indices=np.atleast_1d(roots), return_predecessors=True, min_only=True)
    return d, p


@pytest.mark.parametrize("name, dist, pred, rounds, reached", [
    ("detour", [0, 3, 1, 2, 3.5, inf], [-1, 3, 0, 2, 1, -1], 4, 5),
    ("ties", [0, .5, 1, 2, 3, 1], [-1, 0, 1, 5, 3, 0], 3, 6),
    ("rounding", [0, .5, 1, 1], [-1, 0, 0, 1], 2, 4),
])
def test_hand_graphs(name, dist, pred, rounds, reached):
    states = []
    out, graph = _run(name, states=states)
    np.testing.assert_array_equal(out.dist, np.asarray(dist, F))
    np.testing.assert_array_equal(out.pred, pred)
    assert (out.rounds, out.converged, out.reached) == (rounds, True, reached)
    assert [s[2] > 0 for s in states] == [True] * rounds + [False]     # the changing rounds, then the idle one that ends the run
    np.testing.assert_array_equal(G.dijkstra_f32(*graph), out.dist)


def test_detour_improves_a_vertex_twice_and_ties_keep_the_first_predecessor():
    states = []
    _run("detour", states=states)
    assert [float(s[0][1]) for s in states[:4]] == [4.0, 4.0, 3.0, 3.0] and [int(s[1][1]) for s in states[:3]] == [0, 0, 3]
    states = []
    _run("ties", states=states)
    # vertex 3 is reached through 5 in round 2; the equal candidate through 2 arrives in round 3 and must not replace it
    assert [int(s[1][3]) for s in states[:3]] == [-1, 5, 5] and float(states[2][0][3]) == 2.0


def test_rounding_is_the_float32_contract_not_scipys_float64():
    out, (rowptr, col, length, roots) = _run("rounding")
    assert out.dist[3] == F(1.0) and out.pred[3] == 1                   # both candidates round to 1.0: the lower id wins
    d, p = _scipy(rowptr, col, length, roots)
    assert p[3] == 2 and d[3] == 1.0 + .75 * 2.0 ** -24 and abs(d[3] - 1.00000004) < 1e-8


def test_chain_and_square():
    out, graph = _run("chain")
    assert (out.rounds, out.converged, out.reached) == (299, True, 300)
    np.testing.assert_array_equal(out.dist, np.arange(300, dtype=F) / 4)
    cut, _ = _run("chain", max_rounds=100)
    assert (cut.rounds, cut.converged, cut.reached) == (100, False, 101)
    np.testing.assert_array_equal(cut.dist[:101], out.dist[:101])
    assert np.isinf(cut.dist[101:]).all()
    exact, _ = _run("chain", max_rounds=299)                            # the cap hit exactly at the fixed point: no idle round ran
    np.testing.assert_array_equal(exact.dist, out.dist)
    assert (exact.rounds, exact.converged) == (299, False)
    two, _ = _run("chain2")
    assert two.rounds == 149 and two.dist.max() == F(37.25)
    assert np.flatnonzero(two.dist == two.dist.max()).tolist() == [149, 150] and two.pred[149] == 148 and two.pred[150] == 151
    square, _ = _run("square")
    assert square.pred[3] == 1 and square.dist[3] == 2
    alone, _ = _run("edgeless")                                         # no edge at all: the root, and an idle first round
    assert (alone.rounds, alone.converged, alone.reached) == (0, True, 1) and alone.dist[2] == 0 and np.isinf(np.delete(alone.dist, 2)).all()


@pytest.mark.parametrize("name", ["detour", "ties", "chain", "chain2", "square"])
def test_dyadic_lengths_equal_scipy_exactly(name):
    out, graph = _run(name)
    d, _ = _scipy(*graph)
    np.testing.assert_array_equal(out.dist.astype(np.float64), d)


@pytest.mark.parametrize("B, D, k", [(600, 8, 10), (300, 3, 5), (1000, 16, 15)])
def test_gaussian_graphs_against_dijkstra(B, D, k):
    idx, d2 = G.gaussian(B, D, k, seed=B)
    rowptr, col, length = G.distance_graph(idx, d2)
    out = G.geodesic_rows(rowptr, col, length, 0)
    assert out.converged and 3 <= out.rounds <= 40
    np.testing.assert_array_equal(out.dist, G.dijkstra_f32(rowptr, col, length, 0))      # the fixed point, bit for bit
    d, p = _scipy(rowptr, col, length, 0)
    fin = np.isfinite(d)
    np.testing.assert_array_equal(fin, np.isfinite(out.dist))
    # one rounded add per hop on either side: H x 2^-24 relative, H the larger hop count of the two predecessor trees
    H = max(G.hops(out.pred, out.dist).max(), G.hops(np.where(p < 0, -1, p), d).max())
    rel = np.abs(out.dist[fin].astype(np.float64) - d[fin]) / np.maximum(d[fin], np.finfo(np.float64).tiny)
    print(f"B={B}: {out.rounds} rounds, H={H}, max relative distance to scipy {rel.max() / 2.0 ** -24:.3f} x 2^-24")
    assert rel.max() <= H * 2.0 ** -24


def test_distance_graph_is_symmetric_and_sorted():
    idx, d2 = G.gaussian(300, 3, 5, seed=300)
    rowptr, col, length = G.distance_graph(idx, d2)
    n = len(rowptr) - 1
    m = sp.csr_matrix((length, col, rowptr), shape=(n, n))
    assert (m != m.T).nnz == 0 and m.has_sorted_indices and all((np.diff(col[rowptr[v]:rowptr[v + 1]]) > 0).all() for v in range(n))
    listed = {(i, int(j)) for i in range(n) for j in idx[i]}
    assert {(int(r), int(c)) for r, c in zip(*m.nonzero())} == listed | {(j, i) for i, j in listed}
    at = {(i, int(j)): v for i in range(n) for j, v in zip(idx[i], d2[i])}
    row = np.repeat(np.arange(n), np.diff(rowptr))
    want = np.sqrt(np.asarray([at.get((r, c), at.get((c, r))) for r, c in zip(row.tolist(), col.tolist())], F))
    np.testing.assert_array_equal(length.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arc():
    s, idx, d2 = G.arc()
    rowptr, col, length = G.distance_graph(idx, d2)
    return s, idx, (rowptr, col, length), G.geodesic_rows(rowptr, col, length, 0)


def test_arc_orders_the_cells_along_the_curve(arc):
    s, idx, graph, out = arc
    assert out.converged and out.reached == 800
    rho = spearmanr(out.dist, s)[0]
    print(f"arc: {out.rounds} rounds, Spearman {rho:.4f}")
    assert rho > 0.99
    pt = tables.Pseudotime(distance=out.dist, pseudotime=tables._scaled_pseudotime(out.dist), pred=out.pred.astype(np.int64),
                           root=np.array([0]), reached=out.reached, rounds=out.rounds, converged=out.converged, k=8, space="x",
                           metric="euclidean", label=np.zeros(800, np.int64), max_prob=np.ones(800, F), index=range(800),
                           id2label=["t"])
    assert pt.pseudotime.dtype == np.float64 and pt.pseudotime.max() == 1.0 and pt.pseudotime[0] == 0.0
    np.testing.assert_array_equal(pt.hops(), G.hops(out.pred, out.dist))
    far = int(np.argmax(out.dist))
    path = pt.path(far)
    assert path[0] == 0 and path[-1] == far and len(path) == pt.hops()[far] + 1
    assert (out.pred[path[1:]] == path[:-1]).all() and (np.diff(out.dist[path]) > 0).all()
    assert "800 cells ordered by geodesic distance" in str(pt.summary())


def test_pseudotime_table_with_unreached_cells():
    out, _ = _run("detour")
    pt = tables.Pseudotime(distance=out.dist, pseudotime=tables._scaled_pseudotime(out.dist), pred=out.pred.astype(np.int64),
                           root=np.array([0]), reached=5, rounds=4, converged=True, k=2, space="x", metric="euclidean",
                           label=np.array([0, 1, 0, 0, 1, -1]), max_prob=np.ones(6, F), index=list("abcdef"), id2label=["p", "q"])
    np.testing.assert_array_equal(pt.pseudotime, [0, 3 / 3.5, 1 / 3.5, 2 / 3.5, 1, np.nan])
    assert pt.hops().tolist() == [0, 3, 1, 2, 4, -1] and pt.path(4).tolist() == [0, 2, 3, 1, 4] and pt.path(5).tolist() == []
    by = pt.by_type()
    assert by["cell_type"].tolist() == ["p", "q"] and by["n_cells"].tolist() == [3, 2] and by["median"].tolist() == [1 / 3.5, (3 / 3.5 + 1) / 2]
    assert pt.by_group(np.array([1, 1, 0, 0, -1, 0]))["group"].tolist() == [0, 1]
    frame = pt.frame()
    assert list(frame.columns) == ["index", "pseudotime", "distance", "pred", "label", "max_prob"] and frame["label"].tolist()[-1] == "unsure"
    assert pt.pseudotime_frame().to_csv(index=False).splitlines()[-1] == "f,"           # not reached: written empty
    np.testing.assert_array_equal(tables._scaled_pseudotime(np.array([0, inf, 0], F)), [0, np.nan, 0])


# ---------------------------------------------------------------------------------------------------------------------------
def _abstraction(edges, size, names=None, group=None):
    out_edges, expected, conn = tables._paga_connectivities(edges, size)
    return tables.Abstraction(edges=edges, size=size, out_edges=out_edges, connectivities=conn, expected=expected,
                              group_names=names or [str(i) for i in range(len(size))],
                              n_skipped=0 if group is None else int((group < 0).sum()), group=group)


def _same_tables(edges, size):
    mine, theirs = tables._paga_connectivities(edges, size), G.paga(edges, size)
    for a, b in zip(mine, theirs):
        np.testing.assert_array_equal(a, b)
    return mine


def test_paga_on_the_arc(arc):
    s, idx, _, out = arc
    group = np.floor(4 * s).astype(np.int64)
    edges, size = G.group_edges(idx, group, 4)
    assert size.tolist() == np.bincount(group, minlength=4).tolist() and edges.sum() == 800 * 8
    assert (edges[np.abs(np.subtract.outer(np.arange(4), np.arange(4))) > 1] == 0).all() and (np.diag(edges, 1) > 0).all()
    _, _, conn = _same_tables(edges, size)
    np.testing.assert_array_equal(conn, conn.T)
    near = [conn[a, a + 1] for a in range(3)]
    print("arc connectivities", [f"{c:.4f}" for c in near])
    assert all(0.10 <= c <= 0.13 for c in near) and np.count_nonzero(conn) == 6
    ab = _abstraction(edges, size, group=group)
    assert ab.tree().tolist() == [[0, 1, 0, 0], [1, 0, 1, 0], [0, 1, 0, 1], [0, 0, 1, 0]]
    frame = ab.frame()
    assert list(frame.columns) == ["a", "b", "edges", "expected", "connectivity", "in_tree"]
    assert list(zip(frame["a"], frame["b"])) == [("0", "1"), ("1", "2"), ("2", "3")] and frame["in_tree"].all()
    assert frame["edges"].tolist() == [int(edges[a, a + 1] + edges[a + 1, a]) for a in range(3)]
    assert len(ab.frame(min_connectivity=0.2)) == 0
    # oriented by the median pseudotime: reversing time reverses every pair
    d = ab.directed(tables._scaled_pseudotime(out.dist))
    assert list(zip(d["a"], d["b"])) == [("0", "1"), ("1", "2"), ("2", "3")] and (d["median_a"] < d["median_b"]).all()
    back = ab.directed(1.0 - tables._scaled_pseudotime(out.dist))
    assert list(zip(back["a"], back["b"])) == [("1", "0"), ("2", "1"), ("3", "2")]
    xy = np.stack([s, -s], axis=1)
    np.testing.assert_allclose(ab.centroids(xy), np.stack([[s[group == a].mean(), -s[group == a].mean()] for a in range(4)]), rtol=1e-12)
    assert "800 cells in 4 non-empty groups" in str(ab.summary()) and ab.summary()["n_components"] == 1


def test_paga_hand_tables():
    # six cells, k = 2; groups 0 = {0, 1, 2}, 1 = {3, 4}, cell 5 takes no part
    idx = np.array([[1, 2], [0, 2], [1, 3], [4, 2], [3, 5], [4, -1]])
    group = np.array([0, 0, 0, 1, 1, -1])
    edges, size = G.group_edges(idx, group, 2)
    # 0 -> 0: (0,1) (0,2) (1,0) (1,2) (2,1); 0 -> 1: (2,3); 1 -> 1: (3,4) (4,3); 1 -> 0: (3,2); (4,5) and (5,4) touch cell 5
    assert edges.tolist() == [[5, 1], [1, 2]] and size.tolist() == [3, 2]
    es, expected, conn = _same_tables(edges, size)
    # es = [6, 3], n = 5: den = 6 * 2 + 3 * 3 = 21, inter = 2: expected 21 / 4, connectivity 2 * 4 / 21
    assert es.tolist() == [6, 3] and expected[0, 1] == expected[1, 0] == 21 / 4 and conn[0, 1] == conn[1, 0] == 8 / 21
    assert conn[0, 0] == conn[1, 1] == 0 and expected[0, 0] == 0
    ab = _abstraction(edges, size, names=["x", "y"], group=group)
    assert ab.n_skipped == 1 and ab.tree().tolist() == [[0, 1], [1, 0]] and ab.frame()["connectivity"].tolist() == [8 / 21]


def test_paga_caps_at_one_and_keeps_empty_groups():
    # two pairs of cells that only list each other across the groups: every entry is an inter-group one
    idx = np.array([[2], [3], [0], [1]])
    group = np.array([0, 0, 2, 2])                                       # group 1 is empty
    edges, size = G.group_edges(idx, group, 3)
    assert edges.tolist() == [[0, 0, 2], [0, 0, 0], [2, 0, 0]] and size.tolist() == [2, 0, 2]
    es, expected, conn = _same_tables(edges, size)
    # inter (n - 1) = 4 * 3 = 12 >= den = 2 * 2 + 2 * 2 = 8: capped
    assert conn[0, 2] == conn[2, 0] == 1.0 and np.count_nonzero(conn) == 2 and expected[0, 2] == 8 / 3
    ab = _abstraction(edges, size, group=group)
    assert ab.tree().tolist() == [[0, 0, 1], [0, 0, 0], [1, 0, 0]] and ab.summary()["n_groups"] == 2
    assert np.isnan(ab.centroids(np.zeros((4, 2)))[1]).all()
    with pytest.raises(ValueError):
        tables._paga_connectivities(np.zeros((2, 3), np.int64), np.zeros(2, np.int64))
    with pytest.raises(ValueError):
        tables.Abstraction(edges=edges, size=size, out_edges=es, connectivities=conn, expected=expected, group_names=list("abc"),
                           n_skipped=0).centroids(np.zeros((4, 2)))
