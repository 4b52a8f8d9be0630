"""The numpy restatement of ``ops.snn_graph`` / ``ops.louvain_graph`` (tests/louvain_reference.py) without a GPU: cases worked out by
hand, ``Qnum`` strictly rising, the fallback fixture, the quality against networkx's Louvain, the resolution and the size guard."""
from fractions import Fraction

import numpy as np
import pytest

import louvain_reference as R

# The restatement's modularity over the LOWEST of five seeded networkx runs, measured on the twelve fixtures of
# test_quality_against_networkx: 1.0000 at the lowest (the separated B = 3000 graphs, both weightings), 1.0121 at the highest.
# Required: the lowest measured ratio minus 0.01 for networkx's seed-to-seed spread (profiles/resident_louvain.md).
QUALITY_RATIO = 1.0000 - 0.01

FALLBACK_SEED = 3       # chosen on the CPU: three discarded sweeps on the second level


def csr_of(n, edges, weights=None):
    """A symmetric CSR from undirected edges."""
    pairs = {}
    for e, (i, j) in enumerate(edges):
        pairs[(i, j)] = pairs[(j, i)] = 1 if weights is None else weights[e]
    keys = sorted(pairs)
    rowptr = np.zeros(n + 1, np.int64)
    for i, _ in keys:
        rowptr[i + 1] += 1
    return np.cumsum(rowptr), np.array([j for _, j in keys], np.int32), np.array([pairs[k] for k in keys], np.int32)


def clique(ids):
    return [(a, b) for x, a in enumerate(ids) for b in ids[x + 1:]]


def fallback_points(seed=FALLBACK_SEED):
    """130 cells in 4 dimensions: 3 Gaussian blobs of unit spread, centres drawn at unit scale."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(3, 4))
    return (centres[rng.integers(0, 3, 130)] + rng.normal(size=(130, 4))).astype(np.float32)


def fallback_graph():
    return R.snn_graph(R.knn_lists(fallback_points(), 5), "unit")


def rises(trace):
    return all(b > a for a, b in zip(trace, trace[1:]))


def partition(cluster):
    return sorted(sorted(np.flatnonzero(cluster == c).tolist()) for c in set(cluster.tolist()))


def test_two_cliques_joined_by_one_edge():
    rowptr, col, w = csr_of(8, clique([0, 1, 2, 3]) + clique([4, 5, 6, 7]) + [(3, 4)])
    out = R.louvain_graph(rowptr, col, w)
    assert partition(out.cluster) == [[0, 1, 2, 3], [4, 5, 6, 7]]
    # by hand: 13 undirected edges, M = 26; inside = 2 * 12 = 24 stored entries; each side's tot = 3 + 3 + 3 + 4 = 13
    assert out.M == 26 and out.qnum_trace[-1] == 1 * 26 * 24 - 1 * (13 * 13 + 13 * 13) == 286
    assert out.modularity == 286 / (26 * 26)
    # the start: singletons, IN = 0, the degrees are 3, 3, 3, 4, 4, 3, 3, 3
    assert out.qnum_trace[0] == -(6 * 9 + 2 * 16) and rises(out.qnum_trace) and out.converged
    assert out.level_labels[-1].tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and out.cluster.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]


def test_ring_of_six_triangles():
    edges = []
    for t in range(6):
        edges += clique([3 * t, 3 * t + 1, 3 * t + 2]) + [(3 * t + 2, (3 * t + 3) % 18)]
    out = R.louvain_graph(*csr_of(18, edges))
    # every triangle ends up whole; with 24 edges (M = 48) pairs of triangles may still merge, single vertices never stay alone
    for t in range(6):
        assert len(set(out.cluster[3 * t:3 * t + 3].tolist())) == 1
    assert rises(out.qnum_trace) and out.levels[0]["vertices"] == 18
    # level 0 alone finds the six triangles: Qnum = 48 * 36 - 6 * 8^2 = 1344
    assert sorted(np.bincount(out.level_labels[0]).tolist()) == [3] * 6
    assert 1344 in out.qnum_trace and out.qnum_trace[-1] >= 1344


def test_one_sweep_on_a_path_shows_the_gate_and_the_singleton_rule():
    rowptr, col, w = csr_of(5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    row = np.repeat(np.arange(5), np.diff(rowptr))
    col = col.astype(np.int64)
    deg = np.array([1, 2, 2, 2, 1], np.int64)
    comm, size = np.arange(5, dtype=np.int64), np.ones(5, np.int64)
    one = Fraction(1)
    # M = 8; a singleton's own score is 0 - deg * (deg - deg) = 0, its neighbour's 1 * M - deg[v] * deg[u].
    # t = 0: only lower ids are admissible - every vertex but 0 joins its left neighbour
    nxt, gain = R.sweep(row, col, w, comm, deg, deg.copy(), size, 8, one, 0)
    assert nxt.tolist() == [0, 0, 1, 2, 3]
    assert gain.tolist() == [0, 8 - 2 * 1, 8 - 2 * 2, 8 - 2 * 2, 8 - 1 * 2]
    # t = 1: only higher ids would be admissible, but two singletons never merge upwards: nobody moves
    nxt, gain = R.sweep(row, col, w, comm, deg, deg.copy(), size, 8, one, 1)
    assert nxt.tolist() == [0, 1, 2, 3, 4] and not gain.any()
    # ... while a singleton may move up into a community of two: with 3 and 4 a pair (id 4, tot 3), 2 joins it and nobody else moves
    comm = np.array([0, 1, 2, 4, 4], np.int64)
    tot, size = np.array([1, 2, 2, 0, 3], np.int64), np.array([1, 1, 1, 0, 2], np.int64)
    nxt, gain = R.sweep(row, col, w, comm, deg, tot, size, 8, one, 1)
    assert nxt.tolist() == [0, 1, 4, 4, 4] and gain.tolist() == [0, 0, 8 - 2 * 3, 0, 0]


def test_snn_weights_of_six_cells_are_set_intersections():
    idx = np.array([[1, 2], [0, 2], [0, 1], [2, 4], [3, 5], [4, -1]], np.int64)
    rowptr, col, w = R.snn_graph(idx)
    plus = [set(r[r >= 0].tolist()) | {i} for i, r in enumerate(idx)]
    dense = np.zeros((6, 6), np.int64)
    for i in range(6):
        for j in range(6):
            if i != j and (j in idx[i] or i in idx[j]):
                dense[i, j] = len(plus[i] & plus[j])
    got = np.zeros((6, 6), np.int64)
    got[np.repeat(np.arange(6), np.diff(rowptr)), col] = w
    np.testing.assert_array_equal(got, dense)
    assert dense[0, 1] == 3 and dense[2, 3] == 1 and dense[3, 4] == 2 and dense[4, 5] == 2 and (got == got.T).all()
    assert all((np.diff(col[rowptr[i]:rowptr[i + 1]]) > 0).all() for i in range(6))
    unit = R.snn_graph(idx, "unit")
    np.testing.assert_array_equal(unit[1], col)
    assert (unit[2] == 1).all() and w.min() >= 1 and w.max() <= 3


def test_fallback_fixture_discards_sweeps():
    out = R.louvain_graph(*fallback_graph())
    assert sum(level["fallback_moves"] for level in out.levels) >= 1
    assert out.levels[1]["fallback_moves"] == 3
    assert rises(out.qnum_trace) and out.converged


QUALITY = [(B, k, spread, weights) for B, k in ((64, 4), (300, 5), (3000, 15)) for spread in (4.0, 0.0) for weights in ("snn", "unit")]


def quality_graph(B, k, spread, weights):
    return R.snn_graph(R.knn_lists(R.blobs(B, 8, 5, spread, seed=B), k), weights)


@pytest.mark.parametrize("B,k,spread,weights", QUALITY)
def test_quality_against_networkx(B, k, spread, weights):
    import networkx as nx
    rowptr, col, w = quality_graph(B, k, spread, weights)
    out = R.louvain_graph(rowptr, col, w)
    assert rises(out.qnum_trace) and out.converged
    g = nx.Graph()
    g.add_nodes_from(range(B))
    row = np.repeat(np.arange(B), np.diff(rowptr))
    g.add_weighted_edges_from((int(i), int(j), int(x)) for i, j, x in zip(row, col, w) if i < j)
    lowest = min(nx.community.modularity(g, nx.community.louvain_communities(g, weight="weight", seed=seed), weight="weight")
                 for seed in range(5))
    # the integer modularity is networkx's: the same partition scores the same
    parts = [set(np.flatnonzero(out.cluster == c).tolist()) for c in range(int(out.cluster.max()) + 1)]
    assert abs(nx.community.modularity(g, parts, weight="weight") - out.modularity) < 1e-12
    print(f"B = {B}, k = {k}, spread {spread}, {weights}: Q = {out.modularity:.4f}, networkx's lowest {lowest:.4f}, "
          f"ratio {out.modularity / lowest:.4f}")
    assert out.modularity / lowest >= QUALITY_RATIO


def test_resolution():
    rowptr, col, w = quality_graph(300, 5, 4.0, "snn")
    n = {r: int(R.louvain_graph(rowptr, col, w, resolution=r).cluster.max()) + 1 for r in (0.5, 1, 2)}
    assert n[0.5] <= n[1] <= n[2] and n[0.5] < n[2]
    assert R.resolution_fraction(0.8) == Fraction(4, 5) and R.louvain_graph(rowptr, col, w, resolution=0.8).resolution == Fraction(4, 5)
    assert R.resolution_fraction(1.0) == 1 and R.resolution_fraction(Fraction(1, 3)) == Fraction(1, 3)
    for bad in (0, -1.0, 1e-9):
        with pytest.raises(ValueError):
            R.resolution_fraction(bad)


def test_guard():
    # one edge of weight W stored twice: M = 2 W.  M^2 = 2^62 at W = 2^30: refused; just below it runs
    for res, W, ok in ((1, 2 ** 30, False), (1, 2 ** 30 - 1, True), (2, 2 ** 30 - 1, False), (Fraction(1, 4), 2 ** 29, False),
                       (Fraction(1, 4), 2 ** 29 - 1, True)):
        rowptr, col, w = csr_of(2, [(0, 1)], [W])
        M, frac = 2 * W, R.resolution_fraction(res)
        assert (M * M * max(frac.numerator, frac.denominator) < 2 ** 62) == ok
        if ok:
            assert R.louvain_graph(rowptr, col, w.astype(np.int64), resolution=res).cluster.tolist() == [0, 0]
        else:
            with pytest.raises(ValueError, match="2\\^62"):
                R.louvain_graph(rowptr, col, w.astype(np.int64), resolution=res)


def test_graph_without_an_edge_and_isolated_vertices():
    out = R.louvain_graph(np.zeros(5, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert out.cluster.tolist() == [-1] * 4 and out.M == 0 and out.qnum_trace == [0]
    rowptr, col, w = csr_of(6, clique([0, 1, 2]) + [(4, 5)])
    out = R.louvain_graph(rowptr, col, w)
    assert out.cluster.tolist() == [0, 0, 0, -1, 1, 1]
