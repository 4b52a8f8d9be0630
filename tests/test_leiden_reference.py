"""The numpy restatement of ``ops.leiden_graph`` (tests/leiden_reference.py) without a GPU: the two graphs on which Louvain leaves a
disconnected community, the refinement's fallback, the properties that hold on every graph - connected communities, ``ref`` nested
in ``P``, a rising trace, ``Qnum`` kept across the aggregation - and the modularity against the Louvain restatement's."""
import numpy as np
import pytest

import leiden_reference as L
import louvain_reference as R

# undirected edges (i, j, w); the recipe of leiden_reference.recipe_graph reproduces all three
G30 = ((0, 1, 3), (0, 14, 4), (2, 4, 4), (2, 12, 1), (2, 16, 5), (3, 6, 5), (3, 15, 4), (3, 23, 4), (4, 16, 5), (4, 26, 3), (4, 29, 3),
       (5, 17, 2), (5, 29, 3), (6, 7, 2), (6, 13, 1), (7, 24, 3), (7, 26, 2), (8, 22, 4), (8, 28, 2), (9, 11, 2), (9, 22, 1), (9, 25, 5),
       (9, 27, 4), (9, 29, 5), (10, 13, 4), (11, 26, 3), (12, 14, 5), (12, 17, 5), (12, 23, 4), (12, 25, 2), (14, 24, 5), (14, 27, 5),
       (14, 29, 4), (15, 17, 4), (15, 21, 3), (17, 25, 5), (17, 28, 4), (17, 29, 4), (18, 23, 5), (20, 21, 4), (20, 27, 1), (20, 28, 1),
       (26, 27, 5), (28, 29, 5))
G14 = ((1, 2, 1), (1, 5, 4), (2, 4, 3), (2, 5, 2), (5, 9, 4), (5, 10, 4), (5, 11, 4), (6, 10, 4), (6, 11, 4), (7, 9, 2), (7, 13, 3),
       (8, 11, 4), (9, 11, 1))
# recipe_graph(30, 248): at resolution 0.5 the refinement of level 1 discards a sweep for its single best accepted move
FALLBACK = ((0, 2, 2), (0, 4, 5), (0, 15, 4), (0, 19, 2), (0, 22, 2), (0, 26, 2), (0, 28, 1), (1, 8, 5), (1, 15, 2), (1, 22, 4),
            (1, 28, 5), (2, 6, 4), (2, 9, 2), (2, 16, 1), (2, 27, 1), (3, 20, 2), (3, 24, 1), (4, 8, 3), (4, 10, 5), (4, 13, 2),
            (4, 14, 3), (4, 23, 4), (5, 12, 4), (5, 15, 2), (5, 21, 2), (6, 7, 2), (6, 10, 5), (6, 18, 5), (6, 20, 3), (6, 25, 2),
            (6, 27, 4), (6, 29, 5), (7, 9, 1), (7, 22, 1), (8, 14, 1), (8, 20, 3), (8, 29, 4), (9, 20, 1), (9, 26, 1), (9, 27, 1),
            (10, 18, 4), (10, 19, 3), (10, 20, 3), (10, 28, 2), (10, 29, 3), (11, 24, 5), (11, 27, 1), (11, 28, 2), (12, 18, 5),
            (13, 14, 4), (13, 22, 3), (13, 28, 4), (14, 17, 2), (14, 20, 2), (14, 24, 2), (14, 26, 1), (14, 27, 5), (15, 22, 1),
            (15, 25, 3), (16, 27, 1), (16, 28, 4), (17, 29, 3), (18, 19, 1), (18, 22, 3), (18, 27, 5), (19, 24, 1), (19, 29, 1),
            (20, 27, 2), (21, 28, 1), (22, 23, 5), (23, 24, 2), (24, 27, 4), (24, 29, 2), (25, 29, 1))

# Leiden's modularity over the Louvain restatement's on the twelve graphs of test_quality_against_louvain.  The bound is the
# issue's; the lowest ratio its prototype measured was 0.9909.
QUALITY_RATIO = 0.98
QUALITY = [(64, 4, 3, 2.0, 5, "snn"), (300, 6, 5, 2.0, 6, "snn"), (500, 8, 6, 1.0, 5, "unit"), (1000, 8, 1, 0.0, 10, "snn")]


def g30():
    return L.edges_csr(30, G30)


def g14():
    return L.edges_csr(14, G14)


def fallback_graph():
    return L.edges_csr(30, FALLBACK)


def rises(trace):
    return all(b > a for a, b in zip(trace, trace[1:]))


def check_properties(graph, out, states):
    """What holds on every graph: connected communities, ref inside P, a rising trace, Qnum kept from level to level."""
    rowptr, col, _ = graph
    assert L.disconnected(rowptr, col, out.cluster) == 0
    assert rises(out.qnum_trace) and all(type(q) is int for q in out.qnum_trace)
    assert len(out.level_labels) == len(out.levels) + (out.levels[-1]["split"] > 0) and len(out.refined_labels) == len(out.levels)
    for P, ref in zip(out.level_labels, out.refined_labels):            # per original vertex: ref nests in P
        assert len(np.unique(np.stack([ref, P]), axis=1)[0]) == len(np.unique(ref))
        assert L.disconnected(rowptr, col, ref) == 0                    # a refined community is connected
    frac, M = out.resolution, out.M
    for level, state in zip(out.levels, states):
        assert (state["P"][state["ref"]] == state["P"]).all()           # on the level's own vertices, by the founder
        assert level["refined"] == len(np.unique(state["ref"])) >= level["communities"]
    for before, after in zip(states, states[1:]):                       # the next level starts where the moving phase stopped
        assert R.qnum(after["row"], after["col"], after["w"], after["comm0"], after["deg"], M, frac) == \
            R.qnum(before["row"], before["col"], before["w"], before["P"], before["deg"], M, frac)
    assert [level["vertices"] for level in out.levels[1:]] == [level["refined"] for level in out.levels[:-1]]
    assert all(a["vertices"] > b["vertices"] for a, b in zip(out.levels, out.levels[1:]))
    assert out.levels[-1]["refined"] == out.levels[-1]["vertices"]


def test_the_recipe_reproduces_the_committed_graphs():
    for literal, n, seed in ((g30(), 30, 390), (g14(), 14, 339), (fallback_graph(), 30, 248)):
        for mine, theirs in zip(literal, L.recipe_graph(n, seed)):
            np.testing.assert_array_equal(mine, theirs)


def test_g30_louvain_leaves_a_disconnected_community_and_leiden_none():
    graph = g30()
    louvain = R.louvain_graph(*graph, resolution=0.5)
    assert louvain.M == 310 and louvain.modularity == 0.5891987513007284
    assert L.disconnected(graph[0], graph[1], louvain.cluster) == 1
    states = []
    out = L.leiden_graph(*graph, resolution=0.5, states=states)
    assert out.M == 310 and out.qnum_trace[-1] == 116238 and out.modularity == 0.6047762747138398
    assert out.cluster.tolist() == [1, 1, 3, 2, 3, 0, 2, 1, 0, 0, 2, 0, 0, 2, 1, 2, 3, 0, 2, -1, 0, 0, 0, 2, 1, 0, 1, 1, 0, 0]
    assert len(out.levels) == 4 and out.levels[-1]["split"] == 0 and out.converged
    check_properties(graph, out, states)


def test_g14_needs_the_final_cut():
    graph = g14()
    louvain = R.louvain_graph(*graph, resolution=0.5)
    assert louvain.M == 80 and len(set(louvain.cluster[[2, 4, 7, 13]].tolist())) == 1
    assert L.disconnected(graph[0], graph[1], louvain.cluster) == 1
    states = []
    out = L.leiden_graph(*graph, resolution=0.5, states=states)
    assert out.levels[-1]["split"] == 1 and out.qnum_trace[-1] == 7086
    assert out.cluster.tolist() == [-1, 0, 1, -1, 1, 0, 0, 2, 0, 0, 0, 0, -1, 2]
    before, after = out.level_labels[-2], out.level_labels[-1]          # the cut is one more entry, and it only splits
    assert before[2] == before[4] == before[7] == before[13] and after[2] == after[4] != after[7] == after[13]
    check_properties(graph, out, states)


def test_accept_keeps_a_move_only_when_the_founder_of_its_target_stays():
    ref = np.arange(5)
    prop, gain = np.array([0, 0, 1, 3, 3]), np.array([0, 7, 5, 0, 2])
    nxt, kept = L.accept(ref, prop, gain)                               # 2 -> 1 falls because 1 leaves for 0; 4 -> 3 holds
    assert nxt.tolist() == [0, 0, 2, 3, 3] and kept.tolist() == [0, 7, 0, 0, 2]


def test_one_refinement_sweep_on_a_path():
    """0 - 1 - 2 - 3 with unit weights in one community: M = 6, deg = 1 2 2 1, totP = 6.  Sweep 0 lets a vertex look at lower
    ids only: 1, 2 and 3 propose their left neighbour, and only 1 -> 0 holds, because 1 and 2 leave home themselves."""
    rowptr, col, w = L.edges_csr(4, [(0, 1, 1), (1, 2, 1), (2, 3, 1)])
    row, col, w = np.repeat(np.arange(4), np.diff(rowptr)), col.astype(np.int64), w.astype(np.int64)
    P, ref, deg = np.zeros(4, np.int64), np.arange(4), np.array([1, 2, 2, 1])
    ext, kinP = L.boundary(row, col, w, P, ref)
    assert ext.tolist() == kinP.tolist() == [1, 2, 2, 1]
    one = R.resolution_fraction(1)
    prop, gain = L.refine_sweep(row, col, w, P, ref, deg, np.array([6, 0, 0, 0]), deg, np.ones(4, np.int64), ext, kinP, 6, one, 0)
    assert prop.tolist() == [0, 0, 1, 2] and gain.tolist() == [0, 6 - 2 * 1, 6 - 2 * 2, 6 - 1 * 2]
    nxt, kept = L.accept(ref, prop, gain)
    assert nxt.tolist() == [0, 0, 2, 3] and kept.tolist() == [0, 4, 0, 0]
    # a poorly connected vertex does not move: at resolution 3 vertex 3 has 1 * 6 < 3 * 1 * 5
    prop, _ = L.refine_sweep(row, col, w, P, ref, deg, np.array([6, 0, 0, 0]), deg, np.ones(4, np.int64), ext, kinP, 6,
                             R.resolution_fraction(3), 0)
    assert prop[3] == 3


def test_the_refinement_fallback():
    graph = fallback_graph()
    states = []
    out = L.leiden_graph(*graph, resolution=0.5, states=states)
    assert [level["refine_fallback_moves"] for level in out.levels] == [0, 1, 0, 0]
    check_properties(graph, out, states)
    big = L.recipe_graph(80, 180)
    assert sum(level["refine_fallback_moves"] for level in L.leiden_graph(*big, resolution=1.0).levels) == 1


RECIPE = [(n, seed) for n in (10, 14, 20, 30, 45, 60, 80) for seed in range(10)]


@pytest.mark.parametrize("resolution", [0.5, 1, 2])
def test_properties_on_recipe_graphs(resolution):
    for n, seed in RECIPE:                                              # 3 x 70 graphs
        graph = L.recipe_graph(n, seed)
        if graph[2].sum() == 0:
            continue
        states = []
        out = L.leiden_graph(*graph, resolution=resolution, states=states)
        assert out.converged
        check_properties(graph, out, states)
        assert not L.leiden_graph(*graph, resolution=resolution, max_sweeps=1).converged


@pytest.mark.parametrize("weights", ["snn", "unit"])
def test_properties_on_knn_graphs(weights):
    for B, D, n_blobs, spread, k in ((64, 4, 3, 2.0, 5), (300, 6, 5, 2.0, 6), (200, 8, 1, 0.0, 4)):
        graph = R.snn_graph(R.knn_lists(R.blobs(B, D, n_blobs, spread, seed=B), k), weights)
        states = []
        out = L.leiden_graph(*graph, states=states)
        assert out.converged and out.cluster.min() >= 0
        check_properties(graph, out, states)
        stopped = L.leiden_graph(*graph, max_sweeps=1)
        assert not stopped.converged and L.disconnected(graph[0], graph[1], stopped.cluster) == 0


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("B,D,n_blobs,spread,k,weights", QUALITY)
def test_quality_against_louvain(B, D, n_blobs, spread, k, weights, seed):
    graph = R.snn_graph(R.knn_lists(R.blobs(B, D, n_blobs, spread, seed), k), weights)
    leiden, louvain = L.leiden_graph(*graph), R.louvain_graph(*graph)
    print(f"B = {B}, D = {D}, {n_blobs} blobs, spread {spread}, k = {k}, {weights}, seed {seed}: Leiden {leiden.modularity:.4f}, "
          f"Louvain {louvain.modularity:.4f}, ratio {leiden.modularity / louvain.modularity:.4f}; Louvain left "
          f"{L.disconnected(graph[0], graph[1], louvain.cluster)} disconnected communities")
    assert L.disconnected(graph[0], graph[1], leiden.cluster) == 0
    assert leiden.modularity / louvain.modularity >= QUALITY_RATIO


def test_graph_without_an_edge_and_isolated_vertices():
    out = L.leiden_graph(np.zeros(5, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert out.cluster.tolist() == [-1] * 4 and out.M == 0 and out.qnum_trace == [0] and out.levels[0]["split"] == 0
    out = L.leiden_graph(*L.edges_csr(6, [(0, 1, 1), (0, 2, 1), (1, 2, 1), (4, 5, 1)]))
    assert out.cluster.tolist() == [0, 0, 0, -1, 1, 1]
    with pytest.raises(ValueError, match="2\\^62"):
        L.leiden_graph(*L.edges_csr(2, [(0, 1, 2 ** 30)]))
