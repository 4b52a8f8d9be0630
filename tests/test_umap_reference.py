"""The numpy restatement of the fuzzy graph and the synchronous layout (tests/umap_reference.py) on its own, without a GPU: cases
worked by hand, the bisection's residual, the vectorised epoch against a plain scalar loop over vertices, lanes and edges, and the
quality of the whole scheme on scikit-learn's digits against t-SNE and a plain PCA."""
import math

import numpy as np
import pytest

import umap_reference as R

F = np.float32


def test_a_row_of_equal_distances_has_members_one_and_sigma_at_its_floor():
    idx = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])
    d2 = np.array([[4, 4, 4], [0, 0, 0], [0, 9, 9], [1, 4, np.inf]], F)
    out = R.fuzzy_rows(idx, d2)
    assert out.rho.tolist() == [2.0, 0.0, 3.0, 1.0]
    assert out.member[:3].tolist() == [[1, 1, 1]] * 3 and out.constant.tolist() == [True, True, True, False]
    # p = 3 > log2(4) at every s: s halves 64 times and the floor, 1e-3 of the row's mean distance, takes over
    # (row 1, one point four times: the mean is 0 and 2^-64 stays)
    assert out.sigma[0] == 1e-3 * 2.0 and out.sigma[1] == 2.0 ** -64 and out.sigma[2] == 1e-3 * (6.0 / 3.0)
    assert out.floored.tolist() == [True, False, True, False]
    # row 3 lists two: p(s) = 1 + exp(-1 / s) = log2(4) = 2 has no solution below infinity - s doubles 64 times
    assert out.sigma[3] == 2.0 ** 64 and not out.floored[3]
    assert out.member[3].tolist() == [1.0, float(F(math.exp(-(2.0 ** -64)))), 0.0]


def test_k_equal_to_one():
    out = R.fuzzy_rows(np.array([[1], [0], [-1], [0]]), np.array([[9], [0], [np.inf], [np.nan]], F))
    assert out.rho.tolist() == [3.0, 0.0, 0.0, 0.0] and out.member.reshape(-1).tolist() == [1.0, 1.0, 0.0, 0.0]
    assert out.sigma.tolist() == [2.0 ** 64, 2.0 ** 64, 0.0, 0.0]      # p = 1 = log2(2) is never above the target: s doubles


def test_a_five_vertex_union_worked_by_hand():
    idx = np.array([[1, 2], [0, 2], [0, -1], [4, -1], [-1, -1]])
    member = np.array([[1, .5], [1, .25], [.5, 0], [1, 0], [0, 0]], F)
    rowptr, col, _ = R.snn_graph(idx, "unit")
    assert rowptr.tolist() == [0, 2, 4, 6, 7, 8] and col.tolist() == [1, 2, 0, 2, 0, 1, 4, 3]
    # 0-1: 1 + 1 - 1;  0-2: .5 + .5 - .25;  1-2: .25 + 0 - 0 (2 does not list 1);  3-4: 1 + 0 - 0
    assert R.fuzzy_union(idx, member, rowptr, col).tolist() == [1, .75, 1, .25, .75, .25, 1, 1]


def test_one_epoch_of_a_three_vertex_path_worked_by_hand():
    rowptr, col, w = R.csr_of(3, [(0, 1), (1, 2)], [1.0, 0.5])
    y = np.array([[0, 0], [1, 0], [1, 2]], F)
    # epoch 0 of 2: floor(1 * 1) != floor(0) - edge 0-1 fires; floor(1 * .5) == floor(0) - edge 1-2 does not
    out, fired = R.layout_epoch(rowptr, col, w, 1.0, y, 0, 2, a=1, b=1, gamma=1, alpha=0.5, n_neg=0, seed=0)
    assert fired.tolist() == [1, 1, 0]
    # vertex 0: dx = (-1, 0), q = 1, c = (-2 * 1 / 1) / (1 + 1) = -1, g = (1, 0);  vertex 1: the mirror image
    assert out.tolist() == [[0.5, 0], [0.5, 0], [1, 2]]
    # epoch 1: both fire (floor(2 * .5) = 1 != 0).  Vertex 1: g = (-1, 0) from 0, then from 2 dx = (0, -2), q = 4,
    # c = (-2 * 4 / 4) / (1 + 4) = -2 / 5, g = (0, 4 / 5);  vertex 2: g = (0, -4 / 5)
    out, fired = R.layout_epoch(rowptr, col, w, 1.0, y, 1, 2, a=1, b=1, gamma=1, alpha=0.5, n_neg=0, seed=0)
    up = (F(-2) / F(5)) * F(-2)
    assert fired.tolist() == [1, 2, 1]
    assert out.tolist() == [[0.5, 0], [0.5, float(F(0.5) * up)], [1, float(F(2) + F(0.5) * -up)]]
    # one negative per firing edge pushes away from the drawn vertex, and a far pull is small: nothing moves more than 4 alpha a term
    out, _ = R.layout_epoch(rowptr, col, w, 1.0, y * F(1e-3), 1, 2, a=1, b=1, gamma=1, alpha=1.0, n_neg=3, seed=0)
    assert np.isfinite(out).all() and np.abs(out - y * F(1e-3)).max() <= 4.0 * 8


def _slow_epoch(rowptr, col, w, wmax, y, epoch, n_epochs, a, b, gamma, alpha, n_neg, seed):
    """wgnn_layout_epoch as the header words it: a loop over vertices, their sixteen lanes, each lane's edges and terms."""
    a, b, gamma, alpha, wmax = F(a), F(b), F(gamma), F(alpha), F(wmax)
    n = len(rowptr) - 1
    out = np.array(y, F)
    key = R.epoch_key(seed, epoch)

    def clamp(v):
        return F(-4) if v < F(-4) else (F(4) if v > F(4) else v)

    for i in range(n):
        e0, e1 = int(rowptr[i]), int(rowptr[i + 1])
        if e0 == e1:
            continue
        partial = [[F(0), F(0)] for _ in range(R.LANES)]
        for lane in range(R.LANES):
            g = partial[lane]
            for e in range(e0 + lane, e1, R.LANES):
                r = F(w[e]) / wmax
                if np.floor(F(epoch + 1) * r) == np.floor(F(epoch) * r):
                    continue
                others = [(int(col[e]), True)]
                for s in range(n_neg):
                    h = int(R.mix64(np.array([(int(key) + e * n_neg + s) % 2 ** 64], np.uint64))[0])
                    others.append((((h >> 32) * n) >> 32, False))
                for t, pull in others:
                    if not pull and t == i:
                        continue
                    dx = [y[i][0] - y[t][0], y[i][1] - y[t][1]]
                    q = dx[0] * dx[0] + dx[1] * dx[1]
                    if not q > 0:
                        continue
                    qb = q if b == F(1) else F(np.power(np.float64(q), np.float64(b)))
                    c = (((F(-2) * a) * b) * qb / q) / (F(1) + a * qb) if pull else \
                        ((F(2) * gamma) * b) / ((F(0.001) + q) * (F(1) + a * qb))
                    g[0], g[1] = g[0] + clamp(c * dx[0]), g[1] + clamp(c * dx[1])
        width = R.LANES
        while width > 1:
            width //= 2
            for lane in range(width):
                partial[lane] = [partial[lane][0] + partial[lane + width][0], partial[lane][1] + partial[lane + width][1]]
        out[i] = [y[i][0] + alpha * partial[0][0], y[i][1] + alpha * partial[0][1]]
    return out


@pytest.mark.parametrize("b", [1.0, 0.895])
def test_the_vectorised_epoch_is_the_scalar_loop(b):
    for graph, seed in ((R.star_graph(60), 1), (R.blob_graph(40, 4, seed=2)[:3], 7)):
        rowptr, col, w = graph
        y = R.layout_init(len(rowptr) - 1, seed)
        for epoch in (0, 3):
            args = (rowptr, col, w, w.max(), y, epoch, 10, 1.577, b, 1.0, 0.7, 3, seed)
            fast, _ = R.layout_epoch(*args)
            assert fast.dtype == F and np.array_equal(fast, _slow_epoch(*args))
            assert not np.array_equal(fast, y)
            y = fast


def test_hash_init_and_draws():
    y = R.layout_init(1000, 5)
    assert y.dtype == F and y.shape == (1000, 2) and y.min() >= -10 and y.max() < 10 and abs(float(y.mean())) < 0.5
    assert np.array_equal(y, R.layout_init(1000, 5)) and not np.array_equal(y, R.layout_init(1000, 6))
    assert int(R.mix64(np.array([0], np.uint64))[0]) == 0xE220A8397B1DCDAF          # splitmix64's first output for seed 0


def test_the_bisection_meets_its_target_on_unfloored_rows():
    for k in (3, 15, 64):
        idx, d2 = R.ragged_lists(70, k)
        rows = R.fuzzy_rows(idx, d2)
        res = R.fuzzy_residual(idx, d2, rows.rho, rows.sigma)
        free = ~rows.floored & ~rows.constant & np.isfinite(res) & (rows.sigma < 2.0 ** 60)
        assert free.sum() >= 50 and res[free].max() <= 1e-9
        assert rows.member.dtype == F and rows.member.max() <= 1 and rows.member.min() >= 0
        assert (rows.member[11] == 0).all() and rows.sigma[11] == 0 and (rows.member[5] == 1).all()
        graph = R.fuzzy_graph(idx, d2)
        row = np.repeat(np.arange(70), np.diff(graph.rowptr))
        back = {(int(r), int(c)): v for r, c, v in zip(row, graph.col, graph.w)}
        assert all(back[(c, r)] == v for (r, c), v in back.items()) and 0 <= graph.w.min() and graph.w.max() <= 1


def test_two_runs_agree_and_every_argument_matters():
    graph = R.blob_graph(40, 4, seed=2)[:3]
    base = R.layout_graph(*graph, n_epochs=12, b=1.0)
    assert np.array_equal(base.y, R.layout_graph(*graph, n_epochs=12, b=1.0).y) and base.n_fired > 0
    for other in (dict(seed=1), dict(n_neg=0), dict(a=1.0), dict(gamma=2.0), dict(lr=0.5), dict(n_epochs=13), dict(b=0.895)):
        assert not np.array_equal(base.y, R.layout_graph(*graph, **{**dict(n_epochs=12, b=1.0), **other}).y), other
    assert R.layout_epochs(9999) == 500 and R.layout_epochs(10000) == 200


def test_digits_layout_quality():
    """The scheme on scikit-learn's digits (1797 x 64, k = 15, 200 epochs, PCA init) in trustworthiness(n_neighbors=15): within 0.01
    of ``TSNE(2, random_state=0)`` and 0.10 above a plain two-component PCA, both run here on the same rows.  Measured:
    the layout 0.9851, t-SNE 0.9905, PCA 0.8288 (profiles/resident_umap.md)."""
    from sklearn.datasets import load_digits
    from sklearn.manifold import TSNE, trustworthiness
    x = load_digits().data.astype(np.float64)
    graph = R.fuzzy_graph(*R.knn(x, 15))
    init = R.pca_init(x)
    out = R.layout_graph(graph.rowptr, graph.col, graph.w, init, n_epochs=200)
    assert np.isfinite(out.y).all() and np.abs(out.y).max() < 50
    ours = trustworthiness(x, out.y, n_neighbors=15)
    tsne = trustworthiness(x, TSNE(2, random_state=0).fit_transform(x), n_neighbors=15)
    pca = trustworthiness(x, init, n_neighbors=15)
    print(f"trustworthiness: layout {ours:.4f}, t-SNE {tsne:.4f}, PCA-2 {pca:.4f}")
    assert ours >= tsne - 0.01 and ours >= pca + 0.10
