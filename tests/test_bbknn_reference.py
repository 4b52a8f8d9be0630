"""The fp64 restatement behind the batch-balanced kNN tests (tests/bbknn_reference.py) checked on its own, without a GPU: against
``knn_reference`` and scikit-learn, on fixtures whose ties and short lists are counted here, so that the GPU tests compare the
kernel with something that has itself been compared - and ``NeighborGraph.lisi`` (host numpy) against its loop restatements."""
import numpy as np
import pytest

import scdeepsort_amd as sda

import bbknn_reference as BR
import knn_reference as R


def test_one_segment_is_the_plain_search():
    x = R.lattice(36)
    for k in (1, 15, 64):
        idx, d2, m_idx, m_d2 = BR.segments(x, np.zeros(x.shape[0], np.int64), 1, k)
        want = R.reference("lattice", k, 36)
        np.testing.assert_array_equal(idx[:, 0], want[0]); np.testing.assert_array_equal(d2[:, 0], want[1])
        np.testing.assert_array_equal(m_idx, want[0]); np.testing.assert_array_equal(m_d2, want[1])


def test_lattice_exercises_the_tie_rule_within_and_across_segments():
    group, idx, d2, m_idx, m_d2 = BR.reference("lattice", 3, 3, 36)
    assert (idx >= 0).all() and np.isfinite(d2).all()                              # no list is short
    assert m_idx[7, :2].tolist() == [50, 120] and m_d2[7, :2].tolist() == [0.0, 0.0]
    assert len({group[7], group[50], group[120]}) == 3                             # the copies sit in three different batches
    tie = m_d2[:, 1:] == m_d2[:, :-1]
    across = tie & (group[m_idx[:, 1:]] != group[m_idx[:, :-1]])
    assert int(across.sum()) == 52 and int(across.any(axis=1).sum()) == 33         # adjacent exact ties ACROSS segments
    assert (m_idx[:, 1:][tie] > m_idx[:, :-1][tie]).all()                          # ... go to the lower row id
    within = d2[:, :, 1:] == d2[:, :, :-1]
    assert int(within.sum()) == 3 and (idx[:, :, 1:][within] > idx[:, :, :-1][within]).all()
    # a merged row is its blocked row re-ordered: the same entries, ascending
    assert (np.sort(m_idx, axis=1) == np.sort(idx.reshape(len(idx), -1), axis=1)).all() and (np.diff(m_d2, axis=1) >= 0).all()
    for s in range(3):                                                             # a block lists its own segment, never the query
        assert (group[idx[:, s]] == s).all() and (idx[:, s] != np.arange(len(idx))[:, None]).all()


def test_uneven_segments_leave_the_tails_they_must():
    group, idx, d2, m_idx, m_d2 = BR.reference("uneven", len(BR.UNEVEN_SIZES), 4, 36)
    assert np.bincount(group, minlength=5).tolist() == list(BR.UNEVEN_SIZES)
    assert (np.diff(np.flatnonzero(group == 4)) > 1).any()                         # interleaved: `order` is a real permutation
    empty = (idx < 0).sum(axis=(0, 2))
    assert empty.tolist() == [592, 788, 0, 0, 0]                                   # the one-cell segment, the empty one
    assert (np.isposinf(d2) == (idx < 0)).all()
    n_none = (m_idx < 0).sum(axis=1)
    for i in range(len(m_idx)):                                                    # the -1 entries are last
        assert (m_idx[i, :20 - n_none[i]] >= 0).all() and (m_idx[i, 20 - n_none[i]:] == -1).all()


@pytest.mark.parametrize("case", R.REAL_CASES)
def test_real_rows_agree_with_scikit_learn_per_batch(case):
    from sklearn.neighbors import NearestNeighbors
    x = R.real(*case)
    N, S, k = x.shape[0], 4, 3
    group, idx, d2, m_idx, m_d2 = BR.reference("real", S, k, *case)
    agree = 0
    for s in range(S):
        members = np.flatnonzero(group == s)
        _, found = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(x[members].astype(np.float64)).kneighbors(x.astype(np.float64))
        for i in range(N):
            agree += [members[j] for j in found[i] if members[j] != i][:k] == idx[i, s].tolist()
    near = BR.near_ties(x, group, S, k)
    print(f"{case}: {agree} of {N * S} (cell, batch) lists equal scikit-learn's; {int(near.sum())} of {near.size} near-tie positions")
    assert agree == N * S
    assert near.sum() <= 0.0014 * near.size                                        # what the GPU test may excuse at the most


def _graph(indices, sq_distances, label, metric="euclidean"):
    B = len(indices)
    return sda.NeighborGraph(indices=np.asarray(indices, np.int64), sq_distances=np.asarray(sq_distances, np.float32),
                             k=np.asarray(indices).shape[1], space="hidden", metric=metric, label=np.asarray(label, np.int64),
                             max_prob=np.ones(B, np.float32), index=list(range(B)), id2label=[str(i) for i in range(8)])


def test_lisi_on_lists_whose_answer_is_known():
    B, k = 12, 6
    idx = np.stack([np.delete(np.arange(B), i)[:k] for i in range(B)])
    same = _graph(idx, np.full((B, k), 2.5), np.zeros(B, np.int64))
    # three labels, each twice in every list, at equal distances
    labels = np.zeros(B, np.int64)
    lists = np.tile(np.arange(6), (B, 1)); labels[:6] = [0, 0, 1, 1, 2, 2]
    even = _graph(lists, np.full((B, k), 2.5), labels)
    assert (even.lisi(labels) == 3.0).all()
    assert np.abs(same.lisi(np.zeros(B, np.int64)) - 1.0).max() <= 1e-12           # a single label
    assert np.abs(same.lisi("predicted") - 1.0).max() <= 1e-12
    # a short list of one neighbour, and none: NaN; an unsure neighbour raises the index, a cell with unsure neighbours alone: NaN
    idx2, d = idx.copy(), np.full((B, k), 2.5, np.float32)
    idx2[0, 1:], d[0, 1:] = -1, np.inf
    idx2[1, :], d[1, :] = -1, np.inf
    got = _graph(idx2, d, np.zeros(B, np.int64)).lisi(np.zeros(B, np.int64))
    assert np.isnan(got[:2]).all() and np.abs(got[2:] - 1.0).max() <= 1e-12
    unsure = np.zeros(B, np.int64); unsure[3] = -1
    got = same.lisi(unsure)
    assert (got[idx.__eq__(3).any(axis=1)] > 1.0 + 1e-6).all() and np.isnan(same.lisi(np.full(B, -1))).all()
    for bad in (dict(perplexity=0.5), dict(perplexity=6), dict(perplexity=float("nan")), dict(n_labels=0)):
        with pytest.raises(ValueError):
            same.lisi(np.zeros(B, np.int64), **bad)
    for bad in (np.zeros(B - 1, np.int64), np.zeros(B), np.full(B, -2), "batch"):
        with pytest.raises(ValueError):
            same.lisi(bad)


@pytest.mark.parametrize("case", R.REAL_CASES)
def test_lisi_equals_its_loop_restatement_bit_for_bit(case):
    """The largest relative gap between 64 tries without an exit (``NeighborGraph.lisi``) and the published search (50 tries,
    exit at 1e-5 in the entropy) measured on these fixtures: 6.8e-06 (k = 15, perplexity 5, four random labels; 6.5e-06, 6.0e-06
    and 6.8e-06 per case).  The exit leaves the entropy within 1e-5 of log(perplexity) and d log(LISI) / dH is of order one on
    such lists, which is the size of the gap; the assertion is a tenfold margin over the measured one."""
    x = R.real(*case)
    N, k, L = x.shape[0], 15, 4
    idx, d2 = R.reference("real", k, *case)
    labels = BR.random_groups(N, L, case[2]).copy()
    graph = _graph(idx, d2, labels)
    got = graph.lisi(labels)
    assert got.dtype == np.float64 and got.shape == (N,) and (got >= 1.0).all() and (got <= L).all()
    want = BR.lisi(idx, graph.distances(), labels, k / 3, L)
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    published = BR.lisi_published(idx, graph.distances(), labels, k / 3, L)
    gap = np.abs(got - published) / published
    print(f"{case}: largest relative gap to the tolerance-exit search {gap.max():.2e}")
    assert gap.max() <= 6.8e-5
    # an unsure label among them, another perplexity, the cosine reading of the distances: still the loop's bits
    labels[::7] = -1
    cos = _graph(idx, d2 / d2.max() * 2, labels, metric="cosine")
    for g, p in ((graph, 2.0), (cos, k / 3)):
        np.testing.assert_array_equal(g.lisi(labels, perplexity=p, n_labels=L).view(np.uint64),
                                      BR.lisi(idx, g.distances(), labels, p, L).view(np.uint64))


def test_batch_graph_is_a_neighbor_graph_with_batch_tables():
    case = R.REAL_CASES[2]
    N, S, kw = case[0], 4, 3
    group, idx, d2, m_idx, m_d2 = BR.reference("real", S, kw, *case)
    bg = sda.BatchGraph(indices=m_idx, sq_distances=m_d2.astype(np.float32), k=S * kw, space="hidden", metric="euclidean",
                        label=np.zeros(N, np.int64), max_prob=np.ones(N, np.float32), index=list(range(N)), id2label=["a"],
                        batch=group, batch_names=list("wxyz"), k_within=kw, by_batch_indices=idx,
                        by_batch_sq_distances=d2.astype(np.float32))
    assert isinstance(bg, sda.NeighborGraph)
    assert (bg.batch_share() == (S - 1) / S).all()                                 # all lists are full
    table = bg.by_batch()
    assert table["batch"].tolist() == list("wxyz") and table["n_cells"].tolist() == np.bincount(group).tolist()
    assert (table["n_short"] == 0).all() and list(table.columns[3:]) == [f"nearest_{c}" for c in "wxyz"]
    want = np.median(np.sqrt(d2[group == 1, 2, 0].astype(np.float32)).astype(np.float64))
    assert table["nearest_y"][1] == want
    s = bg.summary()
    assert s["batch_sizes"] == dict(zip("wxyz", np.bincount(group).tolist())) and s["n_batches"] == S and s["n_short"] == 0
    assert "4 batches" in str(s) and f"{N} cells" in str(s) and s["median_batch_share"] == 0.75
    np.testing.assert_array_equal(bg.lisi("batch"), bg.lisi(group))
    # a short list: the share is over what is listed
    short = BR.reference("uneven", 5, 4, 36)
    bg = sda.BatchGraph(indices=short[3], sq_distances=short[4].astype(np.float32), k=20, space="hidden", metric="euclidean",
                        label=np.zeros(197, np.int64), max_prob=np.ones(197, np.float32), index=list(range(197)), id2label=["a"],
                        batch=short[0], batch_names=[str(i) for i in range(5)], k_within=4, by_batch_indices=short[1],
                        by_batch_sq_distances=short[2].astype(np.float32))
    listed = short[3] >= 0
    other = (short[0][np.where(listed, short[3], 0)] != short[0][:, None]) & listed
    np.testing.assert_array_equal(bg.batch_share(), other.sum(1) / listed.sum(1))
    table = bg.by_batch()
    assert table["n_short"].tolist() == list(BR.UNEVEN_SIZES) and np.isnan(table["nearest_1"]).all()
    assert np.isnan(table["nearest_0"][0]) and bg.summary()["n_short"] == 197
