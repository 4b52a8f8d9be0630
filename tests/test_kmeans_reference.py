"""The fp64 k-means reference (tests/kmeans_reference.py) itself, without a GPU: its fixtures meet no near-tie - so the GPU tests
may ask for equal labels -, it agrees with scikit-learn's Lloyd from the same seeds, its seeding follows the contract on
duplicate rows; and the host side of the feature: the ``KMeans`` table's methods and the clusters-file layout."""
import numpy as np
import pandas as pd
import pytest

import scdeepsort_amd as sda
from scdeepsort_amd import tables

import kmeans_reference as M
import knn_reference as R


def test_fixtures_are_what_they_claim():
    for D in M.BLOB_DIMS:
        x = M.blobs(D)
        assert x.shape == (197, D) and x.dtype == np.float32 and (x[50] == x[7]).all() and (x[120] == x[7]).all()
        assert (x * 8 == np.round(x * 8)).all() and np.abs(x).max() <= 3.5            # multiples of 1/8: sums and distances exact
        d = R.sq_distances(x, x)
        assert (d.astype(np.float32).astype(np.float64) == d).all()
    for case in M.OVERLAP_CASES:
        assert M.overlap(*case).shape == case[:2]
    assert 0.0 <= M.draw(0, 0) < 1.0 and M.draw(0, 0) != M.draw(0, 1) != M.draw(1, 1)
    assert M.mix64(0) == 0xE220A8397B1DCDAF                                           # splitmix64's first output from state 0


@pytest.mark.parametrize("D", M.BLOB_DIMS)
@pytest.mark.parametrize("K", M.BLOB_KS)
def test_blobs_meet_no_near_tie(D, K):
    for seed in M.blob_seeds(D, K):
        ref = M.reference("blobs", K, seed, D)
        print(f"blobs({D}) K={K} seed={seed}: {ref['n_iter']} iterations, narrowest gap {ref['min_gap']:.3g} near-tie widths")
        assert ref["converged"] and 2 <= ref["n_iter"] <= 11 and ref["min_gap"] >= 1.0
        assert ref["size"].sum() == 197 and len(set(ref["seed_row"].tolist())) == K
        assert np.all(np.diff(ref["inertia_trace"]) <= 0)


@pytest.mark.parametrize("case", M.OVERLAP_CASES)
@pytest.mark.parametrize("K", M.OVERLAP_KS)
def test_overlap_meets_no_near_tie(case, K):
    ref = M.reference("overlap", K, 0, *case)
    print(f"overlap{case} K={K}: {ref['n_iter']} iterations, narrowest gap {ref['min_gap']:.3g} near-tie widths")
    assert ref["converged"] and 2 <= ref["n_iter"] <= 11 and ref["min_gap"] >= 1.0
    assert np.all(np.diff(ref["inertia_trace"]) <= 0)


@pytest.mark.parametrize("name,K,case", [("blobs", 5, (36,)), ("overlap", 6, (300, 20, 0))])
def test_labels_equal_sklearn_from_the_same_seeds(name, K, case):
    cluster = pytest.importorskip("sklearn.cluster")
    x = getattr(M, name)(*case)
    ref = M.reference(name, K, 0, *case)
    sk = cluster.KMeans(n_clusters=K, init=x[ref["seed_row"]].astype(np.float64), n_init=1, algorithm="lloyd", tol=0,
                        max_iter=100).fit(x.astype(np.float64))
    np.testing.assert_array_equal(sk.labels_, ref["label"])
    np.testing.assert_allclose(sk.cluster_centers_, ref["centers"], rtol=1e-6, atol=1e-6)
    assert abs(sk.inertia_ - ref["inertia_trace"][-1]) <= 1e-6 * sk.inertia_


def test_prefix_order_and_the_draw():
    w = np.random.default_rng(4).random(700)
    P, T = M.prefix(w)
    assert (np.diff(P) >= 0).all() and P[-1] == T and abs(T - w.sum()) < 1e-9
    assert P[255] == np.cumsum(w[:256])[-1] and P[256] == P[255] + w[256]          # chunk sums first, then the chunk's own rows
    for u in (0.0, 0.25, 0.999999):
        i = M.pick(w, u)
        assert P[i] > u * T and (i == 0 or P[i - 1] <= u * T)
    w[:] = 0.0
    assert M.pick(w, 0.5) is None
    w[[3, 9]] = 1.0
    assert M.pick(w, 0.0) == 3 and M.pick(w, 0.5) == 9 and M.pick(w, 0.4999) == 3


def test_duplicate_rows_follow_the_zero_total_rule():
    x = M.duplicates()
    for seed in (0, 1, 2):
        rows, min_d2 = M.seed_rows(x, 5, seed)
        first, rest = rows[:3].tolist(), rows[3:].tolist()
        assert sorted(r % 3 for r in first) == [0, 1, 2]                          # the three distinct rows first ...
        assert rest == sorted(set(range(6)) - set(first))[:2]                     # ... then the lowest indices that are no seed yet
        assert (min_d2 == 0).all()
    bad = x.copy()
    bad[1, 2] = np.inf
    rows, min_d2 = M.seed_rows(bad, 5, 0)
    assert 1 not in rows.tolist() and np.isnan(min_d2[1]) and sorted(rows.tolist()) == [0, 2, 3, 4, 5]
    rows, _ = M.seed_rows(bad, 6, 0)
    assert rows[-1] == -1                                                         # nothing left: the wrapper's ValueError


def test_update_restates_the_chunk_order_and_keeps_empty_clusters():
    x = M.overlap(300, 20, 0)
    group = np.random.default_rng(1).integers(-1, 3, 300)
    group[group == 1] = 0                                                         # cluster 1 is empty, 0 spans several chunks
    total, count = M.group_sums(x, group, 3)
    assert count.tolist() == [int((group == 0).sum()), 0, int((group == 2).sum())] and count[0] > 128
    np.testing.assert_allclose(total[0], x[group == 0].astype(np.float64).sum(0), rtol=1e-12)
    start = np.full((3, 20), 7.0, np.float32)
    out = M.update(x, group, start)
    assert (out[1] == 7.0).all() and (out[0] == (total[0] / count[0]).astype(np.float32)).all()


def _table():
    #                cells:  a  b  c  d  e  f  g  h
    cluster = np.array([0, 0, 0, 2, 2, -1, 2, 0], np.int64)
    label = np.array([1, 1, 0, 2, -1, 1, 2, -1], np.int64)
    return tables.KMeans(cluster=cluster, sq_distance=np.arange(8, dtype=np.float32), centers=np.zeros((3, 4), np.float32),
                         size=np.array([4, 0, 3], np.int64), seed_cells=np.array([0, 5, 3], np.int64), inertia=27.0,
                         inertia_trace=[40.0, 27.0], n_iter=2, converged=True, space="hidden", metric="euclidean", label=label,
                         max_prob=np.full(8, 0.5, np.float32), index=list("abcdefgh"), id2label=["T0", "T1", "T2"])


def test_kmeans_table_host_methods():
    assert sda.KMeans is tables.KMeans is sda.api.KMeans and sda.api.KMeansSummary is tables.KMeansSummary
    km = _table()
    assert km.n_clusters == 3 and km.cluster_names == ["c0000", "c0001", "c0002"]
    comp = km.composition()
    assert list(comp.index) == km.cluster_names and list(comp.columns) == ["T0", "T1", "T2", "unsure"]
    assert comp.to_numpy().tolist() == [[1, 2, 0, 1], [0, 0, 0, 0], [0, 0, 2, 1]]
    purity = km.purity()
    assert purity[0] == 2 / 3 and np.isnan(purity[1]) and purity[2] == 1.0
    frame = km.frame()
    assert list(frame.columns) == ["index", "cell_type", "prob", "cluster", "sq_distance", "cluster_size", "cluster_purity"]
    assert frame["cluster"].tolist() == ["c0000", "c0000", "c0000", "c0002", "c0002", None, "c0002", "c0000"]
    assert frame["cell_type"].tolist() == ["T1", "T1", "T0", "T2", "unsure", "T1", "T2", "unsure"]
    assert frame["cluster_size"].tolist() == [4, 4, 4, 3, 3, 0, 3, 4] and np.isnan(frame["cluster_purity"][5])
    s = km.summary()
    assert isinstance(s, tables.KMeansSummary) and s["n_cells"] == 8 and s["n_clusters"] == 3 and s["n_empty"] == 1
    assert s["n_skipped"] == 1 and s["min_size"] == 3 and s["max_size"] == 4 and s["n_mixed"] == 1 and s["n_unsure"] == 2
    assert "8 cells in 3 clusters" in str(s) and "converged after 2" in str(s)
    wide = tables.KMeans(**{**km.__dict__, "size": np.zeros(12345, np.int64)})
    assert wide.cluster_names[-1] == "c12344" and wide.cluster_names[0] == "c00000"
    assert sorted(wide.cluster_names) == wide.cluster_names                       # sorted order is id order


def test_the_clusters_file_layout_is_read_back(tmp_path):
    km = _table()
    km.cluster = np.where(km.cluster < 0, 1, km.cluster)
    out = km.clusters_frame()
    assert list(out.columns) == ["index", "cell", "cluster"]
    path = tmp_path / "mouse_Rand_kmeans.csv"
    sda.api._write_table(out, tmp_path, "mouse", "Rand", "kmeans")
    names = sda.ResidentPredictor._read_clusters_file(path, "data.csv", pd.Index(list("abcdefgh")))
    assert names == [km.cluster_names[k] for k in km.cluster]
    ids, sorted_names = tables._cluster_ids(names)                                # as annotate factorises them: sorted = id order
    assert sorted_names == km.cluster_names and ids.tolist() == km.cluster.tolist()
    with pytest.raises(ValueError, match="cell order"):
        sda.ResidentPredictor._read_clusters_file(path, "data.csv", pd.Index(list("abcdefhg")))
