"""The numpy restatement of ``wgnn_silhouette_rows`` (tests/silhouette_reference.py) against ``sklearn.metrics.silhouette_samples``
on float64 copies of the fixtures, within the stated bound, and the conventions the kernel shares with it."""
import numpy as np
import pytest

import kmeans_reference as M
import knn_reference as R
import silhouette_reference as S

from sklearn.metrics import silhouette_samples


def _sklearn(x, group, K):
    """scikit-learn's scores of the participating rows (NaN elsewhere), on a float64 copy."""
    on = S.participants(x, group, K)
    out = np.full(x.shape[0], np.nan)
    out[on] = silhouette_samples(np.asarray(x, np.float64)[on], np.asarray(group)[on])
    return out


CASES = [("lattice", D) for D in R.LATTICE_DIMS] + [("blobs", D) for D in M.BLOB_DIMS] + \
        [("overlap",) + c for c in M.OVERLAP_CASES] + [("real",) + c for c in R.REAL_CASES]


def _case(name, *case):
    if name == "lattice":
        return R.lattice(*case), S.lattice_groups(), 7, True
    if name == "blobs":
        return M.blobs(*case), M.reference("blobs", 5, 0, *case)["label"], 5, True
    x = (M.overlap if name == "overlap" else R.real)(*case)
    return x, S.real_groups(x.shape[0]), 4, False


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_restatement_equals_scikit_learn_within_the_bound(case):
    x, g, K, exact_d2 = _case(*case)
    want = _sklearn(x, g, K)
    a, b, s, nearest, size = S.silhouette(x, g, K)
    on = S.participants(x, g, K)
    assert np.isnan(s[~on]).all() and (nearest[~on] == -1).all() and not np.isnan(s[on]).any()
    np.testing.assert_array_equal(size, np.bincount(np.asarray(g)[on], minlength=K))
    worst = np.abs(s[on] - want[on]).max()
    print(case, "worst deviation from scikit-learn", worst)
    assert worst <= (4.0 * R.U if exact_d2 else S.bound(x.shape[1]))
    assert worst <= S.bound(x.shape[1])
    ap, bp, sp, np_, _ = S.plain(x, g, K)                                 # the plain fp64 version: rounding of the sums alone
    assert np.abs(sp[on] - want[on]).max() <= 1e-12
    free = S.two_lowest_gap(x, g, K) > S.bound(x.shape[1])
    np.testing.assert_array_equal(nearest[on & free], np_[on & free])
    assert (a[on] >= 0).all() and (b[on] >= 0).all() and (np.abs(s[on]) <= 1).all()


def test_conventions():
    x = R.lattice(20)
    g = np.array(S.lattice_groups())
    a, b, s, nearest, size = S.silhouette(x, g, 7)
    assert size.tolist()[:3] == [100, 0, 1] and size.sum() == 190
    lone = np.nonzero(g == 2)[0][0]
    assert s[lone] == 0 and a[lone] == 0 and np.isfinite(b[lone]) and nearest[lone] >= 0       # a singleton scores 0
    assert not (nearest == 1).any()                                       # an empty group is nobody's nearest
    assert np.isnan(a[g < 0]).all() and np.isnan(b[g < 0]).all() and np.isnan(s[g < 0]).all() and (nearest[g < 0] == -1).all()
    # duplicate rows (50 and 120 are copies of row 7): in one group they are at distance 0 of each other and score alike
    g[[7, 50, 120]] = 3
    a, b, s, nearest, _ = S.silhouette(x, g, 7)
    assert a[7] == a[50] == a[120] and b[7] == b[50] == b[120] and s[7] == s[50] == s[120] and nearest[7] == nearest[50]
    # ... and a group of nothing but copies has a = 0 and scores 1
    g[[7, 50, 120]] = 1
    a, b, s, _, size = S.silhouette(x, g, 7)
    assert size[1] == 3 and (a[[7, 50, 120]] == 0).all() and (s[[7, 50, 120]] == 1).all()
    # an id outside [0, K) and a non-finite row take no part
    bad = np.array(x)
    bad[3, 5], bad[9, 0] = np.nan, np.inf
    g2 = np.array(S.lattice_groups())
    g2[11] = 9
    out = S.silhouette(bad, g2, 7)
    keep = np.ones(197, bool)
    keep[[3, 9, 11]] = False
    ref = S.silhouette(x[keep], S.lattice_groups()[keep], 7)
    for got, want in zip(out[:4], ref[:4]):
        np.testing.assert_array_equal(got[keep], want)                    # the others' figures are those of the batch without them
    assert np.isnan(out[2][[3, 9, 11]]).all() and (out[3][[3, 9, 11]] == -1).all()
    # all participating cells in one group
    a, b, s, nearest, _ = S.silhouette(x, np.zeros(197, int), 3)
    assert np.isinf(b).all() and (nearest == -1).all() and np.isnan(s).all() and (a > 0).all()
    # max(a, b) == 0: two groups of copies of one row
    same = np.repeat(x[:1], 6, axis=0)
    a, b, s, nearest, _ = S.silhouette(same, np.array([0, 0, 0, 1, 1, 1]), 2)
    assert (a == 0).all() and (b == 0).all() and (s == 0).all() and nearest.tolist() == [1, 1, 1, 0, 0, 0]
    # of equal means the lower group id is the nearest
    a, b, s, nearest, _ = S.silhouette(same, np.array([0, 0, 1, 1, 2, 2]), 3)
    assert nearest.tolist() == [1, 1, 0, 0, 0, 0]


def test_the_addition_order_is_the_kernels():
    """The 16 partials and their tree, on values whose sum depends on the order."""
    g = np.random.default_rng(0)
    d = g.uniform(0.1, 1e6, (3, 150)) * g.choice([1e-9, 1.0, 1e9], (3, 150))
    members = np.arange(150)
    got = S.group_sums(d, members, True)
    for i in range(3):
        part = [0.0] * 16
        for p in range(150):
            part[(p % 64) // 4] += d[i, p]
        for off in (1, 2, 4, 8):
            part = [part[u] + part[u ^ off] for u in range(16)]
        assert len(set(part)) == 1 and got[i] == part[0]
