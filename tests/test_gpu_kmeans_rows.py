"""``ops.group_rows_reduce``, ``ops.kmeans_seed`` and ``ops.kmeans_rows`` on the GPU against the fp64 restatement
(tests/kmeans_reference.py): bit for bit wherever float32 is exact (the lattice, ``blobs``) or the order of additions is restated
(the row sums), up to the stated rounding bound on real-valued rows; two launches always give the same bits."""
import numpy as np
import pytest
import torch

from scdeepsort_amd import ops

import kmeans_reference as M
import knn_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _dev(x):
    return torch.tensor(np.asarray(x), device=DEV)


# --------------------------------------------------------------------------------------------- group_rows_reduce
def _lattice_groups():
    """197 cells in 7 groups: group 0 spans two chunks (100 cells, scattered), 1 is empty, 2 a singleton, 3..6 share 89
    cells, 7 cells take no part (-1)."""
    perm = np.random.default_rng(5).permutation(R.LATTICE_N)
    g = np.full(R.LATTICE_N, -1, np.int64)
    g[perm[:100]] = 0
    g[perm[100]] = 2
    g[perm[101:190]] = 3 + np.arange(89) % 4
    return g


@pytest.mark.parametrize("D", R.LATTICE_DIMS)
def test_reduce_on_the_lattice_is_exact_with_guards(D):
    x, g, K = R.lattice(D), _lattice_groups(), 7
    want_sum, want_count = M.group_sums(x, g, K)
    assert want_count.tolist()[:3] == [100, 0, 1] and want_count.sum() == 190
    wide = torch.full((R.LATTICE_N + 2, D + 12), 777.0, device=DEV)
    wide[1:-1, 4:4 + D] = _dev(x)
    mean_buf = torch.full((K + 2, D + 8), -7.0, device=DEV)
    total = torch.full((K, D), -7.0, dtype=torch.float64, device=DEV)
    count = torch.full((K,), -7, dtype=torch.int64, device=DEV)
    for group in (_dev(g), _dev(g.astype(np.int32))):
        out = ops.group_rows_reduce(wide[1:-1, 4:4 + D], group, K, out=(total, count, mean_buf[1:-1, 4:4 + D]))
        np.testing.assert_array_equal(_bits(out[0].cpu().numpy()), _bits(want_sum))
        np.testing.assert_array_equal(out[1].cpu().numpy(), want_count)
        mean = mean_buf.cpu().numpy()
        on = want_count > 0
        np.testing.assert_array_equal(_bits(mean[1:-1, 4:4 + D][on]), _bits((want_sum[on] / want_count[on, None]).astype(np.float32)))
        assert (mean[1:-1, 4:4 + D][~on] == -7).all()                    # the empty group's row is untouched
        assert (mean[0] == -7).all() and (mean[-1] == -7).all() and (mean[:, :4] == -7).all() and (mean[:, 4 + D:] == -7).all()
    assert (wide[0] == 777).all() and (wide[:, :4] == 777).all() and (wide[:, 4 + D:] == 777).all()
    plain = ops.group_rows_reduce(_dev(x), _dev(g), K)                   # without out=: an empty group's mean is zero
    assert torch.equal(plain[0], total) and torch.equal(plain[1], count) and (plain[2][1] == 0).all()


def test_reduce_restates_the_order_on_real_rows():
    x = M.overlap(300, 20, 0)
    g = np.random.default_rng(1).integers(-1, 4, 300)
    g[g == 1] = 0                                                        # group 0 holds ~ 120 cells: two chunks; group 1 is empty
    g[7] = 9                                                             # an id outside [0, K) takes no part
    want_sum, want_count = M.group_sums(x, np.where(g == 9, -1, g), 4)
    first = ops.group_rows_reduce(_dev(x), _dev(g), 4)
    np.testing.assert_array_equal(_bits(first[0].cpu().numpy()), _bits(want_sum))
    np.testing.assert_array_equal(first[1].cpu().numpy(), want_count)
    again = ops.group_rows_reduce(_dev(x), _dev(g), 4)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    on = want_count > 0
    np.testing.assert_array_equal(_bits(first[2].cpu().numpy()[on]), _bits((want_sum[on] / want_count[on, None]).astype(np.float32)))
    # one group that takes every row of a batch of several chunks, and a width that is no multiple of 64 or 4
    x = M.overlap(300, 200, 0)[:, :197]
    out = ops.group_rows_reduce(_dev(x.copy()), torch.zeros(300, dtype=torch.int32, device=DEV), 1)
    np.testing.assert_array_equal(_bits(out[0].cpu().numpy()), _bits(M.group_sums(x, np.zeros(300, int), 1)[0]))


# --------------------------------------------------------------------------------------------- kmeans_seed
def _assert_seeding_equals_reference(x, K, seed):
    rows, min_d2 = ops.kmeans_seed(_dev(x), K, seed)
    assert rows.dtype == torch.int32 and min_d2.dtype == torch.float32
    want_rows, want_d2 = M.seed_rows(x, K, seed)
    np.testing.assert_array_equal(rows.cpu().numpy(), want_rows)
    got = min_d2.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want_d2))
    np.testing.assert_array_equal(_bits(got)[~np.isnan(got)], _bits(want_d2)[~np.isnan(want_d2)])
    return rows.cpu().numpy(), got


@pytest.mark.parametrize("D", M.BLOB_DIMS)
def test_seeding_on_blobs_is_bit_exact(D):
    x = M.blobs(D)
    for K in (1, 3, 5, 8):
        for seed in (0, 1):
            rows, min_d2 = _assert_seeding_equals_reference(x, K, seed)
            assert (min_d2[rows] == 0).all() and len(set(rows.tolist())) == K
    bad = x.copy()
    bad[[33, 140], [5, D - 1]] = np.nan, np.inf                          # a NaN row and an inf row: never chosen, NaN
    for seed in (0, 1, 2):
        rows, min_d2 = _assert_seeding_equals_reference(bad, 8, seed)
        assert not {33, 140} & set(rows.tolist()) and np.isnan(min_d2[[33, 140]]).all() and np.isnan(min_d2).sum() == 2


def test_seeding_duplicate_rows_follow_the_zero_total_rule():
    x = M.duplicates()
    for seed in (0, 1, 2):
        rows, min_d2 = _assert_seeding_equals_reference(x, 5, seed)
        assert sorted(r % 3 for r in rows[:3]) == [0, 1, 2]
        assert rows[3:].tolist() == sorted(set(range(6)) - set(rows[:3].tolist()))[:2] and (min_d2 == 0).all()
    _assert_seeding_equals_reference(x, 6, 0)                            # all six rows are taken
    with pytest.raises(ValueError, match="finite"):
        ops.kmeans_seed(_dev(x), 7)
    # more rows than one chunk, all equal but two: the prefix runs over several chunk sums, then nothing is left
    many = np.zeros((600, 8), np.float32)
    many[300], many[599] = 1.0, 2.0
    rows, _ = _assert_seeding_equals_reference(many, 5, 0)
    assert rows.tolist() == [391, 300, 599, 0, 1]                        # a zero row, the two rows that carry weight, the lowest left


@pytest.mark.parametrize("case", M.OVERLAP_CASES)
def test_seeding_on_real_rows_draws_from_its_own_weights(case):
    x = M.overlap(*case)
    N, D = x.shape
    K, seed = 16, 0
    rows, min_d2 = ops.kmeans_seed(_dev(x), K, seed)
    again = ops.kmeans_seed(_dev(x), K, seed)
    assert torch.equal(rows, again[0]) and torch.equal(min_d2.view(torch.int32), again[1].view(torch.int32))
    rows, min_d2 = rows.cpu().numpy(), min_d2.cpu().numpy()
    assert len(set(rows.tolist())) == K and rows.min() >= 0 and rows.max() < N
    assert rows[0] == M.seed_rows(x, 1, seed)[0][0]                      # round 0 draws from equal weights: no rounding enters
    exact = np.full(N, np.inf)
    for r in range(K):
        # the fp64 weights from the kernel's OWN earlier seeds: the kernel's f32 weights differ from them by gamma relative,
        # each prefix sum adds at most N roundings of 2^-53 relative - both scale with T
        w = np.ones(N) if r == 0 else exact.copy()
        P, T = M.prefix(w)
        t, s = M.draw(seed, r) * T, int(rows[r])
        tol = (R.gamma(D) + N * 2.0 ** -53) * T
        below = P[s - 1] if s else 0.0
        assert below - tol <= t < P[s] + tol, (r, s, below, t, P[s], tol)
        assert w[s] > 0
        exact = np.minimum(exact, M.distance_to(x, x[s]))
    err = np.abs(min_d2.astype(np.float64) - exact)
    assert (err <= R.gamma(D) * exact).all() and (min_d2[rows] == 0).all()


# --------------------------------------------------------------------------------------------- kmeans_rows
def _assert_run_equals(got, ref, D, centers_bitwise=True):
    np.testing.assert_array_equal(got.label.cpu().numpy(), ref["label"])
    assert got.label.dtype == torch.int32 and got.d2.dtype == torch.float32 and got.size.dtype == torch.int64
    if centers_bitwise:
        np.testing.assert_array_equal(_bits(got.centers.cpu().numpy()), _bits(ref["centers"]))
    np.testing.assert_array_equal(got.size.cpu().numpy(), ref["size"])
    assert (got.n_iter, got.converged) == (ref["n_iter"], ref["converged"])
    assert len(got.inertia_trace) == len(ref["inertia_trace"])
    for a, b in zip(got.inertia_trace, ref["inertia_trace"]):
        assert abs(a - b) <= R.gamma(D) * b
    d2, on = got.d2.cpu().numpy().astype(np.float64), ref["label"] >= 0
    assert (np.abs(d2[on] - ref["d2"][on]) <= R.gamma(D) * ref["d2"][on]).all() and np.isnan(d2[~on]).all()


@pytest.mark.parametrize("D", M.BLOB_DIMS)
@pytest.mark.parametrize("K", M.BLOB_KS)
def test_kmeans_on_blobs_equals_the_reference(D, K):
    x = M.blobs(D)
    for seed in M.blob_seeds(D, K):
        ref = M.reference("blobs", K, seed, D)
        got = ops.kmeans_rows(_dev(x), K, seed=seed)
        np.testing.assert_array_equal(got.seed_row.cpu().numpy(), ref["seed_row"])
        _assert_run_equals(got, ref, D)


@pytest.mark.parametrize("case", M.OVERLAP_CASES)
@pytest.mark.parametrize("K", M.OVERLAP_KS)
def test_kmeans_on_real_rows_from_the_reference_seeds(case, K):
    x = M.overlap(*case)
    ref = M.reference("overlap", K, 0, *case)
    init = x[ref["seed_row"]]
    got = ops.kmeans_rows(_dev(x), K, init=_dev(init))
    assert got.seed_row is None
    _assert_run_equals(got, ref, case[1])                               # no near-tie anywhere: equal labels, so equal centre bits
    again = ops.kmeans_rows(_dev(x), K, init=init)                      # a host array, and a second run: the same bits
    assert torch.equal(again.label, got.label) and torch.equal(again.centers, got.centers) and torch.equal(again.d2, got.d2)
    seeded = ops.kmeans_rows(_dev(x), K, seed=3), ops.kmeans_rows(_dev(x), K, seed=3)
    assert torch.equal(seeded[0].label, seeded[1].label) and torch.equal(seeded[0].centers, seeded[1].centers)
    assert torch.equal(seeded[0].seed_row, seeded[1].seed_row) and seeded[0].inertia_trace == seeded[1].inertia_trace


def test_kmeans_stops_at_max_iter_with_labels_of_the_returned_centres():
    x, K = M.blobs(36), 8
    assert M.reference("blobs", K, 0, 36)["n_iter"] == 10                # the case that needs the most iterations
    for max_iter in (1, 2):
        ref = M.kmeans(x, K, max_iter=max_iter, seed=0)
        got = ops.kmeans_rows(_dev(x), K, max_iter=max_iter, seed=0)
        assert not got.converged and got.n_iter == max_iter and len(got.inertia_trace) == max_iter + 1
        _assert_run_equals(got, ref, 36)
        label, _, gap = M.assign(x, got.centers.cpu().numpy())          # the labels belong to the centres that are returned
        assert gap.min() >= 1.0
        np.testing.assert_array_equal(got.label.cpu().numpy(), label)


def test_kmeans_empty_clusters_keep_their_centre():
    x = M.blobs(20)
    ref = M.reference("blobs", 3, 0, 20)
    far = np.concatenate([x[ref["seed_row"]], np.full((1, 20), 1000.0, np.float32)])
    got = ops.kmeans_rows(_dev(x), 4, init=far)
    assert got.size.cpu().numpy().tolist() == ref["size"].tolist() + [0]
    np.testing.assert_array_equal(_bits(got.centers.cpu().numpy()[3]), _bits(far[3]))
    np.testing.assert_array_equal(_bits(got.centers.cpu().numpy()[:3]), _bits(ref["centers"]))
    np.testing.assert_array_equal(got.label.cpu().numpy(), ref["label"])
    # two equal centres: the lower index takes the rows, the higher stays empty and where it was
    # (the converged centres twice: the lower one's mean is itself, so the two stay equal through the update)
    twin = np.concatenate([ref["centers"][:1], ref["centers"]])         # centres 0 and 1 are equal
    got = ops.kmeans_rows(_dev(x), 4, init=twin)
    size = got.size.cpu().numpy()
    assert size[0] == ref["size"][0] and size[1] == 0 and size[2:].tolist() == ref["size"][1:].tolist()
    assert got.converged and got.n_iter == 2 and not (got.label == 1).any()
    np.testing.assert_array_equal(_bits(got.centers.cpu().numpy()), _bits(twin))
    # rows with a non-finite value get no cluster and move no centre
    bad = np.concatenate([x, np.full((2, 20), np.nan, np.float32)])
    bad[-1, 3] = np.inf
    got = ops.kmeans_rows(_dev(bad), 3, init=x[ref["seed_row"]])
    assert (got.label[-2:] == -1).all() and torch.isnan(got.d2[-2:]).all()
    np.testing.assert_array_equal(got.label.cpu().numpy()[:-2], ref["label"])
    np.testing.assert_array_equal(_bits(got.centers.cpu().numpy()), _bits(ref["centers"]))


def test_argument_errors_and_padding():
    x = _dev(M.blobs(20))
    for kw in (dict(n_clusters=0), dict(n_clusters=4097), dict(n_clusters=198), dict(n_clusters=3, max_iter=0),
               dict(n_clusters=3, init="random"), dict(n_clusters=3, init=np.zeros((3, 24), np.float32)),
               dict(n_clusters=3, init=np.zeros((2, 20), np.float32)), dict(n_clusters=3, init=np.zeros((3, 20))),
               dict(n_clusters=3, init=np.full((3, 20), np.nan, np.float32))):
        with pytest.raises(ValueError):
            ops.kmeans_rows(x, **kw)
    with pytest.raises(ValueError, match="float32"):
        ops.kmeans_rows(x.double(), 3)
    with pytest.raises(ValueError, match="D = 1028"):
        ops.kmeans_rows(torch.zeros((8, 1028), device=DEV), 2)
    for kw in (dict(n_groups=0), dict(n_groups=3, out=(None, None))):
        with pytest.raises(ValueError):
            ops.group_rows_reduce(x, torch.zeros(197, dtype=torch.int64, device=DEV), **kw)
    with pytest.raises(ValueError, match="one int32 / int64 id per row"):
        ops.group_rows_reduce(x, torch.zeros(5, dtype=torch.int64, device=DEV), 3)
    # a width that is no multiple of 4 is zero-padded: the run of the padded rows, with centres of the caller's width
    odd = M.overlap(300, 20, 0)[:, :7].copy()
    a = ops.kmeans_rows(_dev(odd), 6, seed=1)
    b = ops.kmeans_rows(torch.nn.functional.pad(_dev(odd), (0, 1)), 6, seed=1)
    assert a.centers.shape == (6, 7) and torch.equal(a.label, b.label) and torch.equal(a.centers, b.centers[:, :7])
    assert torch.equal(a.seed_row, b.seed_row) and (b.centers[:, 7] == 0).all()
