"""The numpy restatement of the soup-rows contract (tests/soup_reference.py) against the properties ``include/wgnn.h`` states as
consequences of the hash - no GPU: the GPU tests compare the kernels with this reference, these tests check the reference."""
import numpy as np

import soup_reference as S
from lognorm_reference import lognorm_dense


def _dense_counts(ref, units, G):
    x = np.zeros((units, G), np.int64)
    x[np.repeat(np.arange(units), np.diff(ref.rowptr)), ref.col] = ref.cnt
    return x


def test_the_case_holds_what_it_says():
    m = S.batch()
    lens = np.diff(m.rowptr)
    assert lens[[S.ROW_EMPTY, S.ROW_PURE_SOUP, S.ROW_FOREIGN_ONLY]].tolist() == [0, 0, 0]
    assert lens[[S.ROW_ONE, S.ROW_63, S.ROW_64, S.ROW_65, S.ROW_ALL]].tolist() == [1, 63, 64, 65, S.G_CASE]
    assert m.lib[S.ROW_EMPTY] == 0 and m.n_add[S.ROW_EMPTY] == 0 and m.lib[S.ROW_PURE_SOUP] == 0 and m.n_add[S.ROW_PURE_SOUP] == 40
    assert m.lib[S.ROW_FOREIGN_ONLY] == 7 and m.cnt.max() == 2.0 ** 23
    unsorted = m.col[m.rowptr[S.ROW_UNSORTED]:m.rowptr[S.ROW_UNSORTED + 1]]
    assert (np.diff(unsorted) < 0).all()
    twice = m.col[m.rowptr[S.ROW_TWICE]:m.rowptr[S.ROW_TWICE + 1]]
    assert (twice == 7).sum() == 2 and (twice == 299).sum() == 3
    assert set(m.n_add.tolist()) == {0, 1, 40, 63, 64, 65, 513, 3000}
    assert (m.cnt == np.floor(m.cnt)).all() and m.cnt.min() >= 1
    p = S.profiles()
    for cdf in p.values():
        assert cdf.dtype == np.uint64 and cdf.shape == (S.G_CASE + 2,) and cdf[0] == 0 and (np.diff(cdf.astype(object)) >= 0).all()
        assert 0 < int(cdf[-1]) < 2 ** 63
    assert int(p["wide"][-1]) > 2 ** 48
    widths = np.diff(p["uniform"].astype(np.int64))
    assert (widths[:S.G_CASE] == 0).sum() == S.G_CASE // 3 and widths[S.G_CASE] > 0


def test_counts_are_conserved_and_zero_width_bins_are_never_drawn():
    m = S.batch()
    own = np.asarray([m.cnt[m.rowptr[r]:m.rowptr[r + 1]].sum() for r in range(m.B)], np.int64)
    for name, cdf in S.profiles().items():
        ref = S.case(name, 0.0).ref
        x = _dense_counts(ref, m.B * S.N_DRAWS, m.G)
        np.testing.assert_array_equal(x.sum(axis=1), np.repeat(own, S.N_DRAWS) + ref.soup_mapped)
        assert (ref.soup_mapped >= 0).all() and (ref.soup_mapped <= np.repeat(m.n_add, S.N_DRAWS)).all()
        width = np.diff(cdf.astype(object))
        for r in (S.ROW_PURE_SOUP, S.ROW_DEEP_A):
            bins = S.draws(S.CASE_SEED, r, 1, int(m.n_add[r]), cdf)
            assert bins.min() >= 0 and bins.max() <= m.G and all(width[b] > 0 for b in set(bins.tolist()))


def test_the_one_gene_and_the_rest_only_profiles():
    m = S.batch()
    one, rest = S.case("one", 0.0).ref, S.case("rest", 0.0).ref
    np.testing.assert_array_equal(one.soup_mapped, np.repeat(m.n_add, S.N_DRAWS))       # every read hits the one counter
    np.testing.assert_array_equal(rest.soup_mapped, 0)
    x = _dense_counts(one, m.B * S.N_DRAWS, m.G)
    q = S.ROW_PURE_SOUP * S.N_DRAWS
    assert x[q, S.ONE_GENE] == 40 and x[q].sum() == 40 and one.n_out[q] == 1
    # reads that all fall outside the bundle only deepen the library: the cell's own genes, smaller values
    clean = S.soup_rows(m, np.zeros(m.B, np.int64), S.profiles()["rest"], S.N_DRAWS, 0.0, seed=S.CASE_SEED)
    np.testing.assert_array_equal(rest.col, clean.col)
    np.testing.assert_array_equal(rest.cnt, clean.cnt)
    deep = np.repeat(np.repeat(m.n_add, S.N_DRAWS) > 0, np.diff(rest.rowptr))
    assert (rest.v64[deep] < clean.v64[deep]).all() and (rest.v64[~deep] == clean.v64[~deep]).all()
    assert rest.n_out[S.ROW_PURE_SOUP * S.N_DRAWS] == 0                                 # 40 reads, none on a bundle gene


def test_levels_are_nested_and_splits_change_nothing():
    m = S.batch()
    cdf = S.profiles()["wide"]
    for r in (S.ROW_DEEP_B, S.ROW_513):
        full = S.draws(S.CASE_SEED, r, 2, 3000, cdf)
        for n in (0, 1, 64, 513):
            np.testing.assert_array_equal(S.draws(S.CASE_SEED, r, 2, n, cdf), full[:n])
    # a batch split by cells (row0) and by draws (draw0) is the whole
    whole = S.case("uniform", 0.0).ref
    r0 = 5
    part = SimpleSlice(m, r0)
    tail = S.soup_rows(part, m.n_add[r0:], S.profiles()["uniform"], S.N_DRAWS, 0.0, seed=S.CASE_SEED, row0=r0)
    q0 = r0 * S.N_DRAWS
    np.testing.assert_array_equal(tail.n_out, whole.n_out[q0:])
    np.testing.assert_array_equal(tail.col, whole.col[whole.rowptr[q0]:])
    np.testing.assert_array_equal(tail.val.view(np.int32), whole.val[whole.rowptr[q0]:].view(np.int32))
    last = S.soup_rows(m, m.n_add, S.profiles()["uniform"], 1, 0.0, seed=S.CASE_SEED, draw0=S.N_DRAWS - 1)
    np.testing.assert_array_equal(last.n_out, whole.n_out[S.N_DRAWS - 1::S.N_DRAWS])
    np.testing.assert_array_equal(last.soup_mapped, whole.soup_mapped[S.N_DRAWS - 1::S.N_DRAWS])
    # another draw, another cell and another seed are other reads
    a = S.draws(S.CASE_SEED, S.ROW_DEEP_A, 0, 3000, cdf)
    for other in (S.draws(S.CASE_SEED, S.ROW_DEEP_A, 1, 3000, cdf), S.draws(S.CASE_SEED, S.ROW_DEEP_B, 0, 3000, cdf),
                  S.draws(S.CASE_SEED + 1, S.ROW_DEEP_A, 0, 3000, cdf)):
        assert (a != other).mean() > 0.9


def SimpleSlice(m, r0):
    """The batch from row ``r0`` on, as a batch of its own."""
    from types import SimpleNamespace
    e0 = m.rowptr[r0]
    return SimpleNamespace(rowptr=m.rowptr[r0:] - e0, col=m.col[e0:], cnt=m.cnt[e0:], lib=m.lib[r0:])


def test_no_soup_is_the_lognorm_aligned_row_and_the_dense_form_agrees():
    m = S.batch()
    for thr in S.THRESHOLDS:
        for name in ("uniform", "wide"):
            cdf = S.profiles()[name]
            clean = S.soup_rows(m, np.zeros(m.B, np.int64), cdf, 1, thr, seed=S.CASE_SEED)
            x, gmap = S.contaminated_dense(m, np.zeros(m.B, np.int64), cdf, 1, seed=S.CASE_SEED)
            rowptr, col, val = lognorm_dense(x, gmap, thr, S.SCALE)
            np.testing.assert_array_equal(clean.rowptr, rowptr)
            np.testing.assert_array_equal(clean.col, col)
            np.testing.assert_array_equal(clean.val.view(np.int32), val.view(np.int32))
            assert (clean.soup_mapped == 0).all()
            # and with soup: the dense contaminated matrix through the lognorm reference is the reference's CSR
            ref = S.case(name, thr).ref
            x, gmap = S.contaminated_dense(m, m.n_add, cdf, S.N_DRAWS, seed=S.CASE_SEED)
            np.testing.assert_array_equal(x.sum(axis=1, dtype=np.float64), np.repeat(m.lib + m.n_add, S.N_DRAWS))
            rowptr, col, val = lognorm_dense(x, gmap, thr, S.SCALE)
            np.testing.assert_array_equal(ref.rowptr, rowptr)
            np.testing.assert_array_equal(ref.col, col)
            np.testing.assert_array_equal(ref.val.view(np.int32), val.view(np.int32))


def test_permuting_a_rows_entries_changes_nothing():
    from types import SimpleNamespace
    m = S.batch()
    rng = np.random.default_rng(3)
    order = np.concatenate([m.rowptr[r] + rng.permutation(m.rowptr[r + 1] - m.rowptr[r]) for r in range(m.B)])
    shuffled = SimpleNamespace(rowptr=m.rowptr, col=m.col[order], cnt=m.cnt[order], lib=m.lib)
    assert (shuffled.col != m.col).any()
    for thr in S.THRESHOLDS:
        want = S.case("wide", thr).ref
        got = S.soup_rows(shuffled, m.n_add, S.profiles()["wide"], S.N_DRAWS, thr, seed=S.CASE_SEED)
        for name in ("rowptr", "col", "cnt", "soup_mapped"):
            np.testing.assert_array_equal(getattr(got, name), getattr(want, name))
        np.testing.assert_array_equal(got.val.view(np.int32), want.val.view(np.int32))


def test_the_drawn_frequencies_follow_the_widths():
    """The 3000-read rows under the uniform profile, all draws pooled: N = 27 000 reads.  A bin of share p has a binomial standard
    error of sqrt(p (1 - p) / N); the bound is SIX of them - over 201 bins of non-zero width a fair generator exceeds it with
    probability below 1e-6, a generator that misplaces a bin boundary or drops hash bits misses it by tens of errors."""
    m = S.batch()
    cdf = S.profiles()["uniform"]
    bins = np.concatenate([S.draws(S.CASE_SEED, r, d, 3000, cdf) for r in S.DEEP_ROWS for d in range(S.N_DRAWS)])
    N = bins.shape[0]
    assert N == 27_000
    p = np.diff(cdf.astype(np.int64)) / float(cdf[-1])
    freq = np.bincount(bins, minlength=m.G + 1) / N
    err = np.sqrt(p * (1 - p) / N)
    assert (freq[p == 0] == 0).all()
    worst = (np.abs(freq - p)[p > 0] / err[p > 0]).max()
    print(f"worst deviation {worst:.2f} standard errors")
    assert worst <= 6.0


def test_fragile_values_are_rare_in_the_case():
    """The cap that keeps the one-ulp allowance of the GPU test from hiding anything: expected about 1e-7."""
    for name in S.profiles():
        for thr in S.THRESHOLDS:
            ref = S.case(name, thr).ref
            assert ref.v64.size > 1000 or name in ("rest", "one")
            assert S.fragile(ref.v64).mean() <= S.FRAGILE_CAP, (name, thr)
    assert S.FRAGILE_CAP == 0.001
