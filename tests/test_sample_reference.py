"""Why tests/sample_reference.py deserves to be K5's reference (``wgnn_sample_rows``, include/wgnn.h): its two independent
versions agree on every (degree, k) the GPU test uses, every draw is a k-subset, the draws are uniform to first order and over
whole subsets within 5 sigma - a condition set beforehand; the measured figures are printed (``pytest -s``) and recorded in
profiles/sample_rows_parity.md - and every word of the key matters.  No GPU, no library."""
from itertools import combinations

import numpy as np
import pytest

import sample_reference as R

TRIPLES = ((7, 0, 0), (2 ** 63 - 1, 5, 3), (11, 2 ** 40, 1))           # (seed, step, stream_id)
FIRST_ORDER = ((12, 5, 20000), (6, 5, 20000), (66, 65, 20000), (300, 70, 20000), (1000, 256, 4000), (257, 256, 4000))   # (m, k, N)
SUBSETS = ((6, 3), (5, 2), (7, 6))
KEYS = ((7, 0, 0), (2 ** 64 - 1, 2 ** 40 + 3, -1), (0, 1, 7))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(got, want):
    for g, w, name in zip(got, want, ("out_col", "out_val", "out_cnt", "out_self", "out_inv")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.dtype == np.float32:
            g, w = _bits(g), _bits(w)
        np.testing.assert_array_equal(g, w, err_msg=name)


def test_known_answer():
    assert R.mix32(0) == 0xE220A839 and int(R.mix32_np(np.zeros(1, np.uint64))[0]) == 0xE220A839
    xs = [0, 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1, 0x9E3779B97F4A7C15]
    assert [R.mix32(x) for x in xs] == R.mix32_np(np.array(xs, np.uint64)).tolist()


@pytest.mark.parametrize("k", R.KS)
def test_the_two_versions_are_equal_on_the_gpu_fixture(k):
    rowptr, col, val = R.fixture()
    ids = np.array([22, 21, 21, 20, 3, 0, 22, 9], np.int32)
    for seed, step, stream in KEYS:
        for row_ids in (None, ids):
            _assert_same(R.sample(rowptr, col, val, row_ids, k, seed, step, stream),
                         R.sample_scalar(rowptr, col, val, row_ids, k, seed, step, stream))


def test_the_fixture_meets_every_boundary():
    """for every k of the GPU test there are rows with fewer than k (k > 1), exactly k, k + 1, a few times k and far more than k
    candidates; 23 rows are no multiple of the four waves of a workgroup"""
    ms = [d + 1 for d in R.DEGREES]
    assert len(ms) == 23
    for k in R.KS:
        assert k in ms and k + 1 in ms and (k == 1 or min(ms) < k)
        assert (k < 63 or any(k + 1 < m <= 4 * k for m in ms)) and any(m >= 15 * k for m in ms), k
    for q in (1, 2, 3, 4):                                             # on and around every boundary of the lane's registers
        assert 64 * q in R.KS and (q == 4 or 64 * q + 1 in R.KS) and (q == 3 or 64 * q - 1 in R.KS)


def _faulty_lists(fault, rowptr, k, seed, step, stream):
    """the chosen lists of the fixture's rows under one of the faults the exact comparison on the GPU is there to catch"""
    w = 1 << 64
    out = []
    for r in range(len(rowptr) - 1):
        m = int(rowptr[r + 1] - rowptr[r]) + 1
        if m <= k:
            out.append(list(range(m)))
            continue
        base = seed ^ (0 if fault == "no step" else step * R.K_STEP % w) ^ (0 if fault == "no stream" else (stream % (1 << 32)) * R.K_STREAM % w) \
            ^ (0 if fault == "no row" else r * R.K_ROW % w)
        xs = []
        for i in range(k):
            j = m - k + i
            h = R.mix32((base + (i + 1 if fault == "draw counter from 1" else i) * R.K_DRAW) % w)
            t = (h * (j if fault == "t below j" else j + 1)) >> 32
            xs.append(j if t in xs else t)
        out.append(sorted(xs) if fault == "sorted" else xs)
    return out


@pytest.mark.parametrize("k", R.KS)
def test_the_fixture_tells_the_named_faults_apart(k):
    """no vacuity: at every k of the GPU test, each of these faults changes some row's list on the fixture - and without a
    fault the lists are the restatement's"""
    rowptr, _, _ = R.fixture()
    seed, step, stream = 7, 1, 2
    law = [R.chosen(seed, step, stream, r, int(rowptr[r + 1] - rowptr[r]) + 1, k) for r in range(len(rowptr) - 1)]
    assert _faulty_lists(None, rowptr, k, seed, step, stream) == law
    for fault in ("no step", "no stream", "no row", "draw counter from 1", "t below j") + (("sorted",) if k > 1 else ()):
        assert _faulty_lists(fault, rowptr, k, seed, step, stream) != law, fault


@pytest.mark.parametrize("m,k", [(2, 1), (6, 5), (66, 65), (129, 128), (300, 70), (257, 256), (5001, 256), (1000, 193)])
def test_every_draw_is_k_distinct_candidates(m, k):
    for seed, step, stream in TRIPLES:
        x = R.draw(seed, step, stream, np.arange(500), m, k)
        assert x.shape == (500, k) and x.min() >= 0 and x.max() < m
        assert (np.diff(np.sort(x, 1), axis=1) > 0).all()
        for r in (0, 499):
            assert R.chosen(seed, step, stream, r, m, k) == x[r].tolist()


def test_a_row_with_at_most_k_candidates_takes_them_all():
    rowptr, col, val = R.fixture()
    for k in (1, 64, 129, 256):
        oc, ov, cnt, self_, inv = R.sample(rowptr, col, val, None, k, 7, 0, 0)
        for r, d in enumerate(R.DEGREES):
            if d + 1 <= k:
                b = rowptr[r]
                assert cnt[r] == d and self_[r] == 1 and inv[r] == np.float32(1) / np.float32(d + 1)
                np.testing.assert_array_equal(oc[r, :d], col[b: b + d])
                np.testing.assert_array_equal(_bits(ov[r, :d]), _bits(val[b: b + d]))
                assert (oc[r, d:] == R.PAD_COL).all() and (ov[r, d:] == R.PAD_VAL).all()
            else:
                assert cnt[r] + self_[r] == k and inv[r] == np.float32(1) / np.float32(k)
                assert (oc[r, cnt[r]:] == R.PAD_COL).all()


@pytest.mark.parametrize("n_rows", [5, 9, 13, 20])
def test_clamp_lemma(n_rows):
    """an operand whose longest row has L entries: k' = min(k, L + 1) gives the lists of k in every row"""
    rowptr, col, val = R.fixture()
    rowptr = rowptr[: n_rows + 1]
    L = int(np.diff(rowptr).max())
    for k in (1, 5, L, L + 1, L + 2, 200, 256):
        if k > 256:
            continue
        kk = R.block_k(rowptr, k)
        assert kk == min(k, L + 1)
        a, b = R.sample(rowptr, col, val, None, k, 7, 3, 1), R.sample(rowptr, col, val, None, kk, 7, 3, 1)
        _assert_same([a[0][:, :kk], a[1][:, :kk], *a[2:]], b)
        assert (a[0][:, kk:] == R.PAD_COL).all()


def _worst_first_order(m, k, keys):
    """worst |f - p| / sigma over the candidates; ``keys`` yields (seed, step, stream, rows)"""
    worst = 0.0
    for seed, step, stream, rows in keys:
        x = R.draw(seed, step, stream, rows, m, k)
        N = len(x)
        f = np.bincount(x.ravel(), minlength=m) / N
        p = k / m
        worst = max(worst, float(np.abs(f - p).max() / np.sqrt(p * (1 - p) / N)))
    return worst


@pytest.mark.parametrize("m,k,N", FIRST_ORDER)
def test_uniform_to_first_order_over_rows(m, k, N):
    worst = _worst_first_order(m, k, [(s, st, sid, np.arange(N)) for s, st, sid in TRIPLES])
    print(f"SIGMA first-order m={m} k={k} N={N}: worst |f - p| / sigma = {worst:.2f}")
    assert worst < 5.0


def test_uniform_to_first_order_over_steps_of_one_row():
    x = np.concatenate([R.draw(7, st, 0, np.array([33]), 12, 5) for st in range(3000)])
    p = 5 / 12
    worst = float(np.abs(np.bincount(x.ravel(), minlength=12) / 3000 - p).max() / np.sqrt(p * (1 - p) / 3000))
    print(f"SIGMA first-order one row, 3000 steps, m=12 k=5: worst |f - p| / sigma = {worst:.2f}")
    assert worst < 5.0


@pytest.mark.parametrize("m,k", SUBSETS)
def test_uniform_over_whole_subsets(m, k):
    N, n_sub = 40000, len(list(combinations(range(m), k)))
    p = 1 / n_sub
    worst = 0.0
    for seed, step, stream in TRIPLES:
        x = np.sort(R.draw(seed, step, stream, np.arange(N), m, k), 1)
        code, cnt = np.unique((x * m ** np.arange(k)).sum(1), return_counts=True)
        assert len(code) == n_sub                                      # every subset occurs
        worst = max(worst, float(np.abs(cnt / N - p).max() / np.sqrt(p * (1 - p) / N)))
    print(f"SIGMA subsets m={m} k={k} C={n_sub} N={N}: worst |f - p| / sigma = {worst:.2f}")
    assert worst < 5.0


def test_every_key_word_matters():
    m, k, rows = 300, 70, np.arange(1000)
    sets = lambda seed, step, stream, r=rows: np.sort(R.draw(seed, step, stream, r, m, k), 1)
    base = sets(7, 3, 2)
    for name, other in (("seed", sets(8, 3, 2)), ("seed, high bit", sets(7 + 2 ** 63, 3, 2)), ("step", sets(7, 4, 2)),
                        ("step, high word", sets(7, 3 + 2 ** 40, 2)), ("stream_id", sets(7, 3, 3)),
                        ("stream_id, sign", sets(7, 3, 2 - 2 ** 31)), ("row", sets(7, 3, 2, rows + 1000)),
                        ("row, next", sets(7, 3, 2, rows + 1))):
        changed = float((base != other).any(1).mean())
        assert changed > 0.99, (name, changed)
    # what the law reduces a word to: stream_id as uint32, step and seed mod 2^64
    np.testing.assert_array_equal(sets(7, 3, -1), sets(7, 3, 2 ** 32 - 1))
    np.testing.assert_array_equal(sets(7, -1, 2), sets(7, 2 ** 64 - 1, 2))
    # a layer's cell block and gene block (stream ids 2i and 2i + 1) do not share draws, nor do two layers
    for a, b in ((0, 1), (0, 2), (1, 3)):
        assert float((sets(7, 3, a) != sets(7, 3, b)).any(1).mean()) > 0.99


def test_nodeflow_keys_its_blocks_by_layer_and_side():
    rng = np.random.default_rng(5)

    def operand(n_rows, n_cols, longest):
        deg = rng.integers(0, longest + 1, n_rows); deg[0] = longest
        rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
        col = np.concatenate([rng.permutation(n_cols)[:d] for d in deg]).astype(np.int32)
        return rowptr, col, rng.standard_normal(len(col)).astype(np.float32)

    cg, gc = operand(30, 40, 25), operand(40, 30, 9)
    seeds = np.array([4, 0, 17, 4, 29])
    nf = R.nodeflow(cg, gc, seeds, 3, 12, 99, 6)
    assert [gb is None for _, gb in nf] == [False, False, True]
    for i, (cb, gb) in enumerate(nf):
        assert cb[0] == 12 and (gb is None or gb[0] == 10)             # min(k, longest row + 1) per operand
        _assert_same(cb[1], R.sample(*cg, seeds if i == 2 else None, 12, 99, 6, 2 * i, 0, 0.0))
        if gb is not None:
            _assert_same(gb[1], R.sample(*gc, None, 10, 99, 6, 2 * i + 1, 0, 0.0))
