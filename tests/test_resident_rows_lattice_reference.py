"""No GPU: every demand of ``tests/test_gpu_resident_rows_exact.py`` is a fair one, for every tuple of the case tables of
``tests/resident_rows_lattice.py`` (the same objects the GPU file parametrizes over) - the lattice budgets, an fp32 evaluation in
two random orders, fp32-representable expectations, the threshold gap, the designed ties, label fairness on every row, the
reference against the formulas of ``test_gpu_resident_predict.py``, and the coverage of the axes."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import resident_rows_lattice as L
from oracle import agg_backward as AB


def is_f32(a):
    a = np.asarray(a, dtype=np.float64)
    return np.array_equal(a.astype(np.float32).astype(np.float64), a)


def fp32_gather(c, rng):
    """The gather, the self fma and the last fma in fp32, the entries of every row in a random order."""
    m, o, R = c.m, c.o, c.R
    M = sp.csr_matrix((R.w, m.indices, m.indptr), shape=m.shape)
    acc = AB.spmm_fp32_random_order(M, o.table, rng)
    if c.self_rows is not None:
        acc = (acc.astype(np.float64) + o.alpha[-1] * c.self_rows).astype(np.float32)      # one fma: one rounding
    z = (acc.astype(np.float64) * R.invd[:, None] + o.bias).astype(np.float32)            # one fma: one rounding
    return acc, np.maximum(z, np.float32(0))


def fp32_logits(c, h32, rng):
    wh, bh = c.head
    perm = rng.permutation(c.H)
    return (h32[:, perm].astype(np.float32) @ wh[:, perm].T.astype(np.float32) + bh.astype(np.float32)).astype(np.float32)


def check_case(c):
    R = c.R
    # 1. budgets: every row of every case is inside the gather's
    inexact = np.flatnonzero(~R.exact_rows)
    assert inexact.size == 0, f"rows {inexact.tolist()} exceed the gather budget: {R.budget[inexact]}"
    assert R.pow2_rows.sum() >= 8 or c.batch != "main"
    # 2. fp32 in two random orders
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        acc32, h32 = fp32_gather(c, rng)
        assert np.array_equal(acc32[R.exact_rows].astype(np.float64), R.acc[R.exact_rows])
        assert np.array_equal(h32[R.exact_rows].astype(np.float64), R.out[R.exact_rows])
        if c.head is not None:
            lg = fp32_logits(c, R.out.astype(np.float32), rng)
            ex = R.exact_logit_rows
            assert np.array_equal(lg[ex].astype(np.float64), R.logits[ex])
    # 3. fp32-representable expectations
    assert is_f32(R.out) and is_f32(R.acc[R.exact_rows])
    if c.head is None:
        return
    ex = R.exact_logit_rows
    assert ex.any() and is_f32(R.logits[ex]) and (R.logit_budget[ex] < 1.0).all(), R.logit_budget.max()
    assert np.array_equal(ex, R.pow2_rows)
    # 4. the threshold sits in a gap wider than twice the bound of every row
    if R.B > 1 and R.C > 1:
        thr, gap = L.place_threshold(R)
        assert gap > 2 * R.expf_bound.max(), (gap, R.expf_bound.max())
        margin = np.abs(R.max_prob - thr)                   # ... and every row keeps its own whole bound (an inexact row's is wider)
        assert (margin > R.max_prob_bound).all(), (margin - R.max_prob_bound).min()
        lab = L.labels(R, thr)
        assert (lab == -1).any() and (lab >= 0).any()
    # 5. no row is excluded from the label comparison
    fair = L.label_rows_fair(R)
    assert fair.all(), f"rows {np.flatnonzero(~fair).tolist()}: top-two gap {R.gap[~fair]} within twice the logit bound"


@pytest.mark.parametrize("case", L.PREDICT_CASES, ids=L.case_id)
def test_predict_cases_are_fair(case):
    H, head, explicit, i64, a_self = case
    c = L.predict_case(H, head, explicit, a_self)
    check_case(c)
    R = c.R
    print(f"BUDGET {L.case_id(case)} lengths={R.budget[:len(L.LENGTHS)].max():.4f} long={R.budget[L.ROW_LONG]:.4f}"
          + (f" logits={R.logit_budget.max():.4f}" if head else ""))
    assert R.exact_rows[L.ROW_LONG] and R.budget.max() < 1.0
    if head and explicit:                                    # 6. every designed tie is a tie in the reference, the lower class wins
        for i, (ja, jb) in enumerate(L.tie_pairs(H)):
            row = R.logits[L.TIE_ROW0 + i]
            assert ja < jb and row[ja] == row[jb] == row.max() and (row == row.max()).sum() == 2
            assert R.argmax[L.TIE_ROW0 + i] == ja and R.exact_logit_rows[L.TIE_ROW0 + i]
        NG = L.n_groups(H)
        (a0, b0), (a1, b1), (a2, b2) = L.tie_pairs(H)
        assert a0 % NG == b0 % NG and a0 // NG != b0 // NG
        if NG > 1:
            assert a1 % NG != b1 % NG and a1 // NG == b1 // NG
            assert a2 % NG > b2 % NG and a2 // NG < b2 // NG


@pytest.mark.parametrize("case", L.TRIP_CASES, ids=L.case_id)
def test_second_trip_cases_are_fair(case):
    H, head, explicit, i64, a_self = case
    c = L.predict_case(H, head, explicit, a_self, "trip")
    check_case(c)
    lens = np.diff(c.m.indptr)
    assert c.m.shape[0] == 8192 + 9 and lens[:8192].max() <= 7 and 65 in lens[8192:] and 0 in lens[8192:]


@pytest.mark.parametrize("case", L.HEAD_LIMIT_CASES, ids=L.case_id)
def test_head_limit_cases_are_fair(case):
    H, C = case
    c = L.head_limit_case(H, C)
    check_case(c)
    assert c.R.pow2_rows.all()                               # every row of the short batch claims exact logits
    assert C == 1 or C * H * 4 <= L.HEAD_LDS_BYTES < (C + 1) * H * 4
    for Hr, Cr in L.HEAD_REFUSED:
        assert (Cr - 1) * Hr * 4 <= L.HEAD_LDS_BYTES < Cr * Hr * 4


@pytest.mark.parametrize("case", L.ATTRIB_CASES + [L.ATTRIB_TRIP_CASE], ids=L.case_id)
def test_attrib_cases_are_fair(case):
    H, i64, explicit = case
    trip = case is L.ATTRIB_TRIP_CASE
    c = L.predict_case(H, True, explicit, L.A_SMALL, "trip" if trip else "main")
    rng = np.random.default_rng(H)
    A = L.attrib_reference(c, c.R.argmax)
    ex = A.exact_entries
    # (w * invd) * <table[g], v>: both products are fp32 numbers on these rows, so is the sum with a prior score (added, or fused)
    assert ex.sum() > 100 and is_f32(A.score[ex]) and is_f32(A.coef[ex]) and is_f32(A.base) and is_f32(A.v)
    direction = rng.integers(-1, 2, (c.m.shape[0], H)).astype(np.float64)
    prior = rng.integers(-4, 5, c.m.nnz).astype(np.float64)
    for es in (False, True):
        D = L.attrib_reference(c, None, direction, es, prior)
        assert is_f32(D.score[ex]) and is_f32(D.coef[ex]) and is_f32((D.score - prior)[ex])


@pytest.mark.parametrize("case", L.SEEN_CASES, ids=L.case_id)
def test_one_entry_cases_are_fair(case):
    n, pos, H, explicit, a_self = case
    m, moved, row, (ga, gb) = L.seen_batches(n, pos)
    o = L.operands(H, a_self)
    sr = L.self_operand(H, 3) if explicit else None
    o_pos = L.SimpleNamespace(**{**vars(o), "bias": np.full(H, 4.0)})      # keeps the ReLU out of the changed row's way
    base, chg = L.reference(m, o_pos, sr), L.reference(moved, o_pos, sr)
    assert base.exact_rows.all() and chg.exact_rows.all()
    differ = o.table[ga] != o.table[gb]
    assert differ.any() and np.array_equal(base.out[row] != chg.out[row], differ)
    assert np.array_equal(np.delete(base.out, row, 0), np.delete(chg.out, row, 0))


def test_exact_rounding_step_against_fractions():
    """``acc * float32(1 / (deg + 1)) + bias`` in fp64 is the exact rational, on a sample of every main case's elements."""
    rng = np.random.default_rng(5)
    for H, explicit, a_self in ((256, True, L.A_SMALL), (100, False, L.A_BIG), (20, False, L.A_SMALL)):
        c = L.predict_case(H, False, explicit, a_self)
        R = c.R
        for _ in range(300):
            r, k = int(rng.choice(np.flatnonzero(R.exact_rows))), int(rng.integers(H))
            exact = Fraction(R.acc[r, k]) * Fraction(R.invd[r]) + Fraction(c.o.bias[k])
            assert Fraction(R.z[r, k]) == exact


def test_reference_agrees_with_the_restatement_of_the_predict_tests():
    """``reference(lattice=False)`` against ``_ref_layer`` / ``_ref_head`` of test_gpu_resident_predict.py on that file's batch."""
    import test_gpu_resident_predict as P
    rng = np.random.default_rng(3)
    Gn, B, H, C = 6000, 40, 64, 16
    m = P._ragged_batch(rng, B, Gn)
    table = (0.5 * rng.standard_normal((Gn, H))).astype(np.float32)
    alpha = rng.uniform(0.5, 1.5, Gn + 2).astype(np.float32)
    bias = (0.1 * rng.standard_normal(H)).astype(np.float32)
    sr = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    w = (rng.standard_normal((C, H)) / np.sqrt(H)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    o = L.SimpleNamespace(table=table.astype(np.float64), alpha=alpha.astype(np.float64), bias=bias.astype(np.float64), H=H,
                          a_self=float(alpha[-1]))
    for self_rows in (None, sr):
        R = L.reference(m, o, None if self_rows is None else self_rows.astype(np.float64), (w.astype(np.float64), b.astype(np.float64)),
                        lattice=False)
        want_h = P._ref_layer(m.astype(np.float64), table, alpha, bias, self_rows)        # (its S is summed in the matrix's type)
        want_l, want_p = P._ref_head(want_h, w, b)
        np.testing.assert_allclose(R.out, want_h, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(R.logits, want_l, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(R.max_prob, want_p, rtol=1e-12)


def test_float_cases_qualify():
    """The float group's label comparison keeps at least 90 % of the rows at its fixed seeds."""
    for case in L.FLOAT_CASES:
        c = L.float_case(*case)
        share = float(L.clear_rows(c.R, L.place_threshold(c.R)[0]).mean())
        assert share >= 0.9, (case, share)


def test_no_axis_value_is_missing():
    assert {c[0] for c in L.PREDICT_CASES} == set(L.H_ALL)
    assert {L.lpr_of(H) for H in L.H_ALL} == {4, 8, 16, 32, 64} and {L.lpr_of(H) for H in L.H_PER_LPR} == {4, 8, 16, 32, 64}
    edges = {4: (4, 16), 8: (20, 32), 16: (36, 64), 32: (68, 128), 64: (132, 256)}
    for lpr, (lo, hi) in edges.items():
        assert lo in L.H_ALL and hi in L.H_ALL and L.lpr_of(lo) == L.lpr_of(hi) == lpr
    met = {(L.lpr_of(H), head, explicit, i64) for H, head, explicit, i64, _ in L.PREDICT_CASES}
    assert len(met) == 40                                    # 20 (LPR, HEAD, SELF_ROWS) instantiations x both row-pointer types
    assert {c[4] for c in L.PREDICT_CASES} == {L.A_SMALL, L.A_BIG}
    met_a = {(L.lpr_of(H), explicit, i64) for H, i64, explicit in L.ATTRIB_CASES}
    assert {(l, i) for l, _, i in met_a} == {(l, i) for l in (4, 8, 16, 32, 64) for i in (False, True)}
    assert {(H, hd) for H, hd, _ in L.DERIVED_CASES} == {(32, False), (32, True), (128, False), (128, True)}
    assert {(H, hd) for H, hd, *_ in L.TRIP_CASES} >= {(12, False), (12, True), (132, False), (132, True)}
    assert {c[1] for c in L.SEEN_CASES} == {"first", "last", "last_chunk"} and {c[0] for c in L.SEEN_CASES} == {L.LONG, 1025}
    assert set(L.LENGTHS) >= {65, 129, 193, 128, 192, 1, 63, 64, 1025}
    for H in L.H_ALL:
        assert L.classes_for(H) * H * 4 <= L.HEAD_LDS_BYTES and L.classes_for(H) > 2 * L.n_groups(H)
