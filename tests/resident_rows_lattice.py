"""Lattice batches, case tables and the fp64 reference of the resident row ops (``wgnn_predict_rows``, ``wgnn_attrib_rows`` and
the kernels that restate their gather).  No GPU, nothing of ``scdeepsort_amd`` is imported: ``tests/test_resident_rows_lattice_
reference.py`` checks on the CPU that every demand the GPU file ``tests/test_gpu_resident_rows_exact.py`` makes is a fair one, for
every tuple of the tables below (they are the same objects in both files).

The lattice (``profiles/resident_rows_parity.md`` has the measured budgets):

* ``table`` (P(0) = 0.6) and ``w_head`` entries in {-1, 0, 1}; ``alpha[g]`` in {0.5, 1, 1.5}; ``bias`` and ``b_head`` multiples of 1/4;
  ``self_rows`` multiples of 1/2.
* a row of n entries holds positive integers whose sum S = max(32, 2^ceil(log2 n)) is a power of two (every value starts at 1, the
  remainder is spread evenly), so ``S + 1e-6f == S`` in fp32, ``deg * x / S`` and ``a_self / S`` are exact, every weight
  ``w_j = (x_j / S)(alpha_g deg + a_self)`` is an fp32 number and every partial sum of the gather is a multiple of the row's unit
  below 2^24 units - exact in fp32 in any order, with or without FMA contraction.
* two self scales: ``alpha[G+1] = 1.5`` and ``alpha[G+1] = 2048``.  The flat 4096-entry row (all values 1, S = deg = 4096) with the
  self-loop taken from the row has weights that are multiples of 1/2 under the second (budget 6e-4); under 1.5 they are multiples
  of 2^-13 and the row fits only because the table is drawn with P(0) = 0.6 (budget 0.86 at the fixed seeds, asserted on the CPU).
  ``exact_rows`` of the reference says per row whether the budget holds; a row outside it would be held to the derived float
  bound instead (none is, in the tables as they stand).

What is exact where: ``acc`` (the gather) on every lattice row within its budget; ``out = ReLU(fma(acc, invd, bias))`` is then ONE
rounding of an exactly known number, ``invd = float32(1) / float32(deg + 1)`` being a correctly rounded division (exact where
``deg + 1`` is a power of two); ``logits`` on the rows with ``deg + 1`` in {1, 2, 4, .., 128}, whose ``h`` lies on a small lattice;
``label`` on EVERY row (the reference's top-two gap exceeds twice the logit bound, or the row is a designed tie); ``max_prob``
within ``max_prob_bound`` (``expf`` is not exact)."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from oracle import agg_backward as AB

G = 6000                                                   # the flat 4096-entry row needs it
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513,
           1023, 1024, 1025)
LONG = 4096
H_ALL = (4, 16, 20, 32, 36, 64, 68, 100, 128, 132, 200, 252, 256)      # both edges of every LPR branch
H_PER_LPR = (16, 20, 64, 100, 256)
A_SMALL, A_BIG = 1.5, 2048.0
N_TIE_ROWS = 4                                             # three designed ties and one row with h = 0
EXPF_ULP = 1.0                                             # per-call error of expf assumed (HIP math API accuracy table: 1 ULP)
HEAD_LDS_BYTES = 64 * 1024


def lpr_of(H):
    """``wgnn::dispatch_rows``: lanes per table row."""
    q = H // 4
    return 4 if q <= 4 else 8 if q <= 8 else 16 if q <= 16 else 32 if q <= 32 else 64


def n_groups(H):
    return 64 // lpr_of(H)


def classes_for(H):
    """More than two trips of the class loop at every LPR (class j is lane group j % NG's in trip j // NG)."""
    return 2 * n_groups(H) + 3


def tie_pairs(H):
    """(same lane group, different trips), (different groups, same trip; LPR 64 has one group), (different groups AND trips, the
    lower class in the HIGHER group).  The lower class must win each."""
    NG = n_groups(H)
    return ((1, 1 + NG), (2, 3), (NG - 1, NG)) if NG > 1 else ((1, 2), (2, 3), (0, 1))


# ---- case tables (plain data) ---------------------------------------------------------------------------------------------------
def _a_self(hi, head, explicit):
    """Explicit self rows and head cases run under 1.5 (under 2048 the logits grow by three orders of magnitude and ``max_prob``
    with them); the headless row-self cases alternate between the two scales."""
    return A_BIG if (not explicit and not head and hi % 2 == 0) else A_SMALL


# test_predict_rows_exact: (H, head, explicit self rows, int64 row pointers, alpha[G+1]); every H meets the four (HEAD, SELF_ROWS)
# pairs, the row-pointer type alternates so that each (LPR, HEAD, SELF_ROWS) instantiation meets both
PREDICT_CASES = [(H, bool(hd), bool(ex), bool((hi + hd + ex) % 2), _a_self(hi, hd, ex))
                 for hi, H in enumerate(H_ALL) for hd in (0, 1) for ex in (0, 1)]
# test_predict_rows_second_trip: (H, head, explicit, i64, alpha[G+1]) on 8192 + 9 rows
TRIP_ROWS = 8192 + 9
TRIP_CASES = [(H, bool(hd), bool((i + hd) % 2), bool((i + hd + 1) % 2), A_SMALL) for i, H in enumerate((12, 132)) for hd in (0, 1)]
TRIP_CASES += [(12, True, True, True, A_SMALL), (132, False, False, False, A_BIG)]
# test_head_limits: (H, C) at the LDS limit, and one class; refused one class over
HEAD_LIMIT_CASES = [(256, 64), (12, 1365), (64, 1), (12, 1)]
HEAD_REFUSED = [(256, 65), (12, 1366)]
# test_attrib_rows_exact: (H, i64, explicit self rows in head mode)
ATTRIB_CASES = [(H, bool(i64), bool((hi + i64) % 2)) for hi, H in enumerate(H_PER_LPR) for i64 in (0, 1)]
ATTRIB_TRIP_CASE = (132, True, False)
# test_derived_kernels_second_trip: (H, head, explicit) on 1024 + 6 rows (the draw and panel kernels launch one cell per block)
DERIVED_ROWS, DERIVED_G = 1024 + 6, 200
DERIVED_CASES = [(H, bool(hd), bool((i + hd) % 2)) for i, H in enumerate((32, 128)) for hd in (0, 1)]
# test_one_entry_is_seen: (row length, position, H, explicit, alpha[G+1])
SEEN_CASES = [(n, pos, H_PER_LPR[(i + j) % 5], bool((i + j) % 2), A_SMALL if (i + j) % 2 else A_BIG)
              for i, n in enumerate((LONG, 1025)) for j, pos in enumerate(("first", "last", "last_chunk"))]
# test_float_rows_within_bound: (H, i64, explicit)
FLOAT_LENGTHS = (64, 65, 128, 129, 1025)
FLOAT_CASES = [(H, bool(hi % 2), bool((hi + 1) % 2)) for hi, H in enumerate(H_PER_LPR)]
FLOAT_CLASSES = 16


def case_id(c):
    return "-".join(("H%d" % v if i == 0 else str(v)) if not isinstance(v, bool) else "01"[v] for i, v in enumerate(c))


# ---- batches ---------------------------------------------------------------------------------------------------------------------
def lattice_row(n, rng):
    """n positive integers with a power-of-two sum S >= 32."""
    S = max(32, 1 << int(np.ceil(np.log2(n))))
    base, extra = divmod(S, n)
    v = np.full(n, base, dtype=np.float64)
    v[rng.choice(n, extra, replace=False)] += 1
    assert v.sum() == S and v.min() >= 1
    return v


def lattice_batch(lengths, n_genes, seed):
    """CSR [len(lengths), n_genes] of lattice rows (sorted random gene ids)."""
    rng = np.random.default_rng(seed)
    indptr, idx, val = [0], [], []
    for n in lengths:
        idx.append(np.sort(rng.choice(n_genes, n, replace=False)))
        val.append(lattice_row(n, rng) if n else np.zeros(0))
        indptr.append(indptr[-1] + n)
    return sp.csr_matrix((np.concatenate(val), np.concatenate(idx).astype(np.int32), np.asarray(indptr, dtype=np.int64)),
                         shape=(len(lengths), n_genes))


MAIN_LENGTHS = LENGTHS + (0, LONG, 0) + (0,) * N_TIE_ROWS
ROW_LONG = len(LENGTHS) + 1
TIE_ROW0 = len(MAIN_LENGTHS) - N_TIE_ROWS
POW2_LENGTHS = (1, 3, 7, 15, 31, 63, 127, 0, 1, 63)


@functools.lru_cache(maxsize=None)
def main_batch():
    """The length list, two empty rows, the flat 4096 row, and the (empty) rows of the designed ties: 39 rows."""
    m = lattice_batch(MAIN_LENGTHS, G, 11)
    assert m.shape[0] >= 39 and (m[ROW_LONG].data == 1).all() and m[ROW_LONG].nnz == LONG
    return m


@functools.lru_cache(maxsize=None)
def trip_batch(pow2=False):
    """8192 + 9 rows of lengths 1 .. 7; past row 8192 one row of 65 entries and one empty row: a wave's second trip.  ``pow2`` (the
    head cases): lengths 1, 3 and 7 only - the logits of those rows are exact, near-ties among 8 201 rows are then ties or none."""
    lens = [(1, 3, 7)[(r * 5) % 3] if pow2 else 1 + (r * 5) % 7 for r in range(TRIP_ROWS)]
    lens[8192 + 3], lens[8192 + 6], lens[17] = 65, 0, 0
    return lattice_batch(lens, G, 12)


@functools.lru_cache(maxsize=None)
def pow2_batch():
    return lattice_batch(POW2_LENGTHS, G, 13)


@functools.lru_cache(maxsize=None)
def derived_batch():
    """1024 + 6 rows over 200 genes, lengths 0 .. 9 and one row of 65 past row 1024."""
    lens = [(r * 7) % 10 for r in range(DERIVED_ROWS)]
    lens[1024 + 2], lens[1024 + 4] = 65, 0
    return lattice_batch(lens, DERIVED_G, 14)


def seen_batches(n, pos):
    """(batch, changed batch, row, the two gene ids): one value of the row raised by 1 and another, under the same alpha, lowered by
    1 - S stays the same power of two.  ``pos``: the first entry, the last, or the first entry of the last 64-entry chunk."""
    lens = (5, n, 3)
    m = lattice_batch(lens, G, 15)
    alpha = operands(4, A_SMALL).alpha
    b = int(m.indptr[1])
    k = {"first": 0, "last": n - 1, "last_chunk": 64 * ((n - 1) // 64)}[pos]
    same = [j for j in range(n) if j != k and alpha[m.indices[b + j]] == alpha[m.indices[b + k]] and abs(j - k) > 70]
    j = same[len(same) // 2]
    moved = m.copy()
    moved.data[b + k] += 1
    moved.data[b + j] -= 1
    assert moved.data[b + j] >= 0 and moved[1].sum() == m[1].sum()
    return m, moved, 1, (int(m.indices[b + k]), int(m.indices[b + j]))


# ---- operands ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def operands(H, a_self, n_genes=G):
    """table [G, H], alpha [G + 2] with alpha[G+1] = a_self, bias [H]: ONE draw per width (alpha does not depend on the width)."""
    rng = np.random.default_rng(1000 + H)
    table = rng.choice((-1.0, 0.0, 1.0), (n_genes, H), p=(0.2, 0.6, 0.2))      # sparse enough for the flat long row's budget
    alpha = np.random.default_rng(99).choice((0.5, 1.0, 1.5), n_genes + 2)
    alpha[n_genes + 1] = a_self
    bias = rng.integers(-8, 9, H) / 4.0
    return SimpleNamespace(table=table, alpha=alpha, bias=bias, H=H, a_self=a_self)


def self_operand(H, B, seed=0):
    return np.random.default_rng(2000 + H + seed).integers(-4, 5, (B, H)) / 2.0


def head_operands(H, C, ties=True, sparse=False):
    """w_head [C, H] in {-1, 0, 1}, b_head [C] distinct multiples of 1/4 (below 5 in the main cases).  ``ties``: columns 0..2 carry ``tie_pairs(H)`` - w = 1 for the pair,
    -1 or 0 for everyone else, one b_head for every class of a pair.  ``sparse``: one non-zero per class (a wide head)."""
    rng = np.random.default_rng(3000 + 7 * H + C)
    w = rng.integers(-1, 2, (C, H)).astype(np.float64)
    if sparse:
        keep = np.zeros_like(w)
        keep[np.arange(C), rng.integers(0, H, C)] = 1.0
        w = np.where(keep > 0, np.where(w == 0, 1.0, w), 0.0)
    b = (rng.permutation(C) - C // 2) / 4.0                 # all different: classes with equal head rows do not tie
    if ties:
        assert C >= classes_for(H)
        for k, pair in enumerate(tie_pairs(H)):
            w[:, k] = rng.integers(-1, 1, C)
            w[list(pair), k] = 1.0
            b[list(pair)] = 0.5
    return w, b


def tie_self_rows(sr, o):
    """Explicit self rows of the designed-tie rows (the last ``N_TIE_ROWS`` of the main batch, all empty): row i has ONE positive
    column i, h_i = 1.5 * 6 + bias_i >= 7, every other column is clipped by the ReLU; the last row is h = 0."""
    assert o.a_self == A_SMALL and np.abs(o.bias).max() <= 2
    sr = sr.copy()
    sr[TIE_ROW0:] = -8.0
    for i in range(N_TIE_ROWS - 1):
        sr[TIE_ROW0 + i, i] = 6.0
    return sr


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _pow2_unit(*arrays):
    """The largest power of two dividing every given number (multiples of 2^-44 below 2^18), at most 1/4."""
    acc = np.int64(1) << 42
    for a in arrays:
        s = np.abs(np.asarray(a, dtype=np.float64)).ravel() * 2.0 ** 44
        i = s.astype(np.int64)
        assert np.array_equal(i.astype(np.float64), s), "an operand is off the 2^-44 grid"
        if i.size:
            acc = acc | np.bitwise_or.reduce(i)
    return float(acc & -acc) * 2.0 ** -44


def extra_roundings(deg):
    """``c`` of the float bound, from the kernel's code: the fp32 sum S (ceil(n / 64) lane-strided adds and a 6-step butterfly) and
    the self-row fma; the six roundings of the coefficient, the division ``1 / (deg + 1)`` and the final fma are
    ``oracle.agg_backward.K_ROUND`` = 8."""
    return np.ceil(np.asarray(deg) / 64.0) + 7


def reference(m, o, self_rows=None, head=None, lattice=True):
    """fp64 reference of ``wgnn_predict_rows`` on batch ``m`` (CSR, raw values), operands ``o`` (``operands``), ``self_rows``
    [B, H] or None, ``head = (w, b)`` or None.  ``lattice``: the operands are on the lattice - the budgets are computed per row,
    ``out`` is ``acc * float32(1 / (deg + 1)) + bias`` computed exactly and rounded ONCE to fp32, and ``S + 1e-6f`` is S as it is in
    fp32; otherwise everything is plain fp64 (``S + 1e-6``, ``1 / (deg + 1)``)."""
    m = sp.csr_matrix(m).astype(np.float64)
    B, n_genes = m.shape
    H = o.H
    deg = np.diff(m.indptr).astype(np.float64)
    S = np.asarray(m.sum(axis=1)).ravel()
    rows = np.repeat(np.arange(B), np.diff(m.indptr))
    x, a = m.data, o.alpha
    if lattice:
        nz = deg > 0
        assert (S[nz] >= 32).all() and (np.log2(S[nz]) % 1 == 0).all()
        assert np.array_equal((S.astype(np.float32) + np.float32(1e-6))[nz], S.astype(np.float32)[nz])
    w = a[m.indices] * (deg[rows] * x / S[rows])
    if self_rows is None:
        w = w + x * (a[n_genes + 1] / (S[rows] if lattice else S[rows] + 1e-6))
    M = sp.csr_matrix((w, m.indices, m.indptr), shape=m.shape)
    acc = M @ o.table
    abs_acc = abs(M) @ np.abs(o.table)
    if self_rows is not None:
        acc = acc + a[n_genes + 1] * self_rows
        abs_acc = abs_acc + np.abs(a[n_genes + 1] * self_rows)
    R = SimpleNamespace(B=B, H=H, deg=deg, S=S, w=w, acc=acc, abs_acc=abs_acc, n_terms=deg + (self_rows is not None))
    pow2 = (deg + 1 <= 128) & (np.log2(deg + 1) % 1 == 0)
    if lattice:
        assert np.array_equal(w.astype(np.float32).astype(np.float64), w), "a weight is not an fp32 number"
        unit = np.empty(B)
        for r in range(B):
            unit[r] = _pow2_unit(w[m.indptr[r]:m.indptr[r + 1]], [] if self_rows is None else a[n_genes + 1] * self_rows[r])
        R.unit = unit
        R.budget = abs_acc.max(axis=1) / unit / AB.EXACT_LIMIT
        R.exact_rows = R.budget < 1.0
        invd = (np.float32(1) / (deg + 1).astype(np.float32)).astype(np.float64)
        z = acc * invd[:, None] + o.bias
        # the product of two 24-bit numbers (48 bits) plus a multiple of 1/4 below 4: at most 52 bits wide (profiles/resident_rows_parity.md
        # has the argument) - shown here against the 64-bit significand of the long double
        ld = np.longdouble
        if np.finfo(ld).nmant >= 63:
            z_wide = acc.astype(ld) * invd.astype(ld)[:, None] + o.bias.astype(ld)
            assert np.array_equal(z.astype(ld)[R.exact_rows], z_wide[R.exact_rows]), "acc * invd + bias does not fit fp64"
        R.invd = invd
        R.z = z
        h = np.maximum(z.astype(np.float32), np.float32(0)).astype(np.float64)              # ONE rounding, then ReLU
    else:
        R.exact_rows = np.zeros(B, dtype=bool)
        R.invd = 1.0 / (deg + 1)
        R.z = z = acc * R.invd[:, None] + o.bias
        h = np.maximum(z, 0.0)
    R.out = h
    R.abs_out = abs_acc * R.invd[:, None] + np.abs(o.bias)
    R.out_bound = AB.float_bound(R.abs_out, (R.n_terms + extra_roundings(deg))[:, None])
    R.out_bound[R.exact_rows] = 0.0
    R.pow2_rows = pow2 & R.exact_rows
    if head is None:
        return R
    wh, bh = head
    C = wh.shape[0]
    R.C = C
    R.logits = h @ wh.T + bh
    R.abs_logits = np.abs(h) @ np.abs(wh).T + np.abs(bh)
    # logit error: what the error of h carries over, plus an fp32 dot of H terms and the add of b_head
    R.logit_bound = R.out_bound @ np.abs(wh).T + AB.float_bound(R.abs_logits, H + 1)
    if lattice:
        R.exact_logit_rows = R.pow2_rows.copy()
        R.logit_budget = np.zeros(B)
        for r in np.flatnonzero(R.pow2_rows):
            assert np.array_equal(z[r].astype(np.float32).astype(np.float64), z[r]), "h is not exact on a power-of-two row"
            u = _pow2_unit(h[r], bh)
            R.logit_budget[r] = R.abs_logits[r].max() / u / AB.EXACT_LIMIT
        R.logit_bound[R.exact_logit_rows] = 0.0
    else:
        R.exact_logit_rows = np.zeros(B, dtype=bool)
    R.argmax = R.logits.argmax(axis=1)                                  # numpy: the first, i.e. lowest, index among equal maxima
    srt = np.sort(R.logits, axis=1)
    R.gap = srt[:, -1] - srt[:, -2] if C > 1 else np.full(B, np.inf)
    e = np.exp(R.logits - srt[:, -1:])
    R.max_prob = 1.0 / e.sum(axis=1)
    # relative: C calls of expf (EXPF_ULP ulp = 2 * 2^-24 each, on terms <= 1 of a sum >= 1), C adds, one division, and what an
    # error of the logits moves the exponents by (twice the worst logit bound of the row)
    R.expf_bound = R.max_prob * (C * 2 * EXPF_ULP + C + 2) * 2.0 ** -24
    R.max_prob_bound = R.expf_bound + R.max_prob * 2 * R.logit_bound.max(axis=1)
    return R


def place_threshold(R):
    """``unsure_threshold`` as an fp32 number in the middle of the LARGEST gap of the reference's sorted ``max_prob``; returns
    ``(thr, gap)``.  The caller asserts that the gap exceeds twice the bound of every row."""
    p = np.sort(R.max_prob)
    i = int(np.argmax(np.diff(p)))
    thr = float(np.float32((p[i] + p[i + 1]) / 2))
    return thr, float(p[i + 1] - p[i])


def labels(R, thr):
    return np.where(R.max_prob < thr, -1, R.argmax).astype(np.int32)


def label_rows_fair(R):
    """Per row: the reference's arg max is what an fp32 kernel within the logit bound must find - the top-two gap exceeds twice the
    bound, or the logits of the row are exact (then equal maxima are resolved by the tie rule: the lowest index)."""
    worst = R.logit_bound.max(axis=1)
    return R.exact_logit_rows | (R.gap > 2 * worst)


def clear_rows(R, thr):
    """The float group's rows whose label is compared: the fp64 top-two gap exceeds twice the logit bound and ``max_prob`` is
    further from the threshold than its bound."""
    return (R.gap > 2 * R.logit_bound.max(axis=1)) & (np.abs(R.max_prob - thr) > R.max_prob_bound)


# ---- case builders (shared by the CPU and the GPU file) ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def predict_case(H, head, explicit, a_self, batch="main"):
    m = trip_batch(head) if batch == "trip" else {"main": main_batch, "pow2": pow2_batch}[batch]()
    o = operands(H, a_self)
    sr = None
    if explicit:
        sr = self_operand(H, m.shape[0])
        if batch == "main":
            sr = tie_self_rows(sr, o)
    C = classes_for(H) if batch == "main" else 5
    hd = head_operands(H, C, ties=batch == "main") if head else None
    R = reference(m, o, sr, hd)
    return SimpleNamespace(m=m, o=o, self_rows=sr, head=hd, R=R, H=H, explicit=explicit, batch=batch)


def head_limit_case(H, C):
    m = pow2_batch()
    o = operands(H, A_SMALL)
    sr = self_operand(H, m.shape[0])
    hd = head_operands(H, C, ties=False, sparse=C > 64)
    return SimpleNamespace(m=m, o=o, self_rows=sr, head=hd, R=reference(m, o, sr, hd), H=H, explicit=True, batch="pow2")


def attrib_reference(c, target, direction=None, explicit_self=None, prior=None):
    """fp64 reference of ``wgnn_attrib_rows`` on case ``c`` (``predict_case``): per entry ``score = (w / (deg + 1)) <table[g], v>``,
    per row ``base`` and ``v``.  Head mode: ``v = (h > 0) * w_head[target]``, ``base = b_head[t] + <v, bias>``.  Direction mode:
    ``v = direction``, the coefficient without the self term under ``explicit_self``; ``prior``: scores added to."""
    m, o, R = c.m, c.o, c.R
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    if direction is None:
        wh, bh = c.head
        v = (R.out > 0) * wh[target]
        base = bh[target] + v @ o.bias
        w = R.w
    else:
        v, base = direction, None
        w = o.alpha[m.indices] * (R.deg[rows] * m.data / R.S[rows])
        if not explicit_self:
            w = w + m.data * (o.alpha[m.shape[1] + 1] / R.S[rows])
    coef = w * R.invd[rows]
    dot = np.einsum("ij,ij->i", o.table[m.indices], v[rows])
    score = coef * dot + (0.0 if prior is None else prior)
    abs_score = np.abs(coef) * np.einsum("ij,ij->i", np.abs(o.table[m.indices]), np.abs(v[rows])) + (0.0 if prior is None else np.abs(prior))
    return SimpleNamespace(score=score, abs_score=abs_score, coef=coef, v=v, base=base, entry_rows=rows,
                           exact_entries=R.pow2_rows[rows])


@functools.lru_cache(maxsize=None)
def float_case(H, i64, explicit):
    """The float group: the random ragged batch of test_gpu_resident_predict.py (two empty rows, one row of 5000 entries, lengths
    below 300) with rows of 64, 65, 128, 129 and 1025 entries put in, ordinary float operands rounded to fp32, a 16-class head."""
    from test_gpu_resident_predict import _ragged_batch
    rng = np.random.default_rng(500 + H)
    m = _ragged_batch(rng, 40, G).tolil()
    for r, n in zip((5, 6, 7, 8, 9), FLOAT_LENGTHS):
        m[r] = 0
        cols = np.sort(rng.choice(G, n, replace=False))
        m[r, cols] = np.clip(rng.normal(3.0, 1.0, n), 0.2, 7.0)
    m = sp.csr_matrix(m.tocsr().astype(np.float32))
    m.eliminate_zeros()
    assert tuple(np.diff(m.indptr)[5:10]) == FLOAT_LENGTHS
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    o = SimpleNamespace(table=f32(0.5 * rng.standard_normal((G, H))), alpha=f32(rng.uniform(0.5, 1.5, G + 2)),
                        bias=f32(0.1 * rng.standard_normal(H)), H=H, a_self=None)
    sr = f32(0.5 * rng.standard_normal((40, H))) if explicit else None
    hd = (f32(rng.standard_normal((FLOAT_CLASSES, H)) / np.sqrt(H)), f32(0.1 * rng.standard_normal(FLOAT_CLASSES)))
    return SimpleNamespace(m=m, o=o, self_rows=sr, head=hd, R=reference(m, o, sr, hd, lattice=False), H=H, explicit=explicit,
                           batch="float")
