"""The resident row kernels - ``wgnn_predict_rows``, ``wgnn_attrib_rows`` and, through them, the draw / thin / panel kernels that
restate their gather - against the fp64 reference of ``tests/resident_rows_lattice.py``, with the harness of
``tests/test_gpu_backward_ops.py`` (guards, exact comparison and ratios are imported).

Two groups, as in the aggregation files:

* **exact** - operands on the lattice of ``resident_rows_lattice``: ``out``, ``logits`` (rows whose ``deg + 1`` is a power of two up
  to 128), ``label`` (EVERY row), the attribution scores, ``base`` and direction must equal the reference BIT FOR BIT; every case
  runs twice (determinism).  That each demand is fair for every tuple of the case tables is checked without a GPU in
  ``tests/test_resident_rows_lattice_reference.py``.
* **float** - ordinary floats; per element ``float_bound(sum|terms|, n_terms + c)`` from the reference, ``c`` = the extra roundings
  ``resident_rows_lattice.extra_roundings`` counts in the kernel's code; no measured constant.  ``max_prob`` goes through ``expf``
  and is held to ``max_prob_bound`` in both groups.  Every bounded comparison prints ``RATIO``.

Outputs of the entries under test are inner views of SENTINEL-filled tensors holding FILL; ``table``, ``self_rows`` and the
direction have ``ld > H`` with NaN in the pad columns.  ``profiles/resident_rows_parity.md`` maps options to tests."""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import resident_rows_lattice as L
import test_gpu_backward_ops as GB
from oracle import agg_backward as AB
from scdeepsort_amd import _lib, ops
from scdeepsort_amd.graph import _ptr, _stream
from test_gpu_backward_ops import assert_exact, guarded, guards_intact, record_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL, IFILL, IGUARD = -777.0, -5, -7
ERR_UNSUPPORTED = -3                                        # include/wgnn.h WGNN_ERR_UNSUPPORTED


# ---- device side -------------------------------------------------------------------------------------------------------------------
def dev(x, dtype=torch.float32):
    return GB.dev(x, dtype)


def nan_padded(x, pad=4):
    """``x`` [n, D] as the inner columns of a NaN-filled [n, D + 2 * pad] tensor (ld > D, 16-byte aligned rows)."""
    x = dev(x)
    whole = torch.full((x.shape[0], x.shape[1] + 2 * pad), float("nan"), device=DEV)
    view = whole[:, pad:pad + x.shape[1]]
    view.copy_(x)
    return view


def device_csr(m, i64):
    return (dev(m.indptr, torch.int64 if i64 else torch.int32), dev(m.indices, torch.int32), dev(m.data))


def fresh(n, D=None, pad=0):
    return guarded(np.full((n,) if D is None else (n, D), FILL), pad)


def fresh_i32(n):
    whole = torch.full((n + 8,), IGUARD, dtype=torch.int32, device=DEV)
    whole[4:4 + n] = IFILL
    return whole, whole[4:4 + n]


def i32_guard_intact(whole, n):
    return bool((whole[:4] == IGUARD).all()) and bool((whole[4 + n:] == IGUARD).all())


def device_operands(c, i64):
    """The inputs of a case on the device: table and self rows inside NaN columns."""
    m, o = c.m, c.o
    T = SimpleNamespace(B=m.shape[0], G=m.shape[1], H=c.H, csr=device_csr(m, i64), table=nan_padded(o.table), alpha=dev(o.alpha),
                        bias=dev(o.bias), self_rows=None if c.self_rows is None else nan_padded(c.self_rows),
                        flags=_lib.FLAG_ROWPTR_I64 if i64 else 0, head=None)
    if c.head is not None:
        T.head = (dev(c.head[0]), dev(c.head[1]))
    assert T.table.stride(0) > c.H and (T.self_rows is None or T.self_rows.stride(0) > c.H)
    return T


def lead_args(T):
    rp, col, raw = T.csr
    return (_ptr(rp), _ptr(col), _ptr(raw), T.B, _ptr(T.table), T.table.stride(0), T.G, T.H, _ptr(T.alpha), _ptr(T.bias),
            _ptr(T.self_rows), T.self_rows.stride(0) if T.self_rows is not None else 0)


def launch_predict(T, thr=0.0, rc_only=False):
    """``wgnn_predict_rows`` through the C ABI into guarded FILL-holding views: ``out`` with ``ld_out > H``, or ``logits`` with
    ``ld_logits > C``, ``label`` and ``max_prob``.  Checks the guards and that nothing was skipped or holds a NaN."""
    d = torch.device(DEV)
    got = SimpleNamespace()
    if T.head is None:
        whole, got.out = fresh(T.B, T.H, 4)
        assert got.out.stride(0) > T.H
        rc = _lib.call(d, "wgnn_predict_rows", *lead_args(T), _ptr(got.out), got.out.stride(0), None, None, 0, 0.0, None, 0, None,
                       None, T.flags, _stream(d))
        _lib.check(rc, "wgnn_predict_rows")
        torch.cuda.synchronize()
        assert guards_intact(whole, got.out), "out: a guard row / column was written"
        assert not bool((got.out == FILL).any()) and not bool(torch.isnan(got.out).any()), "out: an element was skipped or is NaN"
        return got
    w, b = T.head
    C = w.shape[0]
    lw, got.logits = fresh(T.B, C, 4)
    pw, got.max_prob = fresh(T.B)
    iw, got.label = fresh_i32(T.B)
    assert got.logits.stride(0) > C
    rc = _lib.call(d, "wgnn_predict_rows", *lead_args(T), None, 0, _ptr(w), _ptr(b), C, float(thr), _ptr(got.logits),
                   got.logits.stride(0), _ptr(got.label), _ptr(got.max_prob), T.flags, _stream(d))
    if rc_only:
        return rc
    _lib.check(rc, "wgnn_predict_rows")
    torch.cuda.synchronize()
    assert guards_intact(lw, got.logits) and guards_intact(pw, got.max_prob) and i32_guard_intact(iw, T.B), "a guard was written"
    for name in ("logits", "max_prob"):
        v = getattr(got, name)
        assert not bool((v == FILL).any()) and not bool(torch.isnan(v).any()), f"{name}: an element was skipped or is NaN"
    assert not bool((got.label == IFILL).any()), "label: a row was skipped"
    return got


def rows_exact_or_bounded(entry, what, got, want, exact_rows, bound):
    """Bit for bit on ``exact_rows``; the other rows (none in the lattice cases as they stand) within the reference's bound."""
    ex = torch.from_numpy(np.flatnonzero(exact_rows))
    assert_exact(got.cpu()[ex], want[exact_rows], f"{entry} {what}")
    if not exact_rows.all():
        rest = ~exact_rows
        record_ratio(entry, what, got.cpu()[torch.from_numpy(np.flatnonzero(rest))], want[rest], bound[rest])


def check_predict(entry, c, got, thr):
    R = c.R
    if c.head is None:
        rows_exact_or_bounded(entry, "out", got.out, R.out, R.exact_rows, R.out_bound)
        return
    rows_exact_or_bounded(entry, "logits", got.logits, R.logits, R.exact_logit_rows, R.logit_bound)
    want = torch.from_numpy(L.labels(R, thr))
    bad = (got.label.cpu() != want).nonzero().ravel().tolist()
    assert not bad, f"{entry} label: rows {bad[:8]} differ: got {got.label.cpu()[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}"
    record_ratio(entry, "max_prob", got.max_prob, R.max_prob, R.max_prob_bound)


def run_predict_case(entry, c, i64):
    """Twice at the threshold in the largest ``max_prob`` gap (same bits), once at threshold 0 (the arg max of every row, the
    designed ties among them, is then the label)."""
    T = device_operands(c, i64)
    if c.head is None:
        a, b = launch_predict(T), launch_predict(T)
        check_predict(entry, c, a, 0.0)
        assert torch.equal(a.out, b.out)
        return a
    thr, gap = L.place_threshold(c.R) if c.R.B > 1 and c.R.C > 1 else (0.0, np.inf)
    assert gap > 2 * c.R.expf_bound.max() and (np.abs(c.R.max_prob - thr) > c.R.max_prob_bound).all()
    a, b = launch_predict(T, thr), launch_predict(T, thr)
    check_predict(entry, c, a, thr)
    assert torch.equal(a.logits, b.logits) and torch.equal(a.label, b.label) and torch.equal(a.max_prob, b.max_prob)
    z = launch_predict(T, 0.0)
    check_predict(entry, c, z, 0.0)
    assert bool((z.label >= 0).all()) and torch.equal(z.logits, a.logits)
    return z


# ---- 1. predict_rows, every instantiation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.PREDICT_CASES, ids=L.case_id)
def test_predict_rows_exact(case):
    """Both edges of every LPR branch x head / no head x explicit / row self x int32 / int64 row pointers on the length list, two
    empty rows, the flat 4096 row and the designed-tie rows; every output a guarded view with ``ld > `` its width."""
    H, head, explicit, i64, a_self = case
    c = L.predict_case(H, head, explicit, a_self)
    got = run_predict_case("predict_rows", c, i64)
    if head and explicit:                                    # the designed ties: the lower class of each pair
        for i, (ja, jb) in enumerate(L.tie_pairs(H)):
            r = L.TIE_ROW0 + i
            assert float(got.logits[r, ja]) == float(got.logits[r, jb]) == float(got.logits[r].max())
            assert int(got.label[r]) == ja
    if head:                                                 # every logit equal on every row: class 0, max_prob = 1 / C
        T = device_operands(c, i64)
        C = c.head[0].shape[0]
        T.head = (torch.zeros((C, H), device=DEV), torch.full((C,), 0.75, device=DEV))
        flat = launch_predict(T, 0.0)
        assert bool((flat.label == 0).all()) and bool((flat.logits == 0.75).all())
        bound = np.full(T.B, (C * 2 * L.EXPF_ULP + C + 2) * 2.0 ** -24 / C)
        record_ratio("predict_rows/flat", "max_prob", flat.max_prob, np.full(T.B, 1.0 / C), bound)


# ---- 2. the grid-stride loop's second trip ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.TRIP_CASES, ids=L.case_id)
def test_predict_rows_second_trip(case):
    """8192 + 9 rows: rows from 8192 on are a wave's second trip (the LDS head image used again, ``r * ld`` beyond one grid)."""
    H, head, explicit, i64, a_self = case
    c = L.predict_case(H, head, explicit, a_self, "trip")
    assert c.m.shape[0] == L.TRIP_ROWS
    run_predict_case("predict_rows/trip", c, i64)


# ---- 3. the head's limits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.HEAD_LIMIT_CASES, ids=L.case_id)
def test_head_limits(case):
    """``C * H * 4`` = 64 KiB exactly (C = 64 at H = 256, C = 1365 at H = 12, a sparse head) and C = 1; one class more is refused."""
    H, C = case
    c = L.head_limit_case(H, C)
    assert c.R.exact_logit_rows.all()
    got = run_predict_case("predict_rows/limits", c, bool(C % 2))
    if C == 1:
        assert bool((got.label == 0).all()) and bool((got.max_prob == 1.0).all())
    for Hr, Cr in L.HEAD_REFUSED:
        if Hr != H or C == 1:
            continue
        T = device_operands(c, False)
        T.head = (torch.zeros((Cr, H), device=DEV), torch.zeros(Cr, device=DEV))
        assert launch_predict(T, 0.0, rc_only=True) == ERR_UNSUPPORTED


# ---- 4. attrib_rows ------------------------------------------------------------------------------------------------------------------------
def launch_attrib(T, nnz, *, thr=0.0, direction=None, explicit_self=False, prior=None):
    """``wgnn_attrib_rows`` through the C ABI; ``score`` (and ``dir_out`` with ``ld > H``) guarded.  Head mode unless ``direction``."""
    d = torch.device(DEV)
    got = SimpleNamespace()
    sw, got.score = guarded(np.full(nnz, FILL) if prior is None else prior)
    if direction is None:
        w, b = T.head
        tw, got.target = fresh_i32(T.B)
        iw, got.label = fresh_i32(T.B)
        gw, got.logit = fresh(T.B)
        bw, got.base = fresh(T.B)
        dw, got.dir = fresh(T.B, T.H, 4)
        rc = _lib.call(d, "wgnn_attrib_rows", *lead_args(T), _ptr(w), _ptr(b), w.shape[0], None, float(thr), _ptr(got.label), None, 0,
                       _ptr(got.score), _ptr(got.target), _ptr(got.logit), _ptr(got.base), _ptr(got.dir), got.dir.stride(0), T.flags,
                       _stream(d))
        _lib.check(rc, "wgnn_attrib_rows")
        torch.cuda.synchronize()
        assert guards_intact(gw, got.logit) and guards_intact(bw, got.base) and guards_intact(dw, got.dir)
        assert i32_guard_intact(tw, T.B) and i32_guard_intact(iw, T.B)
        assert not bool((got.dir == FILL).any()) and not bool((got.target == IFILL).any()) and not bool((got.label == IFILL).any())
    else:
        flags = T.flags | (_lib.ATTRIB_EXPLICIT_SELF if explicit_self else 0) | (_lib.ATTRIB_ACCUMULATE if prior is not None else 0)
        lead = lead_args(T)[:9] + (None, None, 0)
        rc = _lib.call(d, "wgnn_attrib_rows", *lead, None, None, 0, None, 0.0, None, _ptr(direction), direction.stride(0),
                       _ptr(got.score), None, None, None, None, 0, flags, _stream(d))
        _lib.check(rc, "wgnn_attrib_rows")
        torch.cuda.synchronize()
    assert guards_intact(sw, got.score), "score: a guard element was written"
    assert not bool(torch.isnan(got.score).any()) and (prior is not None or not bool((got.score == FILL).any()))
    return got


def check_scores(entry, got, A):
    ex = A.exact_entries
    assert_exact(got.score.cpu()[torch.from_numpy(np.flatnonzero(ex))], A.score[ex], f"{entry} score")
    if not ex.all():                                         # w * invd rounds where deg + 1 is no power of two
        rest = torch.from_numpy(np.flatnonzero(~ex))
        record_ratio(entry, "score", got.score.cpu()[rest], A.score[~ex], AB.float_bound(A.abs_score[~ex], 0))


def run_attrib_case(entry, H, i64, explicit, batch):
    c = L.predict_case(H, True, explicit, L.A_SMALL, batch)
    R, nnz = c.R, c.m.nnz
    T = device_operands(c, i64)
    thr, _ = L.place_threshold(R)
    p = launch_predict(T, thr)
    check_predict(entry + "/predict", c, p, thr)
    # head mode: the bits of predict_rows, and base / direction / score against fp64
    a, a2 = launch_attrib(T, nnz, thr=thr), launch_attrib(T, nnz, thr=thr)
    assert all(torch.equal(getattr(a, k), getattr(a2, k)) for k in ("score", "target", "label", "logit", "base", "dir"))
    assert torch.equal(a.label, p.label)
    assert torch.equal(a.target.cpu(), torch.from_numpy(R.argmax.astype(np.int32)))
    assert torch.equal(a.logit, p.logits.gather(1, a.target.long()[:, None]).ravel())
    A = L.attrib_reference(c, R.argmax)
    assert_exact(a.base, A.base, f"{entry} base")
    assert_exact(a.dir, A.v, f"{entry} dir_out")
    check_scores(entry, a, A)
    # direction mode: a lattice direction with ld > H, both coefficient rules, overwrite and accumulate
    rng = np.random.default_rng(H)
    direction = rng.integers(-1, 2, (c.m.shape[0], H)).astype(np.float64)
    prior = rng.integers(-4, 5, nnz).astype(np.float64)
    dirv = nan_padded(direction)
    for es in (False, True):
        check_scores(f"{entry}/dir", launch_attrib(T, nnz, direction=dirv, explicit_self=es), L.attrib_reference(c, None, direction, es))
        acc = launch_attrib(T, nnz, direction=dirv, explicit_self=es, prior=prior)
        check_scores(f"{entry}/dir+acc", acc, L.attrib_reference(c, None, direction, es, prior))


@pytest.mark.parametrize("case", L.ATTRIB_CASES, ids=L.case_id)
def test_attrib_rows_exact(case):
    """One H per LPR x both row-pointer types on the main batch: head mode carries ``predict_rows``' bits (target, logit, label) and
    equals fp64 in ``base``, ``dir_out`` and - on the power-of-two rows bit for bit - ``score``; direction mode with and without
    WGNN_ATTRIB_EXPLICIT_SELF, overwriting and under WGNN_ATTRIB_ACCUMULATE on a lattice score."""
    H, i64, explicit = case
    run_attrib_case("attrib_rows", H, i64, explicit, "main")


def test_attrib_rows_second_trip():
    H, i64, explicit = L.ATTRIB_TRIP_CASE
    run_attrib_case("attrib_rows/trip", H, i64, explicit, "trip")


# ---- 5. the kernels that restate the gather, on their second trip --------------------------------------------------------------------------
def derived_case(H, head, explicit):
    m = L.derived_batch()
    o = L.operands(H, L.A_SMALL, L.DERIVED_G)
    sr = L.self_operand(H, m.shape[0]) if explicit else None
    hd = L.head_operands(H, 5, ties=False) if head else None
    return SimpleNamespace(m=m, o=o, self_rows=sr, head=hd, R=L.reference(m, o, sr, hd), H=H, explicit=explicit, batch="derived")


@pytest.mark.parametrize("case", L.DERIVED_CASES, ids=L.case_id)
def test_derived_kernels_second_trip(case):
    """1024 + 6 cells (the draw and panel kernels launch at most 1024 blocks of one cell): ``predict_rows_dropout(keep=1, n_draws=2)``
    and ``predict_rows_panels`` (an all-genes panel and a half panel) carry the bits of ``predict_rows`` - which is pinned to fp64
    on this very batch first - at H = 32 and H = 128; ``predict_rows_thin(keep=1)`` those of the lognorm-aligned count batch."""
    H, head, explicit = case
    c = derived_case(H, head, explicit)
    m, B = c.m, c.m.shape[0]
    assert B == L.DERIVED_ROWS
    csr = device_csr(m, False)
    table, alpha, bias = dev(c.o.table), dev(c.o.alpha), dev(c.o.bias)
    sr = None if c.self_rows is None else dev(c.self_rows)
    sr2 = None if sr is None else sr.repeat_interleave(2, dim=0)
    hd = None if not head else (dev(c.head[0]), dev(c.head[1]))
    thr = L.place_threshold(c.R)[0] if head else 0.0
    kw = dict(head=hd, unsure_threshold=thr) if head else {}
    base = ops.predict_rows(*csr, table, alpha, bias, self_rows=sr, **kw)
    if head:
        assert_exact(base[0][torch.from_numpy(np.flatnonzero(c.R.exact_logit_rows)).to(DEV)], c.R.logits[c.R.exact_logit_rows], "logits")
        fair = torch.from_numpy(L.label_rows_fair(c.R) & (np.abs(c.R.max_prob - thr) > c.R.max_prob_bound))    # (1 030 rows, 5 classes)
        assert torch.equal(base[1].cpu()[fair], torch.from_numpy(L.labels(c.R, thr))[fair]) and fair.float().mean() > 0.9
    else:
        assert c.R.exact_rows.all()
        assert_exact(base, c.R.out, "out")
    # gene dropout at keep = 1, two draws
    drop = ops.predict_rows_dropout(*csr, table, alpha, bias, self_rows=sr2, n_draws=2, keep=1.0, seed=5, want_draws=head, **kw)
    if head:
        assert torch.equal(drop[4], base[1][:, None].expand(B, 2)) and torch.equal(drop[5], base[2][:, None].expand(B, 2))
    else:
        assert torch.equal(drop.view(B, 2, H), base[:, None, :].expand(B, 2, H))
    # panels: every gene, and the even genes (the bits of predict_rows on the sub-batch)
    even = np.arange(L.DERIVED_G) % 2 == 0
    member = dev(np.where(even, 3, 1), torch.int64)
    keep = even[m.indices]
    rows = np.repeat(np.arange(B), np.diff(m.indptr))
    sub = sp.csr_matrix((m.data[keep], (rows[keep], m.indices[keep])), shape=m.shape)
    sub_out = ops.predict_rows(*device_csr(sub, False), table, alpha, bias, self_rows=sr, **kw)
    pan = ops.predict_rows_panels(*csr, table, alpha, bias, member, 2, self_rows=sr2, want_logits=True, **kw) if head else \
        ops.predict_rows_panels(*csr, table, alpha, bias, member, 2, self_rows=sr2)
    if head:
        C = hd[0].shape[0]
        assert torch.equal(pan[0].view(B, 2, C)[:, 0], base[0]) and torch.equal(pan[0].view(B, 2, C)[:, 1], sub_out[0])
        assert torch.equal(pan[1][:, 0], base[1]) and torch.equal(pan[1][:, 1], sub_out[1])
        assert torch.equal(pan[2][:, 0], base[2]) and torch.equal(pan[2][:, 1], sub_out[2])
    else:
        assert torch.equal(pan.view(B, 2, H)[:, 0], base) and torch.equal(pan.view(B, 2, H)[:, 1], sub_out)
    if H != 32:
        return
    # read thinning at keep = 1: the lattice values as counts, log-normalised on the device
    x = np.zeros((B, L.DERIVED_G + 1), np.float32)
    x[rows, m.indices] = m.data
    gene_map = dev(np.concatenate([np.arange(L.DERIVED_G), [-1]]), torch.int32)
    rp, col, raw = ops.align_rows(dev(x), gene_map, L.DERIVED_G, 0.0, normalize="lognorm", scale=1e4)
    want = ops.predict_rows(rp, col, raw, table, alpha, bias, self_rows=sr, **kw)
    thin = ops.predict_rows_thin(*csr, table, alpha, bias, rest=torch.zeros(B, dtype=torch.int64, device=DEV), scale=1e4, self_rows=sr,
                                 n_draws=1, keep=1.0, seed=3, want_draws=head, **kw)
    if head:
        assert torch.equal(thin[4][:, 0], want[1]) and torch.equal(thin[5][:, 0], want[2])
    else:
        assert torch.equal(thin, want)


# ---- 6. one entry of a long row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.SEEN_CASES, ids=L.case_id)
def test_one_entry_is_seen(case):
    """One value of the flat 4096 row / of a 1025 row raised by 1 and another lowered by 1 (S unchanged): the output equals the
    reference of the changed batch bit for bit and differs from the unchanged output in every column where the two table rows do."""
    n, pos, H, explicit, a_self = case
    m, moved, row, (ga, gb) = L.seen_batches(n, pos)
    o = L.operands(H, a_self)
    o = SimpleNamespace(**{**vars(o), "bias": np.full(H, 4.0)})          # keeps the ReLU out of the changed row's way
    sr = L.self_operand(H, 3) if explicit else None
    outs = []
    for batch in (m, moved):
        c = SimpleNamespace(m=batch, o=o, self_rows=sr, head=None, R=L.reference(batch, o, sr), H=H)
        assert c.R.exact_rows.all()
        got = launch_predict(device_operands(c, n == 1025))
        assert_exact(got.out, c.R.out, "out")
        outs.append(got.out.cpu())
    differ = torch.from_numpy(o.table[ga] != o.table[gb])
    assert bool(differ.any()) and torch.equal(outs[0][row] != outs[1][row], differ)
    assert torch.equal(outs[0][[0, 2]], outs[1][[0, 2]])


# ---- 7. float group --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.FLOAT_CASES, ids=L.case_id)
def test_float_rows_within_bound(case):
    """Ordinary floats: the random ragged batch of test_gpu_resident_predict.py with rows of 64, 65, 128, 129 and 1025 entries, one H
    per LPR, head on.  ``out`` and ``logits`` per element within ``float_bound(sum|terms|, n_terms + c)`` (c: see
    ``resident_rows_lattice.extra_roundings``), ``max_prob`` within its bound, labels on the rows whose fp64 gap exceeds twice the
    logit bound and whose ``max_prob`` is further from the threshold than its bound - at least 90 % of the rows."""
    H, i64, explicit = case
    c = L.float_case(H, i64, explicit)
    R = c.R
    T = device_operands(c, i64)
    thr, _ = L.place_threshold(R)
    got = launch_predict(T, thr)
    record_ratio("predict_rows/float", "logits", got.logits, R.logits, R.logit_bound)
    record_ratio("predict_rows/float", "max_prob", got.max_prob, R.max_prob, R.max_prob_bound)
    clear = L.clear_rows(R, thr)
    print(f"SHARE H={H} rows compared on their label: {clear.mean():.3f}")
    assert clear.mean() >= 0.9
    assert torch.equal(got.label.cpu()[torch.from_numpy(clear)], torch.from_numpy(L.labels(R, thr))[torch.from_numpy(clear)])
    T.head = None
    record_ratio("predict_rows/float", "out", launch_predict(T).out, R.out, R.out_bound)
