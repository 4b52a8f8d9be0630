"""Log-normalising alignment on the GPU: ``wgnn_align_count_ln`` / ``wgnn_align_fill_ln``
(``ops.align_rows(..., normalize="lognorm")``) against the fp64 restatement of tests/lognorm_reference.py, and ``normalize=``
through ``ResidentPredictor``.  Structure is ``array_equal``; values are compared as float32 BIT PATTERNS - equal wherever the
fp64 reference value is not within 16 fp64 ulps of a float32 rounding midpoint (``fragile``), one float32 ulp there - so an
evaluation in float32, or over a float32 total, does not pass.  The wiring tests have no tolerance at all."""
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import api, ops

import align_reference as A
import lognorm_reference as L
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 100          # count_case(SEED + n_cols, ...): the preconditions below hold for these draws


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _strided(x, ld):
    """``x`` on the device as a [B, n_cols] view of rows ``ld`` elements apart, NaN between the rows."""
    B, n = x.shape
    buf = torch.full((max(B * ld - (ld - n), 0),), float("nan"), dtype=torch.float32, device=DEV)
    view = torch.as_strided(buf, (B, n), (ld, 1))
    view.copy_(t(x))
    return view


@lru_cache(maxsize=None)
def _case(B, n_cols, G, thr):
    """One count case per shape and threshold, its reference (computed once, never modified) and the preconditions that are
    asserted on the reference alone."""
    c = L.count_case(SEED + n_cols, B, n_cols, G, thr)
    want = L.lognorm_dense(c.x, c.gene_map, thr, fp64=True)
    every = L.lognorm_dense(c.x, c.gene_map, 0.0)[2]                      # every candidate's value, kept or not
    if thr > 0:                                                          # none within 4 float32 ulps of the threshold
        assert (np.abs(every.astype(np.float64) - thr) > 4 * float(np.spacing(np.float32(thr)))).all()
    assert (every > 0).all()
    assert L.fragile(want[3]).sum() * 10000 <= max(len(want[3]), 1)      # expected: none
    for a in want:
        a.setflags(write=False)
    return c, want


def _same(got, want, where=""):
    rowptr, col, raw = got
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and raw.dtype == torch.float32 and raw.is_cuda
    np.testing.assert_array_equal(rowptr.cpu().numpy(), want[0], err_msg=where)
    np.testing.assert_array_equal(col.cpu().numpy(), want[1], err_msg=where)
    g, w = A.bits(raw.cpu().numpy()).astype(np.int64), A.bits(want[2]).astype(np.int64)
    off = np.abs(g - w)                                                  # positive floats: bit patterns are ordered
    frag = L.fragile(want[3])
    n_off = int((off != 0).sum())
    print(f"{where}: {len(w)} values, {n_off} differ, max {int(off.max()) if len(off) else 0} ulp, {int(frag.sum())} fragile")
    assert (off[~frag] == 0).all(), f"{where}: {int((off[~frag] != 0).sum())} of {len(w)} values differ from the fp64 definition"
    assert (off[frag] <= 1).all(), where


# ------------------------------------------------------------------------------------------------
# 1 / 2 / 3 / 6. structure, values, corners, determinism - every operand form
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", A.THRESHOLDS)
@pytest.mark.parametrize("B,n_cols,G", A.SHAPES)
def test_dense_matches_definition(B, n_cols, G, thr):
    c, want = _case(B, n_cols, G, thr)
    if n_cols >= 63:
        cs = L.corners(c)
        assert cs.zero_row and cs.foreign_only_row and cs.one_big_among_ones and cs.total_beyond_2_24_odd and cs.neg_zero \
            and cs.fractions and cs.foreign_counts
        assert (cs.kept[[L.ROW_ZERO, L.ROW_FOREIGN_ONLY]] == 0).all() and cs.totals[L.ROW_FOREIGN_ONLY] > 0
        assert cs.kept[L.ROW_BEYOND_2_24] > 0 and cs.kept[L.ROW_FRACTIONS] > 0
    gmap = t(c.gene_map)
    for name, ld in A.leading_dims(n_cols).items():          # packed / 16-byte rows (4 columns per lane) / unaligned rows
        x = _strided(c.x, ld)
        got = ops.align_rows(x, gmap, G, thr, normalize="lognorm")
        _same(got, want, f"dense {n_cols} {name} thr={thr}")
        again = ops.align_rows(x, gmap, G, thr, normalize="lognorm")
        assert all(torch.equal(a, b) for a, b in zip(got, again)), name


@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("thr", A.THRESHOLDS)
@pytest.mark.parametrize("B,n_cols,G", A.SHAPES)
def test_csr_matches_definition(B, n_cols, G, thr, i64):
    c, want = _case(B, n_cols, G, thr)
    rowptr, col, val = L.to_csr(c.x)                          # the -0.0 stays stored; foreign entries too
    for g, w in zip(L.lognorm_csr(rowptr, col, val, c.gene_map, thr), want):
        np.testing.assert_array_equal(g, w)
    csr = (t(rowptr.astype(np.int64 if i64 else np.int32)), t(col), t(val))
    got = ops.align_rows(csr, t(c.gene_map), G, thr, normalize="lognorm")
    _same(got, want, f"csr {n_cols} i64={i64} thr={thr}")
    assert all(torch.equal(a, b) for a, b in zip(got, ops.align_rows(csr, t(c.gene_map), G, thr, normalize="lognorm")))


def test_grid_stride_batch():
    B, n_cols, G = A.GRID_STRIDE_SHAPE
    c = L.count_case(3, B, n_cols, G, 0.0, density=0.5)
    want = L.lognorm_dense(c.x, c.gene_map, 0.0, fp64=True)
    assert want[0][-1] > B and (np.diff(want[0])[8192:] > 0).any()       # rows past the first sweep keep entries
    assert not L.fragile(want[3]).any()
    for batch in (t(c.x), _strided(c.x, 9), tuple(t(a) for a in L.to_csr(c.x))):
        _same(ops.align_rows(batch, t(c.gene_map), G, 0.0, normalize="lognorm"), want, "grid stride")


def test_many_rows_that_keep_almost_nothing():
    """More rows than one sweep of the grid and at most one kept entry per row: the outputs are then smaller than the row totals
    (4 + 4 bytes per kept entry against 8 bytes per row), which the fill pass still reads while it writes them."""
    B, n_cols, G = A.GRID_STRIDE_SHAPE
    c = L.count_case(5, B, n_cols, G, 0.0, density=0.5, special=False)
    c.gene_map[:] = -1
    c.gene_map[3] = 2                                                    # one mapped column
    want = L.lognorm_dense(c.x, c.gene_map, 0.0, fp64=True)
    kept = np.diff(want[0])
    assert B > 8192 and kept.max() == 1 and 0 < want[0][-1] < B and (kept[8192:] > 0).any() and not L.fragile(want[3]).any()
    assert len(np.unique(L.totals(c.x))) > 5                             # a wrong row's total gives another value
    for batch in (t(c.x), _strided(c.x, 9), tuple(t(a) for a in L.to_csr(c.x))):
        for _ in range(3):
            _same(ops.align_rows(batch, t(c.gene_map), G, 0.0, normalize="lognorm"), want, "rows that keep almost nothing")


def test_malformed_entries_of_a_row_without_counts_are_still_reported():
    """A row whose total is 0 keeps nothing, but its columns and map values are checked like any other row's."""
    gmap = np.array([0, 1, -1, 2], np.int32)
    rowptr, val = np.array([0, 2, 4], np.int64), np.array([0, 0, 1, 2], np.float32)      # row 0: explicit zeros only
    with pytest.raises(sda.WgnnError, match=r"column is outside \[0, n_cols\)"):
        ops.align_rows((t(rowptr), t(np.array([0, 9, 1, 3], np.int32)), t(val)), t(gmap), 3, 0.0, normalize="lognorm")
    bad_map = np.array([0, 7, -1, 2], np.int32)
    x = np.array([[0, 0, 0, 0], [1, 0, 0, 2]], np.float32)                               # the bad map value meets zeros only
    for batch in (t(x), (t(rowptr), t(np.array([0, 1, 0, 3], np.int32)), t(val))):
        with pytest.raises(sda.WgnnError, match=r"gene_map value is outside \[-1, n_genes\)"):
            ops.align_rows(batch, t(bad_map), 3, 0.0, normalize="lognorm")
    rowptr_out, col, _ = ops.align_rows(t(x), t(gmap), 3, 0.0, normalize="lognorm")
    assert rowptr_out.tolist() == [0, 0, 2] and col.tolist() == [0, 2]


def test_scale_factor():
    c, _ = _case(37, 130, 100, 0.0)
    want = L.lognorm_dense(c.x, c.gene_map, 0.5, scale=1e6, fp64=True)
    assert not L.fragile(want[3]).any()
    _same(ops.align_rows(t(c.x), t(c.gene_map), 100, 0.5, normalize="lognorm", scale=1e6), want, "scale 1e6")


# ------------------------------------------------------------------------------------------------
# 4. bad values are reported, not faulted on (ordinary input checks: the kernel skips the entry and sets the bit)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_bad_counts_raise_on_mapped_and_foreign_columns(bad):
    c, want = _case(37, 130, 100, 0.0)
    gmap = t(c.gene_map)
    for j in (int(np.flatnonzero(c.gene_map >= 0)[7]), int(np.flatnonzero(c.gene_map < 0)[2])):
        x = c.x.copy(); x[9, j] = bad
        for batch in (t(x), _strided(x, 131), tuple(t(a) for a in L.to_csr(x))):
            with pytest.raises(sda.WgnnError, match="a count is negative, NaN or infinite"):
                ops.align_rows(batch, gmap, 100, 0.0, normalize="lognorm")
    _same(ops.align_rows(t(c.x), gmap, 100, 0.0, normalize="lognorm"), want, "after the bad batches")


def test_bad_library_size_raises_only_where_the_row_holds_counts():
    c, want = _case(37, 130, 100, 0.0)
    gmap = t(c.gene_map)
    size = L.totals(c.x)
    assert size[L.ROW_ZERO] == 0 and size[10] > 0
    _same(ops.align_rows(t(c.x), gmap, 100, 0.0, normalize="lognorm", library_size=t(size)), want, "zero size, empty row")
    for v in (0.0, -3.0, float("nan"), float("inf")):
        size2 = size.copy(); size2[10] = v
        with pytest.raises(sda.WgnnError, match="library size of a row that holds counts"):
            ops.align_rows(t(c.x), gmap, 100, 0.0, normalize="lognorm", library_size=t(size2))
    with pytest.raises(ValueError, match="one entry per cell"):
        ops.align_rows(t(c.x), gmap, 100, 0.0, normalize="lognorm", library_size=t(size[:-1]))


# ------------------------------------------------------------------------------------------------
# 5. library_size
# ------------------------------------------------------------------------------------------------
def test_library_size_replaces_the_total():
    c, want = _case(37, 1000, 700, 0.5)
    gmap = t(c.gene_map)
    size = L.totals(c.x)
    default = ops.align_rows(t(c.x), gmap, 700, 0.5, normalize="lognorm")
    for name, lib in (("device", t(size)), ("numpy", size), ("list", size.tolist())):      # fp64 on the device, whatever comes in
        got = ops.align_rows(t(c.x), gmap, 700, 0.5, normalize="lognorm", library_size=lib)
        assert all(torch.equal(a, b) for a, b in zip(got, default)), name
    doubled = L.lognorm_dense(c.x, c.gene_map, 0.5, library_size=2 * size, fp64=True)
    assert not L.fragile(doubled[3]).any() and doubled[0][-1] < want[0][-1]
    for batch in (t(c.x), tuple(t(a) for a in L.to_csr(c.x))):
        _same(ops.align_rows(batch, gmap, 700, 0.5, normalize="lognorm", library_size=t(2 * size)), doubled, "doubled sizes")


# ------------------------------------------------------------------------------------------------
# 9. nothing moved
# ------------------------------------------------------------------------------------------------
def test_unnormalised_align_is_where_it_was():
    c = A.dense_case(130, 37, 130, 100, 0.5)
    want = A.align_dense(c.x, c.gene_map, 0.5)
    for x in (t(c.x), _strided(c.x, 131), _strided(c.x, 136)):
        rowptr, col, raw = ops.align_rows(x, t(c.gene_map), 100, 0.5)
        np.testing.assert_array_equal(rowptr.cpu().numpy(), want[0])
        np.testing.assert_array_equal(col.cpu().numpy(), want[1])
        np.testing.assert_array_equal(A.bits(raw.cpu().numpy()), A.bits(want[2]))


# ------------------------------------------------------------------------------------------------
# 7 / 8. ResidentPredictor: wiring, no tolerance
# ------------------------------------------------------------------------------------------------
def _callers_counts(rp, G, B=60, seed=11, permute=True):
    """Raw counts over a caller's gene list: the bundle's genes (20 missing; permuted or in the bundle's order) with 120 foreign
    genes, expressed, in between.  Returns (names, dense [B, n_cols] f32)."""
    rng = np.random.default_rng(seed)
    order = (rng.permutation(G) if permute else np.arange(G))[: G - 20]
    names = [rp.id2gene[g] for g in order]
    for k in range(120):
        names.insert(int(rng.integers(len(names) + 1)), f"Foreign{k}")
    x = rng.poisson(0.4, (B, len(names))).astype(np.float32)
    x[5] = 0
    return names, x


@pytest.mark.parametrize("n_layers,thr", [(1, 0), (2, 0.5)])
def test_normalize_keyword_end_to_end(tmp_path, n_layers, thr):
    root, G = _random_bundle(tmp_path, n_layers, seed=40 + n_layers)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02, threshold=thr)
    names, x = _callers_counts(rp, G)
    gmap_host = api._gene_map_ids(names, rp._gene2id)
    want_csr = L.lognorm_dense(x, gmap_host, thr, fp64=True)
    assert (x[:, gmap_host < 0] > 0).any() and not L.fragile(want_csr[3]).any()

    aligned = rp.align(x, names, normalize="lognorm")
    _same(aligned, want_csr, "ResidentPredictor.align")
    assert not torch.equal(aligned[2], rp.align(x, names)[2][: len(aligned[2])])          # counts in, values out
    want_label, want_prob, want_logits = rp.classify(aligned)
    want_att = rp.explain(aligned, top_k=5)
    want_tab = rp.markers(aligned)
    want_frame = api._prediction_frame("mouse", "Rand", "matrix", pd.RangeIndex(len(x)), want_label, rp.id2label, rp.bundle, None)
    assert (want_label >= 0).any()

    stored = x != 0
    scipy_csr = sp.csr_matrix((x[stored], np.nonzero(stored)[1], np.concatenate([[0], np.cumsum(stored.sum(1))])), shape=x.shape)
    rp_default = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02, threshold=thr, normalize="lognorm")
    assert rp_default.normalize == sda.LogNormalize()
    for who, kw in ((rp, dict(normalize="lognorm")), (rp, dict(normalize=sda.LogNormalize())), (rp_default, {})):
        for expr in (x, t(x), scipy_csr, (t(scipy_csr.indptr.astype(np.int64)), t(scipy_csr.indices), t(scipy_csr.data))):
            label, prob, logits = who.classify(expr, genes=names, **kw)
            assert who.last_route == "fused" and torch.equal(logits, want_logits)
            np.testing.assert_array_equal(label, want_label)
            np.testing.assert_array_equal(prob, want_prob)
        att = who.explain(x, top_k=5, genes=names, **kw)
        assert torch.equal(att.scores, want_att.scores)
        np.testing.assert_array_equal(att.top_genes, want_att.top_genes)
        tab = who.markers(t(x), genes=names, **kw)
        assert torch.equal(tab.score_sum, want_tab.score_sum) and torch.equal(tab.expr_count, want_tab.expr_count)
        pd.testing.assert_frame_equal(who.predict_matrix(x, names, **kw), want_frame)
        for a, b in zip(who.align(x, names, **kw), aligned):
            assert torch.equal(a, b)
    # the scale factor and the library sizes travel with the dataclass
    spec = sda.LogNormalize(scale_factor=1e6, library_size=2 * L.totals(x))
    _same(rp.align(x, names, normalize=spec), L.lognorm_dense(x, gmap_host, thr, scale=1e6, library_size=2 * L.totals(x), fp64=True),
          "LogNormalize(scale_factor, library_size)")
    # the predictor's default leaves a batch over the bundle's ids alone
    assert torch.equal(rp_default.classify(aligned)[2], want_logits)
    for call in (lambda: rp.classify(aligned, normalize="lognorm"), lambda: rp.explain(aligned, normalize="lognorm"),
                 lambda: rp.markers(aligned, normalize="lognorm")):
        with pytest.raises(ValueError, match="normalize needs genes="):
            call()
    with pytest.raises(ValueError, match="threshold = -1.0 must be >= 0"):
        rp.align(x, names, threshold=-1.0, normalize="lognorm")
    with pytest.raises(ValueError, match="normalize ="):
        rp.align(x, names, normalize="cpm")
    with pytest.raises(sda.WgnnError, match="a count is negative"):
        rp.classify(-x, genes=names, normalize="lognorm")


def test_file_route(tmp_path):
    """A counts file read with ``normalize`` gives the table of ``predict_matrix`` on the same matrix and gene names; without it,
    what ``predict`` has always given."""
    root, G = _random_bundle(tmp_path, 2, seed=33)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02)
    names, x = _callers_counts(rp, G, B=40, seed=5, permute=False)
    cells = [f"Cell{i}" for i in range(x.shape[0])]
    f = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(x.T, index=names, columns=cells).to_csv(f)
    want = rp.predict_matrix(t(x), names, index=pd.Index(cells), normalize="lognorm")
    got = rp.predict(f, normalize="lognorm")
    assert set(want["cell_type"]) - {"unsure"}
    pd.testing.assert_frame_equal(got, want)
    assert [d["cell_type"].tolist() for d in rp.predict_many([f, f], normalize=sda.LogNormalize())] == [want["cell_type"].tolist()] * 2
    rp_default = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02, normalize="lognorm")
    pd.testing.assert_frame_equal(rp_default.predict(f), got)
    att = rp.explain_file(f, top_k=3, normalize="lognorm")
    want_att = rp.explain(x, top_k=3, genes=names, normalize="lognorm")
    assert att["gene"].tolist() == [rp.id2gene[g] for g in want_att.top_genes[want_att.top_genes >= 0]]
    tab = rp.markers_files([f], top_k=4, normalize="lognorm")
    assert tab.equals(rp_default.markers_files([f], top_k=4)) and len(tab)
    # normalize=None: the host reader, as before
    test, index = api._read_test_csr(f, "csv", rp._gene2id, 0)
    pred, _, _ = rp.classify(test)
    today = api._prediction_frame("mouse", "Rand", f, index, pred, rp.id2label, rp.bundle, None)
    pd.testing.assert_frame_equal(rp.predict(f), today)
    pd.testing.assert_frame_equal(rp.predict(f, normalize=None), today)
    assert not torch.equal(rp.classify(x, genes=names, normalize="lognorm")[2], rp.classify(test)[2])
