"""Batch alignment on the GPU: ``wgnn_align_count`` / ``wgnn_align_fill`` (``ops.align_rows``) against the numpy restatement of
tests/align_reference.py, and ``ResidentPredictor`` over the caller's own gene list (``gene_map``, ``align``, ``genes=``,
``predict_matrix``) against the same calls on the reference-aligned batch.  Everything is selection and copy: every comparison
is ``array_equal`` / ``torch.equal``, no tolerance anywhere."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import api, ops

import align_reference as A
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _strided(x, ld):
    """``x`` on the device as a [B, n_cols] view of rows ``ld`` elements apart; the storage ends with the last row's n_cols."""
    B, n = x.shape
    buf = torch.full((max(B * ld - (ld - n), 0),), float("nan"), dtype=torch.float32, device=DEV)    # NaN between the rows
    view = torch.as_strided(buf, (B, n), (ld, 1))
    view.copy_(t(x))
    return view


def _same(got, want):
    rowptr, col, raw = got
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and raw.dtype == torch.float32 and raw.is_cuda
    np.testing.assert_array_equal(rowptr.cpu().numpy(), want[0])
    np.testing.assert_array_equal(col.cpu().numpy(), want[1])
    np.testing.assert_array_equal(A.bits(raw.cpu().numpy()), A.bits(want[2]))


# ------------------------------------------------------------------------------------------------
# 1. the kernels against the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", A.THRESHOLDS)
@pytest.mark.parametrize("B,n_cols,G", A.SHAPES)
def test_dense_matches_reference(B, n_cols, G, thr):
    c = A.dense_case(n_cols, B, n_cols, G, thr)
    want = A.align_dense(c.x, c.gene_map, thr)
    gmap = t(c.gene_map)
    for name, ld in A.leading_dims(n_cols).items():          # packed / 16-byte rows (4 columns per lane) / unaligned rows
        x = _strided(c.x, ld)
        assert x.stride(0) == ld or B == 1
        got = ops.align_rows(x, gmap, G, thr)
        _same(got, want)
        again = ops.align_rows(x, gmap, G, thr)               # two launches equal
        assert all(torch.equal(a, b) for a, b in zip(got, again)), name


@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("thr", A.THRESHOLDS)
@pytest.mark.parametrize("B,n_cols,G", A.SHAPES)
def test_csr_matches_reference(B, n_cols, G, thr, i64):
    c = A.dense_case(n_cols, B, n_cols, G, thr)
    rowptr, col, val = A.dense_to_csr(c.x)                   # explicit sub-threshold, NaN and foreign entries stay stored
    want = A.align_csr(rowptr, col, val, c.gene_map, thr)
    for g, w in zip(want, A.align_dense(c.x, c.gene_map, thr)):
        np.testing.assert_array_equal(g, w)
    csr = (t(rowptr.astype(np.int64 if i64 else np.int32)), t(col), t(val))
    got = ops.align_rows(csr, t(c.gene_map), G, thr)
    _same(got, want)
    assert all(torch.equal(a, b) for a, b in zip(got, ops.align_rows(csr, t(c.gene_map), G, thr)))
    # stored order is kept: the same rows with their entries reversed come out reversed
    rev = np.concatenate([np.arange(rowptr[r], rowptr[r + 1])[::-1] for r in range(B)]) if len(col) else np.zeros(0, np.int64)
    want_rev = A.align_csr(rowptr, col[rev], val[rev], c.gene_map, thr)
    _same(ops.align_rows((csr[0], t(col[rev]), t(val[rev])), t(c.gene_map), G, thr), want_rev)


def test_all_genes_foreign_empty_batch_and_no_columns():
    c = A.dense_case(1, 37, 130, 100, 0.0)
    none = torch.full((130,), -1, dtype=torch.int32, device=DEV)
    for batch in (t(c.x), tuple(t(a) for a in A.dense_to_csr(c.x))):
        rowptr, col, raw = ops.align_rows(batch, none, 100, 0.0)
        assert rowptr.tolist() == [0] * 38 and col.numel() == 0 and raw.numel() == 0
    gmap = t(c.gene_map)
    for batch in (torch.zeros((0, 130), device=DEV), (torch.zeros(1, dtype=torch.int64, device=DEV), t(np.zeros(0, np.int32)),
                                                      t(np.zeros(0, np.float32)))):
        rowptr, col, raw = ops.align_rows(batch, gmap, 100, 0.0)                       # B = 0
        assert rowptr.tolist() == [0] and col.numel() == 0 and raw.numel() == 0
    empty_map = torch.zeros(0, dtype=torch.int32, device=DEV)
    rowptr, col, raw = ops.align_rows(torch.zeros((5, 0), device=DEV), empty_map, 100, 0.0)   # n_cols = 0
    assert rowptr.tolist() == [0] * 6 and col.numel() == 0


def test_grid_stride_batch():
    B, n_cols, G = A.GRID_STRIDE_SHAPE
    c = A.dense_case(3, B, n_cols, G, 0.0, density=0.5)
    want = A.align_dense(c.x, c.gene_map, 0.0)
    assert want[0][-1] > B and (np.diff(want[0])[8192:] > 0).any()                     # rows past the first sweep keep entries
    _same(ops.align_rows(t(c.x), t(c.gene_map), G, 0.0), want)
    _same(ops.align_rows(_strided(c.x, 9), t(c.gene_map), G, 0.0), want)
    _same(ops.align_rows(tuple(t(a) for a in A.dense_to_csr(c.x)), t(c.gene_map), G, 0.0), want)


def test_malformed_operands_raise_and_nothing_faults():
    """Input validation on a valid launch: the kernels skip the entry (no lookup, no store) and flag it."""
    c = A.dense_case(2, 37, 130, 100, 0.0)
    gmap = t(c.gene_map)
    rowptr, col, val = A.dense_to_csr(c.x)
    for bad_col in (130, -1, 2 ** 31 - 1):                                            # col == n_cols and friends
        col2 = col.copy(); col2[len(col) // 2] = bad_col
        with pytest.raises(sda.WgnnError, match=r"column is outside \[0, n_cols\)"):
            ops.align_rows((t(rowptr), t(col2), t(val)), gmap, 100, 0.0)
    for bad_id in (100, -2):                                                          # a map value == n_genes, or below -1
        m2 = c.gene_map.copy(); m2[int(np.flatnonzero(m2 >= 0)[3])] = bad_id
        for batch in (t(c.x), _strided(c.x, 131), (t(rowptr), t(col), t(val))):
            with pytest.raises(sda.WgnnError, match=r"gene_map value is outside \[-1, n_genes\)"):
                ops.align_rows(batch, t(m2), 100, 0.0)
    _same(ops.align_rows(t(c.x), gmap, 100, 0.0), A.align_dense(c.x, c.gene_map, 0.0))   # the device is fine afterwards
    with pytest.raises(sda.WgnnError, match="columns"):
        ops.align_rows(t(c.x[:, :-1]), gmap, 100, 0.0)
    with pytest.raises(sda.WgnnError, match="float32"):
        ops.align_rows(t(c.x).double(), gmap, 100, 0.0)
    with pytest.raises(sda.WgnnError, match="row-major"):
        ops.align_rows(t(c.x.T.copy()).t(), gmap, 100, 0.0)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        ops.align_rows(torch.from_numpy(c.x), gmap, 100, 0.0)
    with pytest.raises(sda.WgnnError, match="int32"):
        ops.align_rows(t(c.x), gmap.long(), 100, 0.0)


# ------------------------------------------------------------------------------------------------
# 2. ResidentPredictor over the caller's gene list
# ------------------------------------------------------------------------------------------------
def _callers_batch(rp, G, thr, B=70, seed=11, permute=True):
    """A bundle-vocabulary batch as a user would hold it: columns permuted, foreign columns (with values) interleaved,
    sub-threshold values added.  Returns (names, dense [B, n_cols] f32)."""
    rng = np.random.default_rng(seed)
    batch = sp.random(B, G, density=0.1, random_state=seed, format="csr", dtype=np.float32)
    batch.data = 1.0 + 4.0 * batch.data
    base = batch.toarray()
    base[5] = 0                                                          # a cell with nothing
    order = rng.permutation(G) if permute else np.arange(G)
    order = order[: G - 20]                                              # the caller lacks 20 bundle genes
    names = [rp.id2gene[g] for g in order]
    cols = [base[:, g] for g in order]
    for k in range(120):                                                 # foreign genes, expressed
        at = int(rng.integers(len(names) + 1))
        names.insert(at, f"Foreign{k}")
        cols.insert(at, np.where(rng.random(B) < 0.3, rng.uniform(1, 5, B), 0).astype(np.float32))
    x = np.ascontiguousarray(np.stack(cols, axis=1), dtype=np.float32)
    low = (x == 0) & (rng.random(x.shape) < 0.05)
    x[low] = np.float32(thr) if thr > 0 else np.float32(-0.75)           # exactly at / below the threshold
    x[(x == 0) & (rng.random(x.shape) < 0.02)] = np.float32(thr) / 2 - np.float32(0.125)
    return names, x


@pytest.mark.parametrize("n_layers,thr", [(1, 0), (2, 0.5)])
def test_genes_keyword_end_to_end(tmp_path, n_layers, thr):
    root, G = _random_bundle(tmp_path, n_layers, seed=20 + n_layers)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02, threshold=thr)
    names, x = _callers_batch(rp, G, thr)
    gmap_host = api._gene_map_ids(names, rp._gene2id)
    want_csr = A.align_dense(x, gmap_host, thr)                          # the reference-aligned batch
    assert (gmap_host < 0).sum() == 120 and (x[:, gmap_host < 0] > thr).any() and ((x <= thr) & (x != 0)).any()
    ref = tuple(t(a) for a in want_csr)
    want_label, want_prob, want_logits = rp.classify(ref)
    want_att = rp.explain(ref, top_k=5)
    want_tab = rp.markers(ref)
    assert (want_label >= 0).any()

    gmap = rp.gene_map(names)
    assert gmap.dtype == torch.int32 and gmap.is_cuda and gmap.cpu().numpy().tolist() == gmap_host.tolist()
    stored = (x != 0)
    scipy_csr = sp.csr_matrix((x[stored], np.nonzero(stored)[1], np.concatenate([[0], np.cumsum(stored.sum(1))])), shape=x.shape)
    forms = {
        "numpy": x, "numpy64": x.astype(np.float64), "tensor": t(x), "host tensor": torch.from_numpy(x),
        "strided tensor": t(np.pad(x, ((0, 0), (0, 3))))[:, : x.shape[1]], "scipy": scipy_csr, "scipy coo": scipy_csr.tocoo(),
        "triple": (t(scipy_csr.indptr.astype(np.int64)), t(scipy_csr.indices.astype(np.int32)), t(scipy_csr.data)),
        "triple32": (t(scipy_csr.indptr.astype(np.int32)), t(scipy_csr.indices.astype(np.int32)), t(scipy_csr.data)),
    }
    for name, expr in forms.items():
        for genes in (names, gmap):                                      # names, or the precomputed map
            got = rp.align(expr, genes)
            for g, w in zip(got, ref):
                assert torch.equal(g, w), name
        label, prob, logits = rp.classify(expr, genes=gmap)
        assert rp.last_route == "fused"
        assert torch.equal(logits, want_logits), name
        np.testing.assert_array_equal(label, want_label)
        np.testing.assert_array_equal(prob, want_prob)
    for expr in (x, forms["tensor"], scipy_csr, forms["triple"]):
        att = rp.explain(expr, top_k=5, genes=names)
        assert torch.equal(att.scores, want_att.scores)
        np.testing.assert_array_equal(att.top_genes, want_att.top_genes)
        np.testing.assert_array_equal(att.base, want_att.base)
        np.testing.assert_array_equal(att.label, want_att.label)
        tab = rp.markers(expr, genes=names)
        assert torch.equal(tab.score_sum, want_tab.score_sum) and torch.equal(tab.expr_count, want_tab.expr_count)
        np.testing.assert_array_equal(tab.n_cells, want_tab.n_cells)
    # an explicit threshold overrides the predictor's
    _same(rp.align(x, gmap, threshold=2.0), A.align_dense(x, gmap_host, 2.0))
    # without genes= nothing changed: the positional forms still run
    assert torch.equal(rp.classify(ref)[2], want_logits)


def test_predict_matrix_equals_predict_on_the_same_data_as_csv(tmp_path):
    """The file's genes in the bundle's order (foreign ones in between): the file route and the in-memory route then list a
    cell's genes in the same order, and the two agree bit for bit."""
    root, G = _random_bundle(tmp_path, 2, seed=31)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02)
    names, x = _callers_batch(rp, G, 0, B=40, seed=5, permute=False)
    cells = [f"Cell{i}" for i in range(x.shape[0])]
    f = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(x.T, index=names, columns=cells).to_csv(f)
    want = rp.predict(f)
    got = rp.predict_matrix(t(x), names, index=pd.Index(cells))
    pd.testing.assert_frame_equal(got, want)
    assert set(want["cell_type"]) - {"unsure"}
    assert rp.predict_matrix(x, names)["index"].tolist() == list(range(x.shape[0]))
    test, _ = api._read_test_csr(f, "csv", rp._gene2id, 0)
    assert torch.equal(rp.classify(x, genes=names)[2], rp.classify(test)[2])
    with pytest.raises(ValueError, match="index names"):
        rp.predict_matrix(x, names, index=cells[:-1])


def test_gene_map_and_width_checks(tmp_path):
    root, G = _random_bundle(tmp_path, 1, seed=8)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    names = ["Gene3", "nope", "Gene1", "Gene3"]
    with pytest.raises(ValueError, match="both name bundle gene 3"):
        rp.gene_map(names)
    with pytest.raises(ValueError, match="none of the 2 gene names"):
        rp.gene_map(["nope", "neither"])
    names = ["Gene3", "nope", "Gene1"]
    x = np.array([[1.0, 2.0, 3.0], [0.0, 5.0, 0.0]], np.float32)
    rowptr, col, raw = rp.align(x, names)
    assert rowptr.tolist() == [0, 2, 2] and col.tolist() == [3, 1] and raw.tolist() == [1.0, 3.0]
    for wide in (np.zeros((2, 4), np.float32), torch.zeros((2, 2), device=DEV), sp.csr_matrix((2, 5), dtype=np.float32)):
        with pytest.raises(ValueError, match="columns, the gene list 3 names"):
            rp.align(wide, names)
        with pytest.raises(ValueError, match="columns, the gene list 3 names"):
            rp.classify(wide, genes=rp.gene_map(names))
    with pytest.raises(ValueError, match="2-D"):
        rp.align(np.zeros(3, np.float32), names)
    # a device triple carries no width: a column past the gene list is caught by the kernel's check
    with pytest.raises(sda.WgnnError, match=r"outside \[0, n_cols\)"):
        rp.align((t(np.array([0, 1], np.int64)), t(np.array([3], np.int32)), t(np.array([1.0], np.float32))), names)
