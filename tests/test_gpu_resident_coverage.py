"""Vocabulary coverage on the GPU: ``wgnn_coverage_rows`` (``ops.coverage_rows``) against the plain-loop restatement of
tests/coverage_reference.py, its ``total`` against the totals ``wgnn_align_count_ln`` stores, and ``ResidentPredictor.coverage``.
Counts are ``array_equal``.  The fp64 sums are ``array_equal`` too on the count cases of ``lognorm_reference`` (multiples of
2^-3 below 2^20, at most 1000 a row: every partial sum is exact in fp64 whatever the order); on non-dyadic values ``total`` must
be align's bits and ``total_mapped`` within the worst-case bound of any summation order of an ``fsum``."""
import math
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, api, ops

import align_reference as A
import coverage_reference as V
import lognorm_reference as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 100          # count_case(SEED + n_cols, ...), as the lognorm suite draws them


def t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # a copy: the cached cases are read-only


def _strided(x, ld):
    """``x`` on the device as a [B, n_cols] view of rows ``ld`` elements apart, NaN between the rows."""
    B, n = x.shape
    buf = torch.full((max(B * ld - (ld - n), 0),), float("nan"), dtype=torch.float32, device=DEV)
    view = torch.as_strided(buf, (B, n), (ld, 1))
    view.copy_(t(x))
    return view


def _csr(x, i64=True):
    rowptr, col, val = V.to_csr(x)
    return t(rowptr.astype(np.int64 if i64 else np.int32)), t(col), t(val)


@lru_cache(maxsize=None)
def _case(B, n_cols, G):
    """One count case per shape and its reference: computed once, never modified."""
    c = L.count_case(SEED + n_cols, B, n_cols, G, 0.0)
    want = V.as_tuple(V.coverage_dense(c.x, c.gene_map))
    for a in (c.x, c.gene_map) + want:
        a.setflags(write=False)
    return c, want


def _same(got, want, where=""):
    """The six device tensors against the reference's six arrays: dtypes, then every value, no tolerance."""
    assert len(got) == 6
    for name, g, w in zip(V.FIELDS, got, want):
        assert g.is_cuda and g.dtype == (torch.float64 if name.startswith("total") else torch.int32), (where, name)
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=f"{where}: {name}")


def _identical(a, b):
    return all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
               for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------
# the definition, every operand form
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n_cols,G", A.SHAPES)
def test_dense_matches_definition(B, n_cols, G):
    c, want = _case(B, n_cols, G)
    if n_cols >= 63:
        cs = L.corners(c)
        assert cs.zero_row and cs.foreign_only_row and cs.total_beyond_2_24_odd and cs.neg_zero and cs.fractions and cs.foreign_counts
        n_expressed, n_mapped, _, total, total_mapped, _ = want
        assert n_expressed[L.ROW_ZERO] == 0 and total[L.ROW_ZERO] == 0
        assert n_expressed[L.ROW_FOREIGN_ONLY] > 0 and n_mapped[L.ROW_FOREIGN_ONLY] == 0 and total_mapped[L.ROW_FOREIGN_ONLY] == 0
        assert total[L.ROW_BEYOND_2_24] > 2 ** 24 and total[L.ROW_BEYOND_2_24] % 2 == 1
    gmap = t(c.gene_map)
    for name, ld in A.leading_dims(n_cols).items():          # packed / 16-byte rows (4 columns per lane) / unaligned rows
        x = _strided(c.x, ld)
        got = ops.coverage_rows(x, gmap, G)
        _same(got, want, f"dense {n_cols} {name}")
        assert _identical(got, ops.coverage_rows(x, gmap, G)), name


@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("B,n_cols,G", A.SHAPES)
def test_csr_matches_definition(B, n_cols, G, i64):
    c, want = _case(B, n_cols, G)
    rowptr, col, val = V.to_csr(c.x)                          # the -0.0 stays stored; foreign entries too
    for g, w in zip(V.as_tuple(V.coverage_csr(rowptr, col, val, c.gene_map)), want):
        np.testing.assert_array_equal(g, w)
    csr = _csr(c.x, i64)
    got = ops.coverage_rows(csr, t(c.gene_map), G)
    _same(got, want, f"csr {n_cols} i64={i64}")
    assert _identical(got, ops.coverage_rows(csr, t(c.gene_map), G))


# ------------------------------------------------------------------------------------------------
# the sums on values whose order of addition shows
# ------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _non_dyadic():
    rng = np.random.default_rng(77)
    B, n_cols, G = 37, 1000, 700
    # 24-bit mantissas over 48 binades: a row's exact sum needs more than fp64's 53 bits, so the order of addition shows
    x = np.where(rng.random((B, n_cols)) < 0.3, (rng.random((B, n_cols)) + 0.01) * 2.0 ** rng.integers(-24, 24, (B, n_cols)), 0.0)
    x = x.astype(np.float32)
    gene_map = A.random_gene_map(rng, n_cols, G)
    x.setflags(write=False); gene_map.setflags(write=False)
    return x, gene_map, G


def _align_totals(batch, gmap, G):
    """The totals ``wgnn_align_count_ln`` stores for ``batch`` (no library sizes): the op keeps them to itself."""
    dev = gmap.device
    dense = isinstance(batch, torch.Tensor)
    B = batch.shape[0] if dense else batch[0].shape[0] - 1
    total = torch.full((B,), -1.0, dtype=torch.float64, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if dense:
        head = (ops._ptr(batch), int(batch.stride(0)), None, None, None)
        flags = 0
    else:
        head = (None, 0, ops._ptr(batch[0]), ops._ptr(batch[1]), ops._ptr(batch[2]))
        flags = _lib.FLAG_ROWPTR_I64 if batch[0].dtype == torch.int64 else 0
    rc = _lib.call(dev, "wgnn_align_count_ln", *head, B, int(gmap.shape[0]), ops._ptr(gmap), G, 0.0, None, ops._ptr(total), 1e4,
                   ops._ptr(counts), ops._ptr(status), flags, ops._stream(dev))
    _lib.check(rc, "wgnn_align_count_ln")
    assert int(status) == 0
    return total


def test_total_is_the_total_align_divides_by():
    x, gene_map, G = _non_dyadic()
    gmap = t(gene_map)
    naive = np.asarray([sum(float(v) for v in row) for row in x])
    batches = [_strided(x, ld) for ld in A.leading_dims(x.shape[1]).values()] + [_csr(x, False), _csr(x, True)]
    differs = 0
    for batch in batches:
        total = ops.coverage_rows(batch, gmap, G)[3]
        want = _align_totals(batch, gmap, G)
        assert torch.equal(total.view(torch.int64), want.view(torch.int64))
        differs += int((total.cpu().numpy() != naive).sum())
    assert differs > 0                   # the case does tell one order of addition from another


def test_non_dyadic_total_mapped():
    x, gene_map, G = _non_dyadic()
    mapped = gene_map >= 0
    terms = [[float(v) for v in row[mapped] if v > 0] for row in x]
    want = np.asarray([math.fsum(r) for r in terms])
    # n positive terms added in ANY order: |sum - exact| <= (n - 1) u sum|terms| (first order, u = 2^-53), and fsum is within
    # u sum|terms| of exact: n u sum|terms| bounds the difference whatever the kernel's order
    bound = np.asarray([len(r) * 2.0 ** -53 * math.fsum(r) for r in terms])
    gmap = t(gene_map)
    for batch in [_strided(x, ld) for ld in A.leading_dims(x.shape[1]).values()] + [_csr(x)]:
        got = ops.coverage_rows(batch, gmap, G)
        err = np.abs(got[4].cpu().numpy() - want)
        print(f"total_mapped: max error {err.max():.3e}, smallest bound {bound.min():.3e}")
        assert (err <= bound).all()
        np.testing.assert_array_equal(got[1].cpu().numpy(), [len(r) for r in terms])
        assert _identical(got, ops.coverage_rows(batch, gmap, G))


# ------------------------------------------------------------------------------------------------
# column counts across workgroups
# ------------------------------------------------------------------------------------------------
def _by_mask(c):
    """The reference by boolean masks - for finite cases too large for the loop (the CPU suite holds the two against each other);
    the cases are dyadic, so the sums are exact in any order."""
    on = c.x > 0
    mapped = c.gene_map >= 0
    v = np.where(on, c.x, 0).astype(np.float64)
    return (on.sum(1).astype(np.int32), on[:, mapped].sum(1).astype(np.int32), np.zeros(c.B, np.int32), v.sum(1),
            v[:, mapped].sum(1), on.sum(0).astype(np.int32))


@pytest.mark.parametrize("B,n_cols,G", [A.GRID_STRIDE_SHAPE, (8300, 70, 50)])
def test_column_counts_over_many_rows(B, n_cols, G):
    c = L.count_case(3, B, n_cols, G, 0.0, density=0.5)
    assert np.isfinite(c.x).all() and (c.x >= 0).all() and B > 8192
    want = _by_mask(c)
    assert (want[0][8192:] > 0).any() and want[5].min() > B // 4          # rows past the first sweep count; every column is busy
    ld_odd = A.leading_dims(n_cols)["odd"]
    for name, batch in (("packed", t(c.x)), ("padded", _strided(c.x, A.leading_dims(n_cols)["padded"])), ("odd", _strided(c.x, ld_odd)),
                        ("csr", _csr(c.x))):
        got = ops.coverage_rows(batch, t(c.gene_map), G)
        _same(got, want, f"{B} x {n_cols} {name}")
        assert _identical(got, ops.coverage_rows(batch, t(c.gene_map), G)), name


# ------------------------------------------------------------------------------------------------
# bad values, malformed operands, empty operands
# ------------------------------------------------------------------------------------------------
def test_bad_values_are_counted_and_left_out():
    c, clean = _case(37, 130, 100)
    on, off = np.flatnonzero(c.gene_map >= 0), np.flatnonzero(c.gene_map < 0)
    x = c.x.copy()
    for r, (j_on, j_off, v) in enumerate(((on[7], off[2], -1.0), (on[11], off[0], np.nan), (on[3], off[5], np.inf)), start=8):
        x[r, j_on] = v
        x[r, j_off] = v
    x[8, on[20]] = np.nan                                                                 # three bad values in one row
    want = V.as_tuple(V.coverage_dense(x, c.gene_map))
    assert want[2].tolist() == [0] * 8 + [3, 2, 2] + [0] * 26
    assert (want[3] <= clean[3]).all() and np.isfinite(want[3]).all() and np.isfinite(want[4]).all()
    gmap = t(c.gene_map)
    for name, batch in (("packed", t(x)), ("padded", _strided(x, 136)), ("odd", _strided(x, 131)), ("csr32", _csr(x, False)),
                        ("csr64", _csr(x, True))):
        _same(ops.coverage_rows(batch, gmap, 100), want, f"bad values {name}")            # and no exception


def test_malformed_operands_raise_as_align_does():
    c, want = _case(37, 130, 100)
    rowptr, col, val = V.to_csr(c.x)
    bad_col = col.copy(); bad_col[len(col) // 2] = 130                                    # == n_cols
    with pytest.raises(sda.WgnnError, match=r"column is outside \[0, n_cols\)"):
        ops.coverage_rows((t(rowptr), t(bad_col), t(val)), t(c.gene_map), 100)
    with pytest.raises(sda.WgnnError, match=r"column is outside \[0, n_cols\)"):
        ops.align_rows((t(rowptr), t(bad_col), t(val)), t(c.gene_map), 100)
    bad_map = c.gene_map.copy(); bad_map[np.flatnonzero(c.gene_map >= 0)[4]] = 100        # == n_genes
    for batch in (t(c.x), _strided(c.x, 131), (t(rowptr), t(col), t(val))):
        with pytest.raises(sda.WgnnError, match=r"gene_map value is outside \[-1, n_genes\)"):
            ops.coverage_rows(batch, t(bad_map), 100)
        with pytest.raises(sda.WgnnError, match=r"gene_map value is outside \[-1, n_genes\)"):
            ops.align_rows(batch, t(bad_map), 100)
    _same(ops.coverage_rows(t(c.x), t(c.gene_map), 100), want, "after the malformed batches")


def test_empty_batch_empty_columns_and_empty_rows():
    gmap = t(np.array([0, -1, 2, 1, -1, 3, 4, -1], np.int32))
    none = ops.coverage_rows(torch.empty(0, 8, dtype=torch.float32, device=DEV), gmap, 5)                     # B = 0, dense
    assert [tuple(a.shape) for a in none] == [(0,)] * 5 + [(8,)] and none[5].tolist() == [0] * 8
    ptr0 = torch.zeros(1, dtype=torch.int64, device=DEV)
    none = ops.coverage_rows((ptr0, torch.empty(0, dtype=torch.int32, device=DEV), torch.empty(0, device=DEV)), gmap, 5)     # B = 0, CSR
    assert [tuple(a.shape) for a in none] == [(0,)] * 5 + [(8,)] and none[5].tolist() == [0] * 8
    empty_map = torch.empty(0, dtype=torch.int32, device=DEV)
    got = ops.coverage_rows(torch.empty(5, 0, dtype=torch.float32, device=DEV), empty_map, 5)                 # n_cols = 0
    assert [tuple(a.shape) for a in got] == [(5,)] * 5 + [(0,)]
    assert all(a.tolist() == [0] * 5 for a in got[:5])
    x = np.zeros((6, 8), np.float32)
    x[1, [0, 1, 5]] = [2.0, 3.0, 0.5]
    x[4, [4, 6]] = [1.0, 7.0]
    rowptr, col, val = V.to_csr(x)
    assert rowptr.tolist() == [0, 0, 3, 3, 3, 5, 5]                                                           # empty rows around
    want = V.as_tuple(V.coverage_dense(x, gmap.cpu().numpy()))
    assert want[0].tolist() == [0, 3, 0, 0, 2, 0] and want[1].tolist() == [0, 2, 0, 0, 1, 0]
    _same(ops.coverage_rows((t(rowptr), t(col), t(val)), gmap, 5), want, "csr with empty rows")
    _same(ops.coverage_rows(t(x), gmap, 5), want, "dense with empty rows")


# ------------------------------------------------------------------------------------------------
# ResidentPredictor.coverage
# ------------------------------------------------------------------------------------------------
def _random_bundle(tmp_path, n_layers, G=500, n_sup=200, dense=16, hidden=12, n_cls=5, seed=0):
    """A bundle written by hand from a randomly initialised GNN (no fit)."""
    from scdeepsort_amd.api import BundlePaths
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    genes = [f"Gene{i}" for i in range(G)]
    b = BundlePaths(tmp_path / f"rand{n_layers}", "mouse", "Rand", layout="flat", for_write=True)
    b.mkdirs()
    b.genes.write_bytes("".join(g + "\r\n" for g in genes).encode())
    b.cell_types.write_bytes("".join(f"type{i}\r\n" for i in range(n_cls)).encode())
    sup = sp.random(n_sup, G, density=0.1, random_state=seed, format="csr", dtype=np.float32)
    sup.data = 1.0 + 4.0 * sup.data
    sp.save_npz(b.support, sup)
    m = sda.GNN(dense, hidden, n_cls, n_layers, G, activation=F.relu)
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
    torch.save({"model": m.state_dict(), "optimizer": {}}, b.model)
    return tmp_path / f"rand{n_layers}", G


def _callers_counts(rp, G, B=60, seed=11):
    """Raw counts over a caller's gene list: the bundle's genes (20 missing, permuted) at Poisson rate 1.5 with 120 foreign genes
    at rate 0.1 in between.  Returns (names, dense [B, n_cols] f32, the bundle ids left out)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(G)
    names = [rp.id2gene[g] for g in perm[: G - 20]]
    for k in range(120):
        names.insert(int(rng.integers(len(names) + 1)), f"Foreign{k}")
    foreign = np.array([n.startswith("Foreign") for n in names])
    x = np.where(foreign[None, :], rng.poisson(0.1, (B, len(names))), rng.poisson(1.5, (B, len(names)))).astype(np.float32)
    x[5] = 0
    return names, x, np.sort(perm[G - 20:])


def _same_coverage(a, b, names=True):
    for f in ("n_columns", "n_matched", "n_bundle_genes", "n_bundle_absent", "n_support_cells"):
        assert getattr(a, f) == getattr(b, f), f
    for f in ("n_expressed", "n_mapped", "n_bad", "total", "total_mapped", "matched", "absent_ids", "absent_support_cells"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    assert torch.equal(a.col_cells, b.col_cells) and a.col_cells.is_cuda
    assert list(a.index) == list(b.index) and a.absent_names == b.absent_names
    if names:
        assert a.columns == b.columns


def test_coverage_end_to_end(tmp_path):
    root, G = _random_bundle(tmp_path, 2, seed=21)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02)
    names, x, left_out = _callers_counts(rp, G)
    gmap_host = api._gene_map_ids(names, rp._gene2id)
    want = V.coverage_dense(x, gmap_host)
    detected = np.bincount(rp.support.indices, minlength=G)

    cov = rp.coverage(x, names)
    assert isinstance(cov, sda.Coverage)
    assert (cov.n_columns, cov.n_matched, cov.n_bundle_genes, cov.n_bundle_absent) == (len(names), G - 20, G, 20)
    for f in V.FIELDS[:5]:
        got = getattr(cov, f)
        assert isinstance(got, np.ndarray)
        np.testing.assert_array_equal(got, getattr(want, f), err_msg=f)
    np.testing.assert_array_equal(cov.col_cells.cpu().numpy(), want.col_cells)
    assert list(cov.index) == list(range(len(x))) and cov.columns == names
    np.testing.assert_array_equal(cov.fraction_counts(), np.divide(want.total_mapped, want.total, out=np.zeros(len(x)), where=want.total > 0))
    assert cov.fraction_counts()[5] == 0 and cov.fraction_genes()[5] == 0                  # the empty cell
    assert 0.9 < np.median(cov.fraction_counts()) < 1 and not cov.below()[np.arange(len(x)) != 5].any() and cov.below()[5]
    assert cov.frame().shape == (len(x), 7)
    np.testing.assert_array_equal(cov.absent(k=50)["gene_id"].to_numpy(), left_out[np.argsort(-detected[left_out], kind="stable")])

    # every form align takes says the same
    stored = x != 0
    scipy_csr = sp.csr_matrix((x[stored], np.nonzero(stored)[1], np.concatenate([[0], np.cumsum(stored.sum(1))])), shape=x.shape)
    triple = (t(scipy_csr.indptr.astype(np.int64)), t(scipy_csr.indices), t(scipy_csr.data))
    for expr in (t(x), scipy_csr, triple, x.astype(np.float64)):
        _same_coverage(rp.coverage(expr, names), cov)
    by_map = rp.coverage(t(x), rp.gene_map(names))
    _same_coverage(by_map, cov, names=False)
    assert by_map.columns is None and "gene" not in by_map.unmatched().columns

    # the same count align keeps (finite batch, threshold 0)
    np.testing.assert_array_equal(cov.n_mapped, np.diff(rp.align(x, names, threshold=0)[0].cpu().numpy()))

    # half of the bundle's names mangled: the model sees about half of every cell's counts
    rng = np.random.default_rng(3)
    hit = np.flatnonzero(gmap_host >= 0)
    mangle = np.sort(rng.choice(hit, size=len(hit) // 2, replace=False))
    mangled = list(names)
    for j in mangle:
        mangled[j] = names[j].lower()                                                      # "gene12": another species' casing
    gmap2 = api._gene_map_ids(mangled, rp._gene2id)
    assert (gmap2[mangle] == -1).all() and (gmap2 >= 0).sum() == len(hit) - len(mangle)
    want2 = V.coverage_dense(x, gmap2)
    cov2 = rp.coverage(t(x), mangled)
    for f in V.FIELDS[:5]:
        np.testing.assert_array_equal(getattr(cov2, f), getattr(want2, f), err_msg=f)
    np.testing.assert_array_equal(cov2.total, cov.total)
    live = cov.total > 0
    assert (cov2.fraction_counts()[live] < cov.fraction_counts()[live]).all()
    assert 0.35 < np.median(cov2.fraction_counts()) < 0.65 and cov2.below(min_counts=0.7)[live].all()
    assert cov2.summary()["n_matched"] == len(hit) - len(mangle) and cov2.summary()["n_bundle_absent"] == 20 + len(mangle)
    assert len(str(cov2.summary()).splitlines()) == 2
    # unmatched: the mangled columns are the busy ones, so they come first, by cells then position
    cells = want2.col_cells.astype(np.int64)
    assert cells[mangle].min() > cells[gmap_host < 0].max()
    u = cov2.unmatched(k=len(mangle))
    np.testing.assert_array_equal(u["position"].to_numpy(), mangle[np.argsort(-cells[mangle], kind="stable")])
    assert u["gene"].tolist() == [mangled[j] for j in u["position"]] and (np.diff(u["cells"].to_numpy()) <= 0).all()
    np.testing.assert_array_equal(u["cells"].to_numpy(), cells[u["position"].to_numpy()])
    assert len(cov2.unmatched(k=10 ** 6)) == len(names) - cov2.n_matched
    # absent: the mangled genes and the 20 the list never had, by the support's detection counts
    gone = np.sort(np.concatenate([left_out, gmap_host[mangle]]))
    a = cov2.absent(k=len(gone))
    np.testing.assert_array_equal(a["gene_id"].to_numpy(), gone[np.argsort(-detected[gone], kind="stable")])
    np.testing.assert_array_equal(a["support_cells"].to_numpy(), detected[a["gene_id"].to_numpy()])
    assert a["gene"].tolist() == [rp.id2gene[g] for g in a["gene_id"]]
    assert cov2.absent()["gene_id"].tolist() == a["gene_id"].tolist()[:20]

    # a file says the same, and names the cells
    cell_names = [f"Cell{i}" for i in range(len(x))]
    f = tmp_path / "mouse_Rand3_data.csv"
    pd.DataFrame(x.T, index=mangled, columns=cell_names).to_csv(f)
    from_file = rp.coverage_file(f)
    assert list(from_file.index) == cell_names and list(from_file.frame().index) == cell_names
    cov2.index = pd.Index(cell_names)
    _same_coverage(from_file, cov2)
    with pytest.raises(ValueError, match="columns, the gene list"):
        rp.coverage(x[:, :-1], names)


def test_nothing_else_moved(tmp_path):
    root, G = _random_bundle(tmp_path, 2, seed=22)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02)
    names, x, _ = _callers_counts(rp, G, B=40, seed=4)

    def snapshot():
        return (rp.align(x, names), rp.align(t(x), names, normalize="lognorm"), rp.classify(x, genes=names),
                rp.classify(t(x), genes=names, normalize="lognorm"), rp.predict_matrix(x, names))

    before = snapshot()
    cov = rp.coverage(t(x), names)
    assert cov.n_matched == G - 20
    after = snapshot()
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert torch.equal(a, b)
    for k in (2, 3):
        np.testing.assert_array_equal(before[k][0], after[k][0])
        np.testing.assert_array_equal(before[k][1], after[k][1])
        assert torch.equal(before[k][2], after[k][2])
    pd.testing.assert_frame_equal(before[4], after[4])
