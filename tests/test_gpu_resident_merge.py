"""The merging log-normalising alignment on the GPU: ``wgnn_align_count_ln_merge`` / ``wgnn_align_fill_ln_merge``
(``ops.align_rows(..., normalize="lognorm", groups=...)``) and ``aliases=`` / ``duplicates=`` through ``ResidentPredictor``.

1. the oracle is the EXISTING walk: on integer counts (every sum exact in float32) the merging walk on the original batch must
   leave, bit for bit, what ``align_rows(normalize="lognorm", library_size=the original totals)`` leaves on a batch whose
   member columns were summed on the host;
2. non-integer counts over many binades against tests/merge_reference.py with ``test_gpu_resident_lognorm``'s comparator: equal
   float32 bits except where the fp64 value lies within 16 fp64 ulps of a float32 rounding midpoint - at most 1 entry in 1 000
   may be excused that way, which is asserted (for the seeds here the reference has none, tests/test_merge_reference.py);
3. identities, 4. malformed operands inside guard elements, 5. end to end on the golden bundles."""
from functools import lru_cache

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, api, ops
from scdeepsort_amd.graph import _ptr, _stream

import align_reference as A
import lognorm_reference as L
import merge_reference as M
from test_gpu_resident_lognorm import _same, _strided, t
from test_gpu_resident_predict import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N_COLS, G = 24, 700, 900              # 700 columns: three 256-entry chunks of the 16-byte form, eleven 64-entry steps
THRESHOLDS = (0.0, M.JOINT_THRESHOLD)


@lru_cache(maxsize=None)
def _case(integer=True):
    c = M.merge_case(11 if integer else 23, B, N_COLS, G, integer=integer)
    c.x.setflags(write=False)
    return c


def _groups(c):
    return t(c.col_group), t(c.group_ptr), t(c.group_cols)


def _merge(batch, c, thr, **kw):
    return ops.align_rows(batch, t(c.gene_map), c.n_genes, thr, normalize="lognorm", groups=_groups(c), **kw)


def _equal(got, want, where):
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
    for g, w, name in zip(got, want, ("rowptr", "col", "raw")):
        g, w = g.cpu().numpy(), (w.cpu().numpy() if isinstance(w, torch.Tensor) else w)
        if name == "raw":
            g, w = A.bits(g), A.bits(w)
        np.testing.assert_array_equal(g, w, err_msg=f"{where}: {name}")


def _csr_forms(x, seed=5):
    rowptr, col, val = L.to_csr(x)
    return {"csr i32": (rowptr.astype(np.int32), col, val), "csr i64": (rowptr, col, val),
            "csr shuffled": M.shuffled_csr(x, seed)}


# ------------------------------------------------------------------------------------------------
# 1. the existing walk on a host-merged batch is the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", THRESHOLDS)
def test_dense_equals_the_existing_walk_on_the_host_merged_batch(thr):
    c = _case()
    pre, totals = M.premerge_dense(c.x, c.col_group), t(L.totals(c.x))
    assert not np.array_equal(pre, c.x)
    for name, ld in (("16-byte rows", 704), ("odd leading dimension", 701)):
        want = ops.align_rows(_strided(pre, ld), t(c.gene_map), G, thr, normalize="lognorm", library_size=totals)
        got = _merge(_strided(c.x, ld), c, thr)
        _equal(got, want, f"dense {name} thr={thr}")
        _equal(got, M.merge_dense(c.x, c.gene_map, c.col_group, thr)[:2], f"dense {name}: structure of the reference")
    kept = np.diff(got[0].cpu().numpy())
    assert kept[M.ROW_EMPTY] == 0 and kept[M.ROW_NO_MEMBER] > 0
    row = got[1][got[0][M.ROW_JOINT]: got[0][M.ROW_JOINT + 1]].cpu().numpy()
    assert c.gene_map[M.GROUP_QUAD[0]] in row                            # kept jointly at either threshold
    if thr > 0:                                                          # ... and by neither member alone
        plain = ops.align_rows(t(c.x), t(c.gene_map), G, thr, normalize="lognorm")
        assert c.gene_map[M.GROUP_QUAD[0]] not in plain[1][plain[0][M.ROW_JOINT]: plain[0][M.ROW_JOINT + 1]].cpu().numpy()


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("form", ["csr i32", "csr i64", "csr shuffled"])
def test_csr_equals_the_existing_walk_on_the_host_merged_batch(form, thr):
    c = _case()
    rowptr, col, val = _csr_forms(c.x)[form]
    pre = M.premerge_csr(rowptr, col, val, c.col_group)
    assert not np.array_equal(pre, val)
    want = ops.align_rows((t(rowptr), t(col), t(pre)), t(c.gene_map), G, thr, normalize="lognorm", library_size=t(L.totals(c.x)))
    got = _merge((t(rowptr), t(col), t(val)), c, thr)
    _equal(got, want, f"{form} thr={thr}")
    _equal(got, M.merge_csr(rowptr, col, val, c.gene_map, c.col_group, thr)[:2], f"{form}: structure of the reference")


def test_more_rows_than_the_grid_holds_waves():
    Bg, n, Gg = A.GRID_STRIDE_SHAPE
    rng = np.random.default_rng(2)
    x = np.where(rng.random((Bg, n)) < 0.5, rng.integers(1, 9, (Bg, n)), 0).astype(np.float32)
    gene_map = np.array([0, 1, -1, 2, 3, 1, 4, 5], np.int32)              # columns 1 and 5 name gene 1
    col_group, group_ptr, group_cols = M.group_tables(gene_map)
    c = type("C", (), dict(gene_map=gene_map, col_group=col_group, group_ptr=group_ptr, group_cols=group_cols, n_genes=Gg))
    both = (x[:, 1] > 0) & (x[:, 5] > 0)
    assert Bg > 8192 and both[8192:].any()
    pre = M.premerge_dense(x, col_group)
    totals = t(x.astype(np.float64).sum(axis=1))                          # integers: exact
    want = ops.align_rows(t(pre), t(gene_map), Gg, 0.0, normalize="lognorm", library_size=totals)
    for name, batch in (("dense", t(x)), ("dense odd ld", _strided(x, 9)), ("csr", tuple(t(a) for a in L.to_csr(x)))):
        _equal(_merge(batch, c, 0.0), want, f"grid stride {name}")


# ------------------------------------------------------------------------------------------------
# 2. non-integer counts against the fp64 definition
# ------------------------------------------------------------------------------------------------
def test_non_integer_counts_match_the_definition():
    c = _case(integer=False)
    want = M.merge_dense(c.x, c.gene_map, c.col_group, 0.0, fp64=True)
    assert L.fragile(want[3]).sum() * 1000 <= len(want[3])                # what the comparator may excuse: at most 1 in 1 000
    for name, ld in (("16-byte rows", 704), ("odd leading dimension", 701)):
        _same(_merge(_strided(c.x, ld), c, 0.0), want, f"merge dense {name}")
    for form, (rowptr, col, val) in _csr_forms(c.x, seed=7).items():
        w = M.merge_csr(rowptr, col, val, c.gene_map, c.col_group, 0.0, fp64=True)
        assert L.fragile(w[3]).sum() * 1000 <= len(w[3])
        _same(_merge((t(rowptr), t(col), t(val)), c, 0.0), w, f"merge {form}")


# ------------------------------------------------------------------------------------------------
# 3. identities
# ------------------------------------------------------------------------------------------------
def test_groups_that_never_meet_leave_the_existing_walk_s_bits():
    c = _case(integer=False)
    x = c.x.copy()
    for grp in c.groups:                                                  # one member per group and row survives
        keep = np.random.default_rng(len(grp)).integers(0, len(grp), B)
        for i, j in enumerate(grp):
            x[keep != i, j] = 0
    assert (x[:, c.col_group >= 0] > 0).sum() > 3 * B
    for batch in (t(x), _strided(x, 701), tuple(t(a) for a in L.to_csr(x)), tuple(t(a) for a in M.shuffled_csr(x, 3))):
        for thr in THRESHOLDS:
            _equal(_merge(batch, c, thr), ops.align_rows(batch, t(c.gene_map), G, thr, normalize="lognorm"), "groups never meet")


def test_two_launches_and_both_forms_give_the_same_bits():
    c = _case(integer=False)
    dense = _merge(t(c.x), c, 0.0)
    _equal(_merge(t(c.x), c, 0.0), dense, "second launch, dense")
    _equal(_merge(_strided(c.x, 701), c, 0.0), dense, "odd leading dimension")
    csr = tuple(t(a) for a in L.to_csr(c.x))
    _equal(_merge(csr, c, 0.0), dense, "csr in column order")
    sh = tuple(t(a) for a in M.shuffled_csr(c.x, 3))
    _equal(_merge(sh, c, 0.0), _merge(sh, c, 0.0), "second launch, shuffled csr")


def test_no_groups_runs_the_existing_kernels():
    c = _case()
    none = (t(np.full(N_COLS, -1, np.int32)), t(np.zeros(1, np.int32)), t(np.zeros(0, np.int32)))
    got = ops.align_rows(t(c.x), t(c.gene_map), G, 0.0, normalize="lognorm", groups=none)
    _equal(got, ops.align_rows(t(c.x), t(c.gene_map), G, 0.0, normalize="lognorm"), "no groups")


def test_a_row_with_more_member_entries_than_the_list_holds():
    """150 groups of two, every member counting in row 0: 300 counting member entries, more than the 256 the CSR walk lists in
    LDS; row 1 is sparse (the list serves it), row 2 holds 256 + 1 of them."""
    rng = np.random.default_rng(9)
    gene_map = rng.permutation(G)[:N_COLS].astype(np.int32)
    cols = rng.permutation(N_COLS)[:300]
    gene_map[cols[150:]] = gene_map[cols[:150]]
    col_group, group_ptr, group_cols = M.group_tables(gene_map)
    assert len(group_ptr) - 1 == 150 and len(group_cols) == 300
    c = type("C", (), dict(gene_map=gene_map, col_group=col_group, group_ptr=group_ptr, group_cols=group_cols, n_genes=G))
    x = np.where(rng.random((3, N_COLS)) < 0.3, rng.integers(1, 2048, (3, N_COLS)) / 8.0, 0).astype(np.float32)
    x[0, cols] = rng.integers(1, 2048, 300) / 8.0
    x[2, cols] = 0
    x[2, cols[:257]] = rng.integers(1, 2048, 257) / 8.0
    assert ((x[:, cols] > 0).sum(axis=1) > 256).tolist() == [True, False, True]
    for rowptr, col, val in (L.to_csr(x), M.shuffled_csr(x, 1)):
        want = M.merge_csr(rowptr, col, val, gene_map, col_group, 0.0, fp64=True)
        assert not L.fragile(want[3]).any()
        _same(_merge((t(rowptr), t(col), t(val)), c, 0.0), want, "long member list")
    _same(_merge(t(x), c, 0.0), M.merge_dense(x, gene_map, col_group, 0.0, fp64=True), "long member list, dense")


# ------------------------------------------------------------------------------------------------
# 4. malformed operands: reported, skipped, nothing written outside its room
# ------------------------------------------------------------------------------------------------
SENTINEL = 12345


def _guarded(n, dtype):
    whole = torch.full((n + 8,), SENTINEL, dtype=dtype, device=DEV)
    return whole, whole[4:4 + n]


def _intact(*pairs):
    torch.cuda.synchronize()
    return all(bool((w[:4] == SENTINEL).all()) and bool((w[4 + v.shape[0]:] == SENTINEL).all()) for w, v in pairs)


def _raw(x, c, shrink_row=None):
    """COUNT then FILL through the C entry points on guarded outputs (dense ``x``).  ``shrink_row``: that row's room in
    out_rowptr is one entry short.  Returns (status bits, out_rowptr, out_col view, out_raw view)."""
    d = torch.device(DEV)
    xb, gm, (cg, gp, gc) = t(x), t(c.gene_map), _groups(c)
    n = x.shape[0]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    counts, totals = _guarded(n, torch.int32), _guarded(n, torch.float64)
    head = (_ptr(xb), x.shape[1], None, None, None, n, x.shape[1], _ptr(gm), c.n_genes, 0.0, _ptr(cg), _ptr(gp), _ptr(gc),
            len(c.group_ptr) - 1, len(c.group_cols))
    assert _lib.call(d, "wgnn_align_count_ln_merge", *head, None, _ptr(totals[1]), 1e4, _ptr(counts[1]), _ptr(status), 0,
                     _stream(d)) == 0
    assert _intact(counts, totals)
    k = counts[1].cpu().numpy().astype(np.int64)
    if shrink_row is not None:
        assert k[shrink_row] > 1
        k[shrink_row] -= 1
    rowptr = np.r_[0, np.cumsum(k)]
    out_rowptr = t(rowptr)
    col, raw = _guarded(int(rowptr[-1]), torch.int32), _guarded(int(rowptr[-1]), torch.float32)
    assert _lib.call(d, "wgnn_align_fill_ln_merge", *head, _ptr(totals[1]), 1e4, _ptr(out_rowptr), _ptr(col[1]), _ptr(raw[1]),
                     _ptr(status), 0, _stream(d)) == 0
    assert _intact(col, raw, counts, totals)
    return int(status), rowptr, col[1], raw[1]


def test_clean_operands_raise_no_bit_and_match_the_binding():
    c = _case()
    bits, rowptr, col, raw = _raw(c.x, c)
    assert bits == 0
    _equal((t(rowptr), col, raw), _merge(t(c.x), c, 0.0), "raw entry points")


@pytest.mark.parametrize("bad", [-1.0, float("nan")])
def test_a_bad_member_that_is_not_the_owner_is_reported(bad):
    c = _case()
    x = c.x.copy()
    first, later = M.GROUP_STEPS
    x[5, first], x[5, later] = 3, bad
    bits, rowptr, col, raw = _raw(x, c)
    assert bits == _lib.ALIGN_BAD_VALUE
    with pytest.raises(sda.WgnnError, match="negative, NaN or infinite"):
        _merge(t(x), c, 0.0)
    with pytest.raises(sda.WgnnError, match="negative, NaN or infinite"):
        _merge(tuple(t(a) for a in M.shuffled_csr(x, 2)), c, 0.0)


def test_a_group_table_that_points_at_column_n_cols_is_reported():
    c = _case()
    group_cols = c.group_cols.copy()
    s = c.col_group[M.GROUP_CHUNKS[0]]
    group_cols[c.group_ptr[s] + 2] = N_COLS                              # the group's last member
    bent = type("C", (), dict(gene_map=c.gene_map, col_group=c.col_group, group_ptr=c.group_ptr, group_cols=group_cols,
                              n_genes=G))
    assert (c.x[:, M.GROUP_CHUNKS[0]] > 0).any()
    bits, *_ = _raw(c.x, bent)
    assert bits == _lib.ALIGN_BAD_MAP
    with pytest.raises(sda.WgnnError, match="group table"):
        _merge(_strided(c.x, 701), bent, 0.0)
    col_group = c.col_group.copy()
    col_group[3] = len(c.group_ptr) - 1                                  # a group that does not exist
    bent = type("C", (), dict(gene_map=c.gene_map, col_group=col_group, group_ptr=c.group_ptr, group_cols=c.group_cols,
                              n_genes=G))
    assert _raw(c.x, bent)[0] == _lib.ALIGN_BAD_MAP
    with pytest.raises(sda.WgnnError, match="group table"):
        _merge(tuple(t(a) for a in L.to_csr(c.x)), bent, 0.0)


def test_a_row_with_too_little_room_on_fill_is_reported():
    c = _case()
    bits, rowptr, col, raw = _raw(c.x, c, shrink_row=6)
    assert bits == _lib.ALIGN_BAD_ROWPTR
    want = _merge(t(c.x), c, 0.0)
    b, e = want[0][6].item(), want[0][7].item()
    np.testing.assert_array_equal(col[rowptr[6]: rowptr[7]].cpu().numpy(), want[1][b: e - 1].cpu().numpy())   # what had room


# ------------------------------------------------------------------------------------------------
# 5. end to end on the golden bundles
# ------------------------------------------------------------------------------------------------
def _golden_bundle(tmp_path, name, species, tissue):
    """A bundle built from a golden fixture (as test_gpu_resident_predict._testis_bundle) and its test cells as integer counts."""
    from scdeepsort_amd.api import BundlePaths
    z = np.load(GOLDEN / f"{name}.npz")
    expr = sp.csr_matrix((z["data"], z["indices"], z["indptr"]), shape=tuple(z["shape"]))
    mask = z["support_mask"].astype(bool)
    genes = [f"Gene{i}" for i in range(expr.shape[1])]
    b = BundlePaths(tmp_path / name, species, tissue, layout="flat", for_write=True)
    b.mkdirs()
    b.genes.write_bytes("".join(g + "\r\n" for g in genes).encode())
    b.cell_types.write_bytes("".join(f"type{i}\r\n" for i in range(int(z["n_classes"]))).encode())
    sp.save_npz(b.support, sp.csr_matrix(expr[mask]))
    state = {k[len("param."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param.")}
    torch.save({"model": state, "optimizer": {}}, b.model)
    test = expr[~mask] if (~mask).any() else expr
    return tmp_path / name, np.ceil(test.toarray() * 4).astype(np.float32), genes


@pytest.mark.parametrize("name,species,tissue", [("testis199", "mouse", "Testis"), ("pancreas11", "human", "Pancreas")])
def test_split_columns_classify_as_the_unsplit_matrix(tmp_path, name, species, tissue):
    root, counts, genes = _golden_bundle(tmp_path, name, species, tissue)
    n = counts.shape[1]
    picked = np.argsort(-(counts > 3).sum(axis=0), kind="stable")[:6]     # six columns with counts a three-way split leaves > 0
    assert ((counts[:, picked] > 3).sum(axis=0) > 0).all()
    # the original column keeps ceil(c / 2) - so it stays the first counting member - and an alias column at the end of the
    # list takes floor(c / 2); the last picked gene is split three ways
    extra = list(picked) + [picked[-1]]
    alias_names = [f"ENS{j:011d}" for j in range(len(extra))]
    aliases = {a: genes[j] for a, j in zip(alias_names, extra)}
    split = np.concatenate([counts, np.zeros((counts.shape[0], len(extra)), np.float32)], axis=1)
    for k, j in enumerate(picked):
        split[:, n + k] = np.floor(counts[:, j] / 2)
        split[:, j] = counts[:, j] - split[:, n + k]
    third = np.floor(split[:, picked[-1]] / 2)
    split[:, n + len(picked)] = third
    split[:, picked[-1]] -= third
    names = genes + alias_names
    assert (split >= 0).all() and split.sum() == counts.sum() and (split[:, n:] > 0).any(axis=0).all()

    rp = sda.ResidentPredictor(species, tissue, model_path=root, aliases=aliases, duplicates="sum", normalize="lognorm")
    want = rp.classify(counts, genes=genes)                               # no collision: the existing kernels
    for batch in (split, sp.csr_matrix(split)):
        got = rp.classify(batch, genes=names)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(A.bits(got[1]), A.bits(want[1]))
        assert torch.equal(got[2], want[2])
    gm = rp.gene_map(names, aliases, "sum")
    assert isinstance(gm, sda.GeneMap) and gm.n_groups == 6 and gm.n_merged_columns == 13
    assert torch.equal(rp.classify(split, genes=gm)[2], want[2])
    with pytest.raises(ValueError, match='duplicates="sum" needs normalize='):
        sda.ResidentPredictor(species, tissue, model_path=root, aliases=aliases, duplicates="sum").classify(split, genes=names)

    cov, cov0 = rp.coverage(split, names), rp.coverage(counts, genes)
    np.testing.assert_array_equal(cov.total.view(np.uint64), cov0.total.view(np.uint64))
    assert cov.n_merged_columns == 13 and cov0.n_merged_columns == 0 and rp.coverage(split, gm).n_merged_columns == 13
    assert cov.n_matched == cov0.n_matched + 7 and cov.n_columns == n + 7

    # "drop": the colliding columns are unmatched - classifying without them, at the same library sizes
    drop = sda.ResidentPredictor(species, tissue, model_path=root, aliases=aliases, duplicates="drop", normalize="lognorm")
    rest = np.setdiff1d(np.arange(n), picked)
    less = sda.ResidentPredictor(species, tissue, model_path=root,
                                 normalize=sda.LogNormalize(library_size=counts.astype(np.float64).sum(axis=1)))
    got, want = drop.classify(split, genes=names), less.classify(counts[:, rest], genes=[genes[j] for j in rest])
    np.testing.assert_array_equal(got[0], want[0])
    assert torch.equal(got[2], want[2])
    assert drop.coverage(split, names).n_matched == n - 6
