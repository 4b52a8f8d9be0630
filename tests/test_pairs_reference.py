"""CPU side of ``ResidentPredictor.doublets``: the partner hash and rule against known answers worked out from the documented
constants in arbitrary-precision integers, the torch restatement of the rule against the numpy one, the ``Doublets`` table
arithmetic on hand-made arrays, the C entries' argument checks (which return before any launch), the host-side operand
helpers, the share of fragile values of every GPU case, and the argument errors of ``doublets``."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, api, ops

import pairs_reference as P

ROOT = Path(__file__).resolve().parent.parent
W = 2 ** 64


def _mix64_long(x):
    x = (x + 0x9E3779B97F4A7C15) % W
    x = ((x ^ (x // 2 ** 30)) * 0xBF58476D1CE4E5B9) % W
    x = ((x ^ (x // 2 ** 27)) * 0x94D049BB133111EB) % W
    return x ^ (x // 2 ** 31)


def _u_long(seed, cell, draw):
    key = (seed % W) ^ ((cell * 0x9FB21C651E98DF25) % W) ^ ((draw * 0xD6E8FEB86659FD93) % W)
    return _mix64_long((key + 0x9E3779B97F4A7C15) % W)


# ------------------------------------------------------------------------------------------------
# the hash and the partner rule
# ------------------------------------------------------------------------------------------------
# key(0, 0, 0) = 0, so u = mix64(GOLDEN) = mix64 applied to splitmix64's state after one step: its SECOND output for seed 0
U_KAT = [((0, 0, 0), 0x6E789E6AA1B965F4)]


@pytest.mark.parametrize("args,want", U_KAT)
def test_partner_hash_known_answer(args, want):
    assert _u_long(*args) == want
    assert int(P.partner_u(*args)) == want


@pytest.mark.parametrize("args", [(0, 0, 0), (1, 2, 3), (2 ** 64 - 1, 59, 15), (0xBEEF, 2 ** 20, 2 ** 31 - 1), (-7, 3, 1)])
def test_partner_hash_in_numpy_and_torch_is_the_integer_one(args):
    seed, cell, draw = args
    want = _u_long(seed, cell, draw)
    assert int(P.partner_u(seed, cell, draw)) == want
    key = (torch.tensor([cell]) * api._i64(0x9FB21C651E98DF25)) ^ (torch.tensor([draw]) * api._i64(0xD6E8FEB86659FD93)) ^ api._i64(seed)
    got = int(api._mix64(key + api._i64(0x9E3779B97F4A7C15))[0])
    assert got % W == want


def test_partner_rule_by_hand():
    # four cells, calls (1, 0, 1, -1): the order by (call, index) is [3, 1, 0, 2]; groups: unsure {3}, type 0 {1}, type 1 {0, 2}
    label = np.array([1, 0, 1, -1])
    got = P.partners(label, 3, 5, "types")
    order = [3, 1, 0, 2]
    for c, (start, size) in enumerate([(2, 2), (1, 1), (2, 2), (0, 1)]):
        for d in range(3):
            k = _u_long(5, c, d) % (4 - size)
            assert got[c, d] == order[k if k < start else k + size]
    anyone = P.partners(label, 3, 5, "any")
    for c in range(4):
        for d in range(3):
            k = _u_long(5, c, d) % 3
            assert anyone[c, d] == k + (k >= c)


@pytest.mark.parametrize("across", ["types", "any"])
def test_torch_partners_are_the_numpy_rule(across):
    rng = np.random.default_rng(3)
    label = rng.integers(-1, 5, 97)
    for seed, draw0 in ((0, 0), (2 ** 63 + 12345, 7)):
        got = api._draw_partners(torch.from_numpy(label), 6, seed, across, draw0).numpy()
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, P.partners(label, 6, seed, across, draw0))
    # draws are a function of (seed, cell, draw): 3 and 3 more are 6 at once
    six = api._draw_partners(torch.from_numpy(label), 6, 9, across).numpy()
    np.testing.assert_array_equal(api._draw_partners(torch.from_numpy(label), 3, 9, across, 3).numpy(), six[:, 3:])


def test_types_never_pairs_two_cells_of_one_group_and_any_never_a_cell_with_itself():
    rng = np.random.default_rng(8)
    label = rng.integers(-1, 4, 200)
    p = P.partners(label, 16, 1, "types")
    assert (label[p] != label[:, None]).all()
    assert len(np.unique(p)) > 150                                    # the partners spread over the batch
    q = P.partners(label, 16, 1, "any")
    assert (q != np.arange(200)[:, None]).all() and (label[q] == label[:, None]).any()
    # uniform over the eligible cells: a chi-square bound on 200 x 64 draws over 199 cells
    counts = np.bincount(P.partners(label, 64, 2, "any").ravel(), minlength=200)
    assert abs(counts - 64).max() < 6 * np.sqrt(64)


def test_single_group_and_single_cell_raise():
    with pytest.raises(ValueError, match="across=\"any\""):
        api._draw_partners(torch.zeros(5, dtype=torch.int64), 2, 0, "types")
    with pytest.raises(ValueError, match="one cell"):
        api._draw_partners(torch.zeros(1, dtype=torch.int64), 2, 0, "any")
    assert api._draw_partners(torch.zeros(5, dtype=torch.int64), 2, 0, "any").shape == (5, 2)


# ------------------------------------------------------------------------------------------------
# the Doublets tables on hand-made arrays
# ------------------------------------------------------------------------------------------------
def _table():
    # cells 0, 1: type 0; cell 2: type 1; cell 3: type 2; cell 4: unsure
    label = np.array([0, 0, 1, 2, -1])
    partner = np.array([[2, 3, 1], [2, 2, 4], [0, 3, 3], [0, 1, 2], [0, 2, 3]], np.int32)
    draw_label = np.array([[0, 1, 0], [2, -1, 0], [1, 0, 0], [2, 2, -1], [0, 1, 2]], np.int32)
    draw_prob = np.full((5, 3), 0.5, np.float32)
    draw_prob[0, 0] = 0.9
    return api.Doublets(label=label, max_prob=np.ones(5, np.float32), partner=partner, draw_label=draw_label, draw_prob=draw_prob,
                        index=list("abcde"), id2label=["T0", "T1", "T2"], seed=3, across="any")


def test_doublets_table_arithmetic():
    d = _table()
    assert d.n_partners == 3
    t = d.pair_table()
    assert t.shape == (4, 4, 4) and t.sum() == 15
    assert t[0, 1, 0] == 1 and t[0, 1, 2] == 1 and t[0, 1, 3] == 1 and t[0, 0, 0] == 1 and t[0, 3, 0] == 1 and t[3].sum() == 3
    # heterotypic pairs (both parents called, different): (0,2)->0 (0,3)->1 | (1,2)->2 (1,2)->-1 | (2,0)->1 (2,3)->0 (2,3)->0 |
    # (3,0)->2 (3,1)->2 (3,2)->-1: ten pairs
    f = d.frame()
    assert list(f.columns) == ["type_a", "type_b", "n", "parent_share", "third_share", "unsure_share", "top_third", "mean_prob"]
    assert f[["type_a", "type_b"]].values.tolist() == [["T0", "T1"], ["T0", "T2"], ["T1", "T2"]] and f["n"].tolist() == [4, 3, 3]
    np.testing.assert_allclose(f["parent_share"], [2 / 4, 2 / 3, 0.0])
    np.testing.assert_allclose(f["third_share"], [1 / 4, 1 / 3, 2 / 3])
    np.testing.assert_allclose(f["unsure_share"], [1 / 4, 0.0, 1 / 3])
    assert f["top_third"].tolist() == ["T2", "T1", "T0"]
    np.testing.assert_allclose(f["mean_prob"], [(0.9 + 1.5) / 4, 0.5, 0.5])
    assert d.caught() == pytest.approx(2 / 10)
    # called T0: (0,2) parent, (2,3) x 2 foreign; T1: (0,3) foreign, (2,0) parent; T2: (1,2) foreign, (3,0), (3,1) parents
    np.testing.assert_allclose(d.sinks(), [2 / 3, 1 / 2, 1 / 3])
    q, r = np.array([2, 1, 1]) / 10, np.array([2, 1, 1]) / 5
    np.testing.assert_allclose(d.artifact_risk(0.1), 0.1 * q / (0.1 * q + 0.9 * r))
    np.testing.assert_allclose(d.artifact_risk(0.0), 0.0)
    with pytest.raises(ValueError, match="rate"):
        d.artifact_risk(1.5)
    np.testing.assert_allclose(d.dominance(), [1 / 2, 0.0, 1 / 3, 2 / 3, np.nan])
    s = d.summary()
    assert s["n_heterotypic"] == 10 and s["parent_share"] == pytest.approx(0.4) and s["third_share"] == pytest.approx(0.4)
    assert s["caught"] == pytest.approx(0.2) and s["top_sink"] == "T0" and s["top_sink_pairs"] == 2
    assert "10 heterotypic pairs" in str(s) and len(str(s).splitlines()) == 3
    d._require_same(5, ["T0", "T1", "T2"], 3, "any")
    for bad in ((4, ["T0", "T1", "T2"], 3, "any"), (5, ["T0"], 3, "any"), (5, ["T0", "T1", "T2"], 4, "any"),
                (5, ["T0", "T1", "T2"], 3, "types")):
        with pytest.raises(ValueError, match="into"):
            d._require_same(*bad)


def test_doublets_tables_of_a_batch_without_heterotypic_pairs():
    d = api.Doublets(label=np.array([0, 0]), max_prob=np.ones(2, np.float32), partner=np.array([[1], [0]], np.int32),
                     draw_label=np.array([[0], [0]], np.int32), draw_prob=np.ones((2, 1), np.float32), index=[0, 1],
                     id2label=["T0", "T1"], across="any")
    assert len(d.frame()) == 0 and np.isnan(d.caught()) and np.isnan(d.sinks()).all() and np.isnan(d.dominance()).all()
    np.testing.assert_array_equal(d.artifact_risk(), [0.0, np.nan])
    assert d.summary()["n_heterotypic"] == 0 and d.summary()["top_sink"] is None


# ------------------------------------------------------------------------------------------------
# the reference's cases
# ------------------------------------------------------------------------------------------------
def test_the_batch_holds_what_the_gpu_tests_need():
    m = P.batch()
    lens = np.diff(m.rowptr)
    assert m.G == 300 and {0, 1, 63, 64, 65, 130, 300} <= set(lens.tolist())
    for r in range(m.B):
        assert (np.diff(m.col[m.rowptr[r]:m.rowptr[r + 1]]) > 0).all()                    # strictly ascending
    assert (m.cnt == np.floor(m.cnt)).all() and m.cnt.min() >= 1 and m.cnt.max() == ops.PAIR_MAX_COUNT
    row = lambda r: set(m.col[m.rowptr[r]:m.rowptr[r + 1]].tolist())
    assert not row(P.ROW_LOW) & row(P.ROW_HIGH) and not row(P.ROW_EVEN) & row(P.ROW_ODD)
    assert row(P.ROW_130) == row(P.ROW_130_TWIN)
    long = sorted(row(P.ROW_LONG))
    assert row(P.ROW_BEFORE).pop() < long[0] and row(P.ROW_AFTER).pop() > long[-1]
    assert row(P.ROW_INSIDE) <= row(P.ROW_LONG) and long[0] < min(row(P.ROW_GAP)) < long[-1] and not row(P.ROW_GAP) & row(P.ROW_LONG)
    merged = sorted([(g, 0) for g in row(P.ROW_EDGE_A)] + [(g, 1) for g in row(P.ROW_EDGE_B)])
    assert merged[63] == (100, 0) and merged[64] == (100, 1)                             # the match straddles the 64-wide step
    assert m.lib[P.ROW_EMPTY] == 0 and m.lib[P.ROW_EMPTY_READS] == 7 and (m.rest > 0).sum() >= 5
    assert (m.lib < 2 ** 31).all()


@pytest.mark.parametrize("threshold", P.THRESHOLDS)
def test_fragile_values_of_the_gpu_cases_stay_under_the_cap(threshold):
    c = P.case(threshold)
    assert c.v64.size > 50_000 and P.fragile(c.v64).mean() <= 1e-4
    kept = np.diff(c.rowptr).reshape(c.m.B, c.m.B)
    assert kept[P.ROW_EMPTY, P.ROW_EMPTY] == 0 and kept[P.ROW_EMPTY, P.ROW_EMPTY_READS] == 0       # both rows empty
    zero = P.case(0.0)
    if threshold > 0:
        assert 0 < c.v64.size < zero.v64.size and c.val.min() > threshold             # the threshold drops entries, not all
    else:
        lens = np.diff(c.m.rowptr)
        assert kept[P.ROW_LOW, P.ROW_HIGH] == 200 and kept[P.ROW_EVEN, P.ROW_ODD] == 300 and kept[P.ROW_130, P.ROW_130_TWIN] == 130
        np.testing.assert_array_equal(np.diag(kept)[lens > 0], lens[lens > 0])          # a self pair keeps the row's genes
        assert kept[P.ROW_LONG, P.ROW_INSIDE] == 99 and kept[P.ROW_LONG, P.ROW_GAP] == 100 and kept[P.ROW_BEFORE, P.ROW_LONG] == 100


def test_reference_is_align_on_the_summed_matrix():
    """The numpy merge against the numpy lognorm alignment of the dense summed counts: the same structure, the same fp64 values."""
    from lognorm_reference import lognorm_dense
    c = P.case(1.5)
    x, gmap = P.summed_dense(c.m.rowptr, c.m.col, c.m.cnt, c.m.lib, c.a, c.b, c.m.G)
    np.testing.assert_array_equal(x.sum(axis=1, dtype=np.float64), (c.m.lib[c.a] + c.m.lib[c.b]).astype(np.float64))
    rowptr, col, val, v64 = lognorm_dense(x, gmap, 1.5, fp64=True)
    np.testing.assert_array_equal(rowptr, c.rowptr); np.testing.assert_array_equal(col, c.col)
    np.testing.assert_array_equal(v64, c.v64)


# ------------------------------------------------------------------------------------------------
# the C ABI (no launch) and the host helpers
# ------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name in ("wgnn_pair_rows_count", "wgnn_pair_rows_fill"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1])
    for bit in ("BAD_INDEX", "UNSORTED", "BAD_ROWPTR"):
        assert int(re.search(r"#define\s+WGNN_PAIR_%s\s+(\d+)" % bit, text).group(1)) == getattr(_lib, "PAIR_" + bit)
    assert lib.wgnn_version() == 206
    assert sda.pair_rows is ops.pair_rows and sda.Doublets is api.Doublets and {"pair_rows", "Doublets"} <= set(sda.__all__)
    from scdeepsort_amd import build
    assert "wgnn_pairs.hip" in [p.name for p in build.SRC]
    src = (ROOT / "scdeepsort_amd" / "csrc" / "wgnn_pairs.hip").read_text()
    assert '#include "wgnn_align_rows.h"' in src and "log1p" not in re.sub(r"//.*", "", src)     # lognorm() is shared, not restated
    assert "atomic" not in re.sub(r"//.*", "", src).replace("atomicOr(p.status", "")             # the status word's OR alone


def test_c_abi_errors_return_before_any_launch():
    """Host memory stands in for the operands: every call below must return from its argument checks with the documented
    code, and ``wgnn_last_error_string`` must name the check."""
    lib = _lib.lib()
    buf = (C.c_double * 4096)()
    base = (C.addressof(buf) + 15) // 16 * 16
    at = lambda i: base + 2048 * i

    def run(fill, rowptr=at(0), col=at(1), cnt=at(2), n_rows=4, nnz=10, lib_=at(3), a=at(4), b=at(5), n_pairs=3, scale=1e4,
            threshold=0.0, n_out=at(6), out_rowptr=at(7), out_col=at(8), out_val=at(9), status=at(10), flags=0):
        head = (rowptr, col, cnt, n_rows, nnz, lib_, a, b, n_pairs, scale, threshold)
        if fill:
            return lib.wgnn_pair_rows_fill(*head, out_rowptr, out_col, out_val, status, flags, None)
        return lib.wgnn_pair_rows_count(*head, n_out, status, flags, None)

    def fails(code, word, only=None, **kw):
        for fill in (False, True) if only is None else (only,):
            assert run(fill, **kw) == code, (fill, kw)
            msg = lib.wgnn_last_error_string(code)
            assert (b"wgnn_pair_rows_fill" if fill else b"wgnn_pair_rows_count") in msg and word in msg, (kw, msg)

    fails(-1, b"status", status=None)
    for name in ("rowptr", "lib_", "a", "b"):
        fails(-1, b"required", **{name: None})
    fails(-1, b"col and cnt", col=None)
    fails(-1, b"col and cnt", cnt=None)
    fails(-1, b"n_out", only=False, n_out=None)
    fails(-1, b"out_rowptr", only=True, out_rowptr=None)
    fails(-1, b"n_rows", n_rows=-1)
    fails(-1, b"n_rows", n_rows=2 ** 31)
    fails(-1, b"nnz", nnz=-1)
    fails(-1, b"n_pairs", n_pairs=-1)
    fails(-1, b"n_pairs", n_pairs=2 ** 31)
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        fails(-1, b"scale", scale=scale)
    for thr in (-0.5, float("nan")):
        fails(-1, b"threshold", threshold=thr)
    fails(-1, b"WGNN_FLAG_ROWPTR_I64", flags=1)
    fails(-1, b"WGNN_FLAG_ROWPTR_I64", flags=16 | 256)
    fails(-2, b"lib", lib_=at(3) + 4)
    fails(-2, b"out_rowptr", only=True, out_rowptr=at(7) + 4)
    fails(-2, b"rowptr", rowptr=at(0) + 4, flags=16)
    fails(-2, b"rowptr", rowptr=at(0) + 2)
    fails(-2, b"4-byte", a=at(4) + 2)
    fails(-2, b"4-byte", cnt=at(2) + 1)
    fails(-2, b"4-byte", only=True, out_val=at(9) + 2)
    assert run(False, n_pairs=0) == 0 and run(True, n_pairs=0, flags=16) == 0        # an empty pair list is a no-op
    assert run(False, n_pairs=0, rowptr=None, lib_=None, a=None, b=None, n_out=None) == 0


def test_ops_refuses_cpu_tensors_and_bad_arguments():
    rp, col, cnt = torch.tensor([0, 1, 2]), torch.zeros(2, dtype=torch.int32), torch.ones(2)
    lib, a = torch.ones(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(sda.WgnnError):
        sda.pair_rows(rp, col, cnt, lib, a, a)


def test_csr_rows_ascending_and_the_count_cap():
    rp = torch.tensor([0, 3, 3, 5])
    col = torch.tensor([4, 9, 7, 0, 2], dtype=torch.int32)
    val = torch.tensor([1., 2., 3., 4., 5.])
    out = ops.csr_rows_ascending(rp, col, val)
    assert out[1].tolist() == [4, 7, 9, 0, 2] and out[2].tolist() == [1., 3., 2., 4., 5.] and out[0] is rp
    same = ops.csr_rows_ascending(rp, out[1], out[2])
    assert same[1] is out[1] and same[2] is out[2]                    # an ascending operand is handed back as it is
    with pytest.raises(sda.WgnnError, match="row 2 lists column 2 twice"):
        ops.csr_rows_ascending(rp, torch.tensor([4, 9, 7, 2, 2], dtype=torch.int32), val)
    with pytest.raises(sda.WgnnError, match="row 0 lists column 9 twice"):
        ops.csr_rows_ascending(rp, torch.tensor([9, 4, 9, 0, 2], dtype=torch.int32), val)
    empty = (torch.tensor([0, 0]), torch.zeros(0, dtype=torch.int32), torch.zeros(0))
    assert ops.csr_rows_ascending(*empty)[1] is empty[1]
    ops.pair_operand_check(rp, torch.tensor([1., 2., 2. ** 23, 4., 5.]))
    with pytest.raises(sda.WgnnError, match="cell 2 holds a count above 2\\^23"):
        ops.pair_operand_check(rp, torch.tensor([1., 2., 3., 2. ** 23 + 1, 5.]))
    # stability's check is as it was: 2^24 passes there
    ops.thin_operand_check(rp, torch.tensor([1., 2., 3., 2. ** 24, 5.]), torch.zeros(3, dtype=torch.float64),
                           torch.tensor([6., 0., 2. ** 24 + 5], dtype=torch.float64))


# ------------------------------------------------------------------------------------------------
# doublets' argument errors (before the device is touched)
# ------------------------------------------------------------------------------------------------
def test_doublets_argument_errors():
    class Fake(api.ResidentPredictor):
        def __init__(self):
            self.hidden_padded, self.n_classes, self.id2label = 12, 3, ["T0", "T1", "T2"]
            self.normalize, self.duplicates, self.aliases = None, "error", None

    rp, batch, genes = Fake(), np.zeros((5, 7), np.float32), [f"g{i}" for i in range(7)]
    with pytest.raises(ValueError, match="across"):
        rp.doublets(batch, genes, normalize="lognorm", across="clusters")
    with pytest.raises(ValueError, match="n_partners"):
        rp.doublets(batch, genes, normalize="lognorm", n_partners=0)
    with pytest.raises(ValueError, match="genes="):
        rp.doublets(batch, None, normalize="lognorm")
    with pytest.raises(ValueError, match="normalize"):
        rp.doublets(batch, genes)
    ids = torch.zeros(7, dtype=torch.int32)
    merged = api.GeneMap(ids=ids, col_group=ids, group_ptr=torch.tensor([0, 2], dtype=torch.int32),
                         group_cols=torch.tensor([0, 1], dtype=torch.int32), n_groups=1, n_merged_columns=2)
    with pytest.raises(ValueError, match="merged"):
        rp.doublets(batch, merged, normalize="lognorm")
    rp.duplicates = "sum"
    with pytest.raises(ValueError, match="merged"):
        rp.doublets(batch, genes, normalize="lognorm")
    rp.duplicates = "error"
    with pytest.raises(ValueError, match="into"):
        rp.doublets(batch, genes, normalize="lognorm", into=_table(), seed=3, across="types")
    with pytest.raises(ValueError, match="index"):
        rp.doublets(batch, genes, normalize="lognorm", index=["a"])
