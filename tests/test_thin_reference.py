"""CPU side of ``ResidentPredictor.stability(thin="reads")``: the read hash of ``wgnn_predict_rows_thin`` against known answers
worked out in arbitrary-precision integers, the binomial statistics, nesting and invariances of the thinning, the reference
of tests/thin_reference.py at ``keep`` 0 and 1, the share of unclear pairs of every GPU case, the C ABI's checks (which return
before any launch) and the host logic and argument errors of ``stability(thin="reads")``."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, api

import stability_reference as R
import thin_reference as T

ROOT = Path(__file__).resolve().parent.parent
W = 2 ** 64


def _mix64_long(x):
    x = (x + 0x9E3779B97F4A7C15) % W
    x = ((x ^ (x // 2 ** 30)) * 0xBF58476D1CE4E5B9) % W
    x = ((x ^ (x // 2 ** 27)) * 0x94D049BB133111EB) % W
    return x ^ (x // 2 ** 31)


# ------------------------------------------------------------------------------------------------
# the hash
# ------------------------------------------------------------------------------------------------
MIX64_KAT = [(0, 0xE220A8397B1DCDAF), (1, 0x910A2DEC89025CC1), (2 ** 64 - 1, 0xE4D971771B652C20)]
# ((seed, cell, draw, gene, read), the read's 32-bit hash), worked out step by step in arbitrary-precision integers
READ_KAT = [((0, 0, 0, 0, 0), 0xA706DD2F), ((1, 2, 3, 4, 5), 0xEC3D7ECD), ((2 ** 64 - 1, 5, 6, 7, 69999), 0xD8131042),
            ((0xBEEF, 2 ** 33 + 1, 2 ** 31 - 1, 6000, 2 ** 40), 0xB9438C53)]


@pytest.mark.parametrize("x,want", MIX64_KAT)
def test_mix64_known_answers(x, want):
    assert _mix64_long(x) == want                                 # splitmix64's first outputs for the states 0 and 1
    assert T.mix64(x) == want and int(T.mix64_np(np.array([x], np.uint64))[0]) == want
    assert R.mix32(x) == want >> 32                               # mix32 == mix64 >> 32


def test_mix32_is_the_upper_half_of_mix64():
    rng = np.random.default_rng(1)
    xs = rng.integers(0, 2 ** 63, 2000, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    np.testing.assert_array_equal(T.mix64_np(xs) >> np.uint64(32), [R.mix32(int(x)) for x in xs])
    np.testing.assert_array_equal(T.mix64_np(xs), [T.mix64(int(x)) for x in xs])


@pytest.mark.parametrize("args,want", READ_KAT)
def test_read_hash_known_answers(args, want):
    seed, cell, draw, gene, read = args
    key = seed ^ ((cell * 0x9FB21C651E98DF25) % W) ^ ((draw * 0xD6E8FEB86659FD93) % W)
    ek = _mix64_long((key + gene * 0xC2B2AE3D27D4EB4F) % W)
    u = _mix64_long((ek + read * 0xA0761D6478BD642F) % W) // 2 ** 32
    assert u == want
    assert T.entry_key(seed, cell, draw, gene) == ek and T.read_u(seed, cell, draw, gene, read) == u
    assert int(T.entry_key_np(seed, np.array([cell]), draw, np.array([gene]))[0]) == ek
    if read < 10 ** 5:                                            # the vectorised count agrees on the read's prefix
        n = T.kept_reads(seed, cell, draw, gene, read + 1, (u + 1) / 2 ** 32)[0] - T.kept_reads(seed, cell, draw, gene, read, (u + 1) / 2 ** 32)[0]
        assert n == 1
        assert T.kept_reads(seed, cell, draw, gene, read + 1, u / 2 ** 32)[0] == T.kept_reads(seed, cell, draw, gene, read, u / 2 ** 32)[0]


def test_constants_are_the_headers():
    text = (ROOT / "include" / "wgnn.h").read_text()
    for const in ("0xA0761D6478BD642F", "0xC2B2AE3D27D4EB4F", "4294967296.0"):
        assert const in text, const
    src = (ROOT / "scdeepsort_amd" / "csrc" / "wgnn_thin.hip").read_text()
    assert f"kTStash = {T.STASH};" in src and f"kTCoop = {T.COOP};" in src and "0xA0761D6478BD642Full" in src
    assert '#include "wgnn_align_rows.h"' in src and "log1p" not in re.sub(r"//.*", "", src)     # lognorm() is shared, not restated
    assert "float lognorm(float" in (ROOT / "scdeepsort_amd" / "csrc" / "wgnn_align_rows.h").read_text()
    assert "float lognorm(float" not in (ROOT / "scdeepsort_amd" / "csrc" / "wgnn_align.hip").read_text()


# ------------------------------------------------------------------------------------------------
# the thinning: statistics, nesting, invariances
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [0.25, 0.5, 0.9])
def test_kept_reads_are_binomial(keep):
    c = 200_000
    p = R.threshold(keep) / 2 ** 32
    for cell, draw, gene in ((0, 0, 0), (17, 3, 5999), (2 ** 33, 31, 6000)):
        got = int(T.kept_reads(99, cell, draw, gene, c, keep)[0])
        assert abs(got - c * p) <= 5 * np.sqrt(c * p * (1 - p)), (got, c * p)


def test_levels_are_nested_and_keep_one_and_zero():
    m, rest = T.count_batch()
    seed = 31337
    by_level = [T.thin_draw(m, rest, seed, 2, k) for k in (0.0, 0.25, 0.5, 0.9, 1.0)]
    for (lo_c, lo_r), (hi_c, hi_r) in zip(by_level, by_level[1:]):
        assert (lo_c <= hi_c).all() and (lo_r <= hi_r).all()
    assert not by_level[0][0].any() and not by_level[0][1].any()                  # keep = 0 keeps no read
    np.testing.assert_array_equal(by_level[-1][0], m.data.astype(np.int64))      # keep = 1 keeps every read
    np.testing.assert_array_equal(by_level[-1][1], rest)
    # read by read: a read kept at 0.25 is kept at 0.5
    ek = T.entry_key(seed, 8, 2, 123)
    u = [R.mix32((ek + i * T.K_READ) % W) for i in range(500)]
    assert all(x < R.threshold(0.5) for x in u if x < R.threshold(0.25))


def test_thinning_follows_the_gene_and_splits_by_row0_and_draw0():
    m, rest = T.count_batch()
    seed, keep = 4242, 0.5
    full_c, full_r = T.thin_draw(m, rest, seed, 3, keep)
    rng = np.random.default_rng(0)
    for r in (0, T.ROW_LONG, T.ROW_SPECIAL, 20):
        b, e = m.indptr[r], m.indptr[r + 1]
        perm = rng.permutation(e - b)
        got = T.kept_reads(seed, r, 3, m.indices[b:e][perm].astype(np.int64), m.data[b:e][perm].astype(np.int64), keep)
        np.testing.assert_array_equal(got, full_c[b:e][perm])
    cut = 17
    top_c, top_r = T.thin_draw(m[:cut], rest[:cut], seed, 3, keep)
    bot_c, bot_r = T.thin_draw(m[cut:], rest[cut:], seed, 3, keep, row0=cut)
    np.testing.assert_array_equal(np.concatenate([top_c, bot_c]), full_c)
    np.testing.assert_array_equal(np.concatenate([top_r, bot_r]), full_r)
    c = T.thin_case(12, 2, False, 0.25, 3)
    shifted = T.thin_case(12, 2, False, 0.25, 2, draw0=1)
    for k in ("label", "prob", "reads", "entries"):
        np.testing.assert_array_equal(c[k][:, 1:], shifted[k])


def test_the_batch_holds_what_the_gpu_tests_need():
    m, rest = T.count_batch()
    lens = np.diff(m.indptr)
    assert m.shape == (40, 6000) and (m.data == np.floor(m.data)).all() and m.data.min() >= 1
    assert lens[T.ROW_EMPTY] == 0 and lens[T.ROW_ONE] == 1 and m.data[m.indptr[T.ROW_ONE]] == 1 and rest[T.ROW_ONE] == 0
    assert lens[T.ROW_LONG] > T.STASH and {63, 64, 65} <= set(lens.tolist())
    assert (m.data[m.indptr[T.ROW_ONES]:m.indptr[T.ROW_ONES + 1]] == 1).all()
    assert {T.COOP - 1, T.COOP, T.COOP + 1, 1000, 70000} <= set(m.data.astype(int).tolist())
    assert {0, 1, 5000, 200000} <= set(rest.tolist())
    for keep in (0.25, 0.5, 0.9):                                # the long row outgrows the stash at every level
        cp, _ = T.thin_draw(m, rest, T.CASE_SEED, 0, keep)
        assert (cp[m.indptr[T.ROW_LONG]:m.indptr[T.ROW_LONG + 1]] > 0).sum() > T.STASH


# ------------------------------------------------------------------------------------------------
# the reference at keep 1 and keep 0, and the GPU cases' unclear pairs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vthr", [0.0, 1.5])
def test_keep_one_is_the_lognorm_batch_and_keep_zero_the_empty_row(vthr):
    H, Cn, D = 12, 5, 3
    m, rest = T.count_batch()
    _, table, alpha, bias = R.operands(H)
    one = T.thin_case(H, Cn, False, 1.0, D, vthr=vthr)
    full = T.lognorm_batch(m, rest, T.SCALE, vthr)
    assert (full.nnz < m.nnz) == (vthr > 0)                       # a positive threshold drops entries
    want = R.layer_draw(full, np.ones(full.nnz, bool), table, alpha, bias)
    for d in range(D):
        np.testing.assert_allclose(one["out"][d::D], want, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(one["reads"], np.repeat((np.asarray(m.sum(axis=1)).ravel().astype(np.int64) + rest)[:, None], D, 1))
    np.testing.assert_array_equal(one["entries"], np.repeat(np.diff(full.indptr)[:, None], D, 1))
    zero = T.thin_case(H, Cn, False, 0.0, D, vthr=vthr)
    assert zero["empty"].all() and not zero["reads"].any()
    np.testing.assert_allclose(zero["out"], np.broadcast_to(np.maximum(bias.astype(np.float64), 0), zero["out"].shape), atol=1e-15)


@pytest.mark.parametrize("case", T.THIN_CASES, ids=str)
def test_unclear_pairs_of_the_gpu_cases_stay_under_the_cap(case):
    H, Cn, explicit, _, keep, D = case
    c = T.thin_case(H, Cn, explicit, keep, D)
    assert c["unclear"].mean() <= 0.05, c["unclear"].mean()
    assert (c["label"] == -1).any() and (c["label"] >= 0).any()
    votes, unsure, empty, _ = R.tallies(c["label"], c["prob"], c["empty"], Cn)
    assert ((votes.sum(axis=1) + unsure) == D).all() and empty[T.ROW_EMPTY] == D


@pytest.mark.parametrize("case", T.MATERIALISED_CASES, ids=str)
def test_unclear_pairs_of_the_materialised_cases_stay_under_the_cap(case):
    H, Cn, explicit, keep, d = case
    c = T.thin_case(H, Cn, explicit, keep, d + 1)
    assert c["unclear"][:, d].mean() <= 0.05
    cp, rp = T.thin_draw(c["m"], c["rest"], T.CASE_SEED, d, keep)
    x = T.materialised(c["m"], cp, rp)
    np.testing.assert_array_equal(x.sum(axis=1).astype(np.int64), c["reads"][:, d])
    assert ((x[:, :-1] > 0).sum(axis=1) == c["entries"][:, d]).all()                 # threshold 0: every surviving gene takes part


# ------------------------------------------------------------------------------------------------
# the C ABI (no launch)
# ------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    assert re.search(r"\bwgnn_predict_rows_thin\s*\(", text)
    assert hasattr(lib, "wgnn_predict_rows_thin") and "wgnn_predict_rows_thin" in _lib.SIGNATURES
    assert int(re.search(r"#define\s+WGNN_THIN_ACCUMULATE\s+(\d+)", text).group(1)) == _lib.THIN_ACCUMULATE
    assert lib.wgnn_version() == 206
    assert sda.predict_rows_thin is sda.ops.predict_rows_thin and "predict_rows_thin" in sda.__all__
    from scdeepsort_amd import build
    assert "wgnn_thin.hip" in [p.name for p in build.SRC]
    n_args = len(re.search(r"\bwgnn_predict_rows_thin\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(","))
    assert n_args == len(_lib.SIGNATURES["wgnn_predict_rows_thin"][1])


def test_c_abi_errors_return_before_any_launch():
    """Host memory stands in for the operands: every call below must return from its argument checks with the documented
    code, and ``wgnn_last_error_string`` must name the check."""
    lib = _lib.lib()
    buf = (C.c_double * 8192)()
    base = (C.addressof(buf) + 15) // 16 * 16
    at = lambda i: base + 4096 * i

    def run(n_rows=4, H=8, ld=8, n_draws=3, row0=0, draw0=0, keep=0.5, out=at(6), head=False, votes=at(9), ld_votes=5, unsure=at(10),
            empty=at(11), conf=at(12), flags=0, self_rows=None, rest=at(14), scale=1e4, threshold=0.0, reads=None, entries=None):
        w, b, c = (at(7), at(8), 5) if head else (None, None, 0)
        return lib.wgnn_predict_rows_thin(at(0), at(1), at(2), n_rows, at(3), ld, 100, H, at(4), at(5), self_rows, ld,
                                          rest, scale, threshold, n_draws, row0, draw0, 12345, keep, None if head else out, ld,
                                          w, b, c, 0.1, votes if head else None, ld_votes, unsure if head else None,
                                          empty if head else None, conf if head else None, None, None, reads, entries, flags, None)

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert b"wgnn_predict_rows_thin" in msg and word in msg, (kw, msg)

    for keep in (-0.1, 1.5, float("nan")):
        fails(-1, b"keep", keep=keep)
        fails(-1, b"keep", keep=keep, head=True)
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        fails(-1, b"scale", scale=scale)
    for thr in (-0.5, float("nan")):
        fails(-1, b"threshold", threshold=thr)
    fails(-1, b"rest", rest=None)
    fails(-1, b"rest", rest=None, head=True)
    fails(-2, b"rest", rest=at(14) + 4)
    fails(-2, b"draw_reads", reads=at(13) + 2)
    fails(-2, b"draw_entries", entries=at(13) + 1)
    fails(-1, b"n_draws", n_draws=0)
    fails(-1, b"2^31", n_rows=2 ** 20, n_draws=2 ** 11)
    fails(-1, b"n_rows", n_rows=2 ** 31)
    fails(-2, b"multiple of 4", H=10, ld=12)
    fails(-3, b"256", H=260, ld=260)
    fails(-1, b"votes", head=True, votes=None)
    fails(-1, b"conf_sum", head=True, conf=None)
    fails(-1, b"ld_votes", head=True, ld_votes=4)
    fails(-1, b"WGNN_THIN_ACCUMULATE", flags=1)
    fails(-1, b"needs a head", flags=256)
    fails(-1, b"row0", row0=-1)
    fails(-1, b"draw0", draw0=-1)
    fails(-1, b"out", out=None)
    fails(-2, b"ld_out", out=at(6) + 4)
    fails(-2, b"conf_sum", head=True, conf=at(12) + 4)
    fails(-2, b"self_rows", self_rows=at(13) + 4)
    assert run(n_rows=0) == 0 and run(n_rows=0, head=True, flags=256 | 16) == 0      # an empty batch is a no-op


def test_ops_refuses_cpu_tensors_and_bad_arguments():
    rp = torch.tensor([0, 1], dtype=torch.int32)
    args = (rp, torch.zeros(1, dtype=torch.int32), torch.ones(1), torch.zeros(3, 8), torch.ones(5), torch.zeros(8))
    with pytest.raises(sda.WgnnError):
        sda.predict_rows_thin(*args, rest=torch.zeros(1, dtype=torch.int64), n_draws=2, keep=0.5, seed=0)


# ------------------------------------------------------------------------------------------------
# the host logic of stability(thin="reads")
# ------------------------------------------------------------------------------------------------
def _table(thin, n_reads=None):
    votes = torch.tensor([[[0, 8], [8, 0]]], dtype=torch.int32)
    return api.Stability(keep=(0.5,), n_draws=8, label=np.array([1, 0]), max_prob=np.array([0.9, 0.8], np.float32), votes=votes,
                         unsure=torch.zeros((1, 2), dtype=torch.int32), empty=torch.zeros((1, 2), dtype=torch.int32),
                         conf_sum=torch.tensor([[7.2, 6.4]], dtype=torch.float64), n_entries=np.array([900, 40]),
                         index=["a", "b"], id2label=["T0", "T1"], seed=5, thin=thin, n_reads=n_reads)


def test_stability_table_carries_thin_and_n_reads():
    reads = _table("reads", np.array([12000, 300]))
    genes = _table("genes")
    assert api.Stability.__dataclass_fields__["thin"].default == "genes"
    assert list(reads.frame().columns)[:5] == ["index", "cell_type", "prob", "n_genes", "n_reads"]
    assert reads.frame()["n_reads"].tolist() == [12000, 300] and "n_reads" not in genes.frame().columns
    assert reads.summary()["thin"] == "reads" and "thinned by reads" in str(reads.summary())
    assert "thinned by genes" in str(genes.summary()) and len(str(reads.summary()).splitlines()) == 3
    reads._require_same((0.5,), 2, ["T0", "T1"], 5, "reads")
    genes._require_same((0.5,), 2, ["T0", "T1"], 5)                # the default is today's
    with pytest.raises(ValueError, match="thin"):
        reads._require_same((0.5,), 2, ["T0", "T1"], 5, "genes")
    with pytest.raises(ValueError, match="thin"):
        genes._require_same((0.5,), 2, ["T0", "T1"], 5, "reads")


def test_stability_thin_argument_errors():
    class Fake(api.ResidentPredictor):                            # the checks run before the device is touched
        def __init__(self):
            self.hidden_padded, self.n_classes, self.id2label = 12, 3, ["T0", "T1", "T2"]
            self.normalize, self.duplicates, self.aliases = None, "error", None

    rp, batch, genes = Fake(), np.zeros((4, 7), np.float32), [f"g{i}" for i in range(7)]
    with pytest.raises(ValueError, match="thin"):
        rp.stability(batch, thin="counts")
    with pytest.raises(ValueError, match="genes="):
        rp.stability(batch, thin="reads", normalize="lognorm")     # no gene list
    with pytest.raises(ValueError, match="normalize"):
        rp.stability(batch, thin="reads", genes=genes)             # no normalize spec
    ids = torch.zeros(7, dtype=torch.int32)
    merged = api.GeneMap(ids=ids, col_group=ids, group_ptr=torch.tensor([0, 2], dtype=torch.int32),
                         group_cols=torch.tensor([0, 1], dtype=torch.int32), n_groups=1, n_merged_columns=2)
    with pytest.raises(ValueError, match="merged"):
        rp.stability(batch, thin="reads", genes=merged, normalize="lognorm")
    rp.duplicates = "sum"
    with pytest.raises(ValueError, match="merged"):
        rp.stability(batch, thin="reads", genes=genes, normalize="lognorm")
    rp.duplicates = "error"
    with pytest.raises(ValueError, match="into"):
        rp.stability(batch, thin="reads", genes=genes, normalize="lognorm", into=_table("genes"), keep=(0.5,), seed=5)
    with pytest.raises(ValueError, match="n_draws"):
        rp.stability(batch, thin="reads", genes=genes, normalize="lognorm", n_draws=0)
    with pytest.raises(ValueError, match="normalize"):
        rp.stability_file("nowhere.csv", thin="reads")
