"""CPU side of ``ResidentPredictor.stability``: the hash of ``wgnn_predict_rows_dropout`` against known answers worked out step
by step in arbitrary-precision integers, the fp64 reference of tests/stability_reference.py at ``keep`` 0 and 1, the mask's
statistics and invariances, the share of unclear pairs of every GPU case, the C ABI's checks (which return before any launch)
and the host logic of ``Stability`` on hand-made tallies."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, api

import stability_reference as R

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------
# the hash and the mask
# ------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), 0xE220A839), ((1, 2, 3, 4), 0x4E13DD59), ((2 ** 64 - 1, 5, 6, 7), 0x7086FD0F),
       ((12345, 2 ** 32 + 17, 1, 5999), 0x9F144077), ((0xC0FFEE, 2 ** 40 + 3, 2 ** 31 - 1, 19999), 0xF4D6B296),
       ((2 ** 64 - 1, 2 ** 33, 31, 0), 0xB1F45BF6), ((7, 39, 32, 123456), 0xB0CB6EDF)]


@pytest.mark.parametrize("args,want", KAT)
def test_hash_known_answers(args, want):
    seed, cell, draw, gene = args
    W = 2 ** 64
    key = seed ^ ((cell * 0x9FB21C651E98DF25) % W) ^ ((draw * 0xD6E8FEB86659FD93) % W)
    x = (key + gene * 0xC2B2AE3D27D4EB4F) % W
    x = (x + 0x9E3779B97F4A7C15) % W
    x = ((x ^ (x // 2 ** 30)) * 0xBF58476D1CE4E5B9) % W
    x = ((x ^ (x // 2 ** 27)) * 0x94D049BB133111EB) % W
    x = x ^ (x // 2 ** 31)
    u = x // 2 ** 32
    assert u == want                                             # (0, 0, 0, 0): splitmix64's first output for state 0, upper half
    assert R.hash_u(*args) == want
    assert int(R.hash_u_np(seed, np.array([cell]), np.array([draw]), np.array([gene]))[0]) == want
    assert bool(R.mask(seed, np.array([cell]), draw, np.array([gene]), 1.0)[0])
    assert not bool(R.mask(seed, np.array([cell]), draw, np.array([gene]), 0.0)[0])
    assert bool(R.mask(seed, np.array([cell]), draw, np.array([gene]), (want + 1) / 2 ** 32)[0])
    assert not bool(R.mask(seed, np.array([cell]), draw, np.array([gene]), want / 2 ** 32)[0])


def test_threshold_is_the_headers():
    assert R.threshold(1.0) == 2 ** 32 and R.threshold(0.0) == 0 and R.threshold(0.5) == 2 ** 31
    assert R.threshold(0.25) == 2 ** 30 and R.threshold(0.9) == int(np.floor(0.9 * 4294967296.0))
    text = (ROOT / "include" / "wgnn.h").read_text()
    for const in ("0x9FB21C651E98DF25", "0xD6E8FEB86659FD93", "0xC2B2AE3D27D4EB4F", "0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9",
                  "0x94D049BB133111EB", "4294967296.0"):
        assert const in text, const


@pytest.mark.parametrize("keep", [0.1, 0.5, 0.9])
def test_kept_share_is_binomial(keep):
    n = 10 ** 6
    cells = np.repeat(np.arange(1000, dtype=np.int64), 1000)
    genes = np.tile(np.arange(1000, dtype=np.int64) * 17 + 3, 1000)
    share = R.mask(99, cells, 4, genes, keep).mean()
    assert abs(share - keep) <= 5 * np.sqrt(keep * (1 - keep) / n), share


def test_mask_follows_the_gene_and_splits_by_row0_and_draw0():
    m, _, _, _ = R.operands(12)
    seed, keep = 31337, 0.5
    full = [R.entry_mask(m, seed, d, keep) for d in range(6)]
    rng = np.random.default_rng(0)
    # permuting a row's entries permutes its mask with them
    for r in (0, 3, 7, 20):
        b, e = m.indptr[r], m.indptr[r + 1]
        perm = rng.permutation(e - b)
        genes = m.indices[b:e].astype(np.int64)
        np.testing.assert_array_equal(R.mask(seed, r, 2, genes[perm], keep), full[2][b:e][perm])
    # the lower part of the batch with row0 = 0, the upper with row0 = 17: the masks of the whole
    top, bottom = m[:17], m[17:]
    for d in (0, 5):
        got = np.concatenate([R.entry_mask(top, seed, d, keep), R.entry_mask(bottom, seed, d, keep, row0=17)])
        np.testing.assert_array_equal(got, full[d])
    # draw0 shifts the draw number
    np.testing.assert_array_equal(R.mask(seed, 3, 4 + 1, m.indices[:50].astype(np.int64), keep),
                                  R.hash_u_np(seed, 3, 5, m.indices[:50].astype(np.int64)) < np.uint64(R.threshold(keep)))
    c = R.masked_case(12, 2, False, 0.25, 3)
    shifted = R.masked_case(12, 2, False, 0.25, 2, draw0=1)
    np.testing.assert_array_equal(c["label"][:, 1:], shifted["label"])
    np.testing.assert_array_equal(c["prob"][:, 1:], shifted["prob"])
    # nested levels: what is kept at 0.25 is kept at 0.5
    assert not (R.entry_mask(m, seed, 1, 0.25) & ~R.entry_mask(m, seed, 1, 0.5)).any()


# ------------------------------------------------------------------------------------------------
# the reference at keep 1 and keep 0, and the GPU cases' unclear pairs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("explicit", [False, True])
def test_keep_one_is_the_full_call_and_keep_zero_the_empty_row(explicit):
    H, Cn, D = 12, 5, 4
    m, table, alpha, bias = R.operands(H)
    w, b = R.head_operands(H, Cn)
    B = m.shape[0]
    one = R.masked_case(H, Cn, explicit, 1.0, D)
    sr = one["self_rows"]
    for d in range(D):
        h_full = R.layer_draw(m, np.ones(m.nnz, bool), table, alpha, bias, None if sr is None else sr[d::D])
        np.testing.assert_array_equal(one["out"][d::D], h_full)
        lg, p = R.head(h_full, w, b)
        np.testing.assert_array_equal(one["label"][:, d], R.labels(lg, p, one["thr"]))
    assert one["empty"].sum(axis=1).tolist() == [D if n == 0 else 0 for n in np.diff(m.indptr)]
    zero = R.masked_case(H, Cn, explicit, 0.0, D)
    assert zero["empty"].all()
    a_self = float(alpha[-1])
    for d in range(D):
        z = bias.astype(np.float64) + (0.0 if sr is None else a_self * zero["self_rows"][d::D].astype(np.float64))
        want = np.broadcast_to(np.maximum(z, 0.0), (B, H))
        np.testing.assert_allclose(zero["out"][d::D], want, rtol=0, atol=1e-15)
        lg, p = R.head(want, w, b)
        np.testing.assert_array_equal(zero["label"][:, d], R.labels(lg, p, zero["thr"]))
    votes, unsure, empty, conf = R.tallies(zero["label"], zero["prob"], zero["empty"], Cn)
    assert (empty == D).all() and ((votes.sum(axis=1) + unsure) == D).all()
    np.testing.assert_allclose(conf, zero["prob"].astype(np.float32).astype(np.float64).sum(axis=1), rtol=1e-12)


def test_label_rule_ties_and_threshold():
    lg = np.array([[1.0, 3.0, 3.0], [0.0, 0.0, 0.0], [5.0, 0.0, 0.0]])
    _, p = R.head(lg, np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    assert R.labels(lg, p, 0.0).tolist() == [1, 0, 0]
    assert R.labels(lg, p, 0.4).tolist() == [1, -1, 0]            # the uniform row has max_prob 1/3
    assert R.unclear(lg, p, 0.4).tolist() == [True, True, False]


@pytest.mark.parametrize("case", R.MASKED_CASES, ids=str)
def test_unclear_pairs_of_the_gpu_cases_stay_under_the_cap(case):
    H, Cn, explicit, _, keep, D = case
    c = R.masked_case(H, Cn, explicit, keep, D)
    assert c["unclear"].mean() <= 0.05, c["unclear"].mean()
    assert (c["label"] == -1).any() and (c["label"] >= 0).any()
    votes, unsure, _, _ = R.tallies(c["label"], c["prob"], c["empty"], Cn)
    assert ((votes.sum(axis=1) + unsure) == D).all()


@pytest.mark.parametrize("case", R.MATERIALISED_CASES, ids=str)
def test_unclear_pairs_of_the_materialised_cases_stay_under_the_cap(case):
    H, Cn, explicit, keep, d = case
    c = R.masked_case(H, Cn, explicit, keep, d + 1)
    assert c["unclear"][:, d].mean() <= 0.05
    kept = R.entry_mask(c["m"], R.CASE_SEED, d, keep)
    t = R.thinned(c["m"], kept)
    assert t.nnz == kept.sum() and (np.diff(t.indptr) == 0).sum() == c["empty"][:, d].sum()
    sr = None if c["self_rows"] is None else c["self_rows"][d::d + 1]
    np.testing.assert_allclose(R.layer_draw(t, np.ones(t.nnz, bool), c["table"], c["alpha"], c["bias"], sr), c["out"][d::d + 1],
                               rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------
# the C ABI (no launch)
# ------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    assert re.search(r"\bwgnn_predict_rows_dropout\s*\(", text)
    assert hasattr(lib, "wgnn_predict_rows_dropout") and "wgnn_predict_rows_dropout" in _lib.SIGNATURES
    assert int(re.search(r"#define\s+WGNN_STABILITY_ACCUMULATE\s+(\d+)", text).group(1)) == _lib.STABILITY_ACCUMULATE
    assert lib.wgnn_version() == 206
    assert sda.predict_rows_dropout is sda.ops.predict_rows_dropout and sda.Stability is api.Stability
    assert "predict_rows_dropout" in sda.__all__ and "Stability" in sda.__all__
    from scdeepsort_amd import build
    assert "wgnn_stability.hip" in [p.name for p in build.SRC]


def test_c_abi_errors_return_before_any_launch():
    """Host memory stands in for the operands: every call below must return from its argument checks with the documented
    code, and ``wgnn_last_error_string`` must name the check."""
    lib = _lib.lib()
    buf = (C.c_double * 8192)()
    base = (C.addressof(buf) + 15) // 16 * 16
    at = lambda i: base + 4096 * i

    def run(n_rows=4, H=8, ld=8, n_draws=3, row0=0, draw0=0, keep=0.5, out=at(6), head=False, votes=at(9), ld_votes=5, unsure=at(10),
            empty=at(11), conf=at(12), flags=0, self_rows=None):
        w, b, c = (at(7), at(8), 5) if head else (None, None, 0)
        return lib.wgnn_predict_rows_dropout(at(0), at(1), at(2), n_rows, at(3), ld, 100, H, at(4), at(5), self_rows, ld,
                                             n_draws, row0, draw0, 12345, keep, None if head else out, ld, w, b, c, 0.1,
                                             votes if head else None, ld_votes, unsure if head else None, empty if head else None,
                                             conf if head else None, None, None, flags, None)

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert b"wgnn_predict_rows_dropout" in msg and word in msg, (kw, msg)

    for keep in (-0.1, 1.5, float("nan")):
        fails(-1, b"keep", keep=keep)
        fails(-1, b"keep", keep=keep, head=True)
    fails(-1, b"n_draws", n_draws=0)
    fails(-1, b"n_draws", n_draws=-3)
    fails(-1, b"2^31", n_rows=2 ** 20, n_draws=2 ** 11)
    fails(-1, b"2^31", n_rows=2 ** 31 - 1, n_draws=2)
    fails(-1, b"n_rows", n_rows=2 ** 31)
    fails(-2, b"multiple of 4", H=10, ld=12)
    fails(-3, b"256", H=260, ld=260)
    fails(-1, b"votes", head=True, votes=None)
    fails(-1, b"votes", head=True, unsure=None)
    fails(-1, b"votes", head=True, empty=None)
    fails(-1, b"conf_sum", head=True, conf=None)
    fails(-1, b"ld_votes", head=True, ld_votes=4)
    fails(-1, b"WGNN_STABILITY_ACCUMULATE", flags=1)
    fails(-1, b"WGNN_STABILITY_ACCUMULATE", flags=512, head=True)
    fails(-1, b"needs a head", flags=256)
    fails(-1, b"row0", row0=-1)
    fails(-1, b"draw0", draw0=-1)
    fails(-1, b"out", out=None)
    fails(-2, b"ld_out", out=at(6) + 4)
    fails(-2, b"conf_sum", head=True, conf=at(12) + 4)
    fails(-2, b"self_rows", self_rows=at(13) + 4)
    assert run(n_rows=0) == 0 and run(n_rows=0, head=True, flags=256 | 16) == 0      # an empty batch is a no-op


def test_ops_refuses_cpu_tensors():
    rp = torch.tensor([0, 1], dtype=torch.int32)
    args = (rp, torch.zeros(1, dtype=torch.int32), torch.ones(1), torch.zeros(3, 8), torch.ones(5), torch.zeros(8))
    with pytest.raises(sda.WgnnError):
        sda.predict_rows_dropout(*args, n_draws=2, keep=0.5, seed=0)


# ------------------------------------------------------------------------------------------------
# Stability's host logic on hand-made tallies
# ------------------------------------------------------------------------------------------------
def _hand_made():
    """4 cells, 3 types, levels (1.0, 0.5), 8 draws.  Cell 0: type 1, stable.  Cell 1: type 0, flips to 2 at 0.5.  Cell 2:
    unsure as given.  Cell 3: type 2, its draws split between 0 and 1 (tie: the lower id) and unsure."""
    votes = torch.tensor([[[0, 8, 0], [8, 0, 0], [0, 0, 0], [0, 0, 8]],
                          [[0, 8, 0], [3, 0, 5], [0, 2, 0], [2, 2, 1]]], dtype=torch.int32)
    unsure = torch.tensor([[0, 0, 8, 0], [0, 0, 6, 3]], dtype=torch.int32)
    empty = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0]], dtype=torch.int32)
    conf = torch.tensor([[7.2, 6.4, 2.8, 8.0], [6.4, 4.0, 3.2, 3.6]], dtype=torch.float64)
    return api.Stability(keep=(1.0, 0.5), n_draws=8, label=np.array([1, 0, -1, 2]), max_prob=np.array([0.9, 0.8, 0.35, 1.0], np.float32),
                         votes=votes, unsure=unsure, empty=empty, conf_sum=conf, n_entries=np.array([900, 40, 300, 12]),
                         index=["a", "b", "c", "d"], id2label=["T0", "T1", "T2"], seed=5)


def test_stability_host_logic():
    st = _hand_made()
    np.testing.assert_array_equal(st.agreement(), [[1, 1, 1, 1], [1, 3 / 8, 6 / 8, 1 / 8]])
    np.testing.assert_allclose(st.mean_prob(), [[0.9, 0.8, 0.35, 1.0], [0.8, 0.5, 0.4, 0.45]])
    ids, share = st.flips_to()
    np.testing.assert_array_equal(ids, [[-1, -1, -1, -1], [-1, 2, 1, 0]])
    np.testing.assert_array_equal(share, [[0, 0, 0, 0], [0, 5 / 8, 2 / 8, 2 / 8]])
    assert st.fragile().tolist() == [False, True, True, True]
    assert st.fragile(at=0.9).tolist() == [False] * 4                       # the level nearest 0.9 is 1.0
    assert st.fragile(at=0.5, min_agreement=0.3).tolist() == [False, False, False, True]
    f = st.frame()
    assert list(f.columns) == ["index", "cell_type", "prob", "n_genes", "agree_1", "flip_1", "flip_share_1", "agree_0.5", "flip_0.5",
                               "flip_share_0.5"]
    assert f["index"].tolist() == ["a", "b", "c", "d"] and f["cell_type"].tolist() == ["T1", "T0", "unsure", "T2"]
    assert f["n_genes"].tolist() == [900, 40, 300, 12] and f["flip_0.5"].tolist() == [None, "T2", "T1", "T0"]
    assert f["flip_1"].tolist() == [None] * 4 and f["agree_0.5"].tolist() == [1, 3 / 8, 6 / 8, 1 / 8]
    s = st.summary()
    assert s["n_cells"] == 4 and s["n_draws"] == 8 and s["n_fragile"] == 3 and s["at"] == 0.5
    assert s["median_agreement"] == [1.0, (3 / 8 + 6 / 8) / 2] and s["median_n_genes_fragile"] == 40 and s["median_n_genes_rest"] == 900
    assert s["p5_agreement"][0] == 1.0 and 1 / 8 <= s["p5_agreement"][1] < 3 / 8
    text = str(s)
    assert "keep 0.5" in text and "3 cells below 0.9" in text and len(text.splitlines()) == 4
    bc = st.by_cluster(["x", "y", "x", "y"])
    assert bc["cluster"].tolist() == ["x", "y"] and bc["n_cells"].tolist() == [2, 2]
    np.testing.assert_allclose(bc["agree_0.5"], [(1 + 6 / 8) / 2, (3 / 8 + 1 / 8) / 2])
    assert st.by_cluster(np.array([2, 2, 2, 7]))["agree_1"].tolist() == [1.0, 1.0]
    with pytest.raises(ValueError, match="one id or name per cell"):
        st.by_cluster(["x", "y"])


def test_stability_into_bookkeeping_and_argument_errors():
    st = _hand_made()
    st._require_same((1.0, 0.5), 4, ["T0", "T1", "T2"], 5)
    for args, what in ((((1.0, 0.25), 4, ["T0", "T1", "T2"], 5), "levels"), (((1.0, 0.5), 5, ["T0", "T1", "T2"], 5), "cells"),
                       (((1.0, 0.5), 4, ["T0", "T1"], 5), "cell types"), (((1.0, 0.5), 4, ["T0", "T1", "T2"], 6), "seed")):
        with pytest.raises(ValueError, match=what):
            st._require_same(*args)
    assert api._keep_levels(0.5) == (0.5,) and api._keep_levels([1, 0.25]) == (1.0, 0.25)
    for bad in (-0.1, 1.5, float("nan"), (0.5, 2.0), ()):
        with pytest.raises(ValueError):
            api._keep_levels(bad)

    class Fake(api.ResidentPredictor):                            # the checks run before the device is touched
        def __init__(self):
            self.hidden_padded, self.n_classes, self.id2label = 12, 3, ["T0", "T1", "T2"]

    rp, batch = Fake(), np.zeros((4, 7), np.float32)
    for kw in (dict(keep=(0.5, 1.5)), dict(keep=float("nan")), dict(n_draws=0), dict(index=["a"]), dict(into=st, keep=(0.5,)),
               dict(into=st, keep=(1.0, 0.5), seed=6), dict(into=st, keep=(1.0, 0.5), seed=5, index=["a"])):
        with pytest.raises(ValueError):
            rp.stability(batch, **kw)
    with pytest.raises(ValueError, match="cells"):
        rp.stability(np.zeros((5, 7), np.float32), into=st, keep=(1.0, 0.5), seed=5)
    rp.hidden_padded = 260
    with pytest.raises(ValueError, match="fused"):
        rp.stability(batch)
