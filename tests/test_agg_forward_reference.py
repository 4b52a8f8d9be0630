"""CPU tests of the forward half of ``oracle/agg_backward.py`` (``fwd`` with its options) - the fp64 reference the GPU file
``test_gpu_forward_ops.py`` compares K1 / K1t / the composed entry with.  No kernel is launched here.

* the extended ``fwd`` equals a dense numpy AND a dense torch evaluation of the formula in ``include/wgnn.h`` under every option;
* for EVERY case tuple of the GPU file's exact group the lattice budget holds (``sum|terms| / unit < 2**24``; ``build_case`` asserts
  it) and an fp32 evaluation that adds a row's terms in a random order reproduces the fp64 result bit for bit - so "bit for bit" is
  a fair demand of a kernel, whatever its order of summation;
* no case passes by vacuity (ReLU clips some elements and leaves others, the bias is non-zero, alpha[row] != 1 somewhere under
  the post-scale, the skipped row factor differs from 1, the seed lists hold the hub row, the empty row and a repeat);
* the case tables cover every value of every axis in every mode;
* every fp16-output case stays below the largest fp16 number.
"""
import itertools

import numpy as np
import pytest
import torch

import test_gpu_backward_ops as GB
import test_gpu_forward_ops as GF
from conftest import small_case
from oracle import agg_backward as AB

MODES = GF.MODES


# ---- the header's formula, dense -----------------------------------------------------------------------------------------------------
def dense_fwd(xp, A, inv, alpha, mode, self_idx, h_src, h_self, ids, compact, bias, relu, no_mean, no_self, osa):
    """``include/wgnn.h`` K1, slot by slot, on dense operands; ``xp`` = numpy or torch (same code for both)."""
    R, S = A.shape
    rows = range(R) if ids is None else [int(r) for r in ids]
    out, neigh = [], []
    for i, r in enumerate(rows):
        if mode == AB.SRC_IS_GENE:
            n = sum((A[r, j] * alpha[j] * h_src[j] for j in range(S) if A[r, j] != 0), 0 * h_src[0])
            o = n
        else:
            n = sum((A[r, j] * h_src[j] for j in range(S) if A[r, j] != 0), 0 * h_src[0])
            o = alpha[r] * n if mode == AB.DST_IS_GENE else n
        if h_self is not None and not no_self:
            o = o + (1.0 if mode == AB.NO_ALPHA else alpha[self_idx]) * h_self[i if compact else r]
        if not no_mean:
            o = o * (inv[r] if inv is not None else 1.0 / (int((A[r] != 0).sum()) + 1))
        if bias is not None:
            o = o + bias
        if relu:
            o = xp.maximum(o, 0 * o)
        if osa:
            o = o * alpha[r]
        out.append(o); neigh.append(n)
    return xp.stack(out), xp.stack(neigh)


@pytest.mark.parametrize("mode", [AB.SRC_IS_GENE, AB.DST_IS_GENE, AB.NO_ALPHA])
def test_fwd_equals_the_dense_formula_under_every_option(mode):
    c = small_case(cells=24, genes=17, dim=8, seed=mode, density=0.3, test_cells=0)
    rng = np.random.default_rng(mode)
    expr = c["expr"].astype(np.float64)
    A = expr if mode != AB.DST_IS_GENE else expr.T.tocsr()
    R, S = A.shape
    G, D = 17, 8
    self_idx = G + 1 if mode != AB.DST_IS_GENE else G
    inv, alpha = rng.uniform(0.1, 1.0, R), rng.uniform(0.5, 1.5, G + 2)
    h_src, h_self, bias = rng.standard_normal((S, D)), rng.standard_normal((R, D)), rng.standard_normal(D)
    ids = np.array([5, 0, 5, R - 1, 3])
    h_compact = rng.standard_normal((len(ids), D))
    Ad = A.toarray()
    n_checked = 0
    for use_bias, relu, no_mean, no_self, osa, seeds, inv_null in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1),
                                                                                    (None, "ids", "compact"), (0, 1)):
        if (osa and mode != AB.DST_IS_GENE) or (inv_null and no_mean):
            continue
        rid = None if seeds is None else ids
        hs = h_compact if seeds == "compact" else h_self
        kw = dict(row_ids=rid, self_compact=seeds == "compact", bias=bias if use_bias else None, relu=bool(relu), no_mean=bool(no_mean),
                  no_self=bool(no_self), out_scale_alpha=bool(osa))
        got = AB.fwd(A, None if inv_null else inv, alpha, mode, self_idx, h_src, hs, **kw)
        args = (None if inv_null else inv, alpha, mode, self_idx, h_src, hs, rid, seeds == "compact", bias if use_bias else None, relu,
                no_mean, no_self, osa)
        want, want_n = dense_fwd(np, Ad, *args)
        np.testing.assert_allclose(got["out"], want, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(got["neigh"], want_n, rtol=1e-12, atol=1e-13)
        t = lambda x: None if x is None else (x if isinstance(x, (int, bool, np.integer)) else torch.tensor(x, dtype=torch.float64))
        t_args = [t(a) if isinstance(a, np.ndarray) and a.dtype.kind == "f" else a for a in args]
        want_t, _ = dense_fwd(torch, torch.tensor(Ad), *t_args)
        np.testing.assert_allclose(got["out"], want_t.numpy(), rtol=1e-12, atol=1e-13)
        assert (got["abs_out"] >= np.abs(got["out"]) - 1e-12).all() and (got["abs_neigh"] >= np.abs(got["neigh"]) - 1e-12).all()
        rows = np.arange(R) if rid is None else rid
        assert np.array_equal(got["n_terms"], np.diff(A.indptr)[rows])
        n_checked += 1
    assert n_checked >= 72
    # the options default to the behaviour before they existed
    base = AB.fwd(A, inv, alpha, mode, self_idx, h_src, h_self)
    np.testing.assert_array_equal(base["out"], AB.fwd(A, inv, alpha, mode, self_idx, h_src, h_self, row_ids=np.arange(R))["out"])
    np.testing.assert_allclose(base["out"], dense_fwd(np, Ad, inv, alpha, mode, self_idx, h_src, h_self, None, False, None, 0, 0, 0, 0)[0],
                               rtol=1e-12, atol=1e-13)


def test_abs_out_follows_bias_and_post_scale():
    """The bias adds |bias| to ``abs_out``; the post-scale multiplies it by |alpha[row]|."""
    L = AB.lattice_case(GF.pattern("small"), 8, 1)
    a = (L["A_gc"], L["inv_gc"], L["alpha"], AB.DST_IS_GENE, L["G"], L["h_cell"], L["h_gene"])
    bias = np.arange(8) - 3.0
    plain, b, bs = AB.fwd(*a), AB.fwd(*a, bias=bias), AB.fwd(*a, bias=bias, out_scale_alpha=True)
    assert np.array_equal(b["abs_out"], plain["abs_out"] + np.abs(bias))
    assert np.array_equal(bs["abs_out"], b["abs_out"] * L["alpha"][:L["G"], None]) and np.array_equal(bs["out"], b["out"] * L["alpha"][:L["G"], None])
    assert AB.fwd_units(AB.DST_IS_GENE, True)["out"] == AB.fwd_units(AB.DST_IS_GENE)["out"] / 2
    assert AB.fwd_units(AB.NO_ALPHA, max_deg=511)["out"] == AB.fwd_units(AB.NO_ALPHA)["out"] / AB.U_SCALE / 512
    with pytest.raises(ValueError):
        AB.fwd(L["A_cg"], L["inv_cg"], L["alpha"], AB.SRC_IS_GENE, L["G"] + 1, L["h_gene"], L["h_cell"], out_scale_alpha=True)


# ---- every case tuple of the GPU file: budget, order independence, no vacuity --------------------------------------------------------
def emulate_fp32(c, rng):
    """The forward in fp32: a row's edge terms added in a random order (weights folded with alpha first, like the kernels), then
    the header's epilogue, every operation rounded to fp32."""
    f32 = np.float32
    A, L = c.A, c.L
    rows = np.arange(A.shape[0]) if c.ids is None else c.ids
    Ar = A[rows] if len(rows) else A[:0]
    alpha = L["alpha"].astype(f32)
    X = (alpha[:A.shape[1], None] * c.h_src.astype(f32)) if c.amode == AB.SRC_IS_GENE else c.h_src.astype(f32)
    neigh = AB.spmm_fp32_random_order(Ar, X, rng)
    o = alpha[rows, None] * neigh if c.amode == AB.DST_IS_GENE else neigh
    if not c.no_self:
        hs = c.h_self if (c.compact or c.ids is None) else c.h_self[rows]
        o = o + (f32(1) if c.amode == AB.NO_ALPHA else alpha[c.sidx]) * hs.astype(f32)
    if not c.no_mean:
        f = f32(1) / (np.diff(Ar.indptr) + 1).astype(f32) if c.inv_null else c.inv[rows].astype(f32)
        o = o * f[:, None]
    if c.bias is not None:
        o = o + c.bias.astype(f32)
    if c.relu:
        o = np.maximum(o, f32(0))
    if c.osa:
        o = o * alpha[rows, None]
    assert o.dtype == f32 and neigh.dtype == f32
    return o, neigh


def check_case(c, seed=0):
    if c.n_out == 0:
        assert c.ref["out"].shape == (0, c.D)
        return
    assert c.budget["out"] < 24 and c.budget["neigh"] < 24
    o32, n32 = emulate_fp32(c, np.random.default_rng(seed))
    assert np.array_equal(n32.astype(np.float64), c.ref["neigh"]) and np.array_equal(o32.astype(np.float64), c.ref["out"])


CASES = ([("k1", c) for c in GF.K1_OPTION_CASES] + [("seed", c) for c in GF.K1_SEED_CASES] + [("dtype", c) for c in GF.K1_DTYPE_CASES]
         + [("k1t", c) for c in GF.K1T_OPTION_CASES] + [("abi", c) for c in GF.K1T_ABI_CASES] + [("null", c) for c in GF.NULL_CASES]
         + [("edge", c) for c in GF.EDGE_CASES] + [("composed", c) for c in GF.COMPOSED_CASES])
BUILD = dict(k1=GF.k1_case, seed=GF.seed_case, dtype=GF.dtype_case, k1t=GF.k1t_case, abi=GF.abi_case, null=GF.null_case,
             edge=GF.edge_case, composed=GF.composed_case)


@pytest.mark.parametrize("table,case", sorted(CASES, key=lambda tc: (str(tc[1][0]), tc[1][2] if tc[0] != "edge" else 0)),
                         ids=lambda c: c if isinstance(c, str) else GB._cid(c))
def test_case_fits_the_lattice_and_is_not_vacuous(table, case):
    """``build_case`` asserts the budget and the non-vacuity of every option the tuple switches on; here also: fp32 in random order
    gives the reference's bits, fp16 outputs stay finite, the composed product fits its own budget."""
    c = BUILD[table](case)
    check_case(c, seed=len(str(case)))
    if table == "dtype" and case[4]:
        assert np.abs(c.ref["out"]).max() < GF.F16_MAX
    if table == "null":
        deg = np.diff(c.A.indptr)
        if case[1] == "genes":
            assert ((deg + 1) & deg).any()
        else:
            assert c.inv_null and not ((deg + 1) & deg).any() and deg.max() == 511 and c.budget["out"] < 14
            assert np.array_equal(c.ref["out"].astype(np.float32).astype(np.float64), c.ref["out"])
    if table == "composed":
        assert c.lin_budget < 24
        x32, w32 = c.ref["out"].astype(np.float32), c.W.astype(np.float32)
        acc = np.zeros((c.n_out, case[3]), dtype=np.float32)
        for k in np.random.default_rng(1).permutation(c.D):
            acc = acc + x32[:, k:k + 1] * w32[None, :, k]
        acc = acc + c.lin_bias.astype(np.float32)
        want = np.maximum(c.lin["out"], 0.0) if case[5] else c.lin["out"]
        assert np.array_equal((np.maximum(acc, 0) if case[5] else acc).astype(np.float64), want)
    if table == "edge" and case[0] == "no_edges":
        assert c.A.nnz == 0 and c.ref["out"].any()


def test_sensitivity_cases_fit_the_budget():
    """The draws of ``test_one_hub_edge_is_seen_forward``, also with every hub weight at its largest, and of
    ``test_flat_kernel_is_reported``."""
    L = GF.lattice("hub", 256)
    for stack in (dict(), dict(bias=True, relu=True, osa=True)):
        for A in (L["A_gc"], L["A_gc"].sign() * 2.0):
            c = GF.build_case(dict(L, A_gc=A), "genes", 256, **stack)
            assert c.budget["out"] < 24
    A = L["A_gc"].copy()
    A.data[A.indptr[0] + 1234] += 0.5 if A.data[A.indptr[0] + 1234] < 2.0 else -0.5
    stack = dict(bias=True, relu=True, osa=True)
    a, b = GF.build_case(L, "genes", 256, **stack).ref["out"], GF.build_case(dict(L, A_gc=A), "genes", 256, **stack).ref["out"]
    assert (a[0] != b[0]).any() and np.array_equal(a[1:], b[1:])
    assert GF.build_case(GF.lattice("mid", 256), "genes", 256, bias=True, relu=True, osa=True).budget["out"] < 24


# ---- coverage of the tables ------------------------------------------------------------------------------------------------------
def test_forward_case_sets_cover_every_axis_in_every_mode():
    """The covering sets of the GPU file: each value of each axis meets each mode at least once."""
    both = {False, True}
    for m in MODES:
        rows = [c for c in GF.K1_OPTION_CASES if c[1] == m]
        assert {c[2] for c in rows} == set(GF.ROWWAVE_D)
        assert {c[3] for c in rows} == {64, 4096}
        for axis in (4, 5, 6, 7, 9, 10):
            assert {bool(c[axis]) for c in rows} == both, (m, axis)
        assert all(c[0] == "small" for c in rows if c[2] >= 400)
        rows = [c for c in GF.K1_SEED_CASES if c[1] == m]
        assert {c[2] for c in rows} == set(GF.SEED_D) and {c[3] for c in rows} == {64, 4096}
        assert {c[4] for c in rows} == {"perm", "compact", "empty"}
        assert {bool(c[5]) for c in rows} == both and {bool(c[6]) for c in rows} == both
        rows = [c for c in GF.K1T_OPTION_CASES if c[1] == m and not c[6] and not c[15]]
        assert {c[2] for c in rows} == set(GF.TILED_D)
        assert {c[3] for c in rows} == set(GF.GEOMS) and {c[4] for c in rows} == set(GF.BLOCK_ROWS) and {c[5] for c in rows} == {0, 1}
        for axis in (7, 8, 9, 10, 13, 14):
            assert {bool(c[axis]) for c in rows} == both, (m, axis)
        assert {c[2] for c in GF.K1T_OPTION_CASES if c[1] == m and c[6]} == set(GF.TALL_D)
        generic = [c for c in GF.K1T_OPTION_CASES if c[1] == m and c[15]]
        assert len(generic) >= 3 and {c[2] for c in generic} == {256}
        for axis in (7, 8, 14):
            assert {bool(c[axis]) for c in generic} == both, (m, axis)
        assert {c[3] for c in GF.K1T_ABI_CASES if c[1] == m} == {"perm", "compact"}
        assert {(c[0], c[3]) for c in GF.NULL_CASES if c[1] == m} == {(r, i) for r in GF.NULL_ROUTES for i in both}
        assert {c[4] for c in GF.COMPOSED_CASES if c[1] == m} == {None, "perm"}
    for table, osa, mode in ((GF.K1_OPTION_CASES, 8, 1), (GF.K1T_OPTION_CASES, 11, 1), (GF.K1_DTYPE_CASES, 7, 1)):
        assert {bool(c[osa]) for c in table if c[mode] == "genes"} == both and not any(c[osa] for c in table if c[mode] != "genes")
    assert {bool(c[12]) for c in GF.K1T_OPTION_CASES if c[1] == "cells"} == both and not any(c[12] for c in GF.K1T_OPTION_CASES if c[1] != "cells")
    for out16 in both:                                            # every dispatch_width branch in both dtype pairs, every mode somewhere
        rows = [c for c in GF.K1_DTYPE_CASES if c[4] == out16]
        assert {c[2] for c in rows} >= set(GF.DTYPE_D) and {c[1] for c in rows} == set(MODES)
        assert {min(b for b in (8, 16, 32, 64, 128, 256) if c[2] // 4 <= b) for c in rows} == {8, 16, 32, 64, 128, 256}
    assert {(c[2], c[3]) for c in GF.COMPOSED_CASES} == {(D, H) for D in (64, 200, 256) for H in (16, 200)}
    assert {c[4] for c in GF.COMPOSED_CASES} == {None, "perm"} and {c[1] for c in GF.COMPOSED_CASES} == set(MODES)
    assert {(c[0], c[1]) for c in GF.EDGE_CASES} == {(s, r) for s in ("one_row", "no_rows", "no_edges") for r in ("rowwave", "tiled")}
    n_exact = sum(len(t) for t in (GF.K1_OPTION_CASES, GF.K1_SEED_CASES, GF.K1_DTYPE_CASES, GF.K1T_OPTION_CASES, GF.K1T_ABI_CASES,
                                   GF.NULL_CASES, GF.EDGE_CASES, GF.COMPOSED_CASES))
    assert 150 <= n_exact <= 250, n_exact
    hub = GF.pattern("hub")
    assert (hub.getnnz(axis=0)).max() > 2900 and hub.getnnz(axis=1).min() == 0 and hub.getnnz(axis=0).min() == 0
    p2 = GF.pow2_pattern()
    assert p2.shape == (200, 600) and set(np.diff(p2.indptr).tolist()) == {2 ** k - 1 for k in range(10)}


def test_float_stacks_name_every_option():
    keys = set().union(*GF.FLOAT_STACKS)
    assert keys == {"bias", "relu", "no_mean", "no_self", "osa", "kind", "f16"}
    assert {s.get("f16") for s in GF.FLOAT_STACKS} == {None, "in", "out"} and {s.get("kind") for s in GF.FLOAT_STACKS} == {None, "perm", "compact"}
    for mode in MODES:
        for route in ("rowwave", "tiled"):
            took = [s for s in GF.FLOAT_STACKS if GF.stack_fits(s, mode, route)]
            assert set().union(*took) >= {"bias", "relu", "no_mean", "no_self"} and (mode != "genes" or any(s.get("osa") for s in took))
