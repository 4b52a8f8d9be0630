"""CPU tests of ``oracle/agg_backward.py`` - the fp64 reference the GPU file ``test_gpu_backward_ops.py`` compares the backward
aggregation kernels with.  No kernel is launched here.

* every formula equals ``torch.autograd`` (fp64) of a dense restatement of the K1 forward;
* for EVERY parameter tuple of the GPU file's exact group the lattice budget holds (``sum|terms| / unit < 2**24``) and an fp32
  emulation that adds the terms in a random order reproduces the fp64 result exactly - so "bit for bit" is a fair demand;
* the derived bound of the float group holds for an fp32 emulation in random order - so it is not too tight.
"""
import numpy as np
import pytest
import torch

import test_gpu_backward_ops as GB
from conftest import small_case
from oracle import agg_backward as AB


def dense_forward(A, inv, alpha, mode, self_idx, h_src, h_self):
    """out = (sum_j val*alpha*h_src + alpha_self*h_self) * inv_deg - include/wgnn.h, K1 - with dense torch ops."""
    R, S = A.shape
    if mode == AB.SRC_IS_GENE:
        neigh = A @ (alpha[:S, None] * h_src)
    elif mode == AB.DST_IS_GENE:
        neigh = alpha[:R, None] * (A @ h_src)
    else:
        neigh = A @ h_src
    a_self = 1.0 if mode == AB.NO_ALPHA else alpha[self_idx]
    return (neigh + a_self * h_self) * inv[:, None]


@pytest.mark.parametrize("mode", [AB.SRC_IS_GENE, AB.DST_IS_GENE, AB.NO_ALPHA])
def test_formulas_equal_autograd_of_the_dense_forward(mode):
    c = small_case(cells=60, genes=40, dim=12, seed=mode, density=0.3, test_cells=0)
    rng = np.random.default_rng(mode)
    expr = c["expr"].astype(np.float64)
    A = expr if mode != AB.DST_IS_GENE else expr.T.tocsr()         # destination-major: cells<-genes | genes<-cells
    R, S = A.shape
    G, D = 40, 12
    self_idx = G + 1 if mode != AB.DST_IS_GENE else G
    inv = rng.uniform(0.1, 1.0, R)
    t = lambda x: torch.tensor(x, dtype=torch.float64, requires_grad=True)
    alpha, h_src, h_self = t(rng.uniform(0.5, 1.5, G + 2)), t(rng.standard_normal((S, D))), t(rng.standard_normal((R, D)))
    gout = rng.standard_normal((R, D))
    Ad = torch.tensor(A.toarray())
    out = dense_forward(Ad, torch.tensor(inv), alpha, mode, self_idx, h_src, h_self)
    fw = AB.fwd(A, inv, alpha.detach().numpy(), mode, self_idx, h_src.detach().numpy(), h_self.detach().numpy())
    np.testing.assert_allclose(fw["out"], out.detach().numpy(), rtol=1e-12, atol=1e-13)
    (out * torch.tensor(gout)).sum().backward()
    a, hs, hf = alpha.detach().numpy(), h_src.detach().numpy(), h_self.detach().numpy()
    k2 = AB.bwd_src(A, inv, a, mode, gout, hs)
    np.testing.assert_allclose(k2["dh_src"], h_src.grad.numpy(), rtol=1e-12, atol=1e-13)
    dalpha = np.zeros(G + 2)
    if mode == AB.SRC_IS_GENE:
        dalpha[:S] += k2["dalpha_src"]
    k3 = AB.bwd_alpha(A, inv, gout, hs, hf)
    if mode == AB.DST_IS_GENE:
        dalpha[:R] += k3["dalpha_row"]
    if mode != AB.NO_ALPHA:
        dalpha[self_idx] += k3["dself_row"].sum()
        np.testing.assert_allclose(dalpha, alpha.grad.numpy(), rtol=1e-12, atol=1e-12)
    else:
        assert alpha.grad is None or not alpha.grad.any()
    # row_ids / self_compact: slot i is row ids[i]; a compact self table holds one row per slot
    ids = np.array([5, 0, 5, R - 1])
    k3s = AB.bwd_alpha(A, inv, gout[ids], hs, hf[ids], ids, self_compact=True)
    np.testing.assert_allclose(k3s["dalpha_row"], AB.bwd_alpha(A, inv, gout, hs, hf)["dalpha_row"][ids], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(k3s["dself_row"], k3["dself_row"][ids], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(AB.bwd_alpha(A, inv, gout[ids], hs, hf, ids)["dself_row"], k3["dself_row"][ids], rtol=1e-12, atol=1e-13)
    # every |term| sum dominates its value
    assert (k2["abs_dh"] >= np.abs(k2["dh_src"]) - 1e-12).all() and (fw["abs_out"] >= np.abs(fw["out"]) - 1e-12).all()


def test_case_sets_cover_every_axis_in_every_mode():
    """The covering sets of the GPU file: each value of each axis meets each mode at least once."""
    for m in ("cells", "genes", "plain"):
        rows = [c for c in GB.K2_ROWWAVE_CASES if c[1] == m]
        assert {c[2] for c in rows} == set(GB.ROWWAVE_D)
        for axis, values in ((3, {64, 4096}), (4, {0, 1}), (5, {False, True}), (6, {False, True})):
            assert {c[axis] for c in rows} == values, (m, axis)
        rows = [c for c in GB.K2_TILED_CASES if c[1] == m and not c[6]]
        assert {c[2] for c in rows} == set(GB.TILED_D)
        assert {c[3] for c in rows} == set(GB.GEOMS) and {c[4] for c in rows} == set(GB.BLOCK_ROWS)
        for axis in (5, 7, 8):
            assert {int(c[axis]) for c in rows} == {0, 1}, (m, axis)
        assert {c[2] for c in GB.K2_TILED_CASES if c[1] == m and c[6]} == set(GB.TALL_D)
    assert {c[9] for c in GB.K2_TILED_CASES if c[1] == "cells"} == {False, True}
    assert 60 <= len(GB.K2_TILED_CASES) <= 100
    assert {c[1] for c in GB.K3_ROWWAVE_CASES} == set(GB.ROWWAVE_D)
    assert {c[3] for c in GB.K3_ROWWAVE_CASES} == {None, "perm", "compact", "empty"} and {c[2] for c in GB.K3_ROWWAVE_CASES} == {False, True}
    flat = [c for c in GB.K3_TILED_CASES if not c[5]]
    assert {c[1] for c in flat} == set(GB.TILED_D) and {c[2] for c in flat} == set(GB.GEOMS) and {c[3] for c in flat} == set(GB.BLOCK_ROWS)
    assert {c[1] for c in GB.K3_TILED_CASES if c[5]} == set(GB.TALL_D)
    assert {c[2] for c in GB.SEED_BLOCK_CASES} == {1, 5, 64, 300} and {c[1] for c in GB.SEED_BLOCK_CASES} == {"cells", "plain"}
    for d in ("cells", "genes"):
        tiled = [c[3] for c in GB.FWD_CASES if c[1] == d and c[3] != "rowwave"]
        assert {r[0] for r in tiled} == set(GB.GEOMS) and any(r[3] for r in tiled)
    hub = GB.pattern("hub")
    assert (hub.getnnz(axis=0)).max() > 2900 and hub.getnnz(axis=1).min() == 0 and hub.getnnz(axis=0).min() == 0


def emulate_T(A, scale, gr, rng):
    """T = A^T (scale o g) in fp32, a source row's terms added in a random order (weights folded first, like the kernels)."""
    At = A.T.tocsr()
    At.data = (At.data.astype(np.float32) * scale.astype(np.float32)[At.indices]).astype(np.float64)      # exact on the lattice
    return AB.spmm_fp32_random_order(At, gr, rng)


@pytest.mark.parametrize("route,case", [("rowwave", c) for c in GB.K2_ROWWAVE_CASES] + [("tiled", c) for c in GB.K2_TILED_CASES],
                         ids=lambda c: c if isinstance(c, str) else GB._cid(c))
def test_k2_lattice_budget_and_fp32_order_independence(route, case):
    name, mode, D = case[:3]                                       # the same lattice draw as the GPU test of this tuple
    acc, dscale, want_da = (case[4], case[5], True) if route == "rowwave" else (case[8], False, case[9])
    L, scale = GB.k2_lattice(name, mode, D, dscale, case)
    ref, want_dh, want_dalpha, prior = GB.k2_reference(L, mode, accumulate=acc, dst_scale=scale, want_dalpha=want_da)
    S = ref["T"].shape[0]
    AB.check_bwd_src_budget(ref, GB.MODE[mode], prior if acc else None, L["prior_dalpha"][:S] if acc else None)
    rng = np.random.default_rng(D)
    _, A, inv, gr, hs, _ = GB.side(None, L, mode)
    inv = inv if scale is None else scale
    fold = inv * L["alpha"][:A.shape[0]] if mode == "genes" else inv
    T32 = emulate_T(A, fold, gr, rng)
    assert np.array_equal(T32.astype(np.float64), ref["T"])
    if mode == "cells" and want_da:
        d32 = AB.dot_fp32_random_order(hs, T32, rng)
        assert np.array_equal(d32.astype(np.float64), ref["dalpha_src"])


@pytest.mark.parametrize("route,case", [("rowwave", c) for c in GB.K3_ROWWAVE_CASES] + [("tiled", c) for c in GB.K3_TILED_CASES],
                         ids=lambda c: c if isinstance(c, str) else GB._cid(c))
def test_k3_lattice_budget_and_fp32_order_independence(route, case):
    name, D = case[:2]
    with_self, kind = (case[2], case[3]) if route == "rowwave" else (case[6], None)
    L = AB.lattice_case(GB.pattern(name), D, GB.case_seed(*case))
    ids, gr, h_self, compact = GB.k3_operands(L, D, with_self, kind, GB.case_seed(*case))
    ref = AB.bwd_alpha(L["A_gc"], L["inv_gc"], gr, L["h_cell"], h_self, ids, compact)
    AB.check_bwd_alpha_budget(ref)
    rng = np.random.default_rng(D)
    rows = np.arange(L["G"]) if ids is None else ids
    if len(rows):
        S32 = AB.spmm_fp32_random_order(L["A_gc"][rows], L["h_cell"], rng)
        d32 = AB.dot_fp32_random_order(gr, S32, rng) * L["inv_gc"][rows].astype(np.float32)
        assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), ref["dalpha_row"])


@pytest.mark.parametrize("case", GB.SEED_BLOCK_CASES, ids=lambda c: GB._cid(c))
def test_seed_block_lattice_budget(case):
    name, mode, B, D = case
    L = AB.lattice_case(GB.pattern(name), D, GB.case_seed(*case))
    rng = np.random.default_rng(GB.case_seed(*case) + 2)
    ids = GB.seed_ids(B, L["C"], B)
    gr = rng.integers(-2, 3, (B, D)).astype(np.float64)
    inv_rows = rng.choice(AB.LATTICE_SCALE, B)
    ref = AB.bwd_src(L["A_cg"][ids], inv_rows, L["alpha"], GB.MODE[mode], gr, L["h_gene"])
    AB.check_bwd_src_budget(ref, GB.MODE[mode])
    assert np.array_equal(emulate_T(L["A_cg"][ids], inv_rows, gr, rng).astype(np.float64), ref["T"])


@pytest.mark.parametrize("case", GB.FWD_CASES, ids=lambda c: GB._cid(c))
def test_forward_lattice_budget_and_fp32_order_independence(case):
    name, direction, D, _ = case
    L = AB.lattice_case(GB.pattern(name), D, GB.case_seed(*case))
    _, A, inv, mode, sidx, hs, hself = GB.fwd_side(None, L, direction)
    ref = AB.fwd(A, inv, L["alpha"], mode, sidx, hs, hself)
    AB.check_fwd_budget(ref, mode)
    X = L["alpha"][:A.shape[1], None] * hs if mode == AB.SRC_IS_GENE else hs
    n32 = AB.spmm_fp32_random_order(A, X, np.random.default_rng(D))
    assert np.array_equal(n32.astype(np.float64), ref["neigh"])


def test_sensitivity_and_fixed_cases_fit_the_budget():
    """The lattice draws of test_one_hub_edge_is_seen (also with the moved weight at its largest), the default-dispatch test and
    the guard test."""
    L = AB.lattice_case(GB.pattern("hub"), 256, 31)
    for A in (L["A_cg"], L["A_cg"].sign() * 2.0):
        ref = AB.bwd_src(A, L["inv_cg"], L["alpha"], AB.SRC_IS_GENE, L["g_cell"], L["h_gene"])
        AB.check_bwd_src_budget(ref, AB.SRC_IS_GENE)
    A = L["A_gc"].sign() * 2.0
    AB.check_fwd_budget(AB.fwd(A, L["inv_gc"], L["alpha"], AB.DST_IS_GENE, L["G"], L["h_cell"], L["h_gene"]), AB.DST_IS_GENE)
    for name, D, seed in (("mid", 128, 77), ("mid", 200, 5)):
        L = AB.lattice_case(GB.pattern(name), D, seed)
        for mode in ("cells", "genes", "plain"):
            AB.check_bwd_src_budget(GB.k2_reference(L, mode, accumulate=0)[0], GB.MODE[mode])
        AB.check_bwd_alpha_budget(AB.bwd_alpha(L["A_gc"], L["inv_gc"], L["g_gene"], L["h_cell"], L["h_gene"]))


def test_lattice_budget_rejects_an_oversized_case():
    with pytest.raises(AssertionError):
        AB.lattice_budget(np.array([2.0 ** 24]), 1.0)
    assert AB.lattice_budget(np.array([2.0 ** 24 - 1]), 1.0) < 24


@pytest.mark.parametrize("D", GB.FLOAT_D)
def test_float_bound_holds_for_fp32_sums_in_random_order(D):
    """Ordinary floats: fp32 accumulation in random order stays inside (n + 8) * 2**-24 * sum|terms| of the fp64 value, for the
    edge sums (K2's T, K1's neighbour sum) and the dot products on top of them (dalpha)."""
    c = small_case(cells=1100, genes=520, dim=4, seed=D, density=0.2, test_cells=0)
    rng = np.random.default_rng(D)
    expr = c["expr"].astype(np.float32).astype(np.float64)
    Cn, G = expr.shape
    deg = np.maximum(1, np.diff(expr.indptr))
    A = expr.multiply((deg / np.maximum(1e-30, np.asarray(expr.sum(1)).ravel()))[:, None]).tocsr()
    A.data = A.data.astype(np.float32).astype(np.float64)
    inv = (1.0 / (deg + 1.0)).astype(np.float32).astype(np.float64)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    alpha, gr, hs = f32(rng.uniform(0.5, 1.5, G + 2)), f32(rng.standard_normal((Cn, D))), f32(rng.standard_normal((G, D)))
    ref = AB.bwd_src(A, inv, alpha, AB.SRC_IS_GENE, gr, hs)
    At = A.T.tocsr()
    At.data = (At.data.astype(np.float32) * inv.astype(np.float32)[At.indices])                 # fp32 weight fold: one rounding
    T32 = AB.spmm_fp32_random_order(At, gr, rng)
    n = ref["n_terms"]
    r_T = AB.worst_ratio(T32, ref["T"], AB.float_bound(ref["abs_T"], n[:, None]))
    d32 = AB.dot_fp32_random_order(hs, T32, rng)
    r_d = AB.worst_ratio(d32, ref["dalpha_src"], AB.float_bound(ref["abs_dalpha"], n + D))
    fw = AB.fwd(A, inv, alpha, AB.SRC_IS_GENE, G + 1, hs, f32(rng.standard_normal((Cn, D))))
    X32 = (alpha[:G, None].astype(np.float32) * hs.astype(np.float32))
    r_n = AB.worst_ratio(AB.spmm_fp32_random_order(A, X32, rng), fw["neigh"], AB.float_bound(fw["abs_neigh"], fw["n_terms"][:, None]))
    assert 0 < r_T <= 1 and 0 < r_d <= 1 and 0 < r_n <= 1, (r_T, r_d, r_n)
