"""CPU tests behind the cached feature sum (no kernel is launched here).

* The identity: layer 1's genes<-cells rows computed project-first - ``sum_c w_rc (X_c W^T)[c]`` - equal ``(S W^T)[r]`` with
  ``S = A_gc X_c`` in fp64, and the whole row ``relu((alpha[r] * sum + alpha[G] * P_g[r]) * inv_deg[r] + b)`` equals the
  two-operand form ``relu((c1 S + c2 X_g) W^T + b)``.  It holds because alpha sits on the DESTINATION on this side; with alpha on
  the SOURCE (the cells<-genes side) the same trick needs the alpha-folded table and is not weight-independent.
* The lattice of ``test_gpu_linear_mix.py``: for every tuple of its exact group ``sum|terms| / unit < 2^24`` (the guard
  ``test_dense_half_reference.py`` uses), an fp32 evaluation in a random order of summation reproduces the fp64 reference
  bit for bit, and no case passes by vacuity.
"""
import numpy as np
import pytest

import linear_mix_reference as LM


def random_graph(C=40, G=30, seed=0):
    rng = np.random.default_rng(seed)
    A = np.where(rng.random((G, C)) < 0.2, rng.uniform(0.5, 3.0, (G, C)), 0.0)       # genes <- cells weights
    A[7] = 0.0                                                                        # a gene with no cells
    return A, 1.0 / ((A != 0).sum(1) + 1.0)


def test_feature_sum_identity_holds_for_both_alpha_placements():
    C, G, D, H = 40, 30, 12, 8
    A, inv_deg = random_graph(C, G)
    rng = np.random.default_rng(1)
    Xg, Xc, W, b = rng.standard_normal((G, D)), rng.standard_normal((C, D)), rng.standard_normal((H, D)), rng.standard_normal(H)
    alpha = rng.uniform(0.5, 1.5, G + 2)
    S = A @ Xc
    Pg, Pc = Xg @ W.T, Xc @ W.T
    np.testing.assert_allclose(A @ Pc, S @ W.T, rtol=1e-12, atol=1e-12)
    # destination-side alpha (genes <- cells): the whole finished row from S, no pass over the edges
    want = np.maximum((alpha[:G, None] * (A @ Pc) + alpha[G] * Pg) * inv_deg[:, None] + b, 0.0)
    c1, c2 = alpha[:G] * inv_deg, alpha[G] * inv_deg
    got = LM.reference(S, c1, Xg, c2, W, b, relu=True)["out"]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    assert not S[7].any() and inv_deg[7] == 1.0                                       # the gene without cells: self-loop only
    np.testing.assert_allclose(got[7], np.maximum(alpha[G] * Pg[7] + b, 0.0), rtol=1e-12, atol=1e-12)
    # source-side alpha (cells <- genes, A^T's pattern): the sum that would have to be cached contains alpha itself
    B = A.T
    by_edges = B @ (alpha[:G, None] * Pg)
    np.testing.assert_allclose(by_edges, (B @ (alpha[:G, None] * Xg)) @ W.T, rtol=1e-12, atol=1e-12)
    assert not np.allclose(by_edges, (B @ Xg) @ W.T)                                  # ... and not the alpha-free one


def test_case_table_covers_every_axis():
    cases = LM.EXACT_CASES
    assert len(cases) == len(set(cases)) == 2 * 6 * 4 * 6
    assert {c[:4] for c in cases} == {(t, m, k, n) for t in LM.MIX_TILES for m in LM.MIX_M for k in LM.MIX_K for n in LM.MIX_N}
    switches = {(b, r, o, l) for b in (False, True) for r in (False, True) for o in LM.OUTPUTS for l in (False, True)}
    for tile in LM.MIX_TILES:
        for axis, values in ((1, LM.MIX_M), (2, LM.MIX_K), (3, LM.MIX_N)):
            for v in values:
                seen = {c[4:] for c in cases if c[0] == tile and c[axis] == v}
                assert seen == switches if axis == 1 else len(seen) >= 12, (tile, axis, v, len(seen))
                assert {s[0] for s in seen} == {s[1] for s in seen} == {s[3] for s in seen} == {False, True}
                assert {s[2] for s in seen} == set(LM.OUTPUTS)


@pytest.mark.parametrize("M,K,N", sorted({c[1:4] for c in LM.EXACT_CASES}))
def test_lattice_budget_and_exactness_in_any_order(M, K, N):
    L = LM.lattice(M, K, N, LM.case_seed("mix", M, K, N))
    for key in ("x1", "x2", "c1", "c2", "w", "bias", "row_scale"):
        assert np.array_equal(L[key].astype(np.float16).astype(np.float64), L[key]), key      # fp32 and the __half loader agree
    a = L["c2"][:, None] * L["x2"] + L["c1"][:, None] * L["x1"]
    assert np.array_equal(a, np.round(a * 2) / 2) and np.abs(a).max() <= 16
    for bias in (None, L["bias"]):
        ref = LM.reference(L["x1"], L["c1"], L["x2"], L["c2"], L["w"], bias, False, L["row_scale"])
        assert float(ref["abs_sum"].max()) / LM.UNIT < 2 ** 24
        assert float((L["row_scale"][:, None] * ref["abs_sum"]).max()) / LM.UNIT_SCALED < 2 ** 24
        assert np.array_equal(ref["out"], np.round(ref["out"] / LM.UNIT) * LM.UNIT)
        # fp32, the loader's two operations, then the sum over k in a random order
        rng = np.random.default_rng(LM.case_seed("order", M, K, N, bias is None))
        c1, c2, x1, x2, w = (L[k].astype(np.float32) for k in ("c1", "c2", "x1", "x2", "w"))
        a32 = (c2[:, None] * x2 + (c1[:, None] * x1).astype(np.float32)).astype(np.float32)
        order = rng.permutation(K)
        acc = np.zeros((M, N), dtype=np.float32)
        for k in order:
            acc = (acc + a32[:, k, None] * w[None, :, k]).astype(np.float32)
        if bias is not None:
            acc = acc + bias.astype(np.float32)
        assert LM.same_bits(acc, ref["out"])
        assert LM.same_bits(L["row_scale"].astype(np.float32)[:, None] * np.maximum(acc, np.float32(0)),
                            LM.reference(L["x1"], L["c1"], L["x2"], L["c2"], L["w"], bias, True, L["row_scale"])["out_scaled"])
    # no vacuity: each operand, the K tail and the ReLU matter
    full = LM.reference(L["x1"], L["c1"], L["x2"], L["c2"], L["w"], L["bias"])["out"]
    assert not np.array_equal(LM.reference(0 * L["x1"], L["c1"], L["x2"], L["c2"], L["w"], L["bias"])["out"], full)
    assert not np.array_equal(LM.reference(L["x1"], L["c1"], 0 * L["x2"], L["c2"], L["w"], L["bias"])["out"], full)
    if (L["c1"] != L["c2"]).any():                                                    # the coefficients are not interchangeable
        assert not np.array_equal(LM.reference(L["x1"], L["c2"], L["x2"], L["c1"], L["w"], L["bias"])["out"], full)
    if K > 4:
        t = (K - 1) // 16 * 16 if K % 16 else K - 16
        assert not np.array_equal(LM.reference(L["x1"][:, :t], L["c1"], L["x2"][:, :t], L["c2"], L["w"][:, :t], L["bias"])["out"], full)
    if M * N >= 64:
        assert (full < 0).any() and (full > 0).any()
