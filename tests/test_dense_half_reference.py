"""CPU tests of ``oracle/dense_half.py`` - the fp64 reference and the lattice operands the GPU file ``test_gpu_dense_ops.py``
holds the dense-half kernels (GEMM forward, weight gradient, ``agg_bwd_prepare``, cross-entropy) to.  No kernel is launched here.

* every reference equals an independent formulation (``np.einsum`` / explicit loops, ``torch`` in fp64 and its autograd);
* for EVERY tuple of the GPU file's exact group (the tables live in ``oracle/dense_half.py``, both files read them) the lattice
  budget holds and an fp32 evaluation in a random order of summation reproduces the fp64 result bit for bit;
* no exact case can pass by vacuity: dropping the last K-slab tail, the last row, one M-slab or one row of ``dbias`` changes it;
* on float operands the same random-order evaluation stays inside ``float_bound`` - the bound is fair for any order;
* saturated cross-entropy rows: the fp64 reference gives the integer sum and the two one-hots.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import agg_backward as AB
from oracle import dense_half as DH


@functools.lru_cache(maxsize=4)
def lin_case(M, N, K):
    return DH.lattice_linear(M, N, K, DH.case_seed("lin", M, N, K))


@functools.lru_cache(maxsize=2)
def prep_case(R, D):
    return DH.lattice_prepare(R, D, DH.case_seed("prep", R, D))


def prep_ref(L, mode, has_out, has_inv):
    R = L["R"]
    return DH.bwd_prepare(L["gout"], L["out"] if has_out else None, L["inv_deg"] if has_inv else None, L["alpha"], DH.MODE[mode],
                          R if mode == "genes" else R + 1, L["h_self"], L["neigh_sum"])


def same_bits(got32, want64):
    want32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return got32.dtype == np.float32 and np.array_equal(want32.astype(np.float64), want64) and np.array_equal(got32, want32)


# ---- the references against independent formulations --------------------------------------------------------------------
@pytest.mark.parametrize("bias,relu", [(False, False), (True, False), (True, True)])
def test_linear_fwd_equals_torch_and_a_loop(bias, relu):
    rng = np.random.default_rng(3)
    x, w, b, s = rng.standard_normal((7, 12)), rng.standard_normal((5, 12)), rng.standard_normal(5), rng.uniform(0.5, 2, 7)
    ref = DH.linear_fwd(x, w, b if bias else None, relu, s)
    want = F.linear(torch.tensor(x), torch.tensor(w), torch.tensor(b) if bias else None)
    want = (torch.relu(want) if relu else want).numpy()
    np.testing.assert_allclose(ref["out"], want, rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(ref["out_scaled"], s[:, None] * want, rtol=1e-13, atol=1e-14)
    for m in range(7):
        for n in range(5):
            terms = [x[m, k] * w[n, k] for k in range(12)] + ([b[n]] if bias else [])
            assert abs(ref["abs_sum"][m, n] - sum(abs(t) for t in terms)) < 1e-12
            assert abs(ref["out"][m, n] - (max(sum(terms), 0.0) if relu else sum(terms))) < 1e-12
    assert DH.linear_fwd(x, w)["out_scaled"] is None


def test_linear_wgrad_equals_autograd_and_einsum():
    rng = np.random.default_rng(4)
    g, x, p = rng.standard_normal((9, 4)), rng.standard_normal((9, 8)), rng.standard_normal((4, 8))
    w = torch.zeros(4, 8, dtype=torch.float64, requires_grad=True)
    (F.linear(torch.tensor(x), w) * torch.tensor(g)).sum().backward()
    ref = DH.linear_wgrad(g, x)
    np.testing.assert_allclose(ref["dW"], w.grad.numpy(), rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(ref["dW"], np.einsum("mn,mk->nk", g, x), rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(ref["abs_sum"], np.einsum("mn,mk->nk", np.abs(g), np.abs(x)), rtol=1e-13)
    acc = DH.linear_wgrad(g, x, p)
    np.testing.assert_allclose(acc["dW"], ref["dW"] + p, rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(acc["abs_sum"], ref["abs_sum"] + np.abs(p), rtol=1e-13)


@pytest.mark.parametrize("mode", ["cells", "genes", "plain"])
@pytest.mark.parametrize("masked", [False, True])
def test_bwd_prepare_equals_autograd_of_the_row_epilogue(mode, masked):
    """The forward these gradients belong to (include/wgnn.h, K1): out = relu((rs * neigh + a_self * h_self) * inv + bias), rs =
    alpha[r] for DST_IS_GENE.  autograd (fp64) of it against the reference: dbias, dh_self, the row dots summed into dalpha, and
    g_scaled as the gradient of what K2t reads (d / d(neigh) for DST_IS_GENE, d / d(neigh) of the unscaled sum otherwise)."""
    rng = np.random.default_rng(5)
    R, D = 6, 8
    m = DH.MODE[mode]
    self_idx = R if mode == "genes" else R + 1
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    alpha, neigh, h_self, bias = t(rng.uniform(0.5, 1.5, R + 2)), t(rng.standard_normal((R, D))), t(rng.standard_normal((R, D))), t(rng.standard_normal(D))
    inv, gout = rng.uniform(0.2, 1.0, R), rng.standard_normal((R, D))
    rs = alpha[:R, None] if mode == "genes" else 1.0
    a_self = 1.0 if mode == "plain" else alpha[self_idx]
    pre = (rs * neigh + a_self * h_self) * torch.tensor(inv)[:, None] + bias
    out = torch.relu(pre) if masked else pre
    (out * torch.tensor(gout)).sum().backward()
    ref = DH.bwd_prepare(gout, out.detach().numpy() if masked else None, inv, alpha.detach().numpy(), m, self_idx, h_self.detach().numpy(),
                         neigh.detach().numpy())
    np.testing.assert_allclose(ref["dbias"], bias.grad.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(ref["dh_self"], h_self.grad.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(ref["g_scaled"], neigh.grad.numpy(), rtol=1e-12, atol=1e-13)
    if mode != "plain":
        dalpha = np.zeros(R + 2)
        dalpha[self_idx] = ref["dself_row"].sum()
        if mode == "genes":
            dalpha[:R] += ref["dalpha_row"]
        np.testing.assert_allclose(dalpha, alpha.grad.numpy(), rtol=1e-12, atol=1e-13)
    g = ref["g"]
    for r in range(R):                                         # explicit loops
        assert abs(ref["abs_dalpha_row"][r] - inv[r] * sum(abs(g[r, c] * neigh[r, c].item()) for c in range(D))) < 1e-12
        assert abs(ref["dself_row"][r] - inv[r] * sum(g[r, c] * h_self[r, c].item() for c in range(D))) < 1e-12
    assert np.allclose(ref["abs_dbias"], np.abs(g).sum(0))
    none = DH.bwd_prepare(gout)
    assert none["dalpha_row"] is None and none["dself_row"] is None and np.array_equal(none["g_scaled"], gout)


def test_ce_sum_equals_torch_and_follows_the_label_rule():
    rng = np.random.default_rng(6)
    x, y = 3 * rng.standard_normal((40, 7)), rng.integers(0, 7, 40)
    xt = torch.tensor(x, requires_grad=True)
    loss = F.cross_entropy(xt, torch.tensor(y), reduction="sum")
    loss.backward()
    ref = DH.ce_sum(x, y)
    assert abs(ref["loss"] - loss.item()) < 1e-11
    np.testing.assert_allclose(ref["dlogits"], xt.grad.numpy(), rtol=1e-12, atol=1e-14)
    y2 = y.copy(); y2[[2, 9]] = -100                          # torch's ignore_index: loss 0, zero row
    xt = torch.tensor(x, requires_grad=True)
    loss = F.cross_entropy(xt, torch.tensor(y2), reduction="sum")
    loss.backward()
    ref = DH.ce_sum(x, y2)
    assert abs(ref["loss"] - loss.item()) < 1e-11 and not ref["dlogits"][[2, 9]].any() and not ref["row_loss"][[2, 9]].any()
    np.testing.assert_allclose(ref["dlogits"], xt.grad.numpy(), rtol=1e-12, atol=1e-14)
    for bad in (-1, 7, (1 << 32) + 1):                       # any other label outside [0, C): NaN, that row only
        y3 = y2.copy(); y3[5] = bad
        r3 = DH.ce_sum(x, y3)
        assert np.isnan(r3["loss"]) and np.isnan(r3["dlogits"][5]).all() and np.isnan(r3["row_loss"][5])
        keep = np.arange(40) != 5
        assert np.array_equal(r3["dlogits"][keep], ref["dlogits"][keep]) and np.array_equal(r3["row_loss"][keep], ref["row_loss"][keep])


# ---- the case tables cover what they claim -----------------------------------------------------------------------------
def test_case_tables_cover_every_axis():
    for inst in DH.LIN_INSTANCES:
        dt, dual, mi = inst
        rows = [c for c in DH.LINEAR_EXACT_CASES if c[0] == dt and c[1] == dual and (c[2] == 64) == (mi == 1)]
        assert len(rows) >= 3
        assert {c[3] for c in rows} == set(DH.LIN_M) and {c[4] for c in rows} == set(DH.LIN_N) and {c[5] for c in rows} == set(DH.LIN_K)
        for axis in (6, 7, 8, 9, 10):
            assert {c[axis] for c in rows} == {False, True}, (inst, axis)
        if mi == 2:
            assert {c[2] for c in rows} == {128, "auto"}
        assert {c[11] for c in rows} == ({False, True} if dual else {False})
    assert len(set(DH.LINEAR_EXACT_CASES)) == len(DH.LINEAR_EXACT_CASES) == 72
    wg = DH.WGRAD_EXACT_CASES
    assert {(c[0], c[3]) for c in wg} == {(m, s) for m in DH.WG_M for s in DH.WG_SLABS}
    assert {(c[1], c[2]) for c in wg} == set(DH.WG_NK) and {c[4] for c in wg} == {0, 1}
    for kind in DH.WG_SLABS:
        assert {c[4] for c in wg if c[3] == kind} == {0, 1}
    for axis in (5, 6, 7):
        assert {c[axis] for c in wg} == {False, True}
    pr = DH.PREPARE_EXACT_CASES
    assert {c[0] for c in pr} >= set(DH.PREP_R) and {c[1] for c in pr} == set(DH.PREP_D) and {c[5] for c in pr} == set(DH.PREP_OUTPUTS)
    for m in ("cells", "genes", "plain"):
        rows = [c for c in pr if c[2] == m]
        assert {c[3] for c in rows} == {False, True} and {c[4] for c in rows} == {False, True} and {c[6] for c in rows} == {False, True}
    assert any(c[0] > 8192 and c[1] == 1024 for c in pr) and any(c[0] > 8192 and c[1] > 768 for c in pr)
    n_part = {min(2048, max(1, -(-c[0] // 4))) for c in pr if "dbias" in DH.PREP_OUTPUTS[c[5]]}   # fold_rows' row count
    assert any(p < 16 for p in n_part) and any(16 <= p <= 49 for p in n_part) and 2048 in n_part
    ce = DH.CE_EXACT_CASES
    assert {c[0] for c in ce} == set(DH.CE_N) and {c[1] for c in ce} == set(DH.CE_C) and (70001, 33) in {(c[0], c[1]) for c in ce}
    assert {c[2] for c in ce} == {False, True} and {c[3] for c in ce} == {False, True}


# ---- exact group: budget, random-order fp32 evaluation, no vacuity ---------------------------------------------------------
@pytest.mark.parametrize("case", DH.LINEAR_EXACT_CASES, ids=DH.lin_id)
def test_linear_lattice_is_exact_in_any_order(case):
    dt, dual, tile, M, N, K, bias, relu = case[:8]
    L = lin_case(M, N, K)
    for key in ("x", "w", "bias", "row_scale"):
        assert np.array_equal(L[key].astype(np.float16).astype(np.float64), L[key]), key      # the __half loader sees the same numbers
    b = L["bias"] if bias else None
    ref = DH.linear_fwd(L["x"], L["w"], b, relu, L["row_scale"])
    assert DH.linear_budget(ref, L["row_scale"]) < 24
    assert float(ref["abs_sum"].max()) / DH.U_OUT <= K * 64 + 64
    rng = np.random.default_rng(DH.case_seed("order", *case))
    got = DH.linear_fp32_random_order(L["x"], L["w"], b, rng)
    got = np.maximum(got, np.float32(0)) if relu else got
    assert same_bits(got, ref["out"])
    assert same_bits(L["row_scale"].astype(np.float32)[:, None] * got, ref["out_scaled"])
    assert DH.linear_sensitive(L, bias, relu)
    # by hand, independent of linear_sensitive: the last K slab, the last x row, the last w row each matter
    t = DH.k_tail(K)
    cut = DH.linear_fwd(L["x"][:, :t], L["w"][:, :t], b, relu)["out"]
    assert not np.array_equal(cut, ref["out"])
    act_b = np.broadcast_to(np.maximum(b, 0) if (relu and bias) else (b if bias else 0.0), (N,))
    assert not np.array_equal(ref["out"][-1], act_b) and not np.array_equal(ref["out"][:, -1], np.full(M, act_b[-1]))


@pytest.mark.parametrize("case", DH.WGRAD_EXACT_CASES, ids=DH.wg_id)
def test_wgrad_lattice_is_exact_in_any_order(case):
    M, N, K, slabs, acc = case[:5]
    L = DH.lattice_wgrad(M, N, K, DH.case_seed("wg", M, N, K))
    for key in ("g", "x", "prior"):
        assert np.array_equal(L[key].astype(np.float32).astype(np.float64), L[key])
    prior = L["prior"] if acc else None
    ref = DH.linear_wgrad(L["g"], L["x"], prior)
    assert DH.wgrad_budget(ref) < 24
    rng = np.random.default_rng(DH.case_seed("order", *case))
    assert same_bits(DH.wgrad_fp32_random_order(L["g"], L["x"], prior, rng, n_slabs=int(rng.integers(1, 9))), ref["dW"])
    # no vacuity: the last row, the first 16-row step (an M slab), the last 16-row step each change the result
    for keep in (slice(0, M - 1), slice(min(16, M), M), slice(0, ((M - 1) // 16) * 16)):
        assert not np.array_equal(DH.linear_wgrad(L["g"][keep], L["x"][keep], prior)["dW"], ref["dW"])
    assert L["g"][-1, -1] * L["x"][-1, -1] != 0                # the last row reaches the last element of dW


@pytest.mark.parametrize("case", DH.PREPARE_EXACT_CASES, ids=DH.prep_id)
def test_prepare_lattice_is_exact_in_any_order(case):
    R, D, mode, has_out, has_inv, outputs, _ = case
    L = prep_case(R, D)
    ref = prep_ref(L, mode, has_out, has_inv)
    assert max(DH.prepare_budget(ref).values()) < 24
    rng = np.random.default_rng(DH.case_seed("order", *case))
    inv32 = (L["inv_deg"] if has_inv else np.ones(R)).astype(np.float32)
    assert same_bits(inv32 * AB.dot_fp32_random_order(ref["g"], L["neigh_sum"], rng), ref["dalpha_row"])
    assert same_bits(inv32 * AB.dot_fp32_random_order(ref["g"], L["h_self"], rng), ref["dself_row"])
    assert same_bits(DH.colsum_fp32_random_order(ref["g"], rng, n_part=int(rng.integers(1, 12))), ref["dbias"])
    f = inv32 * (L["alpha"][:R].astype(np.float32) if mode == "genes" else np.float32(1))
    assert same_bits(f[:, None] * ref["g"].astype(np.float32), ref["g_scaled"])
    a_self = np.float32(1 if mode == "plain" else L["alpha"][R if mode == "genes" else R + 1])
    assert same_bits((a_self * inv32)[:, None] * ref["g"].astype(np.float32), ref["dh_self"])
    # no vacuity: one row of dbias, the last row's dots, the last 256-column slab
    assert DH.prepare_sensitive(L, has_out)
    assert not np.array_equal(ref["g"][:-1].sum(0), ref["dbias"]) and ref["dalpha_row"][-1] != 0 and ref["dself_row"][-1] != 0
    assert ref["g_scaled"][-1, -1] != 0 and ref["dh_self"][-1, -1] != 0
    t = DH.col_tail(D)
    g = ref["g"]
    assert (g[-1, :t] * L["neigh_sum"][-1, :t]).sum() != (g[-1] * L["neigh_sum"][-1]).sum()
    assert (g[-1, :t] * L["h_self"][-1, :t]).sum() != (g[-1] * L["h_self"][-1]).sum()
    if has_out and R * D >= 64:
        assert (ref["g"] != L["gout"]).any()                   # the mask bites


@pytest.mark.parametrize("case", DH.CE_EXACT_CASES, ids=DH.ce_id)
def test_saturated_ce_rows_are_integers_and_one_hots(case):
    n, C = case[:2]
    S = DH.saturated_ce(n, C, DH.case_seed("ce", n, C))
    x, y = S["logits"], S["labels"]
    assert np.array_equal(x, np.round(x)) and (x.max(1) == 0).all() and ((x == 0).sum(1) == 1).all() and (x[x != 0] <= -200).all()
    assert np.float32(np.exp(np.float64(-200.0))) == 0.0 and np.exp(np.float32(-200.0)) == 0.0      # expf underflows to +0
    assert DH.ce_budget(S) < 24
    ref = DH.ce_sum(x, y)
    assert np.array_equal(ref["row_loss"], S["row_loss"]) and ref["loss"] == S["loss"] == float(int(S["loss"]))
    live = y != DH.IGNORE_INDEX
    want = np.zeros((n, C))
    want[np.arange(n), x.argmax(1)] += 1.0
    want[np.arange(n)[live], y[live]] -= 1.0
    want[~live] = 0.0
    assert np.array_equal(S["dlogits"], want)
    # the fp64 softmax differs from the one-hot by e^-200 per entry: far below half an ulp of any fp32 number the kernel could give
    assert np.abs(ref["dlogits"] - want).max() < 1e-80 and np.array_equal(ref["dlogits"].astype(np.float32), want.astype(np.float32))
    if n > 20:
        assert (~live).sum() >= 1
    if C > 1 and n > 20:
        assert S["loss"] >= 200 and (S["row_loss"][live] == 0).any()      # both kinds of row: a wrong label, the maximal class
    # fp32 evaluation of the kernel's formula, rows summed in a random order
    x32 = x.astype(np.float32)
    e = np.exp(x32 - x32.max(1, keepdims=True))
    s = e.sum(1, dtype=np.float32)
    assert (s == 1).all()
    row = np.where(live, (np.log(s) - x32[np.arange(n), np.where(live, y, 0)]).astype(np.float32), np.float32(0))
    acc = np.float32(0)
    for i in np.random.default_rng(n + C).permutation(n)[:5000]:
        acc = acc + row[i]
    assert acc.dtype == np.float32 and float(acc) <= S["loss"] and same_bits(row, S["row_loss"])


# ---- float group: the derived bound is fair for any order ------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,dt", DH.LINEAR_FLOAT_CASES)
def test_linear_float_bound_holds_in_random_order(M, N, K, dt):
    rng = np.random.default_rng(DH.case_seed("flin", M, N, K))
    x, w, b = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    if dt == "f16":
        x = x.astype(np.float16).astype(np.float32)
    ref = DH.linear_fwd(x, w, b)
    got = DH.linear_fp32_random_order(x, w, b, rng)
    r = AB.worst_ratio(got, ref["out"], AB.float_bound(ref["abs_sum"], K + 1))
    assert 0 < r <= 1, r


@pytest.mark.parametrize("M,N,K", DH.WGRAD_FLOAT_CASES)
def test_wgrad_float_bound_holds_in_random_order(M, N, K):
    rng = np.random.default_rng(DH.case_seed("fwg", M, N, K))
    g, x = rng.standard_normal((M, N)).astype(np.float32), rng.standard_normal((M, K)).astype(np.float32)
    ref = DH.linear_wgrad(g, x)
    got = DH.wgrad_fp32_random_order(g, x, None, rng, n_slabs=8)
    r = AB.worst_ratio(got, ref["dW"], AB.float_bound(ref["abs_sum"], M + 8))
    assert 0 < r <= 1, r


@pytest.mark.parametrize("R,D,mode", DH.PREPARE_FLOAT_CASES)
def test_prepare_float_bound_holds_in_random_order(R, D, mode):
    rng = np.random.default_rng(DH.case_seed("fprep", R, D))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    gout, out, h_self, neigh, inv = f(R, D), f(R, D), f(R, D), f(R, D), rng.uniform(0.05, 1, R).astype(np.float32)
    ref = DH.bwd_prepare(gout, out, inv, None, DH.NO_ALPHA, 0, h_self, neigh)
    g32 = ref["g"].astype(np.float32)
    for key, other in (("dalpha_row", neigh), ("dself_row", h_self)):
        got = inv * AB.dot_fp32_random_order(g32, other, rng)
        r = AB.worst_ratio(got, ref[key], AB.float_bound(ref["abs_" + key], D))
        assert 0 < r <= 1, (key, r)
    r = AB.worst_ratio(DH.colsum_fp32_random_order(g32, rng, n_part=9), ref["dbias"], AB.float_bound(ref["abs_dbias"], R))
    assert 0 < r <= 1, r
