"""fp64 reference of the DENSE half of a layer and of the training glue - ``wgnn_linear_fwd[_ex]``, ``wgnn_linear_wgrad``,
``wgnn_agg_bwd_prepare``, ``wgnn_ce_sum_fwd_bwd`` - written from the formulas in ``include/wgnn.h`` with numpy only, the
dyadic-lattice operands that make an fp32 kernel owe the fp64 result BIT FOR BIT, and the case tables of the two test files
that use them (``tests/test_dense_half_reference.py``: CPU; ``tests/test_gpu_dense_ops.py``: the kernels).

TEST INFRASTRUCTURE ONLY (see ``oracle/wgnn_oracle.py``): nothing here imports ``scdeepsort_amd``.

The two demands are those of ``oracle/agg_backward.py``, whose ``lattice_budget`` / ``EXACT_LIMIT`` / ``float_bound`` /
``worst_ratio`` are reused:

* **lattice**: operands are small integers times a power of two (all exact in fp16 too, so the ``__half`` loader of the GEMM is
  covered); every product and every partial sum is a multiple of a fixed unit, and while ``sum|terms| / unit < 2**24`` each is
  exact in fp32 in any order, with or without FMA, through the matrix cores or not.
* **saturated cross-entropy rows**: integer logits with one entry 0 and every other entry <= -200.  ``expf`` of a non-maximal
  entry is 0 in fp32 (e^-200 << 2^-150), the row's exponential sum is exactly 1 and its logarithm exactly 0: the row loss is
  ``-x[y]`` (an integer, 0 when the label is the maximal class), ``dlogits = onehot(argmax) - onehot(y)``, and the total is an
  exact integer below 2**24 - no tolerance at any row count.
* **derived bound** for ordinary floats: ``float_bound(abs_sum, n_terms)``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .agg_backward import (DST_IS_GENE, EXACT_LIMIT, NO_ALPHA, SRC_IS_GENE, dot_fp32_random_order, float_bound,  # noqa: F401
                           lattice_budget, worst_ratio)

MODE = {"cells": SRC_IS_GENE, "genes": DST_IS_GENE, "plain": NO_ALPHA}
IGNORE_INDEX = -100                                    # torch's default ignore_index (include/wgnn.h: loss 0, zero dlogits row)
LIN_BK = 16                                            # K slab of linear_mfma_f32 / row step of wgrad_mfma_f32

# lattice units
U_X, U_W = 0.25, 0.125                                 # forward: x = i/4, w = j/8, bias = b/4  ->  out in units of 1/32
U_OUT = U_X * U_W
U_G = 0.25                                             # wgrad: g = i/4, x = j/4, prior = p/16   ->  dW in units of 1/16
U_DW = U_G * U_X
LATTICE_SCALE = (0.5, 1.0, 2.0)                        # row_scale, inv_deg, alpha
U_SCALE = 0.5
LATTICE_INT = 8                                        # |i|, |j| <= 8
PREP_INT, PREP_NEIGH_INT = 2, 4                        # gout / out / h_self in [-2, 2], neigh_sum in [-4, 4]


def _f64(x) -> Optional[np.ndarray]:
    return None if x is None else np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------------------------------------
# fp64 references
# ------------------------------------------------------------------------------------------------
def linear_fwd(x, w, bias=None, relu: bool = False, row_scale=None) -> dict:
    """``out = act(x . w^T + bias)``, ``out_scaled[m] = row_scale[m] * out[m]`` (None without ``row_scale``) and
    ``abs_sum = |x| . |w|^T + |bias|`` (the sum of the absolute values of the K + 1 terms of an element)."""
    x, w, bias, row_scale = _f64(x), _f64(w), _f64(bias), _f64(row_scale)
    out = x @ w.T
    abs_sum = np.abs(x) @ np.abs(w).T
    if bias is not None:
        out, abs_sum = out + bias, abs_sum + np.abs(bias)
    if relu:
        out = np.maximum(out, 0.0)
    return dict(out=out, out_scaled=None if row_scale is None else row_scale[:, None] * out, abs_sum=abs_sum)


def linear_wgrad(g, x, prior=None) -> dict:
    """``dW[N, K] = sum_m g[m, N] * x[m, K]`` (+ ``prior`` under ``accumulate``) and the abs-sum of its terms."""
    g, x, prior = _f64(g), _f64(x), _f64(prior)
    dW, abs_sum = g.T @ x, np.abs(g).T @ np.abs(x)
    if prior is not None:
        dW, abs_sum = dW + prior, abs_sum + np.abs(prior)
    return dict(dW=dW, abs_sum=abs_sum)


def bwd_prepare(gout, out=None, inv_deg=None, alpha=None, mode: int = NO_ALPHA, self_idx: int = 0, h_self=None,
                neigh_sum=None) -> dict:
    """Every output of ``wgnn_agg_bwd_prepare`` as ``include/wgnn.h`` defines it:

        g = gout * (out > 0)                         g_scaled[r] = inv_deg[r] * (alpha[r] for DST_IS_GENE) * g[r]
        dh_self[r] = alpha[self_idx] * inv_deg[r] * g[r]   (alpha = 1 for NO_ALPHA)
        dalpha_row[r] = inv_deg[r] * <g[r], neigh_sum[r]>  dself_row[r] = inv_deg[r] * <g[r], h_self[r]>
        dbias[c] = sum_r g[r, c]

    (``dalpha_row`` / ``dself_row`` None without their operand; inv_deg None = 1) plus ``abs_dalpha_row``, ``abs_dself_row``,
    ``abs_dbias``: the abs-sums of the reduced outputs."""
    gout, out, inv_deg, alpha, h_self, neigh_sum = map(_f64, (gout, out, inv_deg, alpha, h_self, neigh_sum))
    R = gout.shape[0]
    g = gout if out is None else np.where(out > 0, gout, 0.0)
    inv = np.ones(R) if inv_deg is None else inv_deg
    f_src = inv * (alpha[:R] if mode == DST_IS_GENE else 1.0)
    a_self = 1.0 if mode == NO_ALPHA else alpha[self_idx]
    res = dict(g=g, g_scaled=f_src[:, None] * g, dh_self=(a_self * inv)[:, None] * g, dbias=g.sum(0), abs_dbias=np.abs(g).sum(0),
               dalpha_row=None, abs_dalpha_row=None, dself_row=None, abs_dself_row=None)
    if neigh_sum is not None:
        res["dalpha_row"] = inv * (g * neigh_sum).sum(1)
        res["abs_dalpha_row"] = np.abs(inv) * (np.abs(g) * np.abs(neigh_sum)).sum(1)
    if h_self is not None:
        res["dself_row"] = inv * (g * h_self).sum(1)
        res["abs_dself_row"] = np.abs(inv) * (np.abs(g) * np.abs(h_self)).sum(1)
    return res


def ce_sum(logits, labels) -> dict:
    """CrossEntropyLoss(reduction='sum') and its gradient: ``row_loss[r] = logsumexp(x[r]) - x[r, y]``, ``dlogits[r] =
    softmax(x[r]) - onehot(y)``; a label of -100 gives 0 and a zero row, any other label outside [0, C) NaN and a NaN row
    (``include/wgnn.h``).  Returns ``loss`` (the sum, NaN if any row is), ``row_loss`` and ``dlogits``."""
    x = _f64(logits)
    y = np.asarray(labels, dtype=np.int64)
    n, C = x.shape
    m = x.max(1, keepdims=True) if C else np.zeros((n, 1))
    e = np.exp(x - m)
    s = e.sum(1, keepdims=True)
    lse = (m + np.log(s))[:, 0]
    ignored, ok = y == IGNORE_INDEX, (y >= 0) & (y < C)
    yy = np.where(ok, y, 0)
    onehot = np.zeros_like(x)
    onehot[np.arange(n), yy] = 1.0
    row_loss = np.where(ignored, 0.0, np.where(ok, lse - x[np.arange(n), yy], np.nan))
    d = np.where(ignored[:, None], 0.0, np.where(ok[:, None], e / s - onehot, np.nan))
    return dict(loss=float(row_loss.sum()), row_loss=row_loss, dlogits=d)


# ------------------------------------------------------------------------------------------------
# lattice operands
# ------------------------------------------------------------------------------------------------
def case_seed(*key) -> int:
    return sum((i + 1) * sum(map(ord, str(k))) for i, k in enumerate(key)) % (2 ** 31)


def k_tail(K: int) -> int:
    """First column of the last (possibly partial) 16-wide K slab."""
    return ((K - 1) // LIN_BK) * LIN_BK


def lattice_linear(M: int, N: int, K: int, seed: int) -> dict:
    """x [M, K] = i/4, w [N, K] = j/8, bias [N] = b/4, row_scale [M] in {0.5, 1, 2}; |i|, |j|, |b| <= 8 (float64; exact in fp32
    and fp16).  Drawn again (seed + 1, ...) until the case is SENSITIVE with and without ReLU and bias - see ``linear_sensitive``."""
    for attempt in range(256):
        rng = np.random.default_rng(seed + attempt)
        ri = lambda *s: rng.integers(-LATTICE_INT, LATTICE_INT + 1, s).astype(np.float64)
        L = dict(M=M, N=N, K=K, x=ri(M, K) * U_X, w=ri(N, K) * U_W, bias=ri(N) * U_X, row_scale=rng.choice(LATTICE_SCALE, M))
        if all(linear_sensitive(L, b, r) for b in (False, True) for r in (False, True)):
            return L
    raise AssertionError("no sensitive lattice draw")


def linear_sensitive(L: dict, bias: bool, relu: bool) -> bool:
    """The exact comparison cannot pass by vacuity: zeroing the last K slab's columns changes the last row and the last column of
    the result, and the last row / column is not what a kernel that skipped it (no x row / no w row: act(bias)) would leave."""
    b = L["bias"] if bias else None
    full = linear_fwd(L["x"], L["w"], b, relu)["out"]
    xt = L["x"].copy()
    xt[:, k_tail(L["K"]):] = 0.0
    cut = linear_fwd(xt, L["w"], b, relu)["out"]
    skipped = linear_fwd(np.zeros_like(L["x"]), L["w"], b, relu)["out"]
    return bool((full[-1] != cut[-1]).any() and (full[:, -1] != cut[:, -1]).any() and (full[-1] != skipped[-1]).any()
                and (full[:, -1] != skipped[:, -1]).any())


def linear_budget(ref: dict, row_scale=None) -> float:
    """``lattice_budget`` of the forward: sums in units of 1/32; the scaled copy in units of 1/64."""
    b = lattice_budget(ref["abs_sum"], U_OUT)
    if row_scale is not None:
        b = max(b, lattice_budget(np.abs(_f64(row_scale))[:, None] * ref["abs_sum"], U_OUT * U_SCALE))
    return b


def lattice_wgrad(M: int, N: int, K: int, seed: int) -> dict:
    """g [M, N] = i/4, x [M, K] = j/4 (|i|, |j| <= 8), prior dW [N, K] = p/16 (|p| <= 64).  The last row of both is non-zero in
    its last element (so a dropped last row or last column shows)."""
    rng = np.random.default_rng(seed)
    ri = lambda *s: rng.integers(-LATTICE_INT, LATTICE_INT + 1, s).astype(np.float64)
    g, x = ri(M, N) * U_G, ri(M, K) * U_X
    g[-1, -1], x[-1, -1] = (g[-1, -1] or U_G), (x[-1, -1] or U_X)
    return dict(M=M, N=N, K=K, g=g, x=x, prior=rng.integers(-64, 65, (N, K)).astype(np.float64) * U_DW)


def wgrad_budget(ref: dict) -> float:
    return lattice_budget(ref["abs_sum"], U_DW)


def lattice_prepare(R: int, D: int, seed: int) -> dict:
    """gout, out, h_self [R, D] integers in [-2, 2] (``out`` <= 0 on about 3/5 of the elements: the ReLU mask bites), neigh_sum
    integers in [-4, 4], inv_deg [R] and alpha [R + 2] in {0.5, 1, 2}.  The last row's last element of gout is non-zero and
    unmasked, with non-zero partners in h_self / neigh_sum."""
    for attempt in range(256):
        rng = np.random.default_rng(seed + attempt)
        ri = lambda k, *s: rng.integers(-k, k + 1, s).astype(np.float64)
        L = dict(R=R, D=D, gout=ri(PREP_INT, R, D), out=ri(PREP_INT, R, D), h_self=ri(PREP_INT, R, D),
                 neigh_sum=ri(PREP_NEIGH_INT, R, D), inv_deg=rng.choice(LATTICE_SCALE, R), alpha=rng.choice(LATTICE_SCALE, R + 2))
        if R:
            L["gout"][-1, -1], L["out"][-1, -1], L["h_self"][-1, -1], L["neigh_sum"][-1, -1] = 1.0, 2.0, 1.0, 1.0
        if R == 0 or all(prepare_sensitive(L, m) for m in (False, True)):
            return L
    raise AssertionError("no sensitive lattice draw")


def col_tail(D: int) -> int:
    """First column of the last (possibly partial) 256-column slab of agg_bwd_prepare."""
    return ((D - 1) // 256) * 256


def prepare_sensitive(L: dict, masked: bool) -> bool:
    """The last row's dots are non-zero and change when the last 256-column slab is dropped, its last gradient element
    survives the mask: a dropped last row, last slab or last column shows in every output."""
    last = {k: L[k][-1:] for k in ("gout", "out", "inv_deg", "h_self", "neigh_sum")}
    full = bwd_prepare(last["gout"], last["out"] if masked else None, last["inv_deg"], None, NO_ALPHA, 0, last["h_self"], last["neigh_sum"])
    t = col_tail(L["D"])
    cut = bwd_prepare(last["gout"][:, :t], last["out"][:, :t] if masked else None, last["inv_deg"], None, NO_ALPHA, 0,
                      last["h_self"][:, :t], last["neigh_sum"][:, :t])
    return bool(full["g"][-1, -1] != 0 and all(full[k][-1] != 0 and full[k][-1] != cut[k][-1] for k in ("dalpha_row", "dself_row")))


def prepare_budget(ref: dict) -> dict:
    """``lattice_budget`` of every sum the kernel forms (the row dots before the inv_deg factor and after it, the column sums)
    and of the elementwise products (three lattice factors: exact by construction, checked all the same)."""
    out = dict(dbias=lattice_budget(ref["abs_dbias"], 1.0), g_scaled=lattice_budget(np.abs(ref["g_scaled"]), U_SCALE * U_SCALE),
               dh_self=lattice_budget(np.abs(ref["dh_self"]), U_SCALE * U_SCALE))
    for k in ("dalpha_row", "dself_row"):
        if ref["abs_" + k] is not None:
            out[k] = lattice_budget(ref["abs_" + k], U_SCALE)
    return out


def saturated_ce(n: int, C: int, seed: int, ignore_every: int = 17) -> dict:
    """Saturated rows: logits [n, C] integers, one entry 0 (a random class), every other in [-215, -200]; labels random in
    [0, C), every ``ignore_every``-th row (from row 3) labelled -100.  ``row_loss`` / ``loss`` / ``dlogits``: what the kernel owes,
    written down directly (integers and one-hots) - ``ce_sum`` must agree (CPU test)."""
    rng = np.random.default_rng(seed)
    x = -rng.integers(200, 216, (n, C)).astype(np.float64)
    top = rng.integers(0, C, n)
    x[np.arange(n), top] = 0.0
    y = rng.integers(0, C, n).astype(np.int64)
    y[3::ignore_every] = IGNORE_INDEX
    live = y != IGNORE_INDEX
    yy = np.where(live, y, 0)
    row_loss = np.where(live, -x[np.arange(n), yy], 0.0)
    d = np.zeros((n, C))
    d[np.arange(n), top] += 1.0
    d[np.arange(n), yy] -= 1.0
    d[~live] = 0.0
    return dict(n=n, C=C, logits=x, labels=y, top=top, row_loss=row_loss, loss=float(row_loss.sum()), dlogits=d)


def ce_budget(case: dict) -> float:
    """The total (a sum of non-negative integers: every partial sum in any order is an integer <= the total) stays below 2**24."""
    return lattice_budget(np.array([np.abs(case["row_loss"]).sum()]), 1.0)


# ------------------------------------------------------------------------------------------------
# fp32 evaluation in a random order (CPU tests: the two demands are fair for ANY order)
# ------------------------------------------------------------------------------------------------
def _random_blocks(n: int, rng, max_block: int = 24):
    """A random permutation of range(n) cut into blocks of random length (one fp32 partial product each)."""
    perm = rng.permutation(n)
    i = 0
    while i < n:
        j = min(n, i + int(rng.integers(1, max_block + 1)))
        yield perm[i:j]
        i = j


def linear_fp32_random_order(x, w, bias, rng) -> np.ndarray:
    """``x . w^T + bias`` in fp32: the K axis permuted and cut into random blocks, block products (fp32) added one after the
    other, the bias added after a random block."""
    x32, w32 = np.asarray(x, dtype=np.float32), np.asarray(w, dtype=np.float32)
    blocks = list(_random_blocks(x32.shape[1], rng))
    at = int(rng.integers(0, len(blocks)))
    acc = np.zeros((x32.shape[0], w32.shape[0]), dtype=np.float32)
    for i, idx in enumerate(blocks):
        acc = acc + x32[:, idx] @ w32[:, idx].T
        if bias is not None and i == at:
            acc = acc + np.asarray(bias, dtype=np.float32)
    assert acc.dtype == np.float32
    return acc


def wgrad_fp32_random_order(g, x, prior, rng, n_slabs: int = 5) -> np.ndarray:
    """``g^T . x (+ prior)`` in fp32 as a split reduction: the M axis permuted, dealt to ``n_slabs`` partial sums block by
    block, the partials (and the prior) folded in a random order."""
    g32, x32 = np.asarray(g, dtype=np.float32), np.asarray(x, dtype=np.float32)
    parts = [np.zeros((g32.shape[1], x32.shape[1]), dtype=np.float32) for _ in range(n_slabs)]
    for idx in _random_blocks(g32.shape[0], rng, 64):
        p = int(rng.integers(0, n_slabs))
        parts[p] = parts[p] + g32[idx].T @ x32[idx]
    if prior is not None:
        parts.append(np.asarray(prior, dtype=np.float32))
    acc = np.zeros_like(parts[0])
    for p in rng.permutation(len(parts)):
        acc = acc + parts[p]
    assert acc.dtype == np.float32
    return acc


def colsum_fp32_random_order(g, rng, n_part: int = 7) -> np.ndarray:
    """Column sums in fp32: rows permuted, dealt block by block to ``n_part`` partial rows, the partials folded in a random order."""
    g32 = np.asarray(g, dtype=np.float32)
    parts = np.zeros((n_part, g32.shape[1]), dtype=np.float32)
    for idx in _random_blocks(g32.shape[0], rng, 64):
        p = int(rng.integers(0, n_part))
        for r in idx:
            parts[p] = parts[p] + g32[r]
    acc = np.zeros(g32.shape[1], dtype=np.float32)
    for p in rng.permutation(n_part):
        acc = acc + parts[p]
    return acc


# ------------------------------------------------------------------------------------------------
# case tables (plain data; the CPU file checks the lattice budget of every tuple the GPU file runs)
# ------------------------------------------------------------------------------------------------
# wgnn_linear_fwd_ex.  The eight instantiations of linear_mfma_f32<TX, DUAL, MI>: x stored f32 | f16, single | dual output, the
# 64-row tile (MI = 1: only when forced) | the 128-row tile (MI = 2: forced, or the entry's own choice, which is 128 rows at
# every M here).  Nine cases each: every N, every M and every K meets every instantiation; the options rotate.
#   (x_dtype, dual, tile, M, N, K, bias, relu, ld_x > K, ld_w > K, ld_out > N [and ld_out_scaled != ld_out], out == NULL)
LIN_M = (1, 63, 64, 65, 127, 128, 129, 257)
LIN_N = (1, 5, 31, 33, 127, 128, 129, 200, 257)
LIN_K = (4, 12, 16, 20, 36, 52, 400)
LIN_INSTANCES = [(dt, dual, mi) for dt in ("f32", "f16") for dual in (False, True) for mi in (1, 2)]
LINEAR_EXACT_CASES = [(dt, dual, 64 if mi == 1 else (128, "auto")[(i + q) % 2], LIN_M[(i + q) % 8], LIN_N[i], LIN_K[(i + 2 * q) % 7],
                       (i + q) % 2 == 0, (i // 2 + q) % 2 == 0, (i + q) % 3 == 0, (i // 3 + q) % 2 == 0, (i + 2 * q) % 3 != 0,
                       dual and (i + q) % 4 == 1)
                      for q, (dt, dual, mi) in enumerate(LIN_INSTANCES) for i in range(9)]
# wgnn_linear_wgrad: (M, N, K, n_slabs, accumulate, ld_g > N, ld_x > K, ld_dw > K)
#   n_slabs: a count | "ws" (what wgnn_linear_wgrad_workspace returns) | "over" (M // 16 + 3: trailing slabs own no rows).
#   35 cases: every M meets every n_slabs; the shapes and options rotate.
WG_M = (1, 15, 16, 17, 100, 513, 4099)
WG_NK = ((4, 4), (16, 52), (132, 400), (200, 200), (256, 256), (260, 132))
WG_SLABS = (1, 3, 7, "ws", "over")
WGRAD_EXACT_CASES = [(WG_M[i % 7], *WG_NK[i % 6], WG_SLABS[i % 5], (i // 3) % 2, i % 2 == 0, (i // 2) % 2 == 0, i % 3 != 0)
                     for i in range(35)]
# wgnn_agg_bwd_prepare: (R, D, mode, out given, inv_deg given, outputs, ld > D for gout / out / h_self / dh_self)
#   outputs: which of g_scaled / dh_self / dalpha_row / dself_row / dbias are asked for (the others NULL)
PREP_R = (1, 3, 4, 5, 777, 8191, 8193, 20000)
PREP_D = (4, 252, 256, 260, 768, 772, 1024)
PREP_OUTPUTS = {"all": ("g_scaled", "dh_self", "dalpha_row", "dself_row", "dbias"), "dbias": ("dbias",), "g_scaled": ("g_scaled",),
                "rows": ("dalpha_row", "dself_row"), "dh_self": ("dh_self",), "no_dbias": ("g_scaled", "dh_self", "dalpha_row", "dself_row")}
PREPARE_EXACT_CASES = [(PREP_R[i % 8], PREP_D[i % 7], ("cells", "genes", "plain")[i % 3], (i // 2) % 2 == 0, (i // 3) % 2 == 0,
                        tuple(PREP_OUTPUTS)[(i + i // 6) % 6], i % 2 == 1) for i in range(24)]
PREPARE_EXACT_CASES += [(20000, 1024, "genes", True, True, "all", True),       # the largest operand: grid-stride loop x four slabs
                        (8193, 768, "plain", False, True, "dbias", False),
                        (100, 260, "cells", True, False, "all", True),         # 25 block partials: fold_rows' tail loop alone
                        (196, 4, "genes", True, True, "dbias", False)]         # 49 partials: one thread enters the unrolled loop
# wgnn_ce_sum_fwd_bwd on saturated rows: (n, C, ld_logits > C, ld_dlogits > C)
CE_N = (1, 255, 256, 257, 16384, 16385, 70001)
CE_C = (1, 2, 5, 16, 33)
CE_EXACT_CASES = [(CE_N[i % 7], CE_C[(2 * i + 2) % 5], i % 2 == 0, (i // 2) % 2 == 0) for i in range(14)]
# float group
LINEAR_FLOAT_CASES = [(M, N, K, dt) for (M, N, K) in ((300, 200, 52), (2049, 256, 400), (777, 33, 256)) for dt in ("f32", "f16")]
WGRAD_FLOAT_CASES = [(513, 16, 52), (4099, 132, 400), (2049, 256, 256)]
PREPARE_FLOAT_CASES = [(777, 252, "genes"), (8193, 260, "cells"), (3000, 1024, "plain")]
CE_FLOAT_CASES = [(513, 5), (1000, 16), (70001, 33)]


def lin_id(c) -> str:
    return (f"{c[0]}-dual{int(c[1])}-tile{c[2]}-M{c[3]}-N{c[4]}-K{c[5]}-bias{int(c[6])}-relu{int(c[7])}-ldx{int(c[8])}-ldw{int(c[9])}"
            f"-ldo{int(c[10])}-nullout{int(c[11])}")


def wg_id(c) -> str:
    return f"M{c[0]}-N{c[1]}-K{c[2]}-slabs{c[3]}-acc{c[4]}-ldg{int(c[5])}-ldx{int(c[6])}-lddw{int(c[7])}"


def prep_id(c) -> str:
    return f"R{c[0]}-D{c[1]}-{c[2]}-out{int(c[3])}-inv{int(c[4])}-{c[5]}-ld{int(c[6])}"


def ce_id(c) -> str:
    return f"n{c[0]}-C{c[1]}-ldx{int(c[2])}-ldd{int(c[3])}"
