"""fp64 restatement of per-cell gene attribution (``wgnn_attrib_rows`` / ``ResidentPredictor.explain``), written from the
formulas in ``include/wgnn.h`` - a helper for the CPU and GPU tests, not a test module.

For one test cell with expressed genes g, raw values x_g, deg, S = sum x_g and an L-layer model with tables T_l, biases b_l,
self weights W_l (l >= 2) and head (Wh, bh):

    u_{1,g} = x_g (alpha[g] deg / S + alpha[G+1] / (S + 1e-6)) / (deg + 1)        self-loop from the row
    u_{l,g} = alpha[g] (deg x_g / S) / (deg + 1)                                   explicit-self layers
    z_l     = sum_g u_{l,g} T_l[g] + [explicit] alpha[G+1] / (deg + 1) * self_l + b_l ,   h_l = ReLU(z_l)
    v_L = (z_L > 0) * Wh[t] ,   v_{l-1} = (z_{l-1} > 0) * (W_l^T v_l) * alpha[G+1] / (deg + 1)
    phi_g = sum_l u_{l,g} <T_l[g], v_l> ,   base = bh[t] + sum_l <v_l, b_l> ,   sum_g phi_g + base == logit_t
"""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -24


def ragged_batch(rng, B, G, long_row=5000):
    """The ragged batch of test_gpu_resident_predict.py (same draws in the same order): two empty rows, one row longer than
    4096 entries, the rest 1 .. 300 genes."""
    lens = rng.integers(1, 300, B)
    lens[1] = 0
    lens[B - 2] = 0
    lens[3] = long_row
    rows, cols = [], []
    for r, n in enumerate(lens):
        cols.append(np.sort(rng.choice(G, size=int(n), replace=False)))
        rows.append(np.full(int(n), r))
    cols = np.concatenate(cols); rows = np.concatenate(rows)
    vals = np.clip(rng.normal(3.0, 1.0, cols.shape[0]), 0.2, 7.0).astype(np.float32)
    return sp.csr_matrix((vals, (rows, cols)), shape=(B, G))


KERNEL_CASES = [(H, i64) for H in (12, 16, 64, 200, 256) for i64 in (False, True)]
KERNEL_CLASSES = (2, 5, 16, 40)


def kernel_case(H, i64):
    """The inputs of the kernel test for one (H, rowptr width): seed H * 2 + i64, G 6000, 40 cells, and one head per
    (C, self rule) drawn in the order test_gpu_resident_predict.py draws them."""
    rng = np.random.default_rng(H * 2 + i64)
    G, B = 6000, 40
    c = SimpleNamespace(G=G, B=B, H=H, i64=i64)
    c.m = ragged_batch(rng, B, G)
    c.table = (0.5 * rng.standard_normal((G, H))).astype(np.float32)
    c.alpha = rng.uniform(0.5, 1.5, G + 2).astype(np.float32)
    c.bias = (0.1 * rng.standard_normal(H)).astype(np.float32)
    c.self_rows = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    c.heads = {}
    for C_ in KERNEL_CLASSES:
        for explicit in (False, True):
            w = (rng.standard_normal((C_, H)) / np.sqrt(H)).astype(np.float32)
            b = (0.1 * rng.standard_normal(C_)).astype(np.float32)
            c.heads[(C_, explicit)] = (w, b)
    c.targets = {C_: np.random.default_rng(1000 + H * 2 + i64 + C_).integers(0, C_, B).astype(np.int32) for C_ in KERNEL_CLASSES}
    return c


def message_weights(m, alpha, explicit_self):
    """u per stored entry (CSR order), the entries' row ids and deg per row."""
    m = m.tocsr()
    G = m.shape[1]
    n = np.diff(m.indptr)
    rows = np.repeat(np.arange(m.shape[0]), n)
    deg = n.astype(np.float64)
    x = m.data.astype(np.float64)
    S = np.bincount(rows, weights=x, minlength=m.shape[0])
    a = np.asarray(alpha, np.float64).ravel()
    u = a[m.indices] * deg[rows] * x / S[rows]
    if not explicit_self:
        u = u + x * a[G + 1] / (S[rows] + 1e-6)
    return u / (deg[rows] + 1.0), rows, deg


def direction_scores(m, table, alpha, direction, explicit_self):
    """score_j = u_j <table[g_j], direction[cell_j]> (direction mode of one layer)."""
    u, rows, _ = message_weights(m, alpha, explicit_self)
    T = np.asarray(table, np.float64)[m.tocsr().indices]
    return u * np.einsum("ij,ij->i", T, np.asarray(direction, np.float64)[rows])


def attribution(m, tables, alpha, biases, self_weights, w_head, b_head, target=None, self_rows0=None):
    """The whole quantity for an L = len(tables) layer model.  ``self_weights[l]`` ([H, H], None for l = 0).
    ``self_rows0`` [B, H]: layer 1 takes an explicit self term alpha[G+1] self_rows0 / (deg + 1) instead of the self-loop
    from the row (the kernel's head mode with ``self_rows``); its share stays in the logit, outside ``scores`` and ``base``
    (returned as ``self_share``).

    Returns a namespace: logits [B, C], target, logit, base, scores [nnz], v (list per layer), z (list), undecided (list of
    bool [B, H]: |z_i| <= (2 deg + 16) 2^-24 (sum |terms| + |b_i|), units whose ReLU an fp32 sum may flip), tol [nnz] (the
    per-entry bound, derived below), self_share [B], deg, rows."""
    m = m.tocsr()
    L = len(tables)
    G = m.shape[1]
    a = np.asarray(alpha, np.float64).ravel()
    Ts = [np.asarray(t, np.float64) for t in tables]
    bs = [np.asarray(b, np.float64) for b in biases]
    Ws = [None if w is None else np.asarray(w, np.float64) for w in self_weights]
    Wh, bh = np.asarray(w_head, np.float64), np.asarray(b_head, np.float64)
    us, zs, und = [], [], []
    h = None
    for l in range(L):
        explicit = l > 0 or self_rows0 is not None
        u, rows, deg = message_weights(m, a, explicit)
        M = sp.csr_matrix((u, m.indices, m.indptr), shape=m.shape)
        z = M @ Ts[l]
        mag = abs(M) @ np.abs(Ts[l])
        if explicit:
            sr = np.asarray(self_rows0, np.float64) if l == 0 else h @ Ws[l].T
            sr_mag = np.abs(sr) if l == 0 else np.abs(h) @ np.abs(Ws[l]).T
            z = z + a[G + 1] * sr / (deg + 1.0)[:, None]
            mag = mag + abs(a[G + 1]) * sr_mag / (deg + 1.0)[:, None]
        z = z + bs[l]
        mag = mag + np.abs(bs[l])
        us.append(u); zs.append(z)
        und.append(np.abs(z) <= ((2 * deg + 16) * EPS)[:, None] * mag)
        h = np.maximum(z, 0.0)
    logits = h @ Wh.T + bh
    B = m.shape[0]
    t = logits.argmax(axis=1) if target is None else np.asarray(target).astype(np.int64)
    coef = (a[G + 1] / (deg + 1.0))[:, None]
    H = Ts[0].shape[1]
    v = (zs[L - 1] > 0) * Wh[t]
    vabs = np.abs(v)
    delta = und[L - 1] * np.abs(Wh[t])
    scores = np.zeros(m.nnz)
    tol = np.zeros(m.nnz)
    base = bh[t].copy()
    vs = [None] * L
    self_share = np.zeros(B)
    for l in range(L - 1, -1, -1):
        vs[l] = v
        Tg = Ts[l][m.indices]
        scores += us[l] * np.einsum("ij,ij->i", Tg, v[rows])
        base += v @ bs[l]
        c_l = (H + 2 * deg + 16) * (L - l)
        tol += np.abs(us[l]) * (c_l[rows] * EPS * np.einsum("ij,ij->i", np.abs(Tg), vabs[rows])
                                + np.einsum("ij,ij->i", np.abs(Tg), delta[rows]))
        if l == 0:
            if self_rows0 is not None:
                self_share = coef[:, 0] * np.einsum("ij,ij->i", np.asarray(self_rows0, np.float64), v)
            break
        on = zs[l - 1] > 0
        unmasked = coef * ((vabs + delta) @ np.abs(Ws[l]))
        v, vabs_next = on * coef * (v @ Ws[l]), on * np.abs(coef) * (vabs @ np.abs(Ws[l]))
        delta = np.where(und[l - 1], np.abs(unmasked), on * np.abs(coef) * (delta @ np.abs(Ws[l])))
        vabs = vabs_next
    return SimpleNamespace(logits=logits, target=t, logit=logits[np.arange(B), t], base=base, scores=scores, v=vs, z=zs,
                           undecided=und, tol=tol, self_share=self_share, deg=deg, rows=rows)


# Where ``attribution().tol`` comes from (derived, not tuned).  One layer: the kernel's score is an fp32 coefficient
# (a few roundings, each <= 2^-24 relative, and S summed over deg terms: <= deg 2^-24) times an fp32 dot of H products, so
#
#     |got - want| <= (H + 2 deg + 16) 2^-24 |u_j| sum_i |T[g,i] v_i|  +  |u_j| sum_{i in U(r)} |T[g,i] Wh[t,i]|
#
# where U(r) are the cell's undecided units: flipping such a ReLU adds or removes exactly the unit's |T[g,i] Wh[t,i]|.
# Below the last layer v_{l-1} is itself an fp32 product (a GEMM over H terms and two multiplies) of quantities carrying the
# error of the layer above, so layer l (1-based, of L) takes the factor (L - l + 1) and its |v| is replaced by the
# propagation of |v_L| through |W| (no cancellation assumed); an undecided unit of any layer contributes the same
# propagation of its unmasked direction.  For L = 1 this is the line above, term for term.


def completeness_bound(scores, base, rows, deg, H):
    """|sum_row(score) + base - logit| <= (deg + H + 16) 2^-24 (sum |score| + |base|) per cell."""
    mag = np.bincount(rows, weights=np.abs(scores), minlength=deg.shape[0]) + np.abs(base)
    return (deg + H + 16) * EPS * mag


def stable_topk(rowptr, col, scores, k):
    """Per row the k best (score descending, equal scores by the lower position): gene [B, k] (-1 fill), score [B, k] (0)."""
    B = len(rowptr) - 1
    gene = np.full((B, k), -1, np.int64)
    top = np.zeros((B, k), np.float32)
    for r in range(B):
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        order = np.argsort(-scores[b:e], kind="stable")[:k]
        gene[r, :len(order)] = col[b:e][order]
        top[r, :len(order)] = scores[b:e][order]
    return gene, top
