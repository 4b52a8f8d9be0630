"""fp64 reference of the aggregation operators' BACKWARD entries (K2, K3) and of the K1 forward, written from the
formulas in ``include/wgnn.h`` with numpy / scipy only.

TEST INFRASTRUCTURE ONLY (see ``oracle/wgnn_oracle.py``): nothing here imports ``scdeepsort_amd``.

Every function returns, next to its result, the per-element SUM OF THE ABSOLUTE VALUES OF ITS TERMS and the number
of terms.  They serve two checks:

* **dyadic lattice** (``lattice_case`` / ``lattice_budget``): when every operand is a small multiple of a power of
  two, every product and every partial sum is a multiple of a fixed unit; while ``sum|terms| / unit < 2**24`` each of
  them is exactly representable in fp32, so an fp32 kernel must reproduce the fp64 result BIT FOR BIT, whatever its
  order of summation and whether or not it contracts to FMA.  One dropped, doubled or mis-slotted edge of a
  3 000-edge row is then a failure instead of noise under a mean.
* **derived bound** (``float_bound``) for ordinary floats: ``|err| <= (n + K_ROUND) * 2**-24 * sum|terms|`` - the
  standard bound of an fp32 sum of n products in any order, K_ROUND = 8 for the multiplicative roundings per term.

Operand convention (``include/wgnn.h``): ``A`` is the destination-major operand as a scipy CSR [R, S] (row r lists the
in-edges of destination r), ``inv_deg`` [R] the per-destination factor, ``alpha`` the gene-indexed scale vector.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import scipy.sparse as sp

SRC_IS_GENE, DST_IS_GENE, NO_ALPHA = 0, 1, 2           # WGNN_SRC_IS_GENE / WGNN_DST_IS_GENE / WGNN_NO_ALPHA
K_ROUND = 8                                            # multiplicative roundings allowed per term (weight folds, scales)
EXACT_LIMIT = float(2 ** 24)                           # integers below this are exact in fp32

# lattice of the exact tests: edge weights, per-destination scales, alpha, and integer features / gradients
LATTICE_VAL = (0.5, 1.0, 1.5, 2.0)
LATTICE_SCALE = (0.5, 1.0)
LATTICE_ALPHA = (0.5, 1.0, 2.0)
U_VAL, U_SCALE, U_ALPHA = 0.5, 0.5, 0.5                # lattice units (features / gradients / prior contents: 1)


def _csr64(A) -> sp.csr_matrix:
    A = sp.csr_matrix(A).astype(np.float64)
    return A


def _abs(A: sp.csr_matrix) -> sp.csr_matrix:
    B = A.copy()
    B.data = np.abs(B.data)
    return B


def _f64(x) -> Optional[np.ndarray]:
    return None if x is None else np.asarray(x, dtype=np.float64)


def bwd_src(A, inv_deg, alpha, mode: int, g, h_src=None) -> dict:
    """K2 (``wgnn_agg_bwd_src``): gradient w.r.t. the source rows.

        SRC_IS_GENE: T[s] = sum_r A[r,s]*inv_deg[r]*g[r];  dh_src[s] = alpha[s]*T[s];  dalpha_src[s] = <h_src[s], T[s]>
        DST_IS_GENE: dh_src[s] = sum_r A[r,s]*alpha[r]*inv_deg[r]*g[r]
        NO_ALPHA   : dh_src[s] = sum_r A[r,s]*inv_deg[r]*g[r]

    Returns dh_src [S, D], dalpha_src [S] | None, T, their abs-sums (``abs_dh``, ``abs_dalpha``, ``abs_T``) and the number of
    edge terms per source row (``n_terms`` [S])."""
    A = _csr64(A)
    R, S = A.shape
    inv_deg, g, alpha, h_src = _f64(inv_deg), _f64(g), _f64(alpha), _f64(h_src)
    scale = inv_deg * alpha[:R] if mode == DST_IS_GENE else inv_deg
    G = scale[:, None] * g
    At = A.T.tocsr()
    T = At @ G
    abs_T = _abs(At) @ np.abs(G)
    res = dict(T=T, abs_T=abs_T, n_terms=np.diff(At.indptr).astype(np.int64), dalpha_src=None, abs_dalpha=None)
    if mode == SRC_IS_GENE:
        a = alpha[:S, None]
        res["dh_src"], res["abs_dh"] = a * T, np.abs(a) * abs_T
        if h_src is not None:
            res["dalpha_src"] = (h_src * T).sum(1)
            res["abs_dalpha"] = (np.abs(h_src) * abs_T).sum(1)
    else:
        res["dh_src"], res["abs_dh"] = T, abs_T
    return res


def bwd_alpha(A, inv_deg, g, h_src, h_self=None, row_ids=None, self_compact: bool = False) -> dict:
    """K3 (``wgnn_agg_bwd_alpha``): for each output slot i (row r = row_ids[i] or i)

        dalpha_row[i] = inv_deg[r] * < g[i], sum_j A[r,j]*h_src[j] >
        dself_row[i]  = inv_deg[r] * < g[i], h_self[i if self_compact else r] >

    Returns both (``dself_row`` None without ``h_self``), their abs-sums and ``n_terms`` (row lengths of the slots)."""
    A = _csr64(A)
    inv_deg, g, h_src, h_self = _f64(inv_deg), _f64(g), _f64(h_src), _f64(h_self)
    rows = np.arange(A.shape[0]) if row_ids is None else np.asarray(row_ids, dtype=np.int64)
    Ar = A[rows] if len(rows) else sp.csr_matrix((0, A.shape[1]), dtype=np.float64)
    Ssum = Ar @ h_src
    abs_S = _abs(Ar) @ np.abs(h_src)
    inv = inv_deg[rows]
    res = dict(dalpha_row=inv * (g * Ssum).sum(1), abs_dalpha_row=np.abs(inv) * (np.abs(g) * abs_S).sum(1),
               n_terms=np.diff(Ar.indptr).astype(np.int64), dself_row=None, abs_dself_row=None, abs_S=abs_S)
    if h_self is not None:
        hs = h_self if (self_compact or row_ids is None) else h_self[rows]
        res["dself_row"] = inv * (g * hs).sum(1)
        res["abs_dself_row"] = np.abs(inv) * (np.abs(g) * np.abs(hs)).sum(1)
    return res


def fwd(A, inv_deg, alpha, mode: int, self_idx: int, h_src, h_self=None, *, row_ids=None, self_compact: bool = False, bias=None,
        relu: bool = False, no_mean: bool = False, no_self: bool = False, out_scale_alpha: bool = False) -> dict:
    """K1 (``wgnn_agg_fwd`` / ``wgnn_agg_fwd_tiled``): for each output slot i (row r = row_ids[i] or i), in the header's order

        neigh[i] = sum_j A[r,j] * (alpha[j] if SRC_IS_GENE) * h_src[j]                  the kernels' ``neigh_sum`` (raw sum)
        pre[i]   = (alpha[r] if DST_IS_GENE) * neigh[i] + a_self * h_self[i if self_compact else r]
                   a_self = alpha[self_idx] (1 for NO_ALPHA); no self term with ``no_self`` (WGNN_FLAG_NO_SELF) or h_self None
        out[i]   = pre[i] * f[r]                f[r] = inv_deg[r]; 1 / (row length + 1) for ``inv_deg=None``; 1 with ``no_mean``
        out[i]  += bias ;  out[i] = max(out[i], 0) with ``relu`` ;  out[i] *= alpha[r] with ``out_scale_alpha`` (DST_IS_GENE only)

    ``abs_out`` follows every step (the bias adds ``|bias|``, the post-scale multiplies), ``n_terms`` is the row length of every
    slot, ``row_factor`` the f[r] used, ``pre_relu`` the rows before the ReLU and the post-scale."""
    A = _csr64(A)
    R, S = A.shape
    inv_deg, alpha, h_src, h_self, bias = _f64(inv_deg), _f64(alpha), _f64(h_src), _f64(h_self), _f64(bias)
    if out_scale_alpha and mode != DST_IS_GENE:
        raise ValueError("out_scale_alpha is defined for DST_IS_GENE only")
    rows = np.arange(R) if row_ids is None else np.asarray(row_ids, dtype=np.int64)
    Ar = A[rows] if len(rows) else sp.csr_matrix((0, S), dtype=np.float64)
    X = alpha[:S, None] * h_src if mode == SRC_IS_GENE else h_src
    neigh = Ar @ X
    abs_neigh = _abs(Ar) @ np.abs(X)
    a_row = alpha[rows, None] if mode == DST_IS_GENE else 1.0
    a_self = 1.0 if mode == NO_ALPHA else alpha[self_idx]
    pre, abs_pre = a_row * neigh, np.abs(a_row) * abs_neigh
    if h_self is not None and not no_self:
        hs = h_self if (self_compact or row_ids is None) else h_self[rows]
        pre, abs_pre = pre + a_self * hs, abs_pre + abs(a_self) * np.abs(hs)
    n_terms = np.diff(Ar.indptr).astype(np.int64)
    if no_mean:
        f = np.ones(len(rows))
    elif inv_deg is None:
        f = 1.0 / (n_terms + 1.0)
    else:
        f = inv_deg[rows]
    out, abs_out = pre * f[:, None], abs_pre * np.abs(f)[:, None]
    if bias is not None:
        out, abs_out = out + bias, abs_out + np.abs(bias)
    pre_relu = out
    if relu:
        out = np.maximum(out, 0.0)
    if out_scale_alpha:
        out, abs_out = out * a_row, abs_out * np.abs(a_row)
    return dict(neigh=neigh, abs_neigh=abs_neigh, out=out, abs_out=abs_out, n_terms=n_terms, row_factor=f, pre_relu=pre_relu)


# ------------------------------------------------------------------------------------------------
# dyadic lattice
# ------------------------------------------------------------------------------------------------
def lattice_case(expr, D: int, seed: int, ints: int = 2) -> dict:
    """Lattice operands on the sparsity pattern of ``expr`` (scipy [cells, genes]; ``conftest.small_case`` gives one with a hub
    gene, an empty cell and an unexpressed gene).  Both aggregation directions get their OWN weights (as in the package:
    per-destination normalisation makes them differ), in the CSR order of the direction (columns ascending):

        A_cg [C, G] cells<-genes, A_gc [G, C] genes<-cells : weights in LATTICE_VAL
        inv_cg [C], inv_gc [G]                             : per-destination scales in LATTICE_SCALE
        alpha [G + 2]                                      : LATTICE_ALPHA
        h_gene [G, D], h_cell [C, D], g_cell [C, D], g_gene [G, D], and prior contents for ``accumulate``
        (prior_dh_gene [G, D], prior_dh_cell [C, D], prior_dalpha [G + 2])  : integers in [-ints, ints]
    all float64 (every value is exact in fp32)."""
    rng = np.random.default_rng(seed)
    P = sp.csr_matrix(expr)
    P.sort_indices()
    C, G = P.shape
    A_cg = sp.csr_matrix((rng.choice(LATTICE_VAL, P.nnz), P.indices.copy(), P.indptr.copy()), shape=(C, G))
    Pt = P.T.tocsr()
    Pt.sort_indices()
    A_gc = sp.csr_matrix((rng.choice(LATTICE_VAL, Pt.nnz), Pt.indices.copy(), Pt.indptr.copy()), shape=(G, C))
    ri = lambda *s: rng.integers(-ints, ints + 1, s).astype(np.float64)
    return dict(C=C, G=G, D=D, A_cg=A_cg, A_gc=A_gc, inv_cg=rng.choice(LATTICE_SCALE, C), inv_gc=rng.choice(LATTICE_SCALE, G),
                alpha=rng.choice(LATTICE_ALPHA, G + 2), h_gene=ri(G, D), h_cell=ri(C, D), g_cell=ri(C, D), g_gene=ri(G, D),
                prior_dh_gene=ri(G, D), prior_dh_cell=ri(C, D), prior_dalpha=ri(G + 2))


def lattice_budget(abs_sum, unit: float) -> float:
    """The exactness condition of one output: ``max(sum|terms|) / unit`` must stay below 2**24 (then every partial sum, in any
    order, is a multiple of ``unit`` below 2**24 units: exact in fp32).  Asserts it and returns log2 of the ratio."""
    a = np.asarray(abs_sum, dtype=np.float64)
    ratio = float(a.max()) / unit if a.size else 0.0
    assert ratio < EXACT_LIMIT, f"lattice budget exceeded: sum|terms| / unit = 2^{np.log2(ratio):.2f} >= 2^24 - shrink the case"
    return float(np.log2(ratio)) if ratio > 0 else 0.0


def bwd_src_units(mode: int) -> dict:
    """Lattice units of K2's sums: T (edge sum), dh_src, dalpha_src."""
    u_T = U_VAL * U_SCALE * (U_ALPHA if mode == DST_IS_GENE else 1.0)
    return dict(T=u_T, dh=u_T * (U_ALPHA if mode == SRC_IS_GENE else 1.0), dalpha=u_T)


BWD_ALPHA_UNITS = dict(S=U_VAL, dalpha_row=U_VAL * U_SCALE, dself_row=U_SCALE)


def fwd_units(mode: int, out_scale_alpha: bool = False, max_deg: Optional[int] = None) -> dict:
    """Lattice units of K1's sums.  ``out``: edge sum x row scale and the self term, times the row factor - U_SCALE, or
    1 / (max_deg + 1) when the kernel derives the factor from the row length (``inv_deg=None`` on rows whose length + 1 is a
    power of two: every factor is a multiple of the smallest); the integer bias is a multiple of either; the post-scale by
    alpha[row] halves the unit."""
    u_n = U_VAL * (U_ALPHA if mode == SRC_IS_GENE else 1.0)
    u_pre = min(u_n * (U_ALPHA if mode == DST_IS_GENE else 1.0), U_ALPHA)
    u_out = u_pre * (U_SCALE if max_deg is None else 1.0 / (max_deg + 1))
    return dict(neigh=u_n, out=u_out * (U_ALPHA if out_scale_alpha else 1.0))


def check_bwd_src_budget(ref: dict, mode: int, prior_dh=None, prior_dalpha=None) -> dict:
    """``lattice_budget`` on every sum K2 forms; ``prior_*``: contents added under ``accumulate``."""
    u = bwd_src_units(mode)
    out = dict(T=lattice_budget(ref["abs_T"], u["T"]),
               dh=lattice_budget(ref["abs_dh"] + (0 if prior_dh is None else np.abs(prior_dh)), u["dh"]))
    if ref["abs_dalpha"] is not None:
        out["dalpha"] = lattice_budget(ref["abs_dalpha"] + (0 if prior_dalpha is None else np.abs(prior_dalpha)), u["dalpha"])
    return out


def check_bwd_alpha_budget(ref: dict) -> dict:
    u = BWD_ALPHA_UNITS
    out = dict(S=lattice_budget(ref["abs_S"], u["S"]), dalpha_row=lattice_budget(ref["abs_dalpha_row"], u["dalpha_row"]))
    if ref["abs_dself_row"] is not None:
        out["dself_row"] = lattice_budget(ref["abs_dself_row"], u["dself_row"])
    return out


def check_fwd_budget(ref: dict, mode: int, out_scale_alpha: bool = False, max_deg: Optional[int] = None) -> dict:
    u = fwd_units(mode, out_scale_alpha, max_deg)
    return dict(neigh=lattice_budget(ref["abs_neigh"], u["neigh"]), out=lattice_budget(ref["abs_out"], u["out"]))


# ------------------------------------------------------------------------------------------------
# derived bound for ordinary floats
# ------------------------------------------------------------------------------------------------
def float_bound(abs_sum, n_terms) -> np.ndarray:
    """``(n + K_ROUND) * 2**-24 * sum|terms|`` per element; ``n_terms`` broadcasts against ``abs_sum`` (pass a column for
    per-row counts of a matrix)."""
    return (np.asarray(n_terms, dtype=np.float64) + K_ROUND) * 2.0 ** -24 * np.asarray(abs_sum, dtype=np.float64)


def worst_ratio(got, want, bound) -> float:
    """max |got - want| / bound over the elements (0/0 counts as 0; a non-zero error on a zero bound is inf)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


# ------------------------------------------------------------------------------------------------
# fp32 emulation in a random order (CPU tests: shows the two demands above are fair)
# ------------------------------------------------------------------------------------------------
def spmm_fp32_random_order(A, X, rng) -> np.ndarray:
    """``A @ X`` accumulated in fp32, the entries of every row taken in a random order (scipy's CSR product adds a row's
    entries one after the other in storage order, in the operands' dtype)."""
    A = sp.csr_matrix(A)
    row = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    order = np.lexsort((rng.random(A.nnz), row))
    B = sp.csr_matrix((A.data[order].astype(np.float32), A.indices[order], A.indptr), shape=A.shape)
    B.has_sorted_indices = False
    out = B @ np.ascontiguousarray(X, dtype=np.float32)
    assert out.dtype == np.float32
    return out


def dot_fp32_random_order(X, Y, rng) -> np.ndarray:
    """Row-wise ``<X[i], Y[i]>`` accumulated in fp32 over a random permutation of the columns."""
    X = np.asarray(X, dtype=np.float32); Y = np.asarray(Y, dtype=np.float32)
    acc = np.zeros(X.shape[0], dtype=np.float32)
    for c in rng.permutation(X.shape[1]):
        acc = acc + X[:, c] * Y[:, c]
    return acc
