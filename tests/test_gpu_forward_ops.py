"""The forward aggregation entries - ``wgnn_agg_fwd`` (K1, row-wave ``agg_main`` + ``agg_finalize``), ``wgnn_agg_fwd_tiled`` (K1t:
``agg_tiled_flat4``, the generic ``agg_tiled``, the tall tile, their own two-rows-per-trip epilogue, the ``row_ids`` branch and
``agg_finalize``) and the composed ``wgnn_agg_linear_relu_fwd`` - against the fp64 reference ``oracle.agg_backward.fwd``, with the
harness of ``tests/test_gpu_backward_ops.py`` (its patterns, lattice graphs, tile plans, guards and comparisons are imported).

Two groups, as there:

* **exact** - operands on the dyadic lattice; ``out`` and ``neigh_sum`` must equal the fp64 reference BIT FOR BIT (``torch.equal``;
  an fp16 output equals the reference rounded once to fp16), every case runs twice (determinism).  That the demand is fair for every
  tuple of the tables below (``sum|terms| / unit < 2**24``, an fp32 evaluation in random order gives the same bits, no option passes
  by vacuity, every axis meets every mode) is checked without a GPU in ``tests/test_agg_forward_reference.py`` and asserted again
  here on the reference of each case (``build_case``).
* **float** - operands as the package builds them; tolerance per element ``float_bound(abs_out, n_terms + parts + 1)`` from the
  reference (an fp16 output adds ``2**-11 * |want| + 2**-25``), no measured constant; every case prints ``RATIO ... err/bound``.

Outputs are inner views of SENTINEL-filled tensors (guard rows, and guard columns where ``ld > D``) that hold FILL before the call:
an element the kernel skipped fails the comparison, an element it wrote outside fails the guard check.  The entries are bound
through ``_lib.call`` wherever ``ops`` cannot reach the option (output views, K1t ``row_ids``, ``ld_self > D`` next to a flag,
``inv_deg == NULL``, 64-bit row pointers); the seed, dtype, sensitivity, float and fuzz tests go through ``ops`` (the wrappers are
part of what is pinned).

Option -> test:

    bias, WGNN_FLAG_RELU, _NO_MEAN, _NO_SELF (h_self given AND the flag) ... test_k1_options_exact[*-b1/-relu1/-nomean1/-noself1-*],
                                                                             test_k1t_options_exact[same ids]
    WGNN_FLAG_OUT_SCALE_ALPHA (genes) ...................................... test_k1_options_exact[*-osa1-*], test_k1t_options_exact[*-osa1-*]
    WGNN_FLAG_SRC_PRESCALED (cells, src_scratch NULL) ...................... test_k1t_options_exact[cells-*-pre1-*]
    WGNN_NO_ALPHA forward .................................................. test_k1_options_exact[*-plain-*], test_k1t_options_exact[*-plain-*]
    row_ids unordered / repeated / empty, WGNN_FLAG_SELF_COMPACT (K1) ...... test_k1_seeds_exact[*-perm/-compact/-empty-*]
    row_ids + WGNN_FLAG_SELF_COMPACT on K1t (C ABI only) ................... test_k1t_row_ids_through_the_abi
    inv_deg == NULL, int32 / int64 row pointers (WGNN_FLAG_ROWPTR_I64) ..... test_inv_deg_null_exact
    fp16 in / fp32 out, fp16 in / fp16 out, every dispatch_width branch .... test_k1_dtypes_exact
    all six dispatch_width branches x three modes (fp32) ................... test_k1_options_exact (D = 4 .. 1024)
    ld_src, ld_self, ld_out > D (K1); ld_self, ld_out > D (K1t) ............ test_k1_options_exact[*-ld1-*], test_k1t_options_exact[*-ld1-*]
    neigh_sum given / NULL, guards around out and neigh_sum ................ every exact test ([*-ns0/-ns1-*])
    agg_tiled_flat4 reported at D = 256, generic agg_tiled (bit 19) ........ test_flat_kernel_is_reported, test_k1t_options_exact[*-generic1]
    tile epilogue (pslot < 0) AND agg_finalize (split rows) per option ..... test_k1t_options_exact (asserted from the plans' items)
    tall tile (8 x 49) ..................................................... test_k1t_options_exact[*-tall1-*]
    one row, n_out == 0, a graph without a single edge ..................... test_edge_shapes_exact
    wgnn_agg_linear_relu_fwd (row_ids, lin_flags, ld_out > H) .............. test_composed_entry_exact
    one-edge sensitivity at hub degree, K1 and K1t under bias+ReLU+post-scale test_one_hub_edge_is_seen_forward
    ordinary floats, option stacks, fp16, seeds ............................ test_forward_options_float_bound, test_forward_fuzz_against_fp64

Not covered here: ``ld_src > D`` on K1t (the entry has no such argument: its source table is contiguous by contract); fp16 on K1t
(f32 only by contract); K1t ``row_ids`` with ``inv_deg == NULL`` (one combination of two options that are each pinned above).
The K1t ``row_ids`` test builds its tile plan for the gathered rows (slot i of the plan aggregates CSR row ``row_ids[i]``), so the
seed list itself - unordered, repeated, with the hub and the empty row - is what runs, not an identity list.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import test_gpu_backward_ops as GB
from oracle import agg_backward as AB
from oracle import dense_half as DH
from scdeepsort_amd import _lib
from scdeepsort_amd.graph import _ptr, _stream
from test_gpu_backward_ops import assert_exact, guarded, guards_intact, lattice_graph, pattern, record_ratio, tile_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, FILL = GB.SENTINEL, -777.0
MODE, MODES = GB.MODE, ("cells", "genes", "plain")
ROWWAVE_D, TILED_D, GEOMS, BLOCK_ROWS, TALL_D = GB.ROWWAVE_D, GB.TILED_D, GB.GEOMS, GB.BLOCK_ROWS, GB.TALL_D
SEED_D = (24, 64, 200, 256, 400)
DTYPE_D = (8, 64, 100, 256, 400, 1024)                 # one width per dispatch_width branch (q <= 8, 16, 32, 64, 128, 256)
GENERIC_KERNEL = 1 << 19                               # wgnn_tiled.hip use_flat(): force agg_tiled instead of agg_tiled_flat4
F16_MAX = 65504.0


# ---- the case sets (plain data: tests/test_agg_forward_reference.py checks every tuple on the CPU) --------------------------------
def _graph_for(D, i):
    return GB._graph_for(D, i)


# K1 options: two sweeps over (width, mode); the other axes rotate so that each value of each axis meets each mode:
#   (graph, mode, D, chunk, bias, relu, no_mean, no_self, out_scale_alpha, ld, neigh_sum)
K1_OPTION_CASES = [(_graph_for(D, di + mi + s), m, D, (64, 4096)[(di + mi + s) % 2], (di // 2 + mi + s) % 2 == 0, (di + 2 * mi + s) % 3 == 0,
                    (di // 3 + mi + s) % 2 == 1, (di + mi + 2 * s) % 4 == 1, m == "genes" and (di + s) % 2 == 0,
                    (di // 2 + 2 * mi + s) % 3 == 0, (di + mi + s) % 3 != 2)
                   for s in (0, 1) for di, D in enumerate(ROWWAVE_D) for mi, m in enumerate(MODES)]
# K1 seeds: (graph, mode, D, chunk, kind, bias, relu)   kind: "perm" | "compact" | "empty" (GB.k3_ids' lists + the hub and empty row)
K1_SEED_CASES = [(_graph_for(D, di + mi + s), m, D, (64, 4096)[(di + mi + s) % 2], ("perm", "compact", "empty")[(di + mi + 2 * s) % 3],
                  (di + s) % 2 == 0, (di // 2 + mi + s) % 2 == 0)
                 for s in (0, 1) for di, D in enumerate(SEED_D) for mi, m in enumerate(MODES)]
# K1 dtypes: (graph, mode, D, chunk, out16, bias, relu, osa)
K1_DTYPE_CASES = [(_graph_for(D, di + o), MODES[(di + o) % 3], D, (64, 4096)[(di + o) % 2], bool(o), (di + o) % 2 == 0, di % 3 == 0,
                   MODES[(di + o) % 3] == "genes" and di % 2 == 0)
                  for o in (0, 1) for di, D in enumerate(DTYPE_D)]
K1_DTYPE_CASES += [("hub", "genes", 256, 64, True, True, True, True), ("mid", "cells", 200, 4096, True, True, False, False),
                   ("small", "plain", 24, 64, False, False, True, False), ("mid", "genes", 128, 4096, False, True, True, True)]
# K1t options: two sweeps over (width, mode) + the tall tile + one sweep of the generic kernel at D = 256:
#   (graph, mode, D, geom, block_rows, loaders, tall, bias, relu, no_mean, no_self, osa, src_scaled, ld, neigh_sum, generic)
K1T_OPTION_CASES = [("hub" if GEOMS[(di + mi + s) % 5] == "heuristic" else ("small", "mid")[(di + s) % 2], m, D, GEOMS[(di + mi + s) % 5],
                     BLOCK_ROWS[(di + 2 * mi + s) % 4], (di + mi + s) % 2, False, (di // 2 + mi + s) % 2 == 0, (di + 2 * mi + s) % 3 == 0,
                     (di // 3 + mi + s) % 2 == 1, (di + mi + 2 * s) % 4 == 1, m == "genes" and (di + s) % 2 == 0,
                     m == "cells" and (di + s) % 2 == 1, (di // 2 + 2 * mi + s) % 3 == 0, (di + mi + s) % 3 != 2, False)
                    for s in (0, 1) for di, D in enumerate(TILED_D) for mi, m in enumerate(MODES)]
K1T_OPTION_CASES += [(("hub", "mid", "small")[(di + mi) % 3], m, D, ("heuristic", (2, 1), (3, 2))[(di + mi) % 3], BLOCK_ROWS[(di + mi + 1) % 4],
                      0, True, (di + mi) % 2 == 0, (di + mi) % 3 == 0, (di + mi) % 2 == 1, (di + 2 * mi) % 4 == 1, m == "genes" and di != 1,
                      m == "cells" and di != 1, (di + mi) % 3 == 1, (di + mi) % 3 != 2, False)
                     for di, D in enumerate(TALL_D) for mi, m in enumerate(MODES)]
K1T_OPTION_CASES += [(("mid", "small", "hub")[i % 3], m, 256, GEOMS[(i + mi) % 5],
                      BLOCK_ROWS[(i + mi) % 4], (i + mi) % 2, False, i % 2 == 0, (i + mi) % 2 == 0, i == 1, i == 2, m == "genes" and i != 2,
                      m == "cells" and i != 0, i == 0, i != 1, True)
                     for i in range(3) for mi, m in enumerate(MODES)]
# K1t through the C ABI: (graph, mode, D, kind, geom, bias, relu, ld)   row_ids over a plan built for the gathered rows
K1T_ABI_CASES = [(("mid", "small", "hub")[(i + mi) % 3], m, (64, 200, 256)[(i + mi) % 3], ("perm", "compact")[(i + mi) % 2],
                  ((None, 1), (2, 3), "heuristic")[i], (i + mi) % 2 == 0, i % 2 == 0, (i + mi) % 2 == 1)
                 for i in range(3) for mi, m in enumerate(MODES)]
# inv_deg == NULL on the power-of-two pattern: (route, mode, D, i64)   route: chunk of K1 | K1t geometry
NULL_ROUTES = (64, 4096, (None, 1), (1, 2))
NULL_CASES = [(r, m, (24, 200, 256)[(ri + mi + i64) % 3], bool(i64)) for ri, r in enumerate(NULL_ROUTES) for mi, m in enumerate(MODES)
              for i64 in (0, 1)]
# edge shapes: (shape, route, mode)
EDGE_CASES = [(sh, r, MODES[(i + j) % 3]) for i, sh in enumerate(("one_row", "no_rows", "no_edges")) for j, r in enumerate(("rowwave", "tiled"))]
EDGE_CASES += [("no_edges", "rowwave", "genes"), ("one_row", "tiled", "cells")]
# composed entry: (graph, mode, D, H, kind, lin_relu, ld_out)
COMPOSED_CASES = [(("mid", "small")[(di + hi) % 2], MODES[(di + hi + k) % 3], D, H, (None, "perm")[k], (di + hi + k) % 2 == 0, (di + k) % 2 == 0)
                  for di, D in enumerate((64, 200, 256)) for hi, H in enumerate((16, 200)) for k in (0, 1)]
FLOAT_D = GB.FLOAT_D
FLOAT_STACKS = (dict(), dict(bias=True, relu=True), dict(no_mean=True, bias=True), dict(no_self=True, relu=True),
                dict(bias=True, relu=True, osa=True), dict(bias=True, kind="perm"), dict(relu=True, kind="compact"),
                dict(bias=True, f16="in"), dict(bias=True, relu=True, f16="out"))


def _b(v):
    return int(bool(v))


def k1_id(c):
    return (f"{c[0]}-{c[1]}-D{c[2]}-chunk{c[3]}-b{_b(c[4])}-relu{_b(c[5])}-nomean{_b(c[6])}-noself{_b(c[7])}-osa{_b(c[8])}-ld{_b(c[9])}"
            f"-ns{_b(c[10])}")


def seed_id(c):
    return f"{c[0]}-{c[1]}-D{c[2]}-chunk{c[3]}-{c[4]}-b{_b(c[5])}-relu{_b(c[6])}"


def dtype_id(c):
    return f"{c[0]}-{c[1]}-D{c[2]}-chunk{c[3]}-out{'16' if c[4] else '32'}-b{_b(c[5])}-relu{_b(c[6])}-osa{_b(c[7])}"


def k1t_id(c):
    return (f"{c[0]}-{c[1]}-D{c[2]}-g{GB._cid((c[3],))}-kb{c[4]}-L{c[5]}-tall{_b(c[6])}-b{_b(c[7])}-relu{_b(c[8])}-nomean{_b(c[9])}"
            f"-noself{_b(c[10])}-osa{_b(c[11])}-pre{_b(c[12])}-ld{_b(c[13])}-ns{_b(c[14])}-generic{_b(c[15])}")


# ---- the reference of a case (no GPU: the CPU file calls these too) ---------------------------------------------------------------
@functools.lru_cache(maxsize=6)
def lattice(name, D):
    """ONE lattice draw per (pattern, width), shared by every case on it."""
    return AB.lattice_case(pattern(name), D, GB.case_seed("fwd", name, D))


@functools.lru_cache(maxsize=None)
def pow2_pattern():
    """200 rows x 600 genes; row lengths cycle through 2**k - 1, k = 0..9: 1 / (deg + 1) is a power of two in every row."""
    rng = np.random.default_rng(7)
    indptr, idx = [0], []
    for r in range(200):
        idx.append(np.sort(rng.choice(600, 2 ** (r % 10) - 1, replace=False)))
        indptr.append(indptr[-1] + len(idx[-1]))
    idx = np.concatenate(idx)
    return sp.csr_matrix((np.ones(len(idx), dtype=np.float32), idx, np.asarray(indptr)), shape=(200, 600))


@functools.lru_cache(maxsize=None)
def edge_pattern(shape, mode):
    """[cells, genes] patterns of the edge shapes: no edge at all, or ONE destination row in the direction ``mode`` runs on."""
    if shape == "no_edges":
        return sp.csr_matrix((40, 32), dtype=np.float32)
    row = np.zeros((1, 50), dtype=np.float32)                      # "one_row" (and the operands of "no_rows")
    row[0, np.random.default_rng(3).choice(50, 21, replace=False)] = 1.0
    return sp.csr_matrix(row.T if mode == "genes" else row)        # genes: one gene row over 50 cells


def seed_rows(A, kind, seed):
    """``GB.k3_ids``-style seed list on the rows of ``A``: unordered, with repeats; the longest row twice, an empty row, the last."""
    if kind is None:
        return None
    if kind == "empty":
        return np.zeros(0, dtype=np.int64)
    n = A.shape[0]
    lens = np.diff(A.indptr)
    ids = np.random.default_rng(seed).integers(0, n, 2 * n // 3 + 1)
    ids[:4] = (int(lens.argmax()), int(lens.argmin()), int(lens.argmax()), n - 1)
    return ids


def build_case(L, mode, D, *, side=None, bias=False, relu=False, no_mean=False, no_self=False, osa=False, kind=None, inv_null=False,
               seed=0, vacuity=True, floats=None):
    """Operands, options and the fp64 reference of one forward call on the lattice draw ``L``; asserts the lattice budget and that
    no option passes by vacuity.  cells: SRC_IS_GENE on cells<-genes; genes: DST_IS_GENE on genes<-cells; plain: NO_ALPHA on
    genes<-cells (the hub ROW) unless ``side`` says "cg".  ``floats`` (np.float32 | np.float16; the float group): ``L`` holds
    ordinary floats - bias and a compact self table are drawn standard normal in that type, no lattice demand is made."""
    side = side or ("cg" if mode == "cells" else "gc")
    G = L["G"]
    A, inv = L["A_" + side], L["inv_" + side]
    h_src, h_self = (L["h_gene"], L["h_cell"]) if side == "cg" else (L["h_cell"], L["h_gene"])
    rng = np.random.default_rng(GB.case_seed("extras", mode, D, seed))
    ids = seed_rows(A, kind, GB.case_seed("ids", mode, D, seed))
    n_out = A.shape[0] if ids is None else len(ids)
    compact = kind == "compact"
    if compact:
        h_self = (rng.integers(-2, 3, (n_out, D)) if floats is None else rng.standard_normal((n_out, D)).astype(floats)).astype(np.float64)
    bias_v = None
    if bias:
        bias_v = (rng.integers(-2, 3, D) if floats is None else rng.standard_normal(D).astype(np.float32)).astype(np.float64)
        bias_v[0] = 2.0                                            # never all zero
    c = SimpleNamespace(L=L, mode=mode, amode=MODE[mode], sidx=(G + 1 if side == "cg" else G) if mode != "plain" else 0, side=side, D=D,
                        A=A, inv=inv, h_src=h_src, h_self=h_self, ids=ids, n_out=n_out, compact=compact, bias=bias_v, relu=relu,
                        no_mean=no_mean, no_self=no_self, osa=osa, inv_null=inv_null)
    c.ref = AB.fwd(A, None if inv_null else inv, L["alpha"], c.amode, c.sidx, h_src, h_self, row_ids=ids, self_compact=compact,
                   bias=bias_v, relu=relu, no_mean=no_mean, no_self=no_self, out_scale_alpha=osa)
    max_deg = int(np.diff(A.indptr).max()) if inv_null and not no_mean and A.shape[0] else None
    if floats is not None:
        return c
    c.budget = AB.check_fwd_budget(c.ref, c.amode, osa, max_deg)
    if vacuity and n_out:
        rows = np.arange(A.shape[0]) if ids is None else ids
        if relu:
            assert (c.ref["pre_relu"] < 0).any() and (c.ref["pre_relu"] > 0).any(), "ReLU clips nothing or everything"
        if bias:
            assert bias_v.any()
        if osa:
            assert (L["alpha"][rows] != 1).any(), "alpha[row] == 1 on every row"
        if no_mean:
            assert (inv[rows] != 1).any(), "the skipped row factor is 1 on every row"
        if no_self:
            assert np.abs(h_self).max() > 0
        if kind in ("perm", "compact"):
            lens = np.diff(A.indptr)
            assert lens.argmax() in ids and lens.min() == 0 and lens.argmin() in ids and len(set(ids.tolist())) < len(ids)
    return c


def k1_case(case):
    name, mode, D, chunk, bias, relu, no_mean, no_self, osa, ld, nsum = case
    return build_case(lattice(name, D), mode, D, bias=bias, relu=relu, no_mean=no_mean, no_self=no_self, osa=osa, seed=chunk)


def seed_case(case):
    name, mode, D, chunk, kind, bias, relu = case
    return build_case(lattice(name, D), mode, D, bias=bias, relu=relu, kind=kind, seed=chunk)


def dtype_case(case):
    name, mode, D, chunk, out16, bias, relu, osa = case
    return build_case(lattice(name, D), mode, D, bias=bias, relu=relu, osa=osa, seed=chunk)


def k1t_case(case):
    name, mode, D, geom, kb, loaders, tall, bias, relu, no_mean, no_self, osa, pre, ld, nsum, generic = case
    return build_case(lattice(name, D), mode, D, bias=bias, relu=relu, no_mean=no_mean, no_self=no_self, osa=osa, seed=loaders)


def abi_case(case):
    name, mode, D, kind, geom, bias, relu, ld = case
    return build_case(lattice(name, D), mode, D, bias=bias, relu=relu, kind=kind, seed=7)


def null_lattice(D):
    return AB.lattice_case(pow2_pattern(), D, GB.case_seed("pow2", D))


def null_case(case):
    """cells / plain run on the power-of-two rows (exact against fp64); genes on the transposed pattern (NULL against a given
    numpy 1 / (deg + 1), bit for bit: the reference there is the float group's business)."""
    route, mode, D, i64 = case
    L = null_lattice(D)
    if mode == "genes":
        return build_case(L, mode, D, bias=True, relu=i64, vacuity=False)
    return build_case(L, mode, D, side="cg", bias=not i64, relu=i64, inv_null=True, seed=int(i64))


def edge_case(case):
    shape, route, mode = case
    L = AB.lattice_case(edge_pattern(shape, mode), 24, GB.case_seed("edge", shape))
    return build_case(L, mode, 24, side="cg" if mode != "genes" else "gc", bias=True, relu=shape == "no_edges", osa=mode == "genes",
                      kind="empty" if shape == "no_rows" else None, vacuity=False)


def composed_case(case):
    """fwd, then the linear reference of ``oracle/dense_half.py`` on its exact fp32 result; W and bias are lattice integers."""
    name, mode, D, H, kind, lin_relu, ld = case
    c = build_case(lattice(name, D), mode, D, kind=kind, no_mean=(D + H) % 3 == 0, seed=H)
    rng = np.random.default_rng(GB.case_seed("composed", *case))
    c.W, c.lin_bias = rng.integers(-2, 3, (H, D)).astype(np.float64), rng.integers(-2, 3, H).astype(np.float64)
    c.lin = DH.linear_fwd(c.ref["out"], c.W, c.lin_bias, lin_relu)
    c.lin_budget = AB.lattice_budget(c.lin["abs_sum"], AB.fwd_units(c.amode)["out"])     # |x| |w| + |bias| in units of the agg output
    return c


# ---- device side ------------------------------------------------------------------------------------------------------------------
def dev(x, dtype=torch.float32):
    return GB.dev(x, dtype)


def fresh(n, D, pad=0):
    """A guarded f32 output that holds FILL (what no result here equals)."""
    return guarded(np.full((n, D), FILL), pad)


def agg_csr(A, inv, chunk=None):
    """An ``AggCsr`` straight from a scipy operand (no normalisation, no transpose: the gathered rows of a seed list, the edge
    shapes)."""
    from scdeepsort_amd import graph as GR
    A = sp.csr_matrix(A)
    host = A.indptr.astype(np.int32)
    return GR.AggCsr(dev(host, torch.int32), dev(A.indices, torch.int32), dev(A.data), dev(inv), A.shape[0], A.shape[1],
                     GR.build_plan(host, chunk, device=DEV), host)


@functools.lru_cache(maxsize=3)
def graph(name, D, chunk=None):
    return lattice_graph(name, lattice(name, D), chunk)


def prepare(c, *, ld=False, nsum=True, in16=False, out16=False, wide_src=True):
    """Device tensors of a case: inputs (inside SENTINEL columns when ``ld``), guarded FILL-holding outputs, the flag word."""
    D, n = c.D, c.n_out
    ft = torch.float16 if in16 else torch.float32
    put = (lambda x: GB.strided(x)) if (ld and not in16) else (lambda x: dev(x, ft))
    T = SimpleNamespace(D=D, n_out=n, amode=c.amode, sidx=c.sidx, guards=[], in16=in16, out16=out16)
    T.alpha = None if c.mode == "plain" else dev(c.L["alpha"])
    T.h_src = put(c.h_src) if wide_src else dev(c.h_src, ft)
    T.h_self = put(c.h_self)
    T.ids = None if c.ids is None else dev(c.ids, torch.int32)
    T.inv = None if c.inv_null else dev(c.inv)
    T.bias = None if c.bias is None else dev(c.bias)
    if out16:
        whole = torch.full((n + 2, D), 1024.0, dtype=torch.float16, device=DEV)
        T.out = whole[1:n + 1]
        T.out.fill_(FILL)
        T.out16_whole = whole
    else:
        whole, T.out = fresh(n, D, 4 if ld else 0)
        T.guards.append((whole, T.out))
    T.nsum = None
    if nsum:
        whole, T.nsum = fresh(n, D)
        T.guards.append((whole, T.nsum))
    T.flags = ((_lib.FLAG_RELU if c.relu else 0) | (_lib.FLAG_NO_MEAN if c.no_mean else 0) | (_lib.FLAG_NO_SELF if c.no_self else 0)
               | (_lib.FLAG_SELF_COMPACT if c.compact else 0) | (_lib.FLAG_OUT_SCALE_ALPHA if c.osa else 0))
    return T


def launch_k1(csr, plan, T, rowptr=None, flags=0):
    d = torch.device(DEV)
    part = torch.empty(max(1, plan.n_partials) * T.D, device=DEV)
    rc = _lib.call(d, "wgnn_agg_fwd", _ptr(csr.rowptr if rowptr is None else rowptr), _ptr(csr.col), _ptr(csr.val), _ptr(T.alpha),
                   T.amode, T.sidx, _ptr(T.h_src), T.h_src.stride(0), _ptr(T.h_self), T.h_self.stride(0), _ptr(T.ids), _ptr(T.inv),
                   _ptr(T.bias), _ptr(T.out), T.out.stride(0), _ptr(T.nsum), T.n_out, T.D, _lib.F16 if T.in16 else _lib.F32,
                   _lib.F16 if T.out16 else _lib.F32, T.flags | flags, _ptr(plan.items), plan.n_items,
                   _ptr(plan.long_rows) if plan.n_long else None, plan.n_long, _ptr(part), plan.n_partials, _stream(d))
    _lib.check(rc, "wgnn_agg_fwd")


def launch_k1t(csr, tp, T, c, rowptr=None, flags=0, prescaled=False):
    """``tp`` None: no plan at all (n_tiles == 0)."""
    from scdeepsort_amd import ops
    d = torch.device(DEV)
    h_src, scratch = T.h_src, None
    if c.mode == "cells":
        if prescaled:
            h_src, flags = dev(c.L["alpha"][:c.h_src.shape[0], None] * c.h_src), flags | _lib.FLAG_SRC_PRESCALED
        else:
            scratch = torch.full_like(h_src, SENTINEL)
    if tp is None:
        plan_args = (None, None, 0, 64, None, None, 0, None, 0, None, 0)
    else:
        n_long = tp.long_rows.shape[0]
        part = torch.empty(max(1, tp.n_partials) * T.D, device=DEV)
        plan_args = (_ptr(tp.entries), _ptr(tp.seg_ptr), tp.nblk_max, tp.block_rows_arg, _ptr(tp.items), _ptr(tp.hdr), tp.n_tiles,
                     _ptr(tp.long_rows) if n_long else None, n_long, _ptr(part), tp.n_partials)
    rc = _lib.call(d, "wgnn_agg_fwd_tiled", _ptr(csr.rowptr if rowptr is None else rowptr), _ptr(T.alpha), T.amode, T.sidx, _ptr(h_src),
                   h_src.shape[0], _ptr(scratch), _ptr(T.h_self), T.h_self.stride(0), _ptr(T.ids), _ptr(T.inv), _ptr(T.bias),
                   _ptr(T.out), T.out.stride(0), _ptr(T.nsum), T.n_out, T.D, T.flags | flags | ops.DEBUG_FLAGS, *plan_args, _stream(d))
    _lib.check(rc, "wgnn_agg_fwd_tiled")


def want16(ref_out):
    """The fp64 reference rounded ONCE to fp16, round-to-nearest-even (numpy's conversion)."""
    assert np.abs(ref_out).max(initial=0.0) < F16_MAX
    return torch.from_numpy(np.asarray(ref_out, dtype=np.float64).astype(np.float16))


def check(T, c, what=""):
    torch.cuda.synchronize()
    for whole, view in T.guards:
        assert guards_intact(whole, view), f"{what}: a guard row / column was written"
    if T.out16:
        n = T.n_out
        assert bool((T.out16_whole[0] == 1024.0).all()) and bool((T.out16_whole[n + 1] == 1024.0).all()), f"{what}: a guard row was written"
        got, want = T.out.cpu(), want16(c.ref["out"])
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            raise AssertionError(f"{what} out (fp16): {bad.shape[0]} of {got.numel()} elements differ from the once-rounded fp64 "
                                 f"reference, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()!r}, want "
                                 f"{want[tuple(bad[0])].item()!r}")
    else:
        assert_exact(T.out, c.ref["out"], f"{what} out")
    if T.nsum is not None:
        assert_exact(T.nsum, c.ref["neigh"], f"{what} neigh_sum")
    return T.out.clone(), None if T.nsum is None else T.nsum.clone()


def twice(run, c, what=""):
    """Run, compare with the reference, run again into fresh outputs: same bits."""
    first = check(run(), c, what)
    second = check(run(), c, what + " (second run)")
    assert torch.equal(first[0], second[0]) and (first[1] is None or torch.equal(first[1], second[1]))


def csr_of(g, c):
    return g.cg if c.side == "cg" else g.gc


def plan_kinds(tp):
    """(some row is finished in the tile: pslot < 0, some row is split and finished by agg_finalize) from the plan's items."""
    it = tp.items.reshape(-1, 4).cpu().numpy()
    live = it[:, 0] >= 0
    return bool((live & (it[:, 3] < 0)).any()), bool((live & (it[:, 3] >= 0)).any())


def plans_with_both_kinds(csr, D, geom, kb, loaders, tall):
    """The case's own tile plan and - where that one has only in-tile rows (one column split, no heavy row) or only split rows
    (column splits) - a second plan of the other kind: every option meets the tile epilogue AND agg_finalize."""
    plans = [tile_plan(csr, D, geom, kb, loaders, tall)]
    in_tile, split = plan_kinds(plans[0])
    rt = None if geom == "heuristic" else geom[0]
    if not split:
        plans.append(tile_plan(csr, D, (rt, 2), kb, loaders, tall, strict=False))
    elif not in_tile:
        plans.append(tile_plan(csr, D, (rt, 1), kb, loaders, tall, strict=False))
    kinds = [plan_kinds(p) for p in plans]
    assert any(k[0] for k in kinds) and any(k[1] for k in kinds), "the case lacks an in-tile row or a split row"
    return plans


# ---- K1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K1_OPTION_CASES, ids=k1_id)
def test_k1_options_exact(case):
    """``wgnn_agg_fwd`` through the C ABI == fp64, bit for bit: every width branch x every mode, cut (agg_finalize) and uncut long
    rows, bias, ReLU, NO_MEAN, NO_SELF next to a non-NULL h_self, the post-scale, ld > D for src / self / out, neigh_sum or NULL."""
    name, mode, D, chunk, bias, relu, no_mean, no_self, osa, ld, nsum = case
    c = k1_case(case)
    csr = csr_of(graph(name, D, chunk), c)
    assert (csr.plan.n_long > 0) == (chunk == 64) and csr.plan.chunk == chunk

    def run():
        T = prepare(c, ld=ld, nsum=nsum)
        assert (T.out.stride(0) > D) == ld and (T.h_src.stride(0) > D) == ld and (T.h_self.stride(0) > D) == ld
        launch_k1(csr, csr.plan, T)
        return T
    twice(run, c, "K1")


@pytest.mark.parametrize("case", K1_SEED_CASES, ids=seed_id)
def test_k1_seeds_exact(case, monkeypatch):
    """``ops.agg_fwd`` with ``row_ids`` (unordered, repeated, with the longest and an empty row; empty list) and
    WGNN_FLAG_SELF_COMPACT over the device-built sub-plan, into a guarded ``out=`` view == fp64, bit for bit."""
    from scdeepsort_amd import ops
    name, mode, D, chunk, kind, bias, relu = case
    monkeypatch.setattr(ops, "TILED_MIN_WORK", None)
    c = seed_case(case)
    csr = csr_of(graph(name, D, chunk), c)

    def run():
        T = prepare(c, nsum=kind != "empty")
        out = ops.agg_fwd(csr, T.alpha, c.amode, c.sidx, T.h_src, T.h_self, bias=T.bias, relu=relu, row_ids=T.ids,
                          self_compact=c.compact, out=T.out, neigh_sum=T.nsum)
        assert out.data_ptr() == T.out.data_ptr() and tuple(out.shape) == (c.n_out, D)
        return T
    twice(run, c, "K1 seeds")
    if kind == "empty":
        assert ops.agg_fwd(csr, None if mode == "plain" else dev(c.L["alpha"]), c.amode, c.sidx, dev(c.h_src), dev(c.h_self),
                           row_ids=dev(c.ids, torch.int32)).shape == (0, D)


@pytest.mark.parametrize("case", K1_DTYPE_CASES, ids=dtype_id)
def test_k1_dtypes_exact(case, monkeypatch):
    """fp16 in / fp32 out and fp16 in / fp16 out at one width per ``dispatch_width`` branch: lattice integers are exact in fp16, so
    the fp32 output equals fp64 and the fp16 output equals fp64 rounded once (``st4(__half*)``: ``__floats2half2_rn``)."""
    from scdeepsort_amd import ops
    name, mode, D, chunk, out16, bias, relu, osa = case
    monkeypatch.setattr(ops, "TILED_MIN_WORK", None)
    c = dtype_case(case)
    csr = csr_of(graph(name, D, chunk), c)

    def run():
        T = prepare(c, in16=True, out16=out16)
        out = ops.agg_fwd(csr, T.alpha, c.amode, c.sidx, T.h_src, T.h_self, bias=T.bias, relu=relu, out=T.out, neigh_sum=T.nsum,
                          out_scale_alpha=osa)
        assert out.dtype == (torch.float16 if out16 else torch.float32)
        return T
    twice(run, c, "K1 fp16")


# ---- K1t ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K1T_OPTION_CASES, ids=k1t_id)
def test_k1t_options_exact(case, monkeypatch):
    """``wgnn_agg_fwd_tiled`` through the C ABI == fp64, bit for bit: the flat kernel at every width, the tall tile, the generic
    kernel (``ops.DEBUG_FLAGS = 1 << 19``) at D = 256; every option meets rows finished by the tile epilogue and rows finished by
    ``agg_finalize``."""
    from scdeepsort_amd import ops
    name, mode, D, geom, kb, loaders, tall, bias, relu, no_mean, no_self, osa, pre, ld, nsum, generic = case
    monkeypatch.setattr(ops, "DEBUG_FLAGS", GENERIC_KERNEL if generic else 0)
    c = k1t_case(case)
    csr = csr_of(graph(name, D), c)
    for tp in plans_with_both_kinds(csr, D, geom, kb, loaders, tall):
        def run():
            T = prepare(c, ld=ld, nsum=nsum, wide_src=False)
            launch_k1t(csr, tp, T, c, prescaled=pre)
            return T
        twice(run, c, f"K1t {tp.n_row_tiles}x{tp.n_col_splits}")


def test_flat_kernel_is_reported(monkeypatch):
    """D = 256 without a debug flag runs (and reports through ``ops.PROFILE``) ``agg_tiled_flat4``; the result is the exact one."""
    from scdeepsort_amd import ops
    prof = []
    monkeypatch.setattr(ops, "PROFILE", prof)
    monkeypatch.setattr(ops, "DEBUG_FLAGS", 0)
    c = build_case(lattice("mid", 256), "genes", 256, bias=True, relu=True, osa=True)
    csr = csr_of(graph("mid", 256), c)
    nsum = torch.full((c.n_out, 256), FILL, device=DEV)
    out = ops.agg_fwd_tiled(csr, tile_plan(csr, 256, "heuristic", "full", 1, False), dev(c.L["alpha"]), c.amode, c.sidx, dev(c.h_src),
                            dev(c.h_self), bias=dev(c.bias), relu=True, neigh_sum=nsum, out_scale_alpha=True)
    torch.cuda.synchronize()
    assert len(prof) == 1 and prof[0][0][-2:] == ("kernel", "agg_tiled_flat4")
    assert_exact(out, c.ref["out"], "out"); assert_exact(nsum, c.ref["neigh"], "neigh_sum")


@pytest.mark.parametrize("case", K1T_ABI_CASES, ids=GB._cid)
def test_k1t_row_ids_through_the_abi(case):
    """K1t's ``row_ids != NULL`` branch (reachable through the C ABI only): the tile plan is built for the GATHERED rows (slot i
    aggregates CSR row ``row_ids[i]``), the epilogue reads inv_deg / alpha / h_self at ``row_ids[i]`` (or h_self at i under
    WGNN_FLAG_SELF_COMPACT) from the full-graph tables; ld_self > D and ld_out > D behind guards."""
    name, mode, D, kind, geom, bias, relu, ld = case
    c = abi_case(case)
    sub = agg_csr(c.A[c.ids], np.ones(c.n_out))                    # its inv_deg is never read: the call gets the full graph's
    for tp in plans_with_both_kinds(sub, D, geom, "full", 0, False):
        def run():
            T = prepare(c, ld=ld, wide_src=False)
            launch_k1t(sub, tp, T, c)
            return T
        twice(run, c, f"K1t row_ids {tp.n_row_tiles}x{tp.n_col_splits}")


# ---- inv_deg == NULL ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NULL_CASES, ids=GB._cid)
def test_inv_deg_null_exact(case):
    """``inv_deg == NULL`` (the kernels derive 1 / (row length + 1) from int32 or int64 row pointers).  Rows of length 2**k - 1:
    exact against fp64.  Genes direction (arbitrary degrees): bit for bit what the same entry gives for
    ``float32(1) / float32(deg + 1)`` from numpy - the library is built without fast-math, its division is IEEE."""
    route, mode, D, i64 = case
    c = null_case(case)
    tiled = not isinstance(route, int)
    csr = agg_csr(c.A, c.inv, None if tiled else route)
    tp = tile_plan(csr, D, route, "full", 0, False) if tiled else None
    if route == 64 and mode != "genes":
        assert csr.plan.n_long > 0
    rowptr = csr.rowptr.to(torch.int64) if i64 else csr.rowptr
    flag = _lib.FLAG_ROWPTR_I64 if i64 else 0

    def run(inv):
        T = prepare(c, wide_src=False)
        T.inv = inv
        if tiled:
            launch_k1t(csr, tp, T, c, rowptr=rowptr, flags=flag)
        else:
            launch_k1(csr, csr.plan, T, rowptr=rowptr, flags=flag)
        return T
    if mode != "genes":
        assert c.inv_null and c.budget["out"] < 24
        twice(lambda: run(None), c, "inv_deg NULL")
    else:
        deg = np.diff(c.A.indptr)
        assert ((deg + 1) & deg).any(), "every degree + 1 is a power of two: the comparison would not see a rounding"
        given = np.float32(1) / (deg + 1).astype(np.float32)
        a, b = run(None), run(dev(given))
        torch.cuda.synchronize()
        assert all(guards_intact(w, v) for T in (a, b) for w, v in T.guards)
        assert not bool((a.out == FILL).any())
        assert torch.equal(a.out, b.out) and torch.equal(a.nsum, b.nsum)
        assert_exact(a.nsum, c.ref["neigh"], "neigh_sum")


# ---- edge shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EDGE_CASES, ids=GB._cid)
def test_edge_shapes_exact(case):
    """One row; ``n_out == 0`` (nothing is launched, nothing is written); a graph without a single edge (out = self term + bias).
    The operands are built directly (``agg_csr``), so the graph builder is not asked to accept an edgeless matrix."""
    shape, route, mode = case
    c = edge_case(case)
    csr = agg_csr(c.A, c.inv)
    if shape == "no_rows":
        assert c.n_out == 0
    if shape == "no_edges":
        assert csr.nnz == 0 and not c.ref["neigh"].any() and c.ref["out"].any()

    def run():
        T = prepare(c, ld=True, wide_src=route == "rowwave")
        if route == "rowwave":
            launch_k1(csr, csr.plan if c.ids is None else csr.subplan(T.ids)[1], T)
        else:
            launch_k1t(csr, None if shape == "no_rows" else tile_plan(csr, c.D, (None, 1), 16, 0, False), T, c)
        return T
    twice(run, c, shape)


# ---- composed entry -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", COMPOSED_CASES, ids=GB._cid)
def test_composed_entry_exact(case):
    """``wgnn_agg_linear_relu_fwd`` == ``fwd`` followed by ``oracle.dense_half.linear_fwd``, bit for bit (its neigh_scratch holds the
    exact aggregation, its product is an exact fp32 fmaf chain on lattice integers), with and without row_ids, ld_out > H."""
    name, mode, D, H, kind, lin_relu, ld = case
    c = composed_case(case)
    assert c.lin_budget < 24
    csr = csr_of(graph(name, D), c)
    ids, plan = (None, csr.plan) if c.ids is None else csr.subplan(dev(c.ids, torch.int32))
    d = torch.device(DEV)
    W, lb = dev(c.W), dev(c.lin_bias)

    def run():
        T = prepare(c, nsum=False)
        sw, scratch = fresh(c.n_out, D)
        ow, out = fresh(c.n_out, H, 4 if ld else 0)
        part = torch.empty(max(1, plan.n_partials) * D, device=DEV)
        rc = _lib.call(d, "wgnn_agg_linear_relu_fwd", _ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.val), _ptr(T.alpha), c.amode, c.sidx,
                       _ptr(T.h_src), D, _ptr(T.h_self), D, _ptr(ids), _ptr(T.inv), c.n_out, D, T.flags, _ptr(plan.items), plan.n_items,
                       _ptr(plan.long_rows) if plan.n_long else None, plan.n_long, _ptr(part), plan.n_partials, _ptr(scratch),
                       _ptr(W), D, _ptr(lb), H, _lib.FLAG_RELU if lin_relu else 0, _ptr(out), out.stride(0), _stream(d))
        _lib.check(rc, "wgnn_agg_linear_relu_fwd")
        torch.cuda.synchronize()
        assert guards_intact(sw, scratch) and guards_intact(ow, out)
        assert_exact(scratch, c.ref["out"], "neigh_scratch"); assert_exact(out, c.lin["out"], "out")
        return out.clone()
    assert torch.equal(run(), run())


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["K1", "K1t"])
def test_one_hub_edge_is_seen_forward(entry, monkeypatch):
    """``GB.test_one_hub_edge_is_seen``'s idea for the K1 row-wave kernel (cut hub row: ``agg_finalize``) and for K1t at D = 256
    under bias + ReLU + post-scale: ONE weight of the hub row (~2 940 entries) moved by one lattice step in the kernel's operand
    only - that row differs from the reference, every other row equals it."""
    from scdeepsort_amd import ops
    monkeypatch.setattr(ops, "TILED_MIN_WORK", None)
    D, name = 256, "hub"
    L = lattice(name, D)
    stack = dict(bias=True, relu=True, osa=True) if entry == "K1t" else dict()
    c = build_case(L, "genes", D, **stack)
    A = L["A_gc"].copy()
    assert A.indptr[1] - A.indptr[0] > 2900
    k = A.indptr[0] + 1234
    A.data[k] += 0.5 if A.data[k] < 2.0 else -0.5
    moved = build_case(dict(L, A_gc=A), "genes", D, **stack)
    assert (moved.ref["out"][0] != c.ref["out"][0]).any() and np.array_equal(moved.ref["out"][1:], c.ref["out"][1:])
    worst = build_case(dict(L, A_gc=L["A_gc"].sign() * 2.0), "genes", D, **stack)      # the moved weight at its largest still fits
    assert worst.budget["out"] < 24
    g = lattice_graph(name, dict(L, A_gc=A), 64 if entry == "K1" else None)
    alpha, hs, hself = dev(L["alpha"]), dev(c.h_src), dev(c.h_self)
    if entry == "K1":
        assert g.gc.plan.n_long > 0
        gots = [ops.agg_fwd(g.gc, alpha, c.amode, c.sidx, hs, hself)]
    else:                                                 # the hub row split (agg_finalize) and whole in its tile (tile epilogue)
        gots = [ops.agg_fwd_tiled(g.gc, tp, alpha, c.amode, c.sidx, hs, hself, bias=dev(c.bias), relu=True, out_scale_alpha=True)
                for tp in plans_with_both_kinds(g.gc, D, "heuristic", "full", 1, False)]
    want = torch.from_numpy(c.ref["out"].astype(np.float32))
    for got in gots:
        got = got.cpu()
        assert not torch.equal(got[0], want[0]), "a one-step change of one hub edge went unseen"
        assert torch.equal(got[1:], want[1:])
        assert_exact(got, moved.ref["out"], "out on the moved operand")


# ---- float group: derived per-element bound -----------------------------------------------------------------------------------------
def float_case(L, mode, D, stack, seed):
    """A float-group case: ``build_case`` on the package's operands; fp16 stacks round the feature tables to fp16 first - the
    reference sees what the kernel reads."""
    ft = np.float16 if stack.get("f16") else np.float32
    if stack.get("f16"):
        L = dict(L, h_gene=L["h_gene"].astype(ft).astype(np.float64), h_cell=L["h_cell"].astype(ft).astype(np.float64))
    return build_case(L, mode, D, bias=stack.get("bias", False), relu=stack.get("relu", False), no_mean=stack.get("no_mean", False),
                      no_self=stack.get("no_self", False), osa=stack.get("osa", False) and mode == "genes", kind=stack.get("kind"),
                      seed=seed, floats=ft)


def check_fwd_float(entry, g, L, mode, D, stack, route, seed=0):
    """One forward call through ``ops`` on ordinary floats against the derived bound; ``route``: "rowwave" or a tile plan."""
    from scdeepsort_amd import ops
    c = float_case(L, mode, D, stack, seed)
    csr = csr_of(g, c)
    f16 = stack.get("f16")
    ft = torch.float16 if f16 else torch.float32
    alpha = None if mode == "plain" else dev(L["alpha"])
    hs, hself = dev(c.h_src, ft), None if c.no_self else dev(c.h_self, ft)
    bias = None if c.bias is None else dev(c.bias)
    ns = torch.empty((c.n_out, D), device=DEV)
    if route == "rowwave":
        ids = None if c.ids is None else dev(c.ids, torch.int32)
        out = ops.agg_fwd(csr, alpha, c.amode, c.sidx, hs, hself, bias=bias, relu=c.relu, row_ids=ids, self_compact=c.compact,
                          no_mean=c.no_mean, out_dtype=torch.float16 if f16 == "out" else torch.float32, neigh_sum=ns,
                          out_scale_alpha=c.osa)
        plan = csr.plan if ids is None else csr.subplan(ids)[1]
        parts = GB.parts_per_row(plan.long_rows, c.n_out)
    else:
        out = ops.agg_fwd_tiled(csr, route, alpha, c.amode, c.sidx, hs, hself, bias=bias, relu=c.relu, no_mean=c.no_mean, neigh_sum=ns,
                                out_scale_alpha=c.osa)
        parts = GB.parts_per_row(route.long_rows, c.n_out)
    n = (c.ref["n_terms"] + parts)[:, None]
    record_ratio(entry, "neigh_sum", ns, c.ref["neigh"], AB.float_bound(c.ref["abs_neigh"], n))
    bound = AB.float_bound(c.ref["abs_out"], n + 1)
    if f16 == "out":                                               # its own entry: the one fp16 rounding fills most of that bound
        assert out.dtype == torch.float16
        bound = bound + 2.0 ** -11 * np.abs(c.ref["out"]) + 2.0 ** -25
    record_ratio(entry + "/f16out" if f16 == "out" else entry, "out", out.float(), c.ref["out"], bound)


def stack_fits(stack, mode, route):
    if stack.get("osa") and mode != "genes":
        return False
    return route == "rowwave" or not (stack.get("kind") or stack.get("f16"))          # ops.agg_fwd_tiled: all rows, f32


@pytest.mark.parametrize("route", ["rowwave", "tiled"])
@pytest.mark.parametrize("D", FLOAT_D)
@pytest.mark.parametrize("mode", MODES)
def test_forward_options_float_bound(mode, D, route, monkeypatch):
    """K1 / K1t through ``ops`` on operands as the package builds them, every option stack of ``FLOAT_STACKS`` the route takes:
    ``out`` and ``neigh_sum`` within the derived fp32 bound of the fp64 reference (fp16 output: plus its one rounding)."""
    from scdeepsort_amd import ops
    monkeypatch.setattr(ops, "TILED_MIN_WORK", None)
    g, Lf = GB.float_case_graph(D)
    L = GB.float_operands(g, Lf, D, D + 5)
    for si, stack in enumerate(FLOAT_STACKS):
        if not stack_fits(stack, mode, route):
            continue
        csr = g.cg if mode == "cells" else g.gc
        check_fwd_float("K1" if route == "rowwave" else "K1t", g, L, mode, D, stack,
                        "rowwave" if route == "rowwave" else csr.tile_plan(ops.tiled_block_rows(D)), seed=si)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_forward_fuzz_against_fp64(seed, monkeypatch):
    """Random shape / density / width / chunk / tile geometry (hub column, empty row at random) x random option stacks, both routes
    against the fp64 reference with the derived bound."""
    from scdeepsort_amd import ops
    monkeypatch.setattr(ops, "TILED_MIN_WORK", None)
    rng = np.random.default_rng(2000 + seed)
    for it in range(4):
        C, G = int(rng.integers(20, 2500)), int(rng.integers(10, 1200))
        dens = float(rng.uniform(0.005, 0.4) if rng.random() < 0.75 else rng.uniform(0.4, 0.98))
        D = int(rng.choice([256, 128, 64, 200, 32, 100, 132, 192, 16]))
        m = rng.random((C, G)) < dens
        if rng.random() < 0.5:
            m[:, rng.integers(0, G)] = True
        if rng.random() < 0.5:
            m[rng.integers(0, C), :] = False
        m[0, 0] = True                                              # at least one edge
        expr = sp.csr_matrix(np.where(m, rng.uniform(0.5, 7, (C, G)), 0).astype(np.float32))
        g, Lf = GB.float_graph(expr, chunk=int(rng.choice([64, 256, 2048])))
        L = GB.float_operands(g, Lf, D, int(rng.integers(1 << 30)))
        geom = GEOMS[int(rng.integers(5))]
        kb, loaders = BLOCK_ROWS[int(rng.integers(4))], int(rng.integers(2))
        for mode in MODES:
            stack = {k: True for k in ("bias", "relu", "no_mean", "no_self", "osa") if rng.random() < 0.5}
            seeds = dict(stack, kind=("perm", "compact")[int(rng.integers(2))]) if rng.random() < 0.5 else stack
            print(f"fuzz seed={seed} draw={it} C={C} G={G} density={dens:.3f} D={D} geom={geom} kb={kb} L={loaders} mode={mode} "
                  f"stack={sorted(seeds)}")
            check_fwd_float("K1", g, L, mode, D, seeds, "rowwave", seed=it)
            csr = g.cg if mode == "cells" else g.gc
            check_fwd_float("K1t", g, L, mode, D, stack, tile_plan(csr, D, geom, kb, loaders, False, strict=False), seed=it)
