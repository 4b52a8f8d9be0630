"""The backward aggregation entries (K2 / K2t / K3 / K3t / the seed-block K2) and the K1 / K1t forward on hub rows against the
fp64 reference ``oracle/agg_backward.py`` - this is where the ROW-WAVE backward kernels are pinned to fp64 (the route-vs-route
tests of ``test_gpu_parity.py`` compare kernels that share their epilogue, their finalize pass and their operand).

Two groups:

* **exact** - operands on a dyadic lattice (``oracle.agg_backward.lattice_case``): every product and partial sum is exactly
  representable in fp32, so the kernels must equal the fp64 reference BIT FOR BIT (``torch.equal``) at any row length; the
  condition that makes this a fair demand (``sum|terms| / unit < 2**24``) is asserted on the reference for every case, here and -
  for every parameter tuple of this file - in ``tests/test_agg_backward_reference.py`` (no GPU).
* **float** - operands as the package builds them; tolerance per element ``(n + 8) * 2**-24 * sum|terms|`` from the reference
  (``oracle.agg_backward.float_bound``), no measured constant.  Every case prints its worst ``err / bound``.

Coverage of the ABI options that had no test (option -> test):

    accumulate != 0 for dh_src and dalpha .......... test_k2_rowwave_exact[*-acc1-*], test_k2_tiled_exact[*-acc1-*]
    dst_scale ...................................... test_k2_rowwave_exact[*-dscale1-*]
    prescaled / col_scale == NULL, called directly . test_k2_tiled_exact[*-pre1-*]
    WGNN_NO_ALPHA backward ......................... test_k2_rowwave_exact[*-plain-*], test_k2_tiled_exact[*-plain-*]
    K3 with row_ids / WGNN_FLAG_SELF_COMPACT ....... test_k3_rowwave_exact[*-ids*]
    agg_bwd_src_block with dalpha .................. test_seed_block_exact
    ld != D for g / h_src / dh_src (row-wave) ...... test_k2_rowwave_exact[*-ld1-*]
    explicit tile geometries on K2t / K3t .......... test_k2_tiled_exact, test_k3_tiled_exact (the ``tplan`` keyword)
    guard rows / elements around every output ...... test_k2_rowwave_exact, test_k2_tiled_exact, test_k3_guards_exact
    one-edge sensitivity at hub degree ............. test_one_hub_edge_is_seen
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import scdeepsort_amd as sda
from conftest import small_case
from oracle import agg_backward as AB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0
MODE = {"cells": AB.SRC_IS_GENE, "genes": AB.DST_IS_GENE, "plain": AB.NO_ALPHA}

# sparsity patterns (conftest.small_case: hub gene at 98 %, an empty cell, an unexpressed gene): cells, genes, density, seed
GRAPHS = {"hub": (3000, 1500, 0.25, 11),      # hub source / destination row: ~2 940 entries
          "mid": (900, 640, 0.2, 12),
          "small": (700, 333, 0.25, 13)}
ROWWAVE_D = (4, 8, 24, 64, 100, 128, 200, 256, 400, 1024)          # all six dispatch_width branches
TILED_D = (4, 32, 64, 100, 128, 132, 192, 200, 252, 256)
GEOMS = ((None, 1), (3, 1), (2, 4), (5, 7), "heuristic")            # (row tiles, column splits)
BLOCK_ROWS = (16, 23, 64, "full")                                   # "full" = ops.tiled_block_rows(D)
TALL_D = (64, 200, 256)


def _graph_for(D, i):
    """Widths above 256 keep the dot-product budget on the smaller patterns; the hub pattern takes every third of the rest."""
    if D >= 400:
        return "small"
    return ("hub", "mid", "small")[i % 3]


# ---- the case sets (plain data: tests/test_agg_backward_reference.py checks the lattice budget of every tuple on the CPU) ----
# K2 row-wave: every (width, mode); the other axes rotate so that each value of each axis meets each mode:
#   (graph, mode, D, chunk, accumulate, dst_scale, strided)   chunk 64: long rows are cut (finalize path), 4096: none is
K2_ROWWAVE_CASES = [(_graph_for(D, di + mi), m, D, (64, 4096)[(di + mi) % 2], (di // 2 + mi) % 2, (di + 2 * mi) % 3 == 0,
                     (di // 3 + mi) % 2 == 0)
                    for di, D in enumerate(ROWWAVE_D) for mi, m in enumerate(("cells", "genes", "plain"))]
# K2t: two sweeps over (width, mode) with shifted rotations + the tall tile:
#   (graph, mode, D, geom, block_rows, loaders, tall, prescaled, accumulate, dalpha)
K2_TILED_CASES = [("hub" if GEOMS[(di + mi + s) % 5] == "heuristic" else ("small", "mid")[(di + s) % 2], m, D,
                   GEOMS[(di + mi + s) % 5], BLOCK_ROWS[(di + 2 * mi + s) % 4], (di + mi + s) % 2, False,
                   (di + s) % 2 == 1, (di // 2 + mi + s) % 2, m == "cells" and (di + s) % 3 != 0)
                  for s in (0, 1) for di, D in enumerate(TILED_D) for mi, m in enumerate(("cells", "genes", "plain"))]
K2_TILED_CASES += [(("hub", "mid", "small")[(di + mi) % 3], m, D, ("heuristic", (2, 1), (3, 2))[(di + mi) % 3],
                    BLOCK_ROWS[(di + mi + 1) % 4], 0, True, (di + mi) % 2 == 1, (di + mi + 1) % 2, m == "cells")
                   for di, D in enumerate(TALL_D) for mi, m in enumerate(("cells", "genes", "plain"))]
# K3 row-wave: (graph, D, h_self, ids, chunk)   ids: None | "perm" (unordered, with repeats, incl. the empty row) | "empty" | "compact"
K3_ROWWAVE_CASES = [(_graph_for(D, di), D, di % 3 != 0, (None, "perm", "compact", None, "empty")[di % 5], (64, 4096)[di % 2])
                    for di, D in enumerate(ROWWAVE_D)]
K3_ROWWAVE_CASES += [("small", 64, True, "perm", 4096), ("mid", 200, False, "compact", 64), ("hub", 256, True, None, 64)]
# K3t: (graph, D, geom, block_rows, loaders, tall, h_self)
K3_TILED_CASES = [("hub" if GEOMS[(di + s) % 5] == "heuristic" else ("small", "mid")[(di + s) % 2], D, GEOMS[(di + s) % 5],
                   BLOCK_ROWS[(di + 2 * s) % 4], (di + s) % 2, False, (di + s) % 3 != 0)
                  for s in (0, 2) for di, D in enumerate(TILED_D)]
K3_TILED_CASES += [(("hub", "mid", "small")[di], D, ("heuristic", (2, 2), (2, 3))[di], BLOCK_ROWS[di + 1], 0, True, di != 1)
                   for di, D in enumerate(TALL_D)]
# seed-block K2: (graph, mode, B, D)
SEED_BLOCK_CASES = [("mid", m, B, D) for m in ("cells", "plain") for B, D in ((1, 64), (5, 200), (64, 256), (300, 24))]
# K1 / K1t forward on hub rows: (graph, direction, D, route)   route: "rowwave" | (geom, block_rows, loaders, tall)
FWD_CASES = [("hub", d, D, "rowwave") for d in ("cells", "genes") for D in (64, 256, 400)]
FWD_CASES += [("hub" if GEOMS[(di + k) % 5] == "heuristic" else ("small", "mid")[di % 2], d, D,
               (GEOMS[(di + k) % 5], BLOCK_ROWS[(di + k) % 4], (di + k) % 2, False))
              for k, d in enumerate(("cells", "genes")) for di, D in enumerate(TILED_D)]
FWD_CASES += [("hub", d, D, ("heuristic", "full", 0, True)) for d in ("cells", "genes") for D in (64, 256)]
FLOAT_D = (64, 200, 256)


def _cid(case):
    def one(v):
        if isinstance(v, tuple):
            return "x".join(one(x) for x in v)
        return {None: "auto", True: "1", False: "0"}.get(v, str(v)) if isinstance(v, (bool, type(None))) else str(v)
    return "-".join(one(v) for v in case)


def k2_id(c):
    return f"{c[0]}-{c[1]}-D{c[2]}-chunk{c[3]}-acc{int(c[4])}-dscale{int(c[5])}-ld{int(c[6])}"


def k2t_id(c):
    return (f"{c[0]}-{c[1]}-D{c[2]}-g{_cid((c[3],))}-kb{c[4]}-L{c[5]}-tall{int(c[6])}-pre{int(c[7])}-acc{int(c[8])}"
            f"-dalpha{int(c[9])}")


def k3_id(c):
    return f"{c[0]}-D{c[1]}-self{int(c[2])}-ids{c[3]}-chunk{c[4]}"


# ---- helpers -------------------------------------------------------------------------------------------------------------
def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


@functools.lru_cache(maxsize=None)
def pattern(name):
    cells, genes, density, seed = GRAPHS[name]
    return small_case(cells=cells, genes=genes, dim=4, seed=seed, density=density, test_cells=0)["expr"]


def case_seed(*key):
    return sum((i + 1) * sum(map(ord, str(k))) for i, k in enumerate(key)) % (2 ** 31)


def lattice_graph(name, L, chunk=None):
    """The package's graph on the pattern, its weights and per-destination scales REPLACED by the lattice's before the first
    transposed() / tile plan is built (the kernels take both as opaque numbers)."""
    g = sda.CellGeneGraph.from_expression(pattern(name), device=DEV, chunk=chunk)
    for csr, A, inv in ((g.cg, L["A_cg"], L["inv_cg"]), (g.gc, L["A_gc"], L["inv_gc"])):
        assert np.array_equal(csr.rowptr.cpu().numpy(), A.indptr) and np.array_equal(csr.col.cpu().numpy(), A.indices)
        csr.val, csr.inv_deg = dev(A.data), dev(inv)
        csr._t, csr._tile_plan = None, None
    return g


def float_graph(expr, chunk=None):
    """The package's graph as it comes + its operands read back as fp64 scipy matrices (the reference sees the kernels' inputs)."""
    g = sda.CellGeneGraph.from_expression(expr, device=DEV, chunk=chunk)
    L = {}
    for key, csr in (("cg", g.cg), ("gc", g.gc)):
        L["A_" + key] = sp.csr_matrix((csr.val.cpu().numpy().astype(np.float64), csr.col.cpu().numpy(), csr.rowptr.cpu().numpy()),
                                      shape=(csr.n_rows, csr.n_cols))
        L["inv_" + key] = csr.inv_deg.cpu().numpy().astype(np.float64)
    return g, L


def side(g, L, mode):
    """(csr, A, inv, gradient rows, source rows, prior dh_src) of a K2 call in ``mode``: SRC_IS_GENE and NO_ALPHA run on the
    cells<-genes operand (its transposed structure holds the hub source row), DST_IS_GENE on genes<-cells."""
    if mode == "genes":
        return g and g.gc, L["A_gc"], L["inv_gc"], L["g_gene"], L["h_cell"], L["prior_dh_cell"]
    return g and g.cg, L["A_cg"], L["inv_cg"], L["g_cell"], L["h_gene"], L["prior_dh_gene"]


def guarded(inner, pad_cols=0):
    """``inner`` ([n, D] or [n]) placed inside a larger SENTINEL-filled tensor: one guard row / element on each side and, for
    matrices, ``pad_cols`` guard columns left and right (the view then has ld = D + 2 * pad_cols).  Returns (whole, view)."""
    inner = dev(inner)
    if inner.dim() == 1:
        whole = torch.full((inner.shape[0] + 8,), SENTINEL, device=DEV)
        view = whole[4:4 + inner.shape[0]]
    else:
        n, D = inner.shape
        whole = torch.full((n + 2, D + 2 * pad_cols), SENTINEL, device=DEV)
        view = whole[1:n + 1, pad_cols:pad_cols + D]
    view.copy_(inner)
    return whole, view


def guards_intact(whole, view):
    probe = whole.clone()
    if view.dim() == 1:
        probe[4:4 + view.shape[0]] = SENTINEL
    else:
        off = view.storage_offset() - whole.storage_offset()
        r0, c0 = off // whole.stride(0), off % whole.stride(0)
        probe[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = SENTINEL
    return bool((probe == SENTINEL).all())


def strided(x, pad=4):
    """``x`` as a column slice of a wider tensor (ld = D + 2 * pad, 16-byte aligned)."""
    return guarded(x, pad)[1]


def assert_exact(got, want64, what):
    want32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    assert np.array_equal(want32.astype(np.float64), want64), f"{what}: the reference itself is not an fp32 number"
    got = got.detach().cpu()
    want = torch.from_numpy(want32).reshape(got.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ from the fp64 reference, first at "
                             f"{bad[0].tolist()}: got {got[tuple(bad[0])].item()!r}, want {want[tuple(bad[0])].item()!r}")


def parts_per_row(long_rows, n_rows):
    """Partial sums folded per row (``long_rows`` = {row, first partial, n partials, -} of a row-chunk or tile plan)."""
    v = np.zeros(n_rows, dtype=np.int64)
    if long_rows is not None and long_rows.numel():
        lr = long_rows.cpu().numpy().reshape(-1, 4)
        lr = lr[lr[:, 0] >= 0]
        np.maximum.at(v, lr[:, 0], lr[:, 2])
    return v


def tile_plan(csr, D, geom, kb, loaders, tall, strict=True):
    from scdeepsort_amd import graph as GR, ops
    full = ops.tiled_block_rows(D)
    kb = full if kb == "full" else min(kb, full)
    rt, cs = (None, None) if geom == "heuristic" else geom
    tp = GR.build_tile_plan(csr, rt, cs, block_rows=kb, n_loaders=loaders, geom=GR.GEOM_TALL if tall else GR.GEOM_FLAT)
    if geom != "heuristic" and strict:
        assert tp.n_col_splits == cs
    assert tp.geom.tall == tall and tp.block_rows == kb
    return tp


RATIOS = {}


def record_ratio(entry, what, got, want64, bound):
    r = AB.worst_ratio(got.detach().cpu().numpy(), want64, bound)
    RATIOS[entry] = max(RATIOS.get(entry, 0.0), r)
    print(f"RATIO entry={entry} output={what} err/bound={r:.4f} worst_so_far={RATIOS[entry]:.4f}")
    assert r <= 1.0, f"{entry} {what}: error exceeds the derived bound, err / bound = {r:.3f}"


# ---- K2 / K2t ------------------------------------------------------------------------------------------------------------
def run_k2(g, L, mode, D, *, accumulate, dst_scale=None, ld=False, want_dalpha=True, tplan=None, prescaled=False):
    """One K2 call with guarded outputs; returns (dh_src view, dalpha view | None) after checking the guards."""
    from scdeepsort_amd import ops
    csr, A, inv, gr, hs, prior = side(g, L, mode)
    alpha = dev(L["alpha"]) if mode != "plain" else None
    gt, ht = (strided(gr), strided(hs)) if ld else (dev(gr), dev(hs))
    dh_whole, dh = guarded(prior, 4 if ld else 0)
    da_whole = da = None
    if mode == "cells" and want_dalpha:
        da_whole, da = guarded(L["prior_dalpha"])
    scale = None if dst_scale is None else dev(dst_scale)
    if prescaled:
        gt = ops.agg_bwd_prepare(gt, None, dev(inv if dst_scale is None else dst_scale), alpha, MODE[mode], 0)["g_scaled"]
    out = ops.agg_bwd_src(csr, alpha, MODE[mode], gt, ht if da is not None else None, da, dh, bool(accumulate),
                          dst_scale=scale, prescaled=prescaled, tplan=tplan)
    assert out.data_ptr() == dh.data_ptr()
    torch.cuda.synchronize()
    assert guards_intact(dh_whole, dh), "dh_src: a guard row / column was written"
    if da is not None:
        assert guards_intact(da_whole, da), "dalpha: a guard element was written"
    return dh.clone(), None if da is None else da.clone()


def k2_reference(L, mode, *, accumulate, dst_scale=None, want_dalpha=True):
    _, A, inv, gr, hs, prior = side(None, L, mode)
    ref = AB.bwd_src(A, inv if dst_scale is None else dst_scale, L["alpha"], MODE[mode], gr,
                     hs if (mode == "cells" and want_dalpha) else None)
    want_dh = ref["dh_src"] + (prior if accumulate else 0)
    want_da = None
    if ref["dalpha_src"] is not None:
        want_da = L["prior_dalpha"].copy()                         # entries G, G + 1 (the self-loop scalars) are never written
        G = ref["dalpha_src"].shape[0]
        want_da[:G] = ref["dalpha_src"] + (L["prior_dalpha"][:G] if accumulate else 0)
    return ref, want_dh, want_da, prior


def k2_lattice(name, mode, D, dst_scale, key):
    L = AB.lattice_case(pattern(name), D, case_seed(*key))
    scale = None
    if dst_scale:
        n = L["A_gc"].shape[0] if mode == "genes" else L["A_cg"].shape[0]
        scale = np.random.default_rng(case_seed(*key) + 1).choice(AB.LATTICE_SCALE, n)
    return L, scale


@pytest.mark.parametrize("case", K2_ROWWAVE_CASES, ids=k2_id)
def test_k2_rowwave_exact(case, monkeypatch):
    """``wgnn_agg_bwd_src`` (row-wave) == fp64 reference, bit for bit: every width branch x every mode, cut and uncut long rows,
    accumulate into non-zero dh_src AND dalpha, dst_scale, ld > D for g / h_src / dh_src, guards, determinism."""
    from scdeepsort_amd import ops
    name, mode, D, chunk, acc, dscale, ld = case
    monkeypatch.setattr(ops, "TILED_MIN_WORK", None)
    L, scale = k2_lattice(name, mode, D, dscale, case)
    ref, want_dh, want_da, prior = k2_reference(L, mode, accumulate=acc, dst_scale=scale)
    AB.check_bwd_src_budget(ref, MODE[mode], prior if acc else None, L["prior_dalpha"][:ref["T"].shape[0]] if acc else None)
    g = lattice_graph(name, L, chunk)
    t = side(g, L, mode)[0].transposed()
    assert (t.plan.n_long > 0) == (chunk == 64) and t.plan.chunk == chunk
    dh, da = run_k2(g, L, mode, D, accumulate=acc, dst_scale=scale, ld=ld)
    assert_exact(dh, want_dh, "dh_src")
    if mode == "cells":
        assert_exact(da, want_da, "dalpha")
    dh2, da2 = run_k2(g, L, mode, D, accumulate=acc, dst_scale=scale, ld=ld)
    assert torch.equal(dh, dh2) and (da is None or torch.equal(da, da2))


@pytest.mark.parametrize("case", K2_TILED_CASES, ids=k2t_id)
def test_k2_tiled_exact(case):
    """``wgnn_agg_bwd_src_tiled`` over EXPLICIT tile plans (``ops.agg_bwd_src(..., tplan=)``) == fp64 reference, bit for bit:
    row tiles x column splits x LDS block height x loader waves x tall tile, col_scale given and NULL (rows pre-scaled by
    ``ops.agg_bwd_prepare``), accumulate, dalpha on / off."""
    name, mode, D, geom, kb, loaders, tall, pre, acc, want_da_ = case
    L, _ = k2_lattice(name, mode, D, False, case)
    ref, want_dh, want_da, prior = k2_reference(L, mode, accumulate=acc, want_dalpha=want_da_)
    AB.check_bwd_src_budget(ref, MODE[mode], prior if acc else None, L["prior_dalpha"][:ref["T"].shape[0]] if acc else None)
    g = lattice_graph(name, L)
    tp = tile_plan(side(g, L, mode)[0].transposed(), D, geom, kb, loaders, tall)
    dh, da = run_k2(g, L, mode, D, accumulate=acc, want_dalpha=want_da_, tplan=tp, prescaled=pre)
    assert_exact(dh, want_dh, "dh_src")
    assert (da is not None) == (mode == "cells" and want_da_)
    if da is not None:
        assert_exact(da, want_da, "dalpha")
    dh2, da2 = run_k2(g, L, mode, D, accumulate=acc, want_dalpha=want_da_, tplan=tp, prescaled=pre)
    assert torch.equal(dh, dh2) and (da is None or torch.equal(da, da2))


def test_k2_default_dispatch_takes_the_cached_plan_and_matches_the_explicit_one(monkeypatch):
    """The ``tplan`` keyword changes nothing by default: with the dispatch forced to the tile route, K2t / K3t over the cached
    heuristic plan give the exact results too (and so the same bits as the same plan handed in)."""
    from scdeepsort_amd import ops
    monkeypatch.setattr(ops, "TILED_MIN_WORK", 1)
    D = 128
    L = AB.lattice_case(pattern("mid"), D, 77)
    g = lattice_graph("mid", L)
    for mode in ("cells", "genes", "plain"):
        ref, want_dh, want_da, _ = k2_reference(L, mode, accumulate=0)
        AB.check_bwd_src_budget(ref, MODE[mode])
        dh, da = run_k2(g, L, mode, D, accumulate=0)
        assert_exact(dh, want_dh, "dh_src")
        tp = side(g, L, mode)[0].transposed().tile_plan(ops.tiled_block_rows(D))
        dh2, da2 = run_k2(g, L, mode, D, accumulate=0, tplan=tp)
        assert torch.equal(dh, dh2) and (da is None or torch.equal(da, da2))
        if da is not None:
            assert_exact(da, want_da, "dalpha")
    r3 = AB.bwd_alpha(L["A_gc"], L["inv_gc"], L["g_gene"], L["h_cell"], L["h_gene"])
    AB.check_bwd_alpha_budget(r3)
    d_row, d_self = ops.agg_bwd_alpha(g.gc, dev(L["g_gene"]), dev(L["h_cell"]), dev(L["h_gene"]))
    assert_exact(d_row, r3["dalpha_row"], "dalpha_row"); assert_exact(d_self, r3["dself_row"], "dself_row")


# ---- K3 / K3t ------------------------------------------------------------------------------------------------------------
def k3_ids(kind, n_rows, seed):
    rng = np.random.default_rng(seed)
    if kind is None:
        return None
    if kind == "empty":
        return np.zeros(0, dtype=np.int64)
    # "perm" / "compact":
    ids = rng.integers(0, n_rows, 2 * n_rows // 3 + 1)              # unordered, with repeats
    ids[:4] = (0, 5, 0, n_rows - 1)                                 # the hub gene twice, the unexpressed gene, the last row
    return ids


def k3_operands(L, D, with_self, kind, seed):
    G = L["G"]
    ids = k3_ids(kind, G, seed)
    n_out = G if ids is None else len(ids)
    rng = np.random.default_rng(seed + 1)
    gr = L["g_gene"] if ids is None else rng.integers(-2, 3, (n_out, D)).astype(np.float64)        # one gradient row per SLOT
    compact = kind == "compact"
    h_self = None
    if with_self:
        h_self = rng.integers(-2, 3, (n_out, D)).astype(np.float64) if compact else L["h_gene"]
    return ids, gr, h_self, compact


@pytest.mark.parametrize("case", K3_ROWWAVE_CASES, ids=k3_id)
def test_k3_rowwave_exact(case, monkeypatch):
    """``wgnn_agg_bwd_alpha`` (row-wave) == fp64 reference, bit for bit: every width branch, with and without h_self, cut and
    uncut long rows, row_ids (unordered, repeated, empty) and WGNN_FLAG_SELF_COMPACT."""
    from scdeepsort_amd import ops
    name, D, with_self, kind, chunk = case
    monkeypatch.setattr(ops, "TILED_MIN_WORK", None)
    L = AB.lattice_case(pattern(name), D, case_seed(*case))
    ids, gr, h_self, compact = k3_operands(L, D, with_self, kind, case_seed(*case))
    ref = AB.bwd_alpha(L["A_gc"], L["inv_gc"], gr, L["h_cell"], h_self, ids, compact)
    AB.check_bwd_alpha_budget(ref)
    g = lattice_graph(name, L, chunk)
    assert (g.gc.plan.n_long > 0) == (chunk == 64)

    def run():
        return ops.agg_bwd_alpha(g.gc, dev(gr), dev(L["h_cell"]), None if h_self is None else dev(h_self),
                                 None if ids is None else dev(ids, torch.int32), self_compact=compact)
    d_row, d_self = run()
    assert_exact(d_row, ref["dalpha_row"], "dalpha_row")
    assert (d_self is None) == (h_self is None)
    if d_self is not None:
        assert_exact(d_self, ref["dself_row"], "dself_row")
    again = run()
    assert torch.equal(again[0], d_row) and (d_self is None or torch.equal(again[1], d_self))


@pytest.mark.parametrize("case", K3_TILED_CASES, ids=_cid)
def test_k3_tiled_exact(case):
    """``wgnn_agg_bwd_alpha_tiled`` over explicit tile plans (``ops.agg_bwd_alpha(..., tplan=)``) == fp64 reference, bit for bit."""
    from scdeepsort_amd import ops
    name, D, geom, kb, loaders, tall, with_self = case
    L = AB.lattice_case(pattern(name), D, case_seed(*case))
    h_self = L["h_gene"] if with_self else None
    ref = AB.bwd_alpha(L["A_gc"], L["inv_gc"], L["g_gene"], L["h_cell"], h_self)
    AB.check_bwd_alpha_budget(ref)
    g = lattice_graph(name, L)
    tp = tile_plan(g.gc, D, geom, kb, loaders, tall)
    run = lambda: ops.agg_bwd_alpha(g.gc, dev(L["g_gene"]), dev(L["h_cell"]), None if h_self is None else dev(h_self), tplan=tp)
    d_row, d_self = run()
    assert_exact(d_row, ref["dalpha_row"], "dalpha_row")
    assert (d_self is None) == (h_self is None)
    if d_self is not None:
        assert_exact(d_self, ref["dself_row"], "dself_row")
    again = run()
    assert torch.equal(again[0], d_row) and (d_self is None or torch.equal(again[1], d_self))


@pytest.mark.parametrize("route", ["rowwave", "tiled"])
def test_k3_guards_exact(route):
    """K3 / K3t through the C ABI with dalpha_row / dself_row as views into larger tensors: exact results, guard elements on
    both sides untouched (``ops.agg_bwd_alpha`` allocates its own outputs, so this one binds the entry directly)."""
    from scdeepsort_amd import _lib, ops
    from scdeepsort_amd.graph import _ptr, _stream
    D, name = 200, "mid"
    L = AB.lattice_case(pattern(name), D, 5)
    ref = AB.bwd_alpha(L["A_gc"], L["inv_gc"], L["g_gene"], L["h_cell"], L["h_gene"])
    AB.check_bwd_alpha_budget(ref)
    g = lattice_graph(name, L, 64)
    csr, G = g.gc, L["G"]
    gr, hs, hself = dev(L["g_gene"]), dev(L["h_cell"]), dev(L["h_gene"])
    row_whole, d_row = guarded(np.full(G, 7.0)); self_whole, d_self = guarded(np.full(G, 7.0))
    d = torch.device(DEV)
    if route == "rowwave":
        p = csr.plan
        part = torch.empty(max(1, p.n_partials) * D, device=DEV)
        rc = _lib.call(d, "wgnn_agg_bwd_alpha", _ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.val), _ptr(csr.inv_deg), None,
                       _ptr(gr), D, _ptr(hs), D, _ptr(hself), D, _ptr(d_row), _ptr(d_self), G, D, 0,
                       _ptr(p.items), p.n_items, _ptr(p.long_rows) if p.n_long else None, p.n_long, _ptr(part), p.n_partials,
                       _stream(d))
    else:
        tp = tile_plan(csr, D, (2, 3), 23, 1, False)
        n_long = tp.long_rows.shape[0]
        part = torch.empty(max(1, tp.n_partials) * D, device=DEV)
        rc = _lib.call(d, "wgnn_agg_bwd_alpha_tiled", _ptr(csr.inv_deg), _ptr(gr), D, _ptr(hs), _ptr(hself), D,
                       _ptr(d_row), _ptr(d_self), G, D, _ptr(tp.entries), _ptr(tp.seg_ptr), tp.nblk_max, tp.block_rows_arg,
                       _ptr(tp.items), _ptr(tp.hdr), tp.n_tiles, _ptr(tp.long_rows) if n_long else None, n_long,
                       _ptr(part), tp.n_partials, _stream(d))
    _lib.check(rc, "wgnn_agg_bwd_alpha")
    torch.cuda.synchronize()
    assert_exact(d_row, ref["dalpha_row"], "dalpha_row"); assert_exact(d_self, ref["dself_row"], "dself_row")
    assert guards_intact(row_whole, d_row) and guards_intact(self_whole, d_self)


# ---- seed-block K2 -------------------------------------------------------------------------------------------------------
def seed_ids(B, n_rows, seed):
    ids = np.random.default_rng(seed).integers(0, n_rows, B)
    ids[0] = 3                                                     # the empty cell
    if B >= 5:
        ids[1] = ids[2] = 7                                        # a repeated seed: two slots
    return ids


@pytest.mark.parametrize("case", SEED_BLOCK_CASES, ids=_cid)
def test_seed_block_exact(case):
    """``ops.agg_bwd_src_block`` (K2 over the device-built source-major block of one seed batch, with dalpha) == ``bwd_src`` on
    the CSR restricted to the seed slots, bit for bit; source rows that no seed gathers are exactly 0."""
    from scdeepsort_amd import ops
    name, mode, B, D = case
    L = AB.lattice_case(pattern(name), D, case_seed(*case))
    rng = np.random.default_rng(case_seed(*case) + 2)
    ids = seed_ids(B, L["C"], B)
    gr = rng.integers(-2, 3, (B, D)).astype(np.float64)
    inv_rows = rng.choice(AB.LATTICE_SCALE, B)
    ref = AB.bwd_src(L["A_cg"][ids], inv_rows, L["alpha"], MODE[mode], gr, L["h_gene"])
    AB.check_bwd_src_budget(ref, MODE[mode])
    g = lattice_graph(name, L)

    def run():
        da_whole, da = guarded(L["prior_dalpha"]) if mode == "cells" else (None, None)
        dh = ops.agg_bwd_src_block(g.cg, dev(ids, torch.int64), dev(L["alpha"]) if mode != "plain" else None, MODE[mode], dev(gr),
                                   dev(inv_rows), dev(L["h_gene"]) if mode == "cells" else None, da)
        torch.cuda.synchronize()
        assert da is None or guards_intact(da_whole, da)
        return dh, da
    dh, da = run()
    assert_exact(dh, ref["dh_src"], "dh_src")
    untouched = ref["n_terms"] == 0
    assert untouched.any() and bool((dh[dev(untouched, torch.bool)] == 0).all())
    if da is not None:
        want = L["prior_dalpha"].copy(); want[:L["G"]] = ref["dalpha_src"]
        assert_exact(da, want, "dalpha")
    dh2, da2 = run()
    assert torch.equal(dh, dh2) and (da is None or torch.equal(da, da2))


# ---- K1 / K1t forward on hub rows ----------------------------------------------------------------------------------------
def fwd_side(g, L, direction):
    G = L["G"]
    if direction == "cells":
        return g.cg if g is not None else None, L["A_cg"], L["inv_cg"], AB.SRC_IS_GENE, G + 1, L["h_gene"], L["h_cell"]
    return g.gc if g is not None else None, L["A_gc"], L["inv_gc"], AB.DST_IS_GENE, G, L["h_cell"], L["h_gene"]


def run_fwd(g, L, direction, D, route):
    from scdeepsort_amd import ops
    csr, _, _, mode, sidx, hs, hself = fwd_side(g, L, direction)
    nsum = torch.full((csr.n_rows, D), SENTINEL, device=DEV)
    if route == "rowwave":
        out = ops.agg_fwd(csr, dev(L["alpha"]), mode, sidx, dev(hs), dev(hself), neigh_sum=nsum)
    else:
        out = ops.agg_fwd_tiled(csr, tile_plan(csr, D, *route), dev(L["alpha"]), mode, sidx, dev(hs), dev(hself), neigh_sum=nsum)
    return out, nsum


@pytest.mark.parametrize("case", FWD_CASES, ids=_cid)
def test_forward_on_hub_rows_exact(case, monkeypatch):
    """K1 / K1t on the lattice operands (``inv_deg`` in {0.5, 1}: the mean is exact): ``out`` and ``neigh_sum`` == fp64
    reference, bit for bit, in both directions - a mean over a 3 000-edge row cannot hide a wrong edge here."""
    from scdeepsort_amd import ops
    name, direction, D, route = case
    monkeypatch.setattr(ops, "TILED_MIN_WORK", None)
    L = AB.lattice_case(pattern(name), D, case_seed(*case))
    _, A, inv, mode, sidx, hs, hself = fwd_side(None, L, direction)
    ref = AB.fwd(A, inv, L["alpha"], mode, sidx, hs, hself)
    AB.check_fwd_budget(ref, mode)
    g = lattice_graph(name, L)
    out, nsum = run_fwd(g, L, direction, D, route)
    assert_exact(out, ref["out"], "out"); assert_exact(nsum, ref["neigh"], "neigh_sum")
    out2, nsum2 = run_fwd(g, L, direction, D, route)
    assert torch.equal(out, out2) and torch.equal(nsum, nsum2)


# ---- sensitivity: the harness sees ONE wrong edge of a hub row ---------------------------------------------------------------
@pytest.mark.parametrize("entry", ["K2", "K2t", "K1t"])
def test_one_hub_edge_is_seen(entry, monkeypatch):
    """The weight of ONE entry of the hub row (~2 940 entries) moved by one lattice step (0.5) in the operand the kernel gets, not
    in the reference: the kernel's output differs from the reference in that source / destination row and equals it in every
    other row.  (Valid inputs only: the moved weight stays on the lattice.)"""
    from scdeepsort_amd import ops
    monkeypatch.setattr(ops, "TILED_MIN_WORK", None)
    D, name = 256, "hub"
    L = AB.lattice_case(pattern(name), D, 31)
    Lk = dict(L)
    if entry == "K1t":                                    # destination row = the hub gene (row 0 of genes<-cells)
        A = L["A_gc"].copy()
        assert A.indptr[1] - A.indptr[0] > 2900
        k = A.indptr[0] + 1234
        assert np.abs(L["h_cell"][A.indices[k]]).max() > 0
        key = "A_gc"
    else:                                                 # source row = the hub gene (column 0 of cells<-genes)
        A = L["A_cg"].copy()
        assert (A.indices == 0).sum() > 2900
        r = 1234
        assert A.indices[A.indptr[r]] == 0 and np.abs(L["g_cell"][r]).max() > 0
        k = A.indptr[r]
        key = "A_cg"
    A.data[k] += 0.5 if A.data[k] < 2.0 else -0.5
    Lk[key] = A
    g = lattice_graph(name, Lk)
    if entry == "K1t":
        _, A0, inv, mode, sidx, hs, hself = fwd_side(None, L, "genes")
        ref = AB.fwd(A0, inv, L["alpha"], mode, sidx, hs, hself)
        AB.check_fwd_budget(ref, mode)
        got, _ = run_fwd(g, Lk, "genes", D, ("heuristic", "full", 1, False))
        want = ref["out"]
    else:
        ref, want, _, _ = k2_reference(L, "cells", accumulate=0)
        AB.check_bwd_src_budget(ref, AB.SRC_IS_GENE)
        tp = tile_plan(g.cg.transposed(), D, "heuristic", "full", 1, False) if entry == "K2t" else None
        got, _ = run_k2(g, Lk, "cells", D, accumulate=0, tplan=tp)
    got = got.cpu()
    want = torch.from_numpy(want.astype(np.float32))
    assert not torch.equal(got[0], want[0]), "a one-step change of one hub edge went unseen"
    assert torch.equal(got[1:], want[1:])


# ---- float group: derived per-element bound ----------------------------------------------------------------------------------
def float_operands(g, Lf, D, seed):
    rng = np.random.default_rng(seed)
    C, G = g.num_cells, g.num_genes
    L = dict(Lf, C=C, G=G, D=D, alpha=rng.uniform(0.5, 1.5, G + 2).astype(np.float32).astype(np.float64))
    for k, n in (("h_gene", G), ("h_cell", C), ("g_cell", C), ("g_gene", G), ("prior_dh_gene", G), ("prior_dh_cell", C)):
        L[k] = rng.standard_normal((n, D)).astype(np.float32).astype(np.float64)
    L["prior_dalpha"] = rng.standard_normal(G + 2).astype(np.float32).astype(np.float64)
    return L


def check_k2_float(entry, g, L, mode, D, tplan, acc):
    csr = side(g, L, mode)[0]
    ref, want_dh, want_da, prior = k2_reference(L, mode, accumulate=acc)
    t = csr.transposed()
    parts = parts_per_row((tplan or t.plan).long_rows, t.n_rows)
    n = ref["n_terms"] + parts + (1 if acc else 0)
    dh, da = run_k2(g, L, mode, D, accumulate=acc, tplan=tplan)
    record_ratio(entry, "dh_src", dh, want_dh, AB.float_bound(ref["abs_dh"] + (np.abs(prior) if acc else 0), n[:, None]))
    if da is not None:
        G = L["G"]
        bound = AB.float_bound(ref["abs_dalpha"] + (np.abs(L["prior_dalpha"][:G]) if acc else 0), n + D)
        record_ratio(entry, "dalpha", da[:G], want_da[:G], bound)
        assert_exact(da[G:], want_da[G:], "dalpha[G:]")


def check_k3_float(entry, g, L, D, tplan):
    from scdeepsort_amd import ops
    ref = AB.bwd_alpha(L["A_gc"], L["inv_gc"], L["g_gene"], L["h_cell"], L["h_gene"])
    parts = parts_per_row((tplan or g.gc.plan).long_rows, g.gc.n_rows)
    d_row, d_self = ops.agg_bwd_alpha(g.gc, dev(L["g_gene"]), dev(L["h_cell"]), dev(L["h_gene"]), tplan=tplan)
    record_ratio(entry, "dalpha_row", d_row, ref["dalpha_row"], AB.float_bound(ref["abs_dalpha_row"], ref["n_terms"] + parts + D))
    record_ratio(entry, "dself_row", d_self, ref["dself_row"], AB.float_bound(ref["abs_dself_row"], D))


def check_fwd_float(entry, g, L, direction, D, route):
    csr, A, inv, mode, sidx, hs, hself = fwd_side(g, L, direction)
    ref = AB.fwd(A, inv, L["alpha"], mode, sidx, hs, hself)
    from scdeepsort_amd import ops
    ns = torch.empty((csr.n_rows, D), device=DEV)
    if route == "rowwave":
        out = ops.agg_fwd(csr, dev(L["alpha"]), mode, sidx, dev(hs), dev(hself), neigh_sum=ns)
        parts = parts_per_row(csr.plan.long_rows, csr.n_rows)
    else:
        out = ops.agg_fwd_tiled(csr, route, dev(L["alpha"]), mode, sidx, dev(hs), dev(hself), neigh_sum=ns)
        parts = parts_per_row(route.long_rows, csr.n_rows)
    n = (ref["n_terms"] + parts)[:, None]
    record_ratio(entry, "neigh_sum", ns, ref["neigh"], AB.float_bound(ref["abs_neigh"], n))
    record_ratio(entry, "out", out, ref["out"], AB.float_bound(ref["abs_out"], n + 1))


def check_block_float(g, L, mode, D, B, seed):
    from scdeepsort_amd import ops
    rng = np.random.default_rng(seed)
    ids = seed_ids(B, L["C"], seed)
    gr = rng.standard_normal((B, D)).astype(np.float32).astype(np.float64)
    inv_rows = L["inv_cg"][ids]
    ref = AB.bwd_src(L["A_cg"][ids], inv_rows, L["alpha"], MODE[mode], gr, L["h_gene"])
    da = dev(L["prior_dalpha"]) if mode == "cells" else None
    dh = ops.agg_bwd_src_block(g.cg, dev(ids, torch.int64), dev(L["alpha"]) if mode != "plain" else None, MODE[mode], dev(gr),
                               dev(inv_rows), dev(L["h_gene"]) if mode == "cells" else None, da)
    record_ratio("block", "dh_src", dh, ref["dh_src"], AB.float_bound(ref["abs_dh"], ref["n_terms"][:, None]))
    if da is not None:
        record_ratio("block", "dalpha", da[:L["G"]], ref["dalpha_src"], AB.float_bound(ref["abs_dalpha"], ref["n_terms"] + D))


def float_case_graph(D):
    c = small_case(cells=1100, genes=520, dim=4, seed=D, density=0.2, test_cells=0)
    return float_graph(c["expr"])


@pytest.mark.parametrize("route", ["rowwave", "tiled"])
@pytest.mark.parametrize("D", FLOAT_D)
@pytest.mark.parametrize("mode", ["cells", "genes", "plain"])
def test_k2_float_bound(mode, D, route, monkeypatch):
    """K2 / K2t on operands as the package builds them (normalised weights, 1 / (deg + 1), alpha in [0.5, 1.5], normal g / h):
    every element within the derived fp32 bound of the fp64 reference."""
    from scdeepsort_amd import ops
    monkeypatch.setattr(ops, "TILED_MIN_WORK", None if route == "rowwave" else 1)
    g, Lf = float_case_graph(D)
    L = float_operands(g, Lf, D, D + 1)
    tp = None if route == "rowwave" else side(g, L, mode)[0].transposed().tile_plan(ops.tiled_block_rows(D))
    check_k2_float("K2" if route == "rowwave" else "K2t", g, L, mode, D, tp, acc=int(mode == "genes"))


@pytest.mark.parametrize("route", ["rowwave", "tiled"])
@pytest.mark.parametrize("D", FLOAT_D)
def test_k3_float_bound(D, route, monkeypatch):
    from scdeepsort_amd import ops
    monkeypatch.setattr(ops, "TILED_MIN_WORK", None if route == "rowwave" else 1)
    g, Lf = float_case_graph(D)
    L = float_operands(g, Lf, D, D + 2)
    tp = None if route == "rowwave" else g.gc.tile_plan(ops.tiled_block_rows(D))
    check_k3_float("K3" if route == "rowwave" else "K3t", g, L, D, tp)


@pytest.mark.parametrize("D", FLOAT_D)
@pytest.mark.parametrize("mode", ["cells", "plain"])
def test_seed_block_float_bound(mode, D):
    g, Lf = float_case_graph(D)
    L = float_operands(g, Lf, D, D + 3)
    check_block_float(g, L, mode, D, 64, D)


@pytest.mark.parametrize("route", ["rowwave", "tiled"])
@pytest.mark.parametrize("D", FLOAT_D)
@pytest.mark.parametrize("direction", ["cells", "genes"])
def test_forward_float_bound(direction, D, route, monkeypatch):
    from scdeepsort_amd import ops
    monkeypatch.setattr(ops, "TILED_MIN_WORK", None)
    g, Lf = float_case_graph(D)
    L = float_operands(g, Lf, D, D + 4)
    csr = fwd_side(g, L, direction)[0]
    check_fwd_float("K1" if route == "rowwave" else "K1t", g, L, direction, D,
                    "rowwave" if route == "rowwave" else csr.tile_plan(ops.tiled_block_rows(D)))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_backward_fuzz_against_fp64(seed, monkeypatch):
    """Random shape / density / width / tile geometry (hub column, empty row at random), every entry against the fp64 reference
    with the derived bound - not against the other route."""
    from scdeepsort_amd import ops
    monkeypatch.setattr(ops, "TILED_MIN_WORK", None)
    rng = np.random.default_rng(1000 + seed)
    for it in range(6):
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
        g, Lf = float_graph(expr, chunk=int(rng.choice([64, 256, 2048])))
        L = float_operands(g, Lf, D, int(rng.integers(1 << 30)))
        geom = GEOMS[int(rng.integers(5))]
        kb, loaders = BLOCK_ROWS[int(rng.integers(4))], int(rng.integers(2))
        print(f"fuzz seed={seed} draw={it} C={C} G={G} density={dens:.3f} D={D} geom={geom} kb={kb} L={loaders}")
        for mode in ("cells", "genes", "plain"):
            acc = int(rng.integers(2))
            check_k2_float("K2", g, L, mode, D, None, acc)
            check_k2_float("K2t", g, L, mode, D, tile_plan(side(g, L, mode)[0].transposed(), D, geom, kb, loaders, False), acc)
        check_k3_float("K3", g, L, D, None)
        check_k3_float("K3t", g, L, D, tile_plan(g.gc, D, geom, kb, loaders, False, strict=False))
        for mode in ("cells", "plain"):
            check_block_float(g, L, mode, D, int(rng.integers(1, 80)), it)
        for direction in ("cells", "genes"):
            check_fwd_float("K1", g, L, direction, D, "rowwave")
            check_fwd_float("K1t", g, L, direction, D, tile_plan(fwd_side(g, L, direction)[0], D, geom, kb, loaders, False, strict=False))
