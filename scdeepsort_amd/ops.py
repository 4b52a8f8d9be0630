"""Host-side operators of the hot path: thin wrappers over the C ABI (``include/wgnn.h``)
plus the ``torch.autograd.Function`` that stands where the reference calls

    nf.block_compute(i, self.message_func, fn.mean('m', 'neigh'), layer)   (models/gnn.py:65)

torch is used for device memory, streams and autograd bookkeeping only; all
aggregation arithmetic runs in the HIP kernels.  There is no CPU fallback: a
non-CUDA tensor or a missing ``libwgnn_hip.so`` raises ``WgnnError``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import DST_IS_GENE, NO_ALPHA, SRC_IS_GENE, WgnnError
from .graph import AggCsr, Plan, _ptr, _stream


def _require_cuda(*ts: Optional[torch.Tensor]) -> torch.device:
    dev = None
    for t in ts:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise WgnnError("wgnn operators run on the GPU only (tensor on %s); there is no CPU fallback" % t.device)
        dev = t.device
    return dev


def _rowmajor(t: torch.Tensor) -> torch.Tensor:
    if t.dim() != 2:
        raise ValueError("expected a 2-D feature matrix")
    if t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16:
        t = t.contiguous()
    return t


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return _lib.F32
    if t.dtype == torch.float16:
        return _lib.F16
    raise WgnnError(f"unsupported feature dtype {t.dtype}")


# Optional launch-level timing hook (bench.py): when set to a list, every K1 call appends
# (tag, start_event, end_event) recorded on the stream the kernels are enqueued on.
PROFILE = None
DEBUG_FLAGS = 0      # ablation switches of the tiled kernel (timing experiments only)
# K1 dispatch: passes with nnz*D above this go to the LDS-streamed kernel (None = always row-wave)
SAVE_NEIGH_SUM = True               # training: the forward of gene rows saves its raw neighbour sums (no K3 pass in backward)
SEED_BLOCK_MAX_CAP = 12_000_000     # B x longest row above which a seed batch's backward walks the full transposed graph instead
                                    # (sorting the padded block costs ~0.05 ms per million slots; the full K2t pass 1.2 ms at cfg3)
PAD_NARROW_TO_256 = False           # round-1 behaviour (hidden < 256 carried as 256 zero-padded columns); kept for A/B timing
# nnz * max(D, 128) above which the LDS-streamed kernels take a pass.  The tile kernel's time hardly depends on D (it is bound
# by per-edge instruction issue), the row-wave kernel's gathers scale with it: at BASELINE cfg2's 2.0 M edges a pass costs
# 60 / 59 us tiled against 62 / 71 us row-wave at D = 128 and 62 / 61 against 100 / 129 us at D = 200 (round 4,
# profiles/r04_issue_analysis.md §4) - rounds 1-3 used 5e8 (~2 M edges at D = 256), which left cfg2 and every hidden-200 graph of
# that size on the row-wave kernel.
TILED_MIN_WORK = int(__import__("os").environ.get("WGNN_TILED_MIN_WORK", 250_000_000))
SEED_FULL_PASS_MIN_FRAC = 0.2       # a seed set of at least this share of the rows of a tile-kernel operand runs the FULL LDS-streamed
                                    # pass and gathers its rows (row-wave K1 costs ~5x per edge: 6.2 vs 1.19 ms for all of cfg3)


def tiled_kernel_serves(csr: AggCsr, D: int) -> bool:
    """True when a FULL pass over ``csr`` at width ``D`` is dispatched to the LDS-streamed kernel (K1t)."""
    return (TILED_MIN_WORK is not None and D <= 256 and D % 4 == 0 and csr.nnz * max(D, 128) >= TILED_MIN_WORK
            and csr.ell_cnt is None)


def will_run_tiled(csr: AggCsr, D: int, n_seed_rows: Optional[int] = None) -> bool:
    """True when ``agg_fwd`` on f32 rows of width ``D`` (all rows, or a seed set of ``n_seed_rows`` rows) takes the
    LDS-streamed route - the one that honours ``src_scaled``."""
    return tiled_kernel_serves(csr, D) and (n_seed_rows is None or n_seed_rows >= SEED_FULL_PASS_MIN_FRAC * csr.n_rows)


class _Timed:
    """``with _Timed(dev, tag):`` records one (tag, start, end) HIP-event triple into ``PROFILE`` on the launch stream
    (a no-op when no profile is being collected)."""

    def __init__(self, dev, tag):
        self.dev, self.tag, self.ev = dev, tag, None

    def __enter__(self):
        if PROFILE is not None:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record(torch.cuda.current_stream(self.dev))
        return self

    def __exit__(self, *exc):
        if self.ev is not None and PROFILE is not None:
            self.ev[1].record(torch.cuda.current_stream(self.dev))
            PROFILE.append((self.tag, self.ev[0], self.ev[1]))
        return False


def _partials(plan: Plan, D: int, device) -> Optional[torch.Tensor]:
    return torch.empty(plan.n_partials * D, dtype=torch.float32, device=device) if plan.n_partials else None


def agg_fwd(csr: AggCsr, alpha: Optional[torch.Tensor], mode: int, self_idx: int,
            h_src: torch.Tensor, h_self: Optional[torch.Tensor], *, bias: Optional[torch.Tensor] = None,
            relu: bool = False, row_ids: Optional[torch.Tensor] = None, self_compact: bool = False,
            no_mean: bool = False, out_dtype: Optional[torch.dtype] = None,
            out: Optional[torch.Tensor] = None, neigh_sum: Optional[torch.Tensor] = None,
            src_scaled: Optional[torch.Tensor] = None, out_scale_alpha: bool = False) -> torch.Tensor:
    """K1 ``wgnn_agg_fwd``: weighted mean of in-neighbours incl. the implicit self-loop.  ``neigh_sum`` (f32 [n_out, D],
    contiguous) optionally receives the raw neighbour sum of every output row (saved by training for dalpha).
    ``src_scaled`` (SRC_IS_GENE only): ``alpha[s] * h_src[s]`` already formed (``linear_fwd(..., row_scale=alpha)`` or a
    gene pass run with ``out_scale_alpha``) - the LDS-streamed kernel then reads it in place of its own scale pass; the
    row-wave kernel ignores it (callers check ``will_run_tiled`` before handing over an ONLY-scaled table).
    ``out_scale_alpha`` (DST_IS_GENE): the finished gene rows are written multiplied by alpha[row]
    (WGNN_FLAG_OUT_SCALE_ALPHA) - the next layer's alpha-folded source table, no separate scale launch."""
    dev = _require_cuda(h_src, h_self, alpha, bias, csr.col)
    h_src = _rowmajor(h_src)
    D = h_src.shape[1]
    if D % 4:
        raise WgnnError(f"feature width {D} must be a multiple of 4")
    if out_scale_alpha and mode != DST_IS_GENE:
        raise WgnnError("out_scale_alpha is defined for gene rows (DST_IS_GENE) only")
    tiled_ok = (out is None and h_src.dtype == torch.float32 and (out_dtype in (None, torch.float32))
                and tiled_kernel_serves(csr, D))
    if tiled_ok and row_ids is None:
        return agg_fwd_tiled(csr, csr.tile_plan(tiled_block_rows(D)), alpha, mode, self_idx, h_src, h_self, bias=bias, relu=relu,
                             no_mean=no_mean, neigh_sum=neigh_sum, src_scaled=src_scaled, out_scale_alpha=out_scale_alpha)
    if (tiled_ok and neigh_sum is None and row_ids.shape[0] >= SEED_FULL_PASS_MIN_FRAC * csr.n_rows
            and (h_self is None or h_self.dtype == torch.float32)):
        # a LARGE seed set (predict.py:61-88: every test cell is a seed; fit's accuracy() over the training cells): one full
        # LDS-streamed pass over all rows, then the seeds' rows in seed order.  A compact self table (one row per seed slot)
        # is spread to row positions first; rows outside the seed set produce values nobody reads.
        idl = row_ids.to(device=dev, dtype=torch.long)
        if h_self is not None and self_compact:
            full_self = torch.empty((csr.n_rows, D), dtype=torch.float32, device=dev)
            full_self.index_copy_(0, idl, _rowmajor(h_self))
            h_self = full_self
        full = agg_fwd_tiled(csr, csr.tile_plan(tiled_block_rows(D)), alpha, mode, self_idx, h_src, h_self, bias=bias, relu=relu,
                             no_mean=no_mean, src_scaled=src_scaled, out_scale_alpha=out_scale_alpha)
        return full.index_select(0, idl)
    if src_scaled is not None and src_scaled.data_ptr() == h_src.data_ptr():
        raise WgnnError("an alpha-folded table without its unscaled original reached the row-wave kernel, which folds alpha "
                        "per edge itself (callers check ops.will_run_tiled first)")
    if h_self is not None:
        h_self = _rowmajor(h_self)
        if h_self.dtype != h_src.dtype or h_self.shape[1] != D:
            raise WgnnError("h_self must match h_src in dtype and width")
    if row_ids is not None:
        ids, plan = csr.subplan(row_ids)
        n_out = ids.shape[0]
    else:
        ids, plan, n_out = None, csr.plan, csr.n_rows
    out_dtype = out_dtype or h_src.dtype
    if out is None:
        out = torch.empty((n_out, D), dtype=out_dtype, device=dev)
    if n_out == 0:
        return out
    flags = (_lib.FLAG_RELU if relu else 0) | (_lib.FLAG_NO_MEAN if no_mean else 0) | \
            (_lib.FLAG_NO_SELF if h_self is None else 0) | (_lib.FLAG_SELF_COMPACT if self_compact else 0) | \
            (_lib.FLAG_OUT_SCALE_ALPHA if out_scale_alpha else 0)
    if alpha is not None:
        alpha = alpha.reshape(-1)
        if alpha.dtype != torch.float32 or not alpha.is_contiguous():
            alpha = alpha.float().contiguous()
    if bias is not None:
        bias = bias.float().contiguous()
    part = _partials(plan, D, dev)
    ev = None
    if PROFILE is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record(torch.cuda.current_stream(dev))
    _lib.run(dev, "wgnn_agg_fwd",
        _ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.val), _ptr(alpha), mode, self_idx,
        _ptr(h_src), h_src.stride(0), _ptr(h_self), h_self.stride(0) if h_self is not None else 0,
        _ptr(ids), _ptr(csr.inv_deg), _ptr(bias), _ptr(out), out.stride(0), _ptr(neigh_sum), n_out, D,
        _dtype_code(h_src), _dtype_code(out), flags,
        _ptr(plan.items), plan.n_items, _ptr(plan.long_rows) if plan.n_long else None, plan.n_long,
        _ptr(part), plan.n_partials, _stream(dev))
    if ev is not None:
        ev[1].record(torch.cuda.current_stream(dev))
        PROFILE.append((("rows", csr.n_rows, "cols", csr.n_cols, "nnz", csr.nnz, "D", D, "mode", mode,
                         "kernel", "agg_main"), ev[0], ev[1]))
    return out


def agg_bwd_src(csr: AggCsr, alpha: Optional[torch.Tensor], mode: int, g: torch.Tensor,
                h_src: Optional[torch.Tensor], dalpha: Optional[torch.Tensor] = None,
                dh_src: Optional[torch.Tensor] = None, accumulate: bool = False,
                dst_scale: Optional[torch.Tensor] = None, prescaled: bool = False, tplan=None) -> torch.Tensor:
    """K2 ``wgnn_agg_bwd_src``: gradient w.r.t. the gathered rows (transposed SpMM);
    for SRC_IS_GENE also writes dalpha[0:n_src] = <h_src[s], T[s]>.  ``dst_scale`` replaces the per-destination
    factor 1/(deg+1) (``csr.inv_deg``), e.g. ones for the backward of a plain weighted sum.  ``prescaled``: ``g`` already
    carries the per-destination factors (``agg_bwd_prepare``) - LDS-streamed route only.  ``tplan``: a tile plan of
    ``csr.transposed()`` (``graph.build_tile_plan``) - the LDS-streamed K2t then runs over it, whatever the dispatch rule
    says (default: the rule decides, and K2t takes the cached heuristic plan)."""
    dev = _require_cuda(g, h_src, alpha)
    inv_deg = csr.inv_deg if dst_scale is None else dst_scale.float().contiguous()
    t = csr.transposed()
    g = _rowmajor(g.float())
    D = g.shape[1]
    if g.shape[0] != csr.n_rows:
        raise WgnnError("g must have one row per destination row of the CSR")
    if dh_src is None:
        dh_src = torch.empty((t.n_rows, D), dtype=torch.float32, device=dev)
        accumulate = False
    if h_src is not None:
        h_src = _rowmajor(h_src.float())
    if alpha is not None:
        alpha = alpha.reshape(-1).float().contiguous()
    if tplan is not None or tiled_kernel_serves(csr, D):
        # K2t: LDS-streamed kernel over the transposed structure; per-destination factors folded into g once
        tp = tplan if tplan is not None else t.tile_plan(tiled_block_rows(D))
        g = g.contiguous()
        if prescaled:
            scale, scratch = None, None
        else:
            scale = (inv_deg if mode != DST_IS_GENE else inv_deg * alpha[: csr.n_rows]).contiguous()
            scratch = torch.empty_like(g)
        part = torch.empty(tp.n_partials * D, dtype=torch.float32, device=dev) if tp.n_partials else None
        n_long = tp.long_rows.shape[0]
        with _Timed(dev, ("rows", t.n_rows, "cols", t.n_cols, "nnz", t.nnz, "D", D, "mode", mode, "kernel",
                          "agg_tiled_tall<EPI_BWD_SRC>" if tp.geom.tall else "agg_tiled_flat4<EPI_BWD_SRC>")):
            _lib.run(dev, "wgnn_agg_bwd_src_tiled",
                _ptr(alpha), mode, _ptr(scale), _ptr(g), g.shape[0], _ptr(scratch),
                _ptr(h_src), h_src.stride(0) if h_src is not None else 0, _ptr(dh_src), dh_src.stride(0), _ptr(dalpha),
                int(accumulate), t.n_rows, D, _ptr(tp.entries), _ptr(tp.seg_ptr), tp.nblk_max, tp.block_rows_arg,
                _ptr(tp.items), _ptr(tp.hdr), tp.n_tiles, _ptr(tp.long_rows) if n_long else None, n_long,
                _ptr(part), tp.n_partials, _stream(dev))
        return dh_src
    if prescaled:
        raise WgnnError("prescaled gradient rows are an input of the LDS-streamed K2t only")
    part = _partials(t.plan, D, dev)
    _lib.run(dev, "wgnn_agg_bwd_src",
        _ptr(t.rowptr), _ptr(t.col), _ptr(t.val), _ptr(alpha), mode, _ptr(inv_deg),
        _ptr(g), g.stride(0), _ptr(h_src), h_src.stride(0) if h_src is not None else 0,
        _ptr(dh_src), dh_src.stride(0), _ptr(dalpha), int(accumulate), t.n_rows, D,
        _ptr(t.plan.items), t.plan.n_items, _ptr(t.plan.long_rows) if t.plan.n_long else None, t.plan.n_long,
        _ptr(part), t.plan.n_partials, _stream(dev))
    return dh_src


def agg_bwd_src_block(csr: AggCsr, row_ids: torch.Tensor, alpha: Optional[torch.Tensor], mode: int, g: torch.Tensor,
                      inv_rows: torch.Tensor, h_src: Optional[torch.Tensor], dalpha: Optional[torch.Tensor]) -> torch.Tensor:
    """K2 for ONE seed batch: ``g`` holds one gradient row per seed SLOT ([B, D]); the source-major structure of the
    batch's in-edges comes from ``AggCsr.seed_block_transposed`` (device-built, static shapes).  Writes every source
    row of ``dh_src`` ([n_cols, D]; zero where the batch gathers nothing) and, for SRC_IS_GENE, dalpha[0:n_cols]."""
    dev = _require_cuda(g, h_src, alpha)
    ids32 = row_ids.to(device=dev, dtype=torch.int32).contiguous()
    g = _rowmajor(g.float())
    D = g.shape[1]
    if g.shape[0] != ids32.shape[0]:
        raise WgnnError("g must have one row per seed")
    dh_src = torch.empty((csr.n_cols, D), dtype=torch.float32, device=dev)
    if ids32.shape[0] == 0:
        return dh_src.zero_()
    t_rowptr, t_slot, t_val, items = csr.seed_block_transposed(ids32)
    if h_src is not None:
        h_src = _rowmajor(h_src.float())
    if alpha is not None:
        alpha = alpha.reshape(-1).float().contiguous()
    _lib.run(dev, "wgnn_agg_bwd_src",
        _ptr(t_rowptr), _ptr(t_slot), _ptr(t_val), _ptr(alpha), mode, _ptr(inv_rows.float().contiguous()),
        _ptr(g), g.stride(0), _ptr(h_src), h_src.stride(0) if h_src is not None else 0,
        _ptr(dh_src), dh_src.stride(0), _ptr(dalpha), 0, csr.n_cols, D,
        _ptr(items), items.shape[0], None, 0, None, 0, _stream(dev))
    return dh_src


def agg_bwd_alpha(csr: AggCsr, g: torch.Tensor, h_src: torch.Tensor, h_self: Optional[torch.Tensor],
                  row_ids: Optional[torch.Tensor] = None, self_compact: bool = False, tplan=None):
    """K3 ``wgnn_agg_bwd_alpha``: per-row alpha gradients for DST_IS_GENE rows and the self-loop scalar.  ``tplan``: a tile
    plan of ``csr`` (``graph.build_tile_plan``; all rows only) - the LDS-streamed K3t then runs over it, whatever the
    dispatch rule says."""
    dev = _require_cuda(g, h_src, h_self)
    g = _rowmajor(g.float()); h_src = _rowmajor(h_src.float())
    D = g.shape[1]
    if row_ids is not None:
        ids, plan = csr.subplan(row_ids)
        n_out = ids.shape[0]
    else:
        ids, plan, n_out = None, csr.plan, csr.n_rows
    if h_self is not None:
        h_self = _rowmajor(h_self.float())
    d_row = torch.empty(n_out, dtype=torch.float32, device=dev)
    d_self = torch.empty(n_out, dtype=torch.float32, device=dev) if h_self is not None else None
    if tplan is not None and row_ids is not None:
        raise WgnnError("a tile plan covers all rows: K3t takes no row_ids")
    if row_ids is None and (tplan is not None or tiled_kernel_serves(csr, D)):
        tp = tplan if tplan is not None else csr.tile_plan(tiled_block_rows(D))   # K3t
        h_src = h_src.contiguous()
        part = torch.empty(tp.n_partials * D, dtype=torch.float32, device=dev) if tp.n_partials else None
        n_long = tp.long_rows.shape[0]
        _lib.run(dev, "wgnn_agg_bwd_alpha_tiled",
            _ptr(csr.inv_deg), _ptr(g), g.stride(0), _ptr(h_src), _ptr(h_self),
            h_self.stride(0) if h_self is not None else 0, _ptr(d_row), _ptr(d_self), n_out, D,
            _ptr(tp.entries), _ptr(tp.seg_ptr), tp.nblk_max, tp.block_rows_arg, _ptr(tp.items), _ptr(tp.hdr), tp.n_tiles,
            _ptr(tp.long_rows) if n_long else None, n_long, _ptr(part), tp.n_partials, _stream(dev))
        return d_row, d_self
    part = _partials(plan, D, dev)
    _lib.run(dev, "wgnn_agg_bwd_alpha",
        _ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.val), _ptr(csr.inv_deg), _ptr(ids),
        _ptr(g), g.stride(0), _ptr(h_src), h_src.stride(0), _ptr(h_self), h_self.stride(0) if h_self is not None else 0,
        _ptr(d_row), _ptr(d_self), n_out, D, _lib.FLAG_SELF_COMPACT if self_compact else 0,
        _ptr(plan.items), plan.n_items, _ptr(plan.long_rows) if plan.n_long else None, plan.n_long,
        _ptr(part), plan.n_partials, _stream(dev))
    return d_row, d_self


NARROW_LDS_ROWS = True       # round 4: LDS rows of the flat tile kernel are 256 / 512 / 1024 bytes by width (False: 78-row blocks for
                             # every D, the round-2/3 geometry - the kernel itself always packs; kept for A/B timing)


def flat_lds_row_bytes(D: int) -> int:
    """LDS row stride of ``agg_tiled_flat4`` (csrc/wgnn_tiled.hip::flat_lds_row_bytes): the power of two covering a row."""
    return 256 if D <= 64 else (512 if D <= 128 else 1024)


FUSED_BWD_GLUE = True        # round 4: one wgnn_agg_bwd_prepare launch instead of the ~8 framework elementwise / reduce launches between
                             # the upstream gradient and K2t (A/B switch)


def agg_bwd_prepare(gout: torch.Tensor, out: Optional[torch.Tensor], inv_deg: Optional[torch.Tensor],
                    alpha: Optional[torch.Tensor], mode: int, self_idx: int, *, want_scaled: bool = True,
                    h_self: Optional[torch.Tensor] = None, want_dh_self: bool = False,
                    neigh_sum: Optional[torch.Tensor] = None, want_dself: bool = False, want_dbias: bool = False) -> dict:
    """``wgnn_agg_bwd_prepare``: from the upstream gradient ``gout`` [R, D] of one aggregation pass (and the saved forward
    output ``out`` for the ReLU mask) in ONE read: ``g_scaled`` (K2t's pre-scaled source table), ``dh_self``, ``dalpha_row``
    (needs ``neigh_sum``), ``dself_row`` (needs ``h_self``) and ``dbias`` - whichever are asked for."""
    dev = _require_cuda(gout, out, inv_deg, alpha, h_self, neigh_sum)
    gout = _rowmajor(gout.float())
    R, D = gout.shape
    if out is not None:
        out = _rowmajor(out.float())
    if h_self is not None:
        h_self = _rowmajor(h_self.float())
    if neigh_sum is not None:
        neigh_sum = neigh_sum.float().contiguous()
    if alpha is not None:
        alpha = alpha.reshape(-1).float().contiguous()
    if inv_deg is not None:
        inv_deg = inv_deg.float().contiguous()
    res = {"g_scaled": torch.empty((R, D), dtype=torch.float32, device=dev) if want_scaled else None,
           "dh_self": torch.empty((R, D), dtype=torch.float32, device=dev) if want_dh_self else None,
           "dalpha_row": torch.empty(R, dtype=torch.float32, device=dev) if neigh_sum is not None else None,
           "dself_row": torch.empty(R, dtype=torch.float32, device=dev) if (want_dself and h_self is not None) else None,
           "dbias": torch.empty(D, dtype=torch.float32, device=dev) if want_dbias else None}
    ws, nf = None, C.c_int64(0)
    if want_dbias:
        _lib.check(_lib.lib().wgnn_agg_bwd_prepare_workspace(R, D, C.addressof(nf)), "wgnn_agg_bwd_prepare_workspace")
        ws = torch.empty(max(1, nf.value), dtype=torch.float32, device=dev)
    need_self = res["dh_self"] is not None or res["dself_row"] is not None
    _lib.run(dev, "wgnn_agg_bwd_prepare", _ptr(gout), gout.stride(0), _ptr(out), out.stride(0) if out is not None else 0,
             _ptr(inv_deg), _ptr(alpha), mode, self_idx, _ptr(res["g_scaled"]),
             _ptr(h_self) if need_self else None, h_self.stride(0) if (need_self and h_self is not None) else 0,
             _ptr(res["dh_self"]), D, _ptr(neigh_sum), _ptr(res["dalpha_row"]), _ptr(res["dself_row"]), _ptr(res["dbias"]),
             R, D, _ptr(ws), nf.value, _stream(dev))
    return res


class _CrossEntropySum(torch.autograd.Function):
    """``CrossEntropyLoss(reduction='sum')`` (train.py:36) through ``wgnn_ce_sum_fwd_bwd``: loss and softmax - onehot from one
    read of the logits (the framework's log_softmax / nll_loss pair costs ~0.2 ms per step at 1e5 rows x 16 classes)."""

    @staticmethod
    def forward(ctx, logits, labels):
        dev = _require_cuda(logits, labels)
        x = logits.float()
        if x.stride(1) != 1:
            x = x.contiguous()
        y = labels.to(torch.int64).contiguous()
        n, c = x.shape
        nf = C.c_int64(0)
        _lib.check(_lib.lib().wgnn_ce_sum_workspace(n, C.addressof(nf)), "wgnn_ce_sum_workspace")
        ws = torch.empty(max(1, nf.value), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        d = torch.empty((n, c), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        _lib.run(dev, "wgnn_ce_sum_fwd_bwd", _ptr(x), x.stride(0), _ptr(y), n, c, _ptr(loss), _ptr(d), c, _ptr(ws), nf.value,
                 _stream(dev))
        ctx.save_for_backward(d)
        ctx.in_dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        return (d * g).to(ctx.in_dtype), None


def cross_entropy_sum(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """``F.cross_entropy(logits, labels, reduction='sum')`` on the GPU path (2-D logits, class-index labels)."""
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        raise ValueError("cross_entropy_sum: logits [n, classes], labels [n]")
    if logits.shape[0] == 0:
        return logits.sum() * 0.0
    return _CrossEntropySum.apply(logits, labels)


def tiled_block_rows(D: int) -> int:
    """Source rows per LDS block of the tile kernels: two buffers + the 4 KiB of per-wave weight strips fill the 160 KiB of
    a CU (measured best at D = 256: 78 x 1 KiB x 2).  Narrower rows pack closer (row stride 512 B at D <= 128, 256 B at
    D <= 64): 156 / 255 rows per block - half the per-block barriers and pipeline warm-ups per edge, which measured
    NEUTRAL (cfg2 60.9 / 58.8 -> 60.0 / 59.5 us per pass, cfg3 at D = 128 1.050 / 0.956 -> 1.039 / 0.972 ms: the kernel is
    bound by per-edge issue latency, not by its barriers).  An entry names its source row inside a block with 8 bits, so a
    block holds at most 255 rows."""
    if not NARROW_LDS_ROWS:
        return 78
    return min(255, (160 * 1024 - 4096) // 2 // flat_lds_row_bytes(D))


def agg_fwd_tiled(csr: AggCsr, tplan, alpha: Optional[torch.Tensor], mode: int, self_idx: int,
                  h_src: torch.Tensor, h_self: Optional[torch.Tensor], *, bias: Optional[torch.Tensor] = None,
                  relu: bool = False, no_mean: bool = False, neigh_sum: Optional[torch.Tensor] = None,
                  src_scaled: Optional[torch.Tensor] = None, out_scale_alpha: bool = False) -> torch.Tensor:
    """K1t ``wgnn_agg_fwd_tiled``: same result as :func:`agg_fwd`, source table streamed through LDS.  ``src_scaled``: the
    alpha-folded source table (SRC_IS_GENE) when the caller already has it (WGNN_FLAG_SRC_PRESCALED)."""
    dev = _require_cuda(h_src, h_self, alpha, bias, csr.col)
    if h_src.dtype != torch.float32:
        raise WgnnError("tiled kernel is f32 only")
    h_src = h_src.contiguous()
    D = h_src.shape[1]
    if h_self is not None:
        h_self = _rowmajor(h_self)
    out = torch.empty((csr.n_rows, D), dtype=torch.float32, device=dev)
    flags = (_lib.FLAG_RELU if relu else 0) | (_lib.FLAG_NO_MEAN if no_mean else 0) | \
            (_lib.FLAG_NO_SELF if h_self is None else 0) | (_lib.FLAG_OUT_SCALE_ALPHA if out_scale_alpha else 0) | DEBUG_FLAGS
    if alpha is not None:
        alpha = alpha.reshape(-1)
        if alpha.dtype != torch.float32 or not alpha.is_contiguous():
            alpha = alpha.float().contiguous()
    if bias is not None:
        bias = bias.float().contiguous()
    part = torch.empty(tplan.n_partials * D, dtype=torch.float32, device=dev) if tplan.n_partials else None
    ev = None
    if PROFILE is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record(torch.cuda.current_stream(dev))
    n_long = tplan.long_rows.shape[0]
    scratch = None
    if mode == SRC_IS_GENE:
        if src_scaled is not None and src_scaled.shape == h_src.shape and src_scaled.dtype == torch.float32:
            h_src, flags = src_scaled.contiguous(), flags | _lib.FLAG_SRC_PRESCALED
        else:
            scratch = torch.empty_like(h_src)
    _lib.run(dev, "wgnn_agg_fwd_tiled",
        _ptr(csr.rowptr), _ptr(alpha), mode, self_idx,
        _ptr(h_src), h_src.shape[0], _ptr(scratch), _ptr(h_self), h_self.stride(0) if h_self is not None else 0,
        None, _ptr(csr.inv_deg), _ptr(bias), _ptr(out), out.stride(0), _ptr(neigh_sum), csr.n_rows, D, flags,
        _ptr(tplan.entries), _ptr(tplan.seg_ptr), tplan.nblk_max, tplan.block_rows_arg, _ptr(tplan.items), _ptr(tplan.hdr), tplan.n_tiles,
        _ptr(tplan.long_rows) if n_long else None, n_long, _ptr(part), tplan.n_partials, _stream(dev))
    if ev is not None:
        ev[1].record(torch.cuda.current_stream(dev))
        PROFILE.append((("rows", csr.n_rows, "cols", csr.n_cols, "nnz", csr.nnz, "D", D, "mode", mode,
                         "kernel", "agg_tiled_tall" if tplan.geom.tall else "agg_tiled_flat4"), ev[0], ev[1]))
    return out


class WeightedMeanAggregate(torch.autograd.Function):
    """Differentiable ``block_compute(message_func, fn.mean)`` (+ fused bias / ReLU).

    forward  = K1;  backward = K2 (dh_src, dalpha[genes] for gene->cell edges),
    K3 (dalpha for cell->gene edges + self-loop scalar) and a row scale for dh_self.
    Gradients follow train.py:84's autograd through gnn.py:47-56,65:
      dh[u]     = sum_{e=(u->v)} alpha[k(e)] w_e g[v]/deg(v)
      dalpha[k] = sum_{e:k(e)=k} w_e <g[v], h[u]>/deg(v)           (w has no grad)
    """

    @staticmethod
    def forward(ctx, h_src, h_self, alpha, bias, csr: AggCsr, mode: int, self_idx: int, relu: bool,
                row_ids, self_compact: bool):
        # gene rows (DST_IS_GENE) in training: keep the raw neighbour sum S[r]; dalpha[r] = inv_deg[r]*<g[r], S[r]> is then
        # a row dot product in backward instead of a second pass over all edges (K3)
        nsum = None
        if (mode == DST_IS_GENE and row_ids is None and ctx.needs_input_grad[2] and h_src.dtype == torch.float32
                and SAVE_NEIGH_SUM):
            nsum = torch.empty((csr.n_rows, h_src.shape[1]), dtype=torch.float32, device=h_src.device)
        out = agg_fwd(csr, alpha, mode, self_idx, h_src, h_self, bias=bias, relu=relu, row_ids=row_ids,
                      self_compact=self_compact, neigh_sum=nsum)
        ctx.csr, ctx.mode, ctx.self_idx, ctx.relu, ctx.self_compact = csr, mode, self_idx, relu, self_compact
        ctx.has_bias = bias is not None
        ctx.save_for_backward(h_src, h_self, alpha, out if relu else None, row_ids, nsum)
        return out

    @staticmethod
    def backward(ctx, gout):
        h_src, h_self, alpha, out, row_ids, nsum = ctx.saved_tensors
        csr: AggCsr = ctx.csr
        mode, self_idx = ctx.mode, ctx.self_idx
        Dg = gout.shape[1]
        if (FUSED_BWD_GLUE and row_ids is None and gout.is_cuda and Dg % 4 == 0 and tiled_kernel_serves(csr, Dg)
                and (mode != DST_IS_GENE or nsum is not None or not ctx.needs_input_grad[2])
                and (h_self is None or h_self.dtype == torch.float32) and h_src.dtype == torch.float32):
            # full pass on the LDS-streamed route: ONE fused launch turns the upstream gradient into K2t's pre-scaled source
            # table, the self-row gradient, the alpha row dots and the bias gradient
            a = alpha.reshape(-1)
            want_dalpha = ctx.needs_input_grad[2] and mode != NO_ALPHA
            want_src_dalpha = want_dalpha and mode == SRC_IS_GENE
            need_k2 = ctx.needs_input_grad[0] or want_src_dalpha
            res = agg_bwd_prepare(gout, out if ctx.relu else None, csr.inv_deg, a if mode != NO_ALPHA else None, mode, self_idx,
                                  want_scaled=need_k2, h_self=h_self, want_dh_self=h_self is not None and ctx.needs_input_grad[1],
                                  neigh_sum=nsum if (want_dalpha and mode == DST_IS_GENE) else None,
                                  want_dself=want_dalpha and h_self is not None, want_dbias=ctx.has_bias)
            dalpha = torch.zeros_like(a) if ctx.needs_input_grad[2] else None
            dh_src = None
            if need_k2:
                dh_src = agg_bwd_src(csr, a if mode != NO_ALPHA else None, mode, res["g_scaled"], h_src if want_src_dalpha else None,
                                     dalpha if want_src_dalpha else None, prescaled=True)
                dh_src = dh_src.to(h_src.dtype) if ctx.needs_input_grad[0] else None
            if dalpha is not None:
                if res["dalpha_row"] is not None:
                    dalpha[: csr.n_rows] += res["dalpha_row"]
                if res["dself_row"] is not None:
                    dalpha[self_idx] += res["dself_row"].sum()
                dalpha = dalpha.reshape(alpha.shape)
            return dh_src, res["dh_self"], dalpha, res["dbias"], None, None, None, None, None, None
        g = gout.float()
        if ctx.relu:
            g = g * (out > 0)
        g = g.contiguous()
        dbias = g.sum(0) if ctx.has_bias else None
        D = g.shape[1]
        dev = g.device
        a = alpha.reshape(-1)
        rows = row_ids.long() if row_ids is not None else None
        inv_rows = csr.inv_deg if rows is None else csr.inv_deg[rows]
        dalpha = torch.zeros_like(a) if ctx.needs_input_grad[2] else None
        need_src = ctx.needs_input_grad[0]
        want_src_dalpha = dalpha is not None and mode == SRC_IS_GENE
        dh_src = None
        if need_src or want_src_dalpha:
            if rows is None:
                dh_src = agg_bwd_src(csr, a if mode != NO_ALPHA else None, mode, g, h_src if want_src_dalpha else None, dalpha)
            elif mode != DST_IS_GENE and rows.shape[0] * max(1, csr.max_row_nnz) <= SEED_BLOCK_MAX_CAP:
                # seed mini-batch (train.py:71-87): K2 over the source-major view of just the batch's in-edges, built on
                # the device with static shapes - no [n_rows, D] zero-padded gradient, no pass over the whole graph, no
                # host synchronisation.  Repeated seeds are separate slots, so their gradients add up.
                dh_src = agg_bwd_src_block(csr, row_ids, a if mode != NO_ALPHA else None, mode, g, inv_rows,
                                           h_src if want_src_dalpha else None, dalpha)
            else:                                       # gene rows as a subset (not produced by GNN) or a "batch" of most of the
                                                        # graph (block capacity B x longest row too large): generic route
                g_full = torch.zeros((csr.n_rows, D), dtype=torch.float32, device=dev).index_add_(0, rows, g)
                dh_src = agg_bwd_src(csr, a if mode != NO_ALPHA else None, mode, g_full, h_src if want_src_dalpha else None, dalpha)
            dh_src = dh_src.to(h_src.dtype)
        dh_self = None
        hs_rows = None
        if h_self is not None:
            hs_rows = h_self if (rows is None or ctx.self_compact) else h_self[rows]
            coef = (a[self_idx] if mode != NO_ALPHA else 1.0) * inv_rows
            if ctx.needs_input_grad[1]:
                d = (g * coef.unsqueeze(1)).to(h_self.dtype)
                if rows is None or ctx.self_compact:
                    dh_self = d
                else:
                    dh_self = torch.zeros_like(h_self).index_add_(0, rows, d)      # a repeated seed contributes twice
        if dalpha is not None and mode != NO_ALPHA:
            if mode == DST_IS_GENE and nsum is not None:
                dalpha[: csr.n_rows] += (g * nsum).sum(1) * inv_rows
                if hs_rows is not None:
                    dalpha[self_idx] += ((g * hs_rows.float()).sum(1) * inv_rows).sum()
            elif mode == DST_IS_GENE:
                d_row, d_self = agg_bwd_alpha(csr, g, h_src, hs_rows, row_ids, self_compact=True if rows is not None else False)
                if rows is None:
                    dalpha[: csr.n_rows] += d_row
                else:
                    dalpha.index_add_(0, rows, d_row)
                if d_self is not None:
                    dalpha[self_idx] += d_self.sum()
            elif hs_rows is not None:
                dalpha[self_idx] += ((g * hs_rows.float()).sum(1) * inv_rows).sum()
        if dalpha is not None:
            dalpha = dalpha.reshape(alpha.shape)
        return dh_src, dh_self, dalpha, dbias, None, None, None, None, None, None


def weighted_mean_aggregate(csr: AggCsr, alpha: torch.Tensor, mode: int, self_idx: int, h_src: torch.Tensor,
                            h_self: Optional[torch.Tensor], bias: Optional[torch.Tensor] = None, relu: bool = False,
                            row_ids: Optional[torch.Tensor] = None, self_compact: bool = False,
                            src_scaled: Optional[torch.Tensor] = None, out_scale_alpha: bool = False) -> torch.Tensor:
    """Differentiable K1 (+ fused bias / ReLU).  ``src_scaled``: the caller's alpha-folded source table; ``out_scale_alpha``:
    gene rows written alpha-folded for the next layer (see ``agg_fwd``) - both only when nothing is recorded for backward
    (they are functions of alpha that autograd does not see)."""
    if out_scale_alpha and torch.is_grad_enabled():
        raise WgnnError("out_scale_alpha is an inference-path fusion: not differentiable")
    if (src_scaled is not None or out_scale_alpha) and not torch.is_grad_enabled():
        return agg_fwd(csr, alpha, mode, self_idx, h_src, h_self, bias=bias, relu=relu, row_ids=row_ids,
                       self_compact=self_compact, src_scaled=src_scaled, out_scale_alpha=out_scale_alpha)
    return WeightedMeanAggregate.apply(h_src, h_self, alpha, bias, csr, mode, self_idx, relu, row_ids, self_compact)


class _WeightedSum(torch.autograd.Function):
    """out = A @ h_src (plain weighted sum: NO_ALPHA, no mean, no self-loop) - the per-shard partial of the
    genes<-cells pass.  backward: dh_src = A^T g (K2 over the transposed structure, unit column scale)."""

    @staticmethod
    def forward(ctx, h_src, csr: AggCsr):
        ctx.csr = csr
        return agg_fwd(csr, None, NO_ALPHA, 0, h_src, None, no_mean=True)

    @staticmethod
    def backward(ctx, g):
        csr: AggCsr = ctx.csr
        ones = getattr(csr, "_ones", None)
        if ones is None or ones.shape[0] != csr.n_rows:
            ones = torch.ones(csr.n_rows, dtype=torch.float32, device=g.device)
            csr._ones = ones
        return agg_bwd_src(csr, None, NO_ALPHA, g, None, dst_scale=ones), None      # plain A^T g: unit factor


def weighted_sum(csr: AggCsr, h_src: torch.Tensor) -> torch.Tensor:
    return _WeightedSum.apply(h_src, csr)


# ------------------------------------------------------------------------------------------------
# dense half of a layer through the C ABI (fp32 matrix cores) - see csrc/wgnn_linear.hip
# ------------------------------------------------------------------------------------------------
# GNN's projections on the no-grad path: which of them run through wgnn_linear_fwd_ex instead of the library GEMM
#   "auto"  - fp16-stored inputs (never materialised in fp32) and shapes where the kernel measured faster than hipBLASLt
#             (>= 50k rows, K >= 384: 215 vs 231 us on 100k x 400 x 256, profiles/r03_kernel_stats_*.txt);
#   "always" / "never" - A/B switches.
# WGNN_LINEAR_DUAL: also produce the gene table P_g together with alpha * P_g (one kernel, no scale_rows launch).  Off by
# default: on the 20k-row gene projections the 128 x 128-tile kernel runs 69 us against the library's 31 us + 8 us of
# scale_rows (314 tiles = one thin round over 256 CUs), so the fusion costs more than it saves at cfg3.
WGNN_LINEAR = __import__("os").environ.get("WGNN_LINEAR", "auto")
WGNN_LINEAR_DUAL = __import__("os").environ.get("WGNN_LINEAR_DUAL", "0") == "1"
WGNN_LINEAR_MIN_ROWS, WGNN_LINEAR_MIN_K = 50_000, 384


def use_wgnn_linear(x: torch.Tensor, weight: torch.Tensor, dual: bool = False) -> bool:
    """Routing rule of the model's no-grad projections (see WGNN_LINEAR)."""
    if WGNN_LINEAR == "never" or not x.is_cuda or x.dim() != 2 or x.shape[1] % 4 or torch.is_grad_enabled() and (
            x.requires_grad or weight.requires_grad):
        return False
    if weight.dtype != torch.float32:          # wgnn_linear_fwd computes and returns fp32: a .half() / .bfloat16() model keeps
        return False                           # F.linear's "output in the parameter dtype"
    if dual:
        return WGNN_LINEAR_DUAL
    if WGNN_LINEAR == "always":
        return True
    if x.dtype == torch.float16:
        return True                            # fp16-stored rows: widened in the kernel's loader, never materialised in fp32
    from . import tuning
    if tuning.active():
        # with the tracked per-shape picks loaded the LIBRARY wins the one fp32 shape this kernel used to take: 155 us (tuned
        # rocBLAS pick) vs 207 us here vs 232 us (the libraries' own heuristic) on 100k x 400 x 256 (round 4, scratch/tune_gemms.py)
        return False
    return x.shape[0] >= WGNN_LINEAR_MIN_ROWS and x.shape[1] >= WGNN_LINEAR_MIN_K


def linear_fwd(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False,
               row_scale: Optional[torch.Tensor] = None, tile_rows: Optional[int] = None):
    """``act(x @ weight.T + bias)`` with ``wgnn_linear_fwd_ex`` (v_mfma_f32_32x32x2_f32, exact fp32).  ``x`` may be stored
    in fp16 (widened in registers, no fp32 copy).  With ``row_scale`` ([M]) returns ``(out, row_scale[:, None] * out)``,
    both written by the one kernel.  ``tile_rows`` (64 | 128) overrides the kernel's own choice of tile height (timing
    experiments).  Inference helper: no autograd (training keeps torch's Linear, whose backward is a
    library GEMM as well)."""
    dev = _require_cuda(x, weight, bias, row_scale)
    if x.dtype not in (torch.float32, torch.float16):
        x = x.float()
    x = _rowmajor(x) if x.dtype == torch.float32 else (x if x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 8 == 0
                                                       else x.contiguous())
    weight = _rowmajor(weight.float())
    M, K = x.shape
    N = weight.shape[0]
    if weight.shape[1] != K:
        raise WgnnError("x and weight disagree on K")
    if K % 4:
        raise WgnnError(f"K = {K} must be a multiple of 4")
    out = torch.empty((M, N), dtype=torch.float32, device=dev)
    out2 = None
    if row_scale is not None:
        row_scale = row_scale.reshape(-1).float().contiguous()
        if row_scale.shape[0] < M:
            raise WgnnError("row_scale needs one entry per row of x")
        out2 = torch.empty((M, N), dtype=torch.float32, device=dev)
    if bias is not None:
        bias = bias.float().contiguous()
    _lib.run(dev, "wgnn_linear_fwd_ex", _ptr(x), _dtype_code(x), x.stride(0), _ptr(weight), weight.stride(0), _ptr(bias),
             _ptr(out), out.stride(0), _ptr(row_scale), _ptr(out2), N if out2 is not None else 0, M, N, K,
             (_lib.FLAG_RELU if relu else 0) | {None: 0, 64: 1 << 16, 128: 1 << 17}[tile_rows], _stream(dev))
    return out if out2 is None else (out, out2)


# Layer 1's genes<-cells pass served from the graph's cached feature sum (graph.CellGeneGraph.feature_sum) where a caller
# asks for it (sharded.ShardedWgnn from its second forward over the same features, api.fit's accuracy());
# WGNN_FEATURE_SUM_CACHE=0 switches it off everywhere (A/B timing).
FEATURE_SUM_CACHE = __import__("os").environ.get("WGNN_FEATURE_SUM_CACHE", "1") != "0"


def mix_coeffs(alpha: torch.Tensor, self_idx: int, inv_deg: torch.Tensor):
    """``(alpha[:n] * inv_deg, alpha[self_idx] * inv_deg)`` in one launch (``wgnn_mix_coeffs``): the row coefficients of
    :func:`linear_mix_fwd` for gene rows."""
    dev = _require_cuda(alpha, inv_deg)
    alpha = alpha.detach().reshape(-1).float().contiguous()
    inv_deg = inv_deg.reshape(-1).float().contiguous()
    n = inv_deg.shape[0]
    if alpha.shape[0] < n or not 0 <= self_idx < alpha.shape[0]:
        raise WgnnError("mix_coeffs: alpha needs one entry per row and one at self_idx")
    c = torch.empty((2, n), dtype=torch.float32, device=dev)
    _lib.run(dev, "wgnn_mix_coeffs", _ptr(alpha), self_idx, _ptr(inv_deg), _ptr(c[0]), _ptr(c[1]), n, _stream(dev))
    return c[0], c[1]


def linear_mix_fwd(x1: torch.Tensor, c1: torch.Tensor, x2: torch.Tensor, c2: torch.Tensor, weight: torch.Tensor,
                   bias: Optional[torch.Tensor] = None, relu: bool = False, row_scale: Optional[torch.Tensor] = None,
                   want_out: bool = True, tile_rows: Optional[int] = None, out: Optional[torch.Tensor] = None,
                   out_scaled: Optional[torch.Tensor] = None):
    """``act(a @ weight.T + bias)`` with ``a[m, k] = fmaf(c2[m], x2[m, k], c1[m] * x1[m, k])`` formed in the GEMM's loader
    (``wgnn_linear_mix_fwd``; no [M, K] intermediate in HBM).  ``x1`` fp32, ``x2`` fp32 or fp16.  Returns ``out``, or with
    ``row_scale`` ``(out, row_scale[:, None] * out)``; ``want_out=False`` (only with ``row_scale``) skips the unscaled copy
    and returns ``(None, scaled)``.  ``out`` / ``out_scaled``: caller-owned [M, >= N] fp32 row tables to write into (their
    row stride is the leading dimension).  Inference helper: no autograd."""
    dev = _require_cuda(x1, c1, x2, c2, weight, bias, row_scale)
    x1 = _rowmajor(x1.float())
    if x2.dtype not in (torch.float32, torch.float16):
        x2 = x2.float()
    x2 = _rowmajor(x2) if x2.dtype == torch.float32 else (x2 if x2.stride(1) == 1 and x2.stride(0) % 4 == 0 and x2.data_ptr() % 8 == 0
                                                          else x2.contiguous())
    weight = _rowmajor(weight.float())
    M, K = x1.shape
    N = weight.shape[0]
    if tuple(x2.shape) != (M, K) or weight.shape[1] != K:
        raise WgnnError("linear_mix_fwd: x1 [M, K], x2 [M, K] and weight [N, K] disagree")
    if K % 4:
        raise WgnnError(f"K = {K} must be a multiple of 4")
    c1, c2 = c1.reshape(-1).float().contiguous(), c2.reshape(-1).float().contiguous()
    if c1.shape[0] < M or c2.shape[0] < M:
        raise WgnnError("c1 / c2 need one entry per row")
    if not want_out and row_scale is None:
        raise WgnnError("want_out=False needs row_scale (the scaled copy is then the only output)")

    def table(t):
        if t is None:
            return torch.empty((M, N), dtype=torch.float32, device=dev)
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != M or t.shape[1] < N or t.stride(1) != 1 or t.device != dev:
            raise WgnnError("out / out_scaled must be fp32 [M, >= N] row tables on the operands' device")
        return t

    out = table(out) if want_out else None
    if row_scale is not None:
        row_scale = row_scale.reshape(-1).float().contiguous()
        if row_scale.shape[0] < M:
            raise WgnnError("row_scale needs one entry per row")
        out_scaled = table(out_scaled)
    else:
        out_scaled = None
    if bias is not None:
        bias = bias.float().contiguous()
    # tagged like the wgrad entries (kernel, rows, N, K); cols / nnz / D as well, because bench.py's pass table reads them from
    # every record of a forward: two row tables of K columns in, no edges
    with _Timed(dev, ("rows", M, "cols", M, "nnz", 0, "D", K, "N", N, "K", K, "kernel", "linear_mix_mfma_f32")):
        _lib.run(dev, "wgnn_linear_mix_fwd", _ptr(x1), x1.stride(0), _ptr(c1), _ptr(x2), _dtype_code(x2), x2.stride(0),
                 _ptr(c2), _ptr(weight), weight.stride(0), _ptr(bias), _ptr(out), out.stride(0) if out is not None else 0,
                 _ptr(row_scale), _ptr(out_scaled), out_scaled.stride(0) if out_scaled is not None else 0, M, N, K,
                 (_lib.FLAG_RELU if relu else 0) | {None: 0, 64: 1 << 16, 128: 1 << 17}[tile_rows], _stream(dev))
    return out if row_scale is None else (out, out_scaled)


WGRAD_MIN_ROWS = 16384       # from this many rows on, the weight gradient of a Linear runs through wgnn_linear_wgrad


def linear_wgrad(g: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """``dW = g.T @ x`` ([N, K]) with ``wgnn_linear_wgrad``: split along the row (node) axis, fp32 matrix cores, partial
    products folded in fixed order."""
    dev = _require_cuda(g, x)
    g = _rowmajor(g.float()); x = _rowmajor(x.float())
    M, N = g.shape
    K = x.shape[1]
    if x.shape[0] != M or N % 4 or K % 4:
        raise WgnnError("linear_wgrad: g [M, N] and x [M, K] with N, K multiples of 4")
    ns, nb = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().wgnn_linear_wgrad_workspace(M, N, K, C.addressof(ns), C.addressof(nb)), "wgnn_linear_wgrad_workspace")
    ws = torch.empty(max(1, nb.value // 4), dtype=torch.float32, device=dev)
    dW = torch.empty((N, K), dtype=torch.float32, device=dev)
    with _Timed(dev, ("rows", M, "N", N, "K", K, "kernel", "wgrad_mfma_f32 + wgrad_reduce")):
        _lib.run(dev, "wgnn_linear_wgrad", _ptr(g), g.stride(0), _ptr(x), x.stride(0), _ptr(dW), K, M, N, K, 0, _ptr(ws),
                 ns.value, _stream(dev))
    return dW


class _LinearBigM(torch.autograd.Function):
    """``F.linear`` whose weight gradient - a [N, K] product reduced over up to 1e5-1e6 node rows - runs through
    ``wgnn_linear_wgrad`` instead of the library GEMM the framework picks for that shape (0.9 ms = 22 TF at cfg3)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        dx = g @ weight if ctx.needs_input_grad[0] else None
        dw = linear_wgrad(g, x).to(weight.dtype) if ctx.needs_input_grad[1] else None
        db = g.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, dw, db


class _LinearReluBigM(torch.autograd.Function):
    """``relu(x W^T + b)`` of the aggregate-first order in TRAINING (gnn.py:65-66 under train.py:84): bias and ReLU ride in the
    library GEMM's epilogue as on the no-grad path; backward masks the upstream gradient and reduces the bias gradient in ONE
    ``wgnn_agg_bwd_prepare`` launch (instead of a threshold pass + a column-sum pass over [rows, H]), the weight gradient runs
    on ``wgnn_linear_wgrad``."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        try:
            out = torch._addmm_activation(bias, x, weight.t())
        except (RuntimeError, TypeError):                          # private torch entry point: fall back to the plain composition
            out = torch.relu(torch.nn.functional.linear(x, weight, bias))
        ctx.save_for_backward(x, weight, out)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, weight, out = ctx.saved_tensors
        res = agg_bwd_prepare(gout, out, None, None, NO_ALPHA, 0, want_scaled=True, want_dbias=ctx.needs_input_grad[2])
        g = res["g_scaled"]                                           # gout * (out > 0)
        dx = g @ weight if ctx.needs_input_grad[0] else None
        dw = linear_wgrad(g, x).to(weight.dtype) if ctx.needs_input_grad[1] else None
        return dx, dw, res["dbias"]


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.linear`` for the model's projections; in training on many rows the weight gradient uses the matrix-core kernel;
    with nothing to differentiate, fp16-stored inputs and the shapes where it wins run through ``wgnn_linear_fwd_ex``."""
    if use_wgnn_linear(x, weight):
        return linear_fwd(x, weight, bias)
    if x.dtype != weight.dtype:
        x = x.to(weight.dtype)
    if (torch.is_grad_enabled() and weight.requires_grad and x.is_cuda and x.dim() == 2 and x.shape[0] >= WGRAD_MIN_ROWS
            and x.dtype == torch.float32 and weight.dtype == torch.float32 and weight.shape[0] % 4 == 0
            and weight.shape[1] % 4 == 0):
        return _LinearBigM.apply(x, weight, bias)
    return torch.nn.functional.linear(x, weight, bias)


linear.widens_fp16 = True


def linear_act(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], relu: bool) -> torch.Tensor:
    """``act(x W^T + b)`` of the aggregate-first order (gnn.py:65-66: neigh -> fc_neigh -> activation).  With nothing to
    differentiate the bias and the ReLU ride in the library GEMM's epilogue (one launch, no [n, H] elementwise pass);
    otherwise the plain composition."""
    if (relu and bias is not None and not torch.is_grad_enabled() and x.is_cuda and x.dim() == 2
            and x.dtype == weight.dtype == bias.dtype and not use_wgnn_linear(x, weight)
            and hasattr(torch, "_addmm_activation")):
        try:                                       # a private torch entry point: any change of its contract falls back to
            return torch._addmm_activation(bias, x, weight.t())      # the plain composition below
        except (RuntimeError, TypeError):
            pass
    if (FUSED_BWD_GLUE and relu and bias is not None and torch.is_grad_enabled() and weight.requires_grad and x.is_cuda
            and x.dim() == 2 and x.shape[0] >= WGRAD_MIN_ROWS and x.dtype == weight.dtype == bias.dtype == torch.float32
            and weight.shape[0] % 4 == 0 and weight.shape[1] % 4 == 0 and weight.shape[0] <= 1024
            and hasattr(torch, "_addmm_activation")):
        return _LinearReluBigM.apply(x, weight, bias)
    out = linear(x, weight, bias)
    return torch.relu(out) if relu else out


HEAD_LDS_BYTES = 64 * 1024          # the resident row kernels stage a fused head [C, H] in LDS up to this size


def _pad_cols(t: torch.Tensor, width: int) -> torch.Tensor:
    t = t.float()
    if t.shape[-1] != width:
        t = torch.nn.functional.pad(t, (0, width - t.shape[-1]))
    return t.contiguous()


def check_gene_ids(col: torch.Tensor, n_genes: int) -> None:
    """``0 <= col < n_genes`` over a batch's CSR: one device reduction and a read-back."""
    if col.numel():
        lo, hi = torch.aminmax(col)
        if int(lo) < 0 or int(hi) >= n_genes:
            raise WgnnError(f"gene id out of range [0, {n_genes}) in the batch's CSR (min {int(lo)}, max {int(hi)})")


# The operand layer of the resident row ops: each host-side chore of the wrappers below has its one place here.  ``name`` is the op
# that speaks in a message, ``exc`` the class of its argument errors.

def _csr_operand(name, exc, rowptr, col, val, val_name):
    """A device CSR - ``rowptr`` int32 / int64 [B + 1], ``col`` int32 and the float32 values the op calls ``val_name``, one of each
    per stored entry - checked: ``(rowptr, col, val, B, nnz, flags)``, the tensors contiguous as the C entries take them,
    ``flags`` = ``FLAG_ROWPTR_I64`` for an int64 ``rowptr``."""
    if rowptr.dtype not in (torch.int32, torch.int64) or col.dtype != torch.int32 or val.dtype != torch.float32:
        raise exc(f"{name} takes rowptr int32 / int64, col int32, {val_name} float32")
    if rowptr.dim() != 1 or rowptr.shape[0] < 1 or col.dim() != 1 or col.shape != val.shape:
        raise exc(f"malformed CSR: rowptr {tuple(rowptr.shape)}, col {tuple(col.shape)}, {val_name} {tuple(val.shape)}; "
                  f"col has {col.numel()} entries, {val_name} {val.numel()}")
    flags = _lib.FLAG_ROWPTR_I64 if rowptr.dtype == torch.int64 else 0
    return rowptr.contiguous(), col.contiguous(), val.contiguous(), int(rowptr.shape[0]) - 1, int(col.shape[0]), flags


def _graph_operand(name, rowptr, col, val, val_name, dtype):
    """A device CSR graph - ``rowptr`` int64 [B + 1], ``col`` int32 [nnz] and one ``dtype`` value the op calls ``val_name`` per
    stored entry - checked: ``(rowptr, col, val, B, nnz)``, the tensors contiguous as the C entries take them.  Whether ``rowptr``
    runs from 0 to ``nnz`` is the caller's to check: each reports it in its own way."""
    if rowptr.dim() != 1 or rowptr.dtype != torch.int64 or rowptr.shape[0] < 1 or col.dim() != 1 or col.dtype != torch.int32 or \
            val.dtype != dtype or val.shape != col.shape:
        raise ValueError(f"{name}: rowptr int64 [B + 1], col int32 [nnz] and {val_name} {str(dtype)[6:]} [nnz] are expected")
    B, nnz = int(rowptr.shape[0]) - 1, int(col.shape[0])
    if B >= 2 ** 31:
        raise ValueError(f"{name}: B must be below 2^31")
    return rowptr.contiguous(), col.contiguous(), val.contiguous(), B, nnz


def _group_operand(name, exc, group, B, K, check, dtypes=(torch.int32, torch.int64), says=None):
    """The per-cell group vector [B] - an id in ``[0, K)``, or -1 = the cell takes no part - checked: shape and dtype (``says``:
    the op's own words for that refusal), and with ``check`` the range (one ``aminmax`` and a read-back).  Returns ``group`` as
    it came."""
    if group.dtype not in dtypes or tuple(group.shape) != (B,):
        raise exc(f"{says or f'{name}: group must hold one id per cell ([{B}]), int32 / int64'}, got {group.dtype} "
                  f"{tuple(group.shape)}")
    if check and B:
        lo, hi = torch.aminmax(group)
        if int(lo) < -1 or int(hi) >= K:
            raise exc(f"{name}: group id out of range [-1, {K}) (min {int(lo)}, max {int(hi)})")
    return group


def _group_major(group, K):
    """``(order int32 [B], seg_ptr int64 [K + 1])``: the cells group-major, ascending within a group - group ``k`` holds
    ``order[seg_ptr[k]:seg_ptr[k + 1]]``, the ids outside ``[0, K)`` sort last.  A stable sort of the ids and a search for the
    groups' bounds in the sorted ids, all on the device: no read-back."""
    ids = group.to(torch.int64)
    ids = torch.where((ids < 0) | (ids >= K), torch.full_like(ids, K), ids)
    ids, order = torch.sort(ids, stable=True)
    seg_ptr = torch.searchsorted(ids, torch.arange(K + 1, dtype=torch.int64, device=group.device)).contiguous()
    return order.to(torch.int32), seg_ptr


def _gene_major(rowptr, col, val, B, G, group):
    """``(t_rowptr int32 [G + 1], t_cell int32, t_val f32)``: a checked batch gene-major, cells ascending within a gene and the
    cells with ``group < 0`` left out - the library's stable transpose, a stable sort above that kernel's 32 768 columns.
    ``rowptr`` is narrowed to int32 (the callers refuse ``nnz >= 2^31``); an empty batch has nothing to transpose."""
    from .graph import _transpose_by_sort, _transpose_on_device
    if B == 0:
        return torch.zeros(G + 1, dtype=torch.int32, device=col.device), col[:0], val[:0]
    transpose = _transpose_on_device if G <= 32768 else _transpose_by_sort
    return transpose(rowptr.to(torch.int32).contiguous(), col, val, B, G, group >= 0)


def _workspace_bytes(query, *sizes) -> int:
    """What the size query ``query`` of a C entry answers for ``sizes``."""
    nb = C.c_int64()
    _lib.check(getattr(_lib.lib(), query)(*sizes, C.addressof(nb)), query)
    return nb.value


def _workspace(dev, query, *sizes, have=(None, 0)):
    """``(workspace | None, n_bytes)`` for the C entry whose size query is ``query``: ``have`` where that already holds the bytes
    asked for (``(None, 0)`` when none are), else a new 8-byte aligned buffer, rounded up to whole int64 elements."""
    nb = _workspace_bytes(query, *sizes)
    if nb <= have[1]:
        return have
    ws = torch.empty((nb + 7) // 8, dtype=torch.int64, device=dev)
    return ws, ws.numel() * 8


def _row_strided(t, rows, cols) -> bool:
    """Whether the 2-D ``t`` has unit column stride and a row stride ``>= cols``, where its shape lets a stride speak."""
    return (t.shape[1] <= 1 or t.stride(1) == 1) and (rows <= 1 or t.stride(0) >= cols)


def _view_2d(name, exc, what, t, dtype, rows, cols, at_least_cols=False):
    """``t`` checked as a row-strided ``dtype`` [rows, cols] tensor (``at_least_cols``: [rows, >= cols]) - contiguous, or a view
    into wider rows.  ``what`` names it in the message, after ``name`` where the op gives one."""
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 2 or t.shape[0] != rows
            or (t.shape[1] < cols if at_least_cols else t.shape[1] != cols) or not _row_strided(t, rows, cols)):
        raise exc(f"{name + ': ' if name else ''}{what} must be {str(dtype)[6:]} [{rows}, {'>= ' if at_least_cols else ''}{cols}] "
                  f"with unit column stride and a row stride >= {cols}")
    return t


def _ld(t, rows, cols) -> int:
    """The leading dimension a C entry takes for the row-strided [rows, cols] ``t``: a single row's stride says nothing."""
    return int(t.stride(0)) if rows > 1 else cols


class _RowOperands(NamedTuple):
    """The batch, the table and ``alpha`` of a resident row op, ready for the C call."""
    rowptr: torch.Tensor
    col: torch.Tensor
    raw: torch.Tensor
    table: torch.Tensor
    alpha: torch.Tensor
    B: int
    G: int
    Hp: int
    flags: int

    @property
    def c_args(self) -> tuple:
        """the arguments every ``wgnn_*_rows`` entry starts with"""
        return (_ptr(self.rowptr), _ptr(self.col), _ptr(self.raw), self.B, _ptr(self.table), self.table.stride(0), self.G, self.Hp,
                _ptr(self.alpha))


def _row_operands(name, rowptr, col, raw, table, alpha, H, check_cols, nnz_below_2_31=True) -> _RowOperands:
    """The batch / table / alpha handling ``predict_rows``, ``predict_rows_dropout``, ``predict_rows_thin`` and ``attrib_rows``
    share: shapes and dtypes, the column range (``check_cols``), the table zero-padded to ``Hp = ceil(H / 4) * 4`` columns.
    ``nnz_below_2_31``: refuse a batch of 2^31 entries or more (``predict_rows``' kernel indexes entries with 64 bits and takes
    one)."""
    G = table.shape[0]
    Hp = -(-H // 4) * 4
    if table.dim() != 2 or table.shape[1] < H:
        raise WgnnError(f"table must be [G, >= {H}]")
    if alpha.numel() != G + 2:
        raise WgnnError(f"alpha has {alpha.numel()} entries, the table {G} rows (want G + 2)")
    rowptr, col, raw, B, nnz, flags = _csr_operand(name, WgnnError, rowptr, col, raw, "raw")
    if nnz_below_2_31 and nnz >= 2 ** 31:
        raise WgnnError(f"{name}: nnz >= 2^31 (split the batch)")
    if check_cols:
        check_gene_ids(col, G)
    if Hp != H or table.shape[1] % 4 or table.stride(1) != 1 or table.stride(0) % 4 or table.data_ptr() % 16:
        table = _pad_cols(table[:, :H], Hp)
    alpha = alpha.reshape(-1)
    if alpha.dtype != torch.float32 or not alpha.is_contiguous():
        alpha = alpha.float().contiguous()
    return _RowOperands(rowptr, col, raw, table, alpha, B, G, Hp, flags)


def _self_rows(self_rows, n_rows, batch, H, Hp, exc):
    """``self_rows`` [n_rows, H] as the kernels read it (float32, ``Hp`` columns, aligned rows); ``batch`` says in ``exc``'s
    message what ``n_rows`` is."""
    if self_rows is None:
        return None
    if self_rows.shape[0] != n_rows:
        raise exc(f"self_rows has {self_rows.shape[0]} rows, the batch {batch}")
    return _rowmajor(self_rows.float()) if self_rows.shape[1] == Hp else _pad_cols(self_rows[:, :H], Hp)


def _fused_head(head, Hp, refuse=None):
    """``(w_head [C, Hp], b_head [C], C)`` as the kernels stage a head in LDS.  A head beyond ``HEAD_LDS_BYTES``: the exception
    ``refuse(C)`` is raised, or None is returned where the caller has another route for it (``refuse`` None)."""
    w_head, b_head = head
    n_cls = w_head.shape[0]
    if n_cls * Hp * 4 > HEAD_LDS_BYTES:
        if refuse is None:
            return None
        raise refuse(n_cls)
    return _pad_cols(w_head, Hp), b_head.float().contiguous(), n_cls


def _headless_out(out, n_rows, Hp, dev, exc):
    """The ``ReLU(z)`` buffer [n_rows, Hp] of a call without a head: ``out`` checked, or a new one."""
    if out is None:
        return torch.empty((n_rows, Hp), dtype=torch.float32, device=dev)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (n_rows, Hp)
            or not _row_strided(out, n_rows, Hp) or _ld(out, n_rows, Hp) % 4 or out.data_ptr() % 16):
        raise exc(f"out must be float32 [{n_rows}, {Hp}], unit column stride, 16-byte aligned rows")
    return out


def _draw_outputs(out, B, n_cls, n_draws, accumulate, want_draws, dev, exc):
    """``(votes, unsure, empty, conf_sum, draw_label | None, draw_prob | None)`` of a call with a head: ``out`` (the first four
    or all six) checked, what it does not hold allocated."""
    if out is None:
        if accumulate:
            raise exc("accumulate needs the tables to add to (out=)")
        out = (torch.empty((B, n_cls), dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float64, device=dev))
    if len(out) not in (4, 6):
        raise exc("out must be (votes, unsure, empty, conf_sum[, draw_label, draw_prob])")
    votes, unsure, empty, conf_sum = out[:4]
    draw_label, draw_prob = out[4:] if len(out) == 6 else (None, None)
    if draw_label is None and want_draws:
        draw_label = torch.empty((B, n_draws), dtype=torch.int32, device=dev)
        draw_prob = torch.empty((B, n_draws), dtype=torch.float32, device=dev)
    _require_cuda(votes, unsure, empty, conf_sum, draw_label, draw_prob)
    _view_2d(None, exc, "votes", votes, torch.int32, B, n_cls)
    want = ((unsure, torch.int32, (B,)), (empty, torch.int32, (B,)), (conf_sum, torch.float64, (B,)))
    if any(t.dtype != d or tuple(t.shape) != s or not t.is_contiguous() for t, d, s in want):
        raise exc(f"unsure and empty must be contiguous int32 [{B}], conf_sum float64 [{B}]")
    if draw_label is not None:
        per = ((draw_label, torch.int32), (draw_prob, torch.float32))
        if any(t is None or t.dtype != d or tuple(t.shape) != (B, n_draws) or not t.is_contiguous() for t, d in per):
            raise exc(f"draw_label / draw_prob must be contiguous int32 / float32 [{B}, {n_draws}]")
    return votes, unsure, empty, conf_sum, draw_label, draw_prob


def predict_rows(rowptr: torch.Tensor, col: torch.Tensor, raw: torch.Tensor, table: torch.Tensor, alpha: torch.Tensor,
                 bias: torch.Tensor, *, self_rows: Optional[torch.Tensor] = None,
                 head: Optional[tuple] = None, unsure_threshold: float = 0.0, want_logits: bool = True,
                 check_cols: bool = True):
    """``wgnn_predict_rows``: one layer of a trained model over a batch of test cells given as a device CSR of RAW values
    (``rowptr`` int32 / int64 [B+1], ``col`` int32 gene ids, ``raw`` f32), against the resident gene table ``table`` [G, H]
    (H = ``bias.shape[0]`` valid columns).  ``self_rows`` [B, H] = None: the self-loop comes from the row (layer 1);
    else it is the explicit ``h_{l-1}[c] . W_l^T``.

    Without ``head`` returns ``ReLU(z)`` [B, H].  With ``head = (w_head [C, H], b_head [C])`` returns
    ``(logits [B, C] | None, label int32 [B], max_prob f32 [B])``; ``label`` is -1 where ``max_prob < unsure_threshold``
    (pass ``float32(unsure_rate / C)``).  A head wider than the kernel stages in LDS runs as ``linear_fwd`` plus the same
    softmax rule instead.  Widths that are not a multiple of 4 are zero-padded here (table, bias, head and self columns).
    ``check_cols``: verify ``0 <= col < G`` (one device reduction and a read-back) - CSRs built by the predictor from a
    parsed file are in range by construction and skip it."""
    dev = _require_cuda(rowptr, col, raw, table, alpha, bias, self_rows, *(head or ()))
    H = bias.shape[0]
    o = _row_operands("predict_rows", rowptr, col, raw, table, alpha, H, check_cols, nnz_below_2_31=False)
    B, Hp = o.B, o.Hp
    bias = _pad_cols(bias, Hp)
    self_rows = _self_rows(self_rows, B, B, H, Hp, WgnnError)
    fused = _fused_head(head, Hp) if head is not None else None
    w_head, b_head, n_cls = fused or (None, None, 0)
    out = None if fused else torch.empty((B, Hp), dtype=torch.float32, device=dev)
    logits = label = max_prob = None
    if fused:
        logits = torch.empty((B, n_cls), dtype=torch.float32, device=dev) if want_logits else None
        label = torch.empty(B, dtype=torch.int32, device=dev)
        max_prob = torch.empty(B, dtype=torch.float32, device=dev)
    _lib.run(dev, "wgnn_predict_rows", *o.c_args, _ptr(bias), _ptr(self_rows),
             self_rows.stride(0) if self_rows is not None else 0, _ptr(out), Hp if out is not None else 0,
             _ptr(w_head), _ptr(b_head), n_cls, float(unsure_threshold), _ptr(logits),
             logits.shape[1] if logits is not None else 0, _ptr(label), _ptr(max_prob), o.flags, _stream(dev))
    if head is None:
        return out if Hp == H else out[:, :H]
    if fused:
        return logits, label, max_prob
    # a head too wide for LDS: the GEMM, then the softmax rule of predict.py:78-88 on the [B, C] logits
    w_head, b_head = head
    logits = linear_fwd(out, _pad_cols(w_head, Hp), b_head)
    mx, arg = torch.softmax(logits, dim=1).max(dim=1)
    label = torch.where(mx < unsure_threshold, torch.full_like(arg, -1), arg).to(torch.int32)
    return (logits if want_logits else None), label, mx


def _predict_rows_draws(name, exc, accumulate_flag, thin, rowptr, col, raw, table, alpha, bias, self_rows, head, unsure_threshold,
                        check_cols, n_draws, keep, seed, row0, draw0, out, accumulate, want_draws):
    """``predict_rows_dropout`` and ``predict_rows_thin`` behind their signatures: the entry point ``name``, the class ``exc`` of
    its argument errors, its accumulate bit, and ``thin`` = None or ``(rest, scale, threshold, want_reads)`` - the operands
    ``wgnn_predict_rows_thin`` takes after ``ld_self`` and the two per-pair tables it writes after ``draw_prob``."""
    rest, scale, threshold, want_reads = thin or (None, None, None, False)
    dev = _require_cuda(rowptr, col, raw, table, alpha, bias, rest, self_rows, *(head or ()))
    n_draws = int(n_draws)
    keep = float(keep)
    if n_draws < 1:
        raise exc(f"{name}: n_draws = {n_draws} must be >= 1")
    if not 0.0 <= keep <= 1.0:
        raise exc(f"{name}: keep = {keep} must be in [0, 1]")
    if int(row0) < 0 or int(draw0) < 0:
        raise exc(f"{name}: row0 and draw0 must not be negative")
    if thin and not 0 < float(scale) < float("inf"):
        raise exc(f"{name}: scale = {scale} must be positive and finite")
    if thin and not float(threshold) >= 0:
        raise exc(f"{name}: threshold = {threshold} must be >= 0")
    H = bias.shape[0]
    o = _row_operands(name, rowptr, col, raw, table, alpha, H, check_cols)
    B, Hp = o.B, o.Hp
    if thin:
        if rest.dtype != torch.int64 or tuple(rest.shape) != (B,):
            raise exc(f"{name}: rest must be int64 [{B}]")
        rest = rest.contiguous()
    if B * n_draws >= 2 ** 31:
        raise exc(f"{name}: B * n_draws >= 2^31 (split the batch or the draws)")
    bias = _pad_cols(bias, Hp)
    self_rows = _self_rows(self_rows, B * n_draws, f"{B} cells x {n_draws} draws", H, Hp, exc)
    lead = (*o.c_args, _ptr(bias), _ptr(self_rows), self_rows.stride(0) if self_rows is not None else 0,
            *((_ptr(rest), float(scale), float(threshold)) if thin else ()),
            n_draws, int(row0), int(draw0), int(seed) & (2 ** 64 - 1), keep)
    reads = ()
    if want_reads:
        reads = (torch.empty((B, n_draws), dtype=torch.int32, device=dev), torch.empty((B, n_draws), dtype=torch.int32, device=dev))
    read_ptrs = tuple(_ptr(t) for t in reads or (None, None)) if thin else ()
    if head is None:
        if accumulate or want_draws:
            raise exc(f"{name}: accumulate and want_draws need a head")
        out = _headless_out(out, B * n_draws, Hp, dev, exc)
        _lib.run(dev, "wgnn_" + name, *lead, _ptr(out), _ld(out, B * n_draws, Hp),
                 None, None, 0, 0.0, None, 0, None, None, None, None, None, *read_ptrs, o.flags, _stream(dev))
        h = out if Hp == H else out[:, :H]
        return (h, *reads) if want_reads else h
    w_head, b_head, n_cls = _fused_head(
        head, Hp, lambda c: exc(f"{name}: a [{c}, {Hp}] head is beyond the {HEAD_LDS_BYTES} bytes the kernel stages"))
    votes, unsure, empty, conf_sum, draw_label, draw_prob = _draw_outputs(out, B, n_cls, n_draws, accumulate, want_draws, dev, exc)
    _lib.run(dev, "wgnn_" + name, *lead, None, 0, _ptr(w_head), _ptr(b_head), n_cls,
             float(unsure_threshold), _ptr(votes), _ld(votes, B, n_cls),
             _ptr(unsure), _ptr(empty), _ptr(conf_sum), _ptr(draw_label), _ptr(draw_prob), *read_ptrs,
             o.flags | (accumulate_flag if accumulate else 0), _stream(dev))
    return (votes, unsure, empty, conf_sum, draw_label, draw_prob, *reads)


def predict_rows_dropout(rowptr: torch.Tensor, col: torch.Tensor, raw: torch.Tensor, table: torch.Tensor, alpha: torch.Tensor,
                         bias: torch.Tensor, *, self_rows: Optional[torch.Tensor] = None,
                         head: Optional[tuple] = None, unsure_threshold: float = 0.0, check_cols: bool = True,
                         n_draws: int, keep: float, seed: int, row0: int = 0, draw0: int = 0, out=None,
                         accumulate: bool = False, want_draws: bool = False):
    """``wgnn_predict_rows_dropout``: one layer of ``predict_rows`` for every (cell, draw) pair of a batch, a draw keeping
    each stored entry with probability ``keep`` - the mask a pure function of ``(seed, row0 + cell, draw0 + draw, gene id)``
    (``include/wgnn.h``), so a batch split by cells (``row0``) or by draws (``draw0``) gets the same masks.  The batch, the
    table, ``alpha``, ``bias``, ``head``, ``unsure_threshold`` and ``check_cols`` as ``predict_rows`` takes them, widths
    that are not a multiple of 4 zero-padded in the same way.  ``self_rows`` [B * n_draws, H]: row ``r * n_draws + d``
    belongs to draw ``d`` of cell ``r``.  With ``keep == 1`` every draw carries the bits of ``predict_rows``.

    Without ``head`` returns ``ReLU(z)`` [B * n_draws, H], rows laid out like ``self_rows`` (``out``: a float32
    [B * n_draws, Hp] buffer to write into).  With ``head = (w_head [C, H], b_head [C])`` returns ``(votes int32 [B, C],
    unsure int32 [B], empty int32 [B], conf_sum f64 [B], draw_label int32 [B, n_draws] | None, draw_prob f32 [B, n_draws] |
    None)``: the draws per label, the draws labelled -1, the draws that kept no entry, and the draws' ``max_prob`` added in
    fp64 in draw order; the last two with ``want_draws``.  ``out``: the first four (``votes`` may be a view with a row stride
    ``>= C``), or all six, to write into - every element is written, or added to with ``accumulate`` (further draws of the
    same cells: pass ``draw0``).  There is no GEMM route for a head beyond what the kernel stages in LDS."""
    return _predict_rows_draws("predict_rows_dropout", WgnnError, _lib.STABILITY_ACCUMULATE, None, rowptr, col, raw, table, alpha,
                               bias, self_rows, head, unsure_threshold, check_cols, n_draws, keep, seed, row0, draw0, out,
                               accumulate, want_draws)


def predict_rows_thin(rowptr: torch.Tensor, col: torch.Tensor, raw: torch.Tensor, table: torch.Tensor, alpha: torch.Tensor,
                      bias: torch.Tensor, *, rest: torch.Tensor, scale: float = 1e4, threshold: float = 0.0,
                      self_rows: Optional[torch.Tensor] = None, head: Optional[tuple] = None, unsure_threshold: float = 0.0,
                      check_cols: bool = True, n_draws: int, keep: float, seed: int, row0: int = 0, draw0: int = 0, out=None,
                      accumulate: bool = False, want_draws: bool = False, want_reads: bool = False):
    """``wgnn_predict_rows_thin``: ``predict_rows_dropout`` with READ-LEVEL thinning.  ``raw`` holds the cells' COUNTS over the
    bundle's genes (float32 integers in [1, 2^24]), ``rest`` int64 [B] a cell's reads outside the bundle; in a draw every read
    survives with probability ``keep`` - a pure hash of ``(seed, row0 + cell, draw0 + draw, gene id, read number)``
    (``include/wgnn.h``) - and the surviving counts are log-normalised against the draw's own library size (``scale``, and
    ``threshold`` on the normalised value, as ``align_rows(normalize="lognorm")`` takes them) before the layer runs.  With
    ``keep == 1`` every draw carries the bits of ``predict_rows`` on the lognorm-aligned batch.

    Every other argument, the layouts and the return values as ``predict_rows_dropout``.  ``want_reads``: two more per-pair
    tables ``draw_reads`` / ``draw_entries`` int32 [B, n_draws] - a draw's library size and its participating entries -
    appended to the return value (without a head: ``(out, draw_reads, draw_entries)``).  CPU tensors are refused; argument
    errors are ``ValueError``."""
    return _predict_rows_draws("predict_rows_thin", ValueError, _lib.THIN_ACCUMULATE, (rest, scale, threshold, want_reads), rowptr,
                               col, raw, table, alpha, bias, self_rows, head, unsure_threshold, check_cols, n_draws, keep, seed,
                               row0, draw0, out, accumulate, want_draws)


PANELS_PER_LAUNCH = 64              # bits of a ``member`` word (include/wgnn.h)


def predict_rows_panels(rowptr: torch.Tensor, col: torch.Tensor, raw: torch.Tensor, table: torch.Tensor, alpha: torch.Tensor,
                        bias: torch.Tensor, member: torch.Tensor, n_panels: int, *, lib: Optional[torch.Tensor] = None,
                        scale: float = 1e4, threshold: float = 0.0, self_rows: Optional[torch.Tensor] = None,
                        head: Optional[tuple] = None, unsure_threshold: float = 0.0, want_logits: bool = False,
                        want_entries: bool = False, check_cols: bool = True, out=None):
    """``wgnn_predict_rows_panels``: one layer of ``predict_rows`` for every (cell, panel) pair of a batch, a panel being a GIVEN
    subset of the genes.  ``member`` int64 [G] holds the uint64 membership words: bit ``p`` of ``member[g]`` says that gene ``g``
    belongs to panel ``p`` (``n_panels`` in [1, 64]; higher bits are ignored).  The batch, the table, ``alpha``, ``bias``,
    ``head``, ``unsure_threshold`` and ``check_cols`` as ``predict_rows`` takes them.  ``self_rows`` [B * n_panels, H]: row
    ``r * n_panels + p`` belongs to panel ``p`` of cell ``r``.

    ``lib`` None (values mode): a pair keeps the row's entries whose gene is in the panel, values as given, and carries the
    bits of ``predict_rows`` on that sub-row.  ``lib`` int64 [B, n_panels] (counts mode; may be a view with a wider row
    stride): ``raw`` holds counts, ``lib[r, p]`` the cell's reads inside the panel over all of the caller's columns; the kept
    counts are log-normalised against it (``scale``, and ``threshold`` on the normalised value, as
    ``align_rows(normalize="lognorm")`` takes them) - the bits of ``predict_rows`` on the lognorm-aligned count matrix with
    the other columns zeroed.  ``lib[r, p] <= 0`` is the empty row.

    Without ``head`` returns ``ReLU(z)`` [B * n_panels, H] (``out``: a float32 [B * n_panels, Hp] buffer to write into).  With
    ``head = (w_head [C, H], b_head [C])`` returns ``(logits [B * n_panels, C] | None, label int32 [B, n_panels], max_prob f32
    [B, n_panels])``.  ``want_entries``: the pairs' kept entries, int32 [B, n_panels], appended to the return value (without a
    head: ``(out, entries)``).  There is no GEMM route for a head beyond what the kernel stages in LDS.  CPU tensors are
    refused; argument errors are ``ValueError``."""
    name, exc = "predict_rows_panels", ValueError
    dev = _require_cuda(rowptr, col, raw, table, alpha, bias, member, lib, self_rows, *(head or ()))
    P = int(n_panels)
    if not 1 <= P <= PANELS_PER_LAUNCH:
        raise exc(f"{name}: n_panels = {P} must be in [1, {PANELS_PER_LAUNCH}] (split the panels)")
    if lib is not None and not 0 < float(scale) < float("inf"):
        raise exc(f"{name}: scale = {scale} must be positive and finite")
    if lib is not None and not float(threshold) >= 0:
        raise exc(f"{name}: threshold = {threshold} must be >= 0")
    H = bias.shape[0]
    o = _row_operands(name, rowptr, col, raw, table, alpha, H, check_cols)
    B, Hp = o.B, o.Hp
    if member.dtype != torch.int64 or tuple(member.shape) != (o.G,):
        raise exc(f"{name}: member must be int64 [{o.G}] (the uint64 membership words)")
    member = member.contiguous()
    if lib is not None:
        _view_2d(name, exc, "lib", lib, torch.int64, B, P)
    if B * P >= 2 ** 31:
        raise exc(f"{name}: B * n_panels >= 2^31 (split the batch or the panels)")
    bias = _pad_cols(bias, Hp)
    self_rows = _self_rows(self_rows, B * P, f"{B} cells x {P} panels", H, Hp, exc)
    ld_lib = _ld(lib, B, P) if lib is not None else 0
    lead = (*o.c_args, _ptr(bias), _ptr(self_rows), self_rows.stride(0) if self_rows is not None else 0,
            _ptr(member), P, _ptr(lib), ld_lib, float(scale), float(threshold))
    entries = torch.empty((B, P), dtype=torch.int32, device=dev) if want_entries else None
    if head is None:
        out = _headless_out(out, B * P, Hp, dev, exc)
        _lib.run(dev, "wgnn_" + name, *lead, _ptr(out), _ld(out, B * P, Hp),
                 None, None, 0, 0.0, None, 0, None, None, _ptr(entries), o.flags, _stream(dev))
        h = out if Hp == H else out[:, :H]
        return (h, entries) if want_entries else h
    w_head, b_head, n_cls = _fused_head(
        head, Hp, lambda c: exc(f"{name}: a [{c}, {Hp}] head is beyond the {HEAD_LDS_BYTES} bytes the kernel stages"))
    logits = torch.empty((B * P, n_cls), dtype=torch.float32, device=dev) if want_logits else None
    label = torch.empty((B, P), dtype=torch.int32, device=dev)
    max_prob = torch.empty((B, P), dtype=torch.float32, device=dev)
    _lib.run(dev, "wgnn_" + name, *lead, None, 0, _ptr(w_head), _ptr(b_head), n_cls, float(unsure_threshold),
             _ptr(logits), n_cls if logits is not None else 0, _ptr(label), _ptr(max_prob), _ptr(entries), o.flags,
             _stream(dev))
    return (logits, label, max_prob, entries) if want_entries else (logits, label, max_prob)


SETS_PER_LAUNCH = 64                # bits of a ``member`` word (include/wgnn.h)
RANK_SETS_MAX_RANK = 2 ** 30        # wgnn_rank_sets_rows' largest ``max_rank``


def rank_sets_rows(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, member: torch.Tensor, n_sets: int, max_rank: int,
                   n_genes: int, check_cols: bool = True, out=None):
    """``wgnn_rank_sets_rows``: for every (cell, set) pair of a batch the capped, doubled mid-ranks of the set's genes within
    the cell's own row, added up - the integer part of UCell's rank-based signature score (``include/wgnn.h`` has the
    definition).  The batch is a device CSR over ``n_genes`` gene ids (``rowptr`` int32 / int64 [B+1], ``col`` int32, ``val``
    f32); ``member`` int64 [n_genes] holds the uint64 membership words of ``predict_rows_panels`` (bit ``p`` = the gene belongs
    to set ``p``; ``n_sets`` in [1, 64], higher bits are ignored); ``max_rank`` in [1, 2^30] is UCell's ``maxRank``.
    ``check_cols`` as ``predict_rows`` takes it.

    Returns ``(rank2_sum int64 [B, n_sets], present int32 [B, n_sets])``.  ``out``: that pair to write into - either may be a
    view with unit column stride and a wider row stride; columns beyond ``n_sets`` are left untouched.  CPU tensors are refused;
    argument errors are ``ValueError``."""
    name = "rank_sets_rows"
    dev = _require_cuda(rowptr, col, val, member, *(out or ()))
    P, R, G = int(n_sets), int(max_rank), int(n_genes)
    if not 1 <= P <= SETS_PER_LAUNCH:
        raise ValueError(f"{name}: n_sets = {P} must be in [1, {SETS_PER_LAUNCH}] (split the sets)")
    if not 1 <= R <= RANK_SETS_MAX_RANK:
        raise ValueError(f"{name}: max_rank = {R} must be in [1, 2^30]")
    if G <= 0:
        raise ValueError(f"{name}: n_genes = {G} must be positive")
    rowptr, col, val, B, _, flags = _csr_operand(name, ValueError, rowptr, col, val, "val")
    if member.dtype != torch.int64 or tuple(member.shape) != (G,):
        raise ValueError(f"{name}: member must be int64 [{G}] (the uint64 membership words)")
    if check_cols:
        check_gene_ids(col, G)
    member = member.contiguous()
    if out is None:
        out = (torch.empty((B, P), dtype=torch.int64, device=dev), torch.empty((B, P), dtype=torch.int32, device=dev))
    rank2_sum, present = out
    _view_2d(name, ValueError, "out's rank2_sum", rank2_sum, torch.int64, B, P, at_least_cols=True)
    _view_2d(name, ValueError, "out's present", present, torch.int32, B, P, at_least_cols=True)
    _lib.run(dev, "wgnn_" + name, _ptr(rowptr), _ptr(col), _ptr(val), B, G, _ptr(member), P, R,
             _ptr(rank2_sum), _ld(rank2_sum, B, P), _ptr(present), _ld(present, B, P), flags, _stream(dev))
    return rank2_sum[:, :P], present[:, :P]


def thin_operand_check(rowptr: torch.Tensor, raw: torch.Tensor, rest: torch.Tensor, total: torch.Tensor) -> None:
    """The one fused device check ``stability(thin="reads")`` makes of its operand: every count of ``raw`` an integer in
    [1, 2^24], every ``rest`` (float64 [B], exact) a non-negative integer, every cell's ``total`` below 2^31.  One reduction to
    the first offending cell and one read-back; ``WgnnError`` naming that cell."""
    B = int(rowptr.shape[0]) - 1
    if B == 0:
        return
    bad_entry = (raw != torch.floor(raw)) | (raw < 1) | (raw > 16777216.0) if raw.numel() else raw.new_zeros(0, dtype=torch.bool)
    rows = torch.repeat_interleave(torch.arange(B, device=raw.device), (rowptr[1:] - rowptr[:-1]).long(), output_size=raw.shape[0])
    bad_cell = (rest != torch.floor(rest)) | (rest < 0) | ~(total < 2.0 ** 31)
    first = torch.where(bad_cell, torch.arange(B, device=raw.device), B).min()
    if raw.numel():
        first = torch.minimum(first, torch.where(bad_entry, rows, B).min())
    first = int(first)
    if first < B:
        raise WgnnError(f"thin=\"reads\" takes integer counts: cell {first} holds a count that is no integer in [1, 2^24], reads "
                        f"outside the bundle that are no non-negative integer (a library size below the cell's matched reads?), "
                        f"or 2^31 reads or more")


PAIR_MAX_COUNT = float(2 ** 23)     # pair_rows adds two counts in float32: exact up to here


def pair_operand_check(rowptr: torch.Tensor, raw: torch.Tensor, what: str = "doublets adds two cells' counts in float32") -> None:
    """What ``doublets`` asks of its counts beyond ``thin_operand_check``: none above 2^23, so that the float32 sum of two
    cells' counts is exact (``pseudobulk`` asks the same for the 32-bit partial sums of ``pool_rows`` and says so in ``what``).
    One reduction to the first offending cell and one read-back; ``WgnnError`` naming that cell."""
    B = int(rowptr.shape[0]) - 1
    if B == 0 or not raw.numel():
        return
    rows = torch.repeat_interleave(torch.arange(B, device=raw.device), (rowptr[1:] - rowptr[:-1]).long(), output_size=raw.shape[0])
    first = int(torch.where(raw > PAIR_MAX_COUNT, rows, B).min())
    if first < B:
        raise WgnnError(f"{what}: cell {first} holds a count above 2^23")


def csr_rows_ascending(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor):
    """``(rowptr, col, val)`` with every row strictly ascending in ``col``, as ``pair_rows`` takes it: the operand itself when it
    already is (one device reduction and a read-back), else the entries stably sorted by ``(row, col)``.  A column listed twice
    within a row raises ``WgnnError``.  Torch ops only; off the hot path."""
    n = int(col.shape[0])
    if n < 2:
        return rowptr, col, val
    B = int(rowptr.shape[0]) - 1
    rows = torch.repeat_interleave(torch.arange(B, device=col.device), (rowptr[1:] - rowptr[:-1]).long(), output_size=n)
    lo, hi = torch.aminmax(col)
    key = rows * (int(hi) - int(lo) + 1) + (col.long() - int(lo))         # ascending in (row, col)
    if bool((key[1:] > key[:-1]).all()):
        return rowptr, col, val
    key, order = torch.sort(key, stable=True)
    twice = key[1:] == key[:-1]
    if bool(twice.any()):
        at = int(torch.nonzero(twice)[0])
        raise WgnnError(f"row {int(rows[order[at]])} lists column {int(col[order[at]])} twice")
    return rowptr, col[order].contiguous(), val[order].contiguous()


def _check_lognorm(name, scale, threshold) -> None:
    """The ``scale`` / ``threshold`` check ``pair_rows``, ``pool_rows_grouped``, ``soup_rows`` and ``hood_rows`` open with."""
    if not 0 < float(scale) < float("inf"):
        raise ValueError(f"{name}: scale = {scale} must be positive and finite")
    if not float(threshold) >= 0:
        raise ValueError(f"{name}: threshold = {threshold} must be >= 0")


def _count_csr(name, rowptr, col, cnt, lib=None):
    """The operand of those four ops - a device CSR of raw counts over the bundle's gene ids, and ``lib`` int64 [B] where the op
    takes library sizes - checked (``ValueError`` under the op's ``name``): ``(rowptr, col, cnt, lib, B, nnz, flags)``, the
    tensors contiguous, as the C entries take them."""
    rowptr, col, cnt, B, nnz, flags = _csr_operand(name, ValueError, rowptr, col, cnt, "cnt")
    if lib is not None and (lib.dtype != torch.int64 or tuple(lib.shape) != (B,)):
        raise ValueError(f"{name}: lib must be int64 [{B}]")
    return rowptr, col, cnt, None if lib is None else lib.contiguous(), B, nnz, flags


def _scan(n_out: torch.Tensor):
    """A count pass's ``n_out`` int32 [n] -> ``(out_rowptr int64 [n + 1], total)``: the scan, and the one read-back that sizes
    the outputs of the fill pass."""
    out_rowptr = torch.zeros(n_out.shape[0] + 1, dtype=torch.int64, device=n_out.device)
    torch.cumsum(n_out, 0, dtype=torch.int64, out=out_rowptr[1:])
    return out_rowptr, int(out_rowptr[-1])


def _check_status(name, bits: int, table, extra=()) -> None:
    """The status word after the passes: ``WgnnError`` with the text of every bit of ``table`` that is set (then ``extra``)."""
    if bits:
        raise WgnnError(name + ": " + "; ".join([text for bit, text in table if bits & bit] + list(extra)))


_PAIR_STATUS = ((_lib.PAIR_BAD_INDEX, "a pair names a row outside [0, n_rows)"),
                (_lib.PAIR_UNSORTED, "a row is not strictly ascending in col (csr_rows_ascending sorts a batch)"),
                (_lib.PAIR_BAD_ROWPTR, "rowptr points outside col / cnt, or a pair kept more entries than were counted"))


def pair_rows(rowptr: torch.Tensor, col: torch.Tensor, cnt: torch.Tensor, lib: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
              scale: float = 1e4, threshold: float = 0.0):
    """``wgnn_pair_rows_count`` / ``wgnn_pair_rows_fill``: pairs of cells merged into the log-normalised rows of their summed
    counts - synthetic doublets.  ``(rowptr int32 / int64 [B+1], col int32, cnt float32)``: a device CSR of raw counts over the
    bundle's gene ids, every row strictly ascending in ``col``, every count an integer in [1, 2^23] (``pair_operand_check``);
    ``lib`` int64 [B]: each cell's library size, columns outside the bundle included; ``a``, ``b`` int32 [n_pairs]: the rows of
    a pair (``a[q] == b[q]`` is allowed).

    Pair ``q`` leaves, in ascending gene id, ``float32(log1p(float64(c) / (lib[a] + lib[b]) * scale))`` for every gene of
    either row with ``c = cnt_a + cnt_b > 0`` and a value ``> threshold`` (``>= 0``) - the bits
    ``align_rows(..., normalize="lognorm")`` leaves on the summed count matrix (the contract in ``include/wgnn.h``).  Returns
    ``(rowptr int64 [n_pairs + 1], col int32, val float32)`` on the device, which ``predict_rows`` takes: the count pass, a
    ``torch.cumsum``, one read-back of the total to size the outputs, the fill pass, and a read-back of the status word - a pair
    index out of range, a row that is not ascending or a ``rowptr`` outside ``col`` raises ``WgnnError`` (the kernels skip it).
    Argument errors are ``ValueError``."""
    dev = _require_cuda(rowptr, col, cnt, lib, a, b)
    _check_lognorm("pair_rows", scale, threshold)
    rowptr, col, cnt, lib, B, nnz, flags = _count_csr("pair_rows", rowptr, col, cnt, lib)
    if a.dtype != torch.int32 or b.dtype != torch.int32 or a.dim() != 1 or a.shape != b.shape:
        raise ValueError("pair_rows: a and b must be int32 vectors of one length")
    n_pairs = int(a.shape[0])
    if n_pairs >= 2 ** 31:
        raise ValueError("pair_rows: n_pairs >= 2^31 (split the pair list)")
    a, b = a.contiguous(), b.contiguous()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    n_out = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    head = (_ptr(rowptr), _ptr(col), _ptr(cnt), B, nnz, _ptr(lib), _ptr(a), _ptr(b), n_pairs, float(scale), float(threshold))
    _lib.run(dev, "wgnn_pair_rows_count", *head, _ptr(n_out), _ptr(status), flags, _stream(dev))
    out_rowptr, total = _scan(n_out)
    out_col = torch.empty(total, dtype=torch.int32, device=dev)
    out_val = torch.empty(total, dtype=torch.float32, device=dev)
    _lib.run(dev, "wgnn_pair_rows_fill", *head, _ptr(out_rowptr), _ptr(out_col), _ptr(out_val), _ptr(status), flags,
             _stream(dev))
    _check_status("pair_rows", int(status), _PAIR_STATUS)
    return out_rowptr, out_col, out_val


POOL_CHUNK_BYTES = 256 << 20        # pool_rows: the [groups of a chunk, n_genes] uint64 accumulator stays under this

_POOL_STATUS = ((_lib.POOL_BAD_INDEX, "a member names a row outside [0, n_rows)"),
                (_lib.POOL_BAD_ROWPTR, "rowptr points outside col / cnt, group_ptr is not ascending within [0, n_rows], or a "
                                       "group kept more entries than were counted"),
                (_lib.POOL_BAD_COL, "a gene id is outside [0, n_genes)"))


def pool_rows_grouped(rowptr: torch.Tensor, col: torch.Tensor, cnt: torch.Tensor, group_ptr: torch.Tensor, members: torch.Tensor,
                      total: torch.Tensor, n_genes: int, scale: float = 1e4, threshold: float = 0.0, seed=None,
                      cells_per_unit: int = 0, slab_genes: int = 0, max_bytes: int = POOL_CHUNK_BYTES):
    """``wgnn_pool_rows_accumulate`` / ``_count`` / ``_fill`` on group lists that are already made - the core of ``pool_rows``,
    which documents the operands and the result.  ``group_ptr`` int64 [K + 1] (ascending) and ``members`` int32 [B]: the cells of
    group ``k`` are ``members[group_ptr[k]:group_ptr[k + 1]]`` (``members`` always holds one entry per row, the groups use
    ``[group_ptr[0], group_ptr[K])`` of them); ``total`` int64 [K]: the pooled library sizes.  ``seed``: ``(rowptr, col, cnt)``
    of an earlier result over the same K groups, written into the accumulator before the kernel adds to it (``total`` already
    holds the seed's share).  Returns ``(rowptr int64 [K + 1], col int32, val float32, cnt int64)``."""
    dev = _require_cuda(rowptr, col, cnt, group_ptr, members, total)
    _check_lognorm("pool_rows", scale, threshold)
    rowptr, col, cnt, _, B, nnz, flags = _count_csr("pool_rows", rowptr, col, cnt)
    G = int(n_genes)
    if group_ptr.dtype != torch.int64 or group_ptr.dim() != 1 or group_ptr.shape[0] < 1:
        raise ValueError("pool_rows: group_ptr must be an int64 vector [n_groups + 1]")
    K = int(group_ptr.shape[0]) - 1
    if members.dtype != torch.int32 or tuple(members.shape) != (B,):
        raise ValueError(f"pool_rows: members must be int32 [{B}], one entry per row")
    if total.dtype != torch.int64 or tuple(total.shape) != (K,):
        raise ValueError(f"pool_rows: total must be int64 [{K}]")
    if not 0 <= G < 2 ** 31 or B >= 2 ** 31 or K >= 2 ** 31:
        raise ValueError("pool_rows: n_genes, the rows and the groups must each be below 2^31")
    if not 0 <= int(cells_per_unit) <= _lib.POOL_MAX_CELLS_PER_UNIT:
        raise ValueError(f"pool_rows: cells_per_unit = {cells_per_unit} must be in [0, {_lib.POOL_MAX_CELLS_PER_UNIT}]")
    if not 0 <= int(slab_genes) <= _lib.POOL_MAX_SLAB_GENES:
        raise ValueError(f"pool_rows: slab_genes = {slab_genes} must be in [0, {_lib.POOL_MAX_SLAB_GENES}]")
    if int(max_bytes) < 1:
        raise ValueError(f"pool_rows: max_bytes = {max_bytes} must be positive")
    if seed is not None:
        s_rowptr, s_col, s_cnt = seed
        _require_cuda(s_rowptr, s_col, s_cnt)
        if tuple(s_rowptr.shape) != (K + 1,) or s_col.shape != s_cnt.shape or s_col.dim() != 1 or s_cnt.dtype != torch.int64:
            raise ValueError(f"pool_rows: seed must be an earlier result over the same {K} groups")
        if s_col.numel() and (int(s_col.min()) < 0 or int(s_col.max()) >= G):
            raise ValueError(f"pool_rows: seed holds a gene id outside [0, {G})")
    group_ptr, members, total = group_ptr.contiguous(), members.contiguous(), total.contiguous()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    step = max(1, int(max_bytes) // max(8 * G, 1))
    parts = []
    for k0 in range(0, K, step):
        k1 = min(K, k0 + step)
        n = k1 - k0
        acc = torch.zeros((n, G), dtype=torch.int64, device=dev)          # the kernels' uint64: the same bits below 2^63
        if seed is not None:
            e0, e1 = int(s_rowptr[k0]), int(s_rowptr[k1])
            rows = torch.repeat_interleave(torch.arange(n, device=dev), s_rowptr[k0 + 1:k1 + 1] - s_rowptr[k0:k1], output_size=e1 - e0)
            acc[rows, s_col[e0:e1].long()] = s_cnt[e0:e1]                 # a seeded group's genes are unique: plain stores
        gp, tot = group_ptr[k0:k1 + 1], total[k0:k1]
        _lib.run(dev, "wgnn_pool_rows_accumulate", _ptr(rowptr), _ptr(col), _ptr(cnt), B, nnz, _ptr(gp), _ptr(members),
                 n, G, _ptr(acc), G, int(cells_per_unit), int(slab_genes), _ptr(status), flags, _stream(dev))
        head = (_ptr(acc), G, _ptr(tot), n, G, float(scale), float(threshold))
        n_out = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.run(dev, "wgnn_pool_rows_count", *head, _ptr(n_out), _ptr(status), _stream(dev))
        ptr, kept = _scan(n_out)
        out_col = torch.empty(kept, dtype=torch.int32, device=dev)
        out_val = torch.empty(kept, dtype=torch.float32, device=dev)
        out_cnt = torch.empty(kept, dtype=torch.int64, device=dev)
        _lib.run(dev, "wgnn_pool_rows_fill", *head, _ptr(ptr), _ptr(out_col), _ptr(out_val), _ptr(out_cnt), _ptr(status),
                 _stream(dev))
        parts.append((n_out, out_col, out_val, out_cnt))
    _check_status("pool_rows", int(status), _POOL_STATUS)
    out_rowptr = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    if parts:
        torch.cumsum(torch.cat([p[0] for p in parts]), 0, dtype=torch.int64, out=out_rowptr[1:])
        return (out_rowptr,) + tuple(torch.cat([p[i] for p in parts]) for i in (1, 2, 3))
    return (out_rowptr, torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float32, device=dev),
            torch.empty(0, dtype=torch.int64, device=dev))


def pool_rows(rowptr: torch.Tensor, col: torch.Tensor, cnt: torch.Tensor, lib: torch.Tensor, group: torch.Tensor, n_groups: int,
              scale: float = 1e4, threshold: float = 0.0, seed=None, cells_per_unit: int = 0, slab_genes: int = 0,
              max_bytes: int = POOL_CHUNK_BYTES, n_genes: Optional[int] = None):
    """``wgnn_pool_rows_accumulate`` / ``_count`` / ``_fill``: the cells of every group pooled into one log-normalised row of
    their summed counts - pseudobulk profiles.  ``(rowptr int32 / int64 [B+1], col int32, cnt float32)``: a device CSR of raw
    counts over the bundle's gene ids, every count an integer in [1, 2^23] (``pair_operand_check``); the rows need not be
    sorted.  ``lib`` int64 [B]: each cell's library size, columns outside the bundle included.  ``group`` int32 [B]: the cell's
    group in ``[0, n_groups)``, -1 = the cell takes no part.  ``n_genes``: the width of the vocabulary (default: the largest
    gene id of ``col`` and of ``seed``, plus one - a read-back).

    Group ``k`` leaves, in ascending gene id, ``float32(log1p(float64(c) / total[k] * scale))`` for every gene with
    ``c`` = the group's summed count ``> 0`` and a value ``> threshold`` (``>= 0``), ``total[k]`` = the group's summed ``lib``
    (the contract in ``include/wgnn.h``): integer sums, exact, the same bits for any order of the cells, any
    ``cells_per_unit`` / ``slab_genes`` (the kernel's unit geometry, 0 = its defaults) and any ``max_bytes`` - the groups are
    processed in chunks whose uint64 ``[groups, n_genes]`` accumulator stays under it.  Returns ``(rowptr int64 [K + 1], col
    int32, val float32, cnt int64, total int64 [K], n_cells int64 [K])`` on the device; the first three are what
    ``predict_rows`` takes, ``cnt`` holds the summed count of every kept entry.

    ``seed``: an earlier result's ``(rowptr, col, cnt, total, n_cells)`` over the same groups, made at a threshold that dropped
    nothing (0): this batch is pooled ON TOP of it - its counts are written into the accumulator before the kernel adds, its
    totals and cell counts are added - so two halves of a cohort equal the whole, bit for bit.

    A group whose summed library size reaches 2^53 raises ``ValueError`` naming it; a malformed operand the kernels skipped (a
    ``rowptr`` outside ``col``, a gene id outside ``[0, n_genes)``) raises ``WgnnError``; argument errors are ``ValueError``."""
    dev = _require_cuda(rowptr, col, cnt, lib, group)
    if rowptr.dim() != 1 or rowptr.shape[0] < 1:
        raise ValueError(f"malformed CSR: rowptr {tuple(rowptr.shape)}")
    B, K = int(rowptr.shape[0]) - 1, int(n_groups)
    if K < 0:
        raise ValueError(f"pool_rows: n_groups = {n_groups} must not be negative")
    if lib.dtype != torch.int64 or tuple(lib.shape) != (B,):
        raise ValueError(f"pool_rows: lib must be int64 [{B}]")
    _group_operand("pool_rows", ValueError, group, B, K, True, dtypes=(torch.int32,), says=f"pool_rows: group must be int32 [{B}]")
    s_total = s_cells = None
    if seed is not None:
        if len(seed) != 5:
            raise ValueError("pool_rows: seed is an earlier result's (rowptr, col, cnt, total, n_cells)")
        *seed, s_total, s_cells = seed
        if tuple(s_total.shape) != (K,) or tuple(s_cells.shape) != (K,):
            raise ValueError(f"pool_rows: seed must be an earlier result over the same {K} groups")
    if n_genes is None:
        n_genes = max(int(col.max()) + 1 if col.numel() else 0, int(seed[1].max()) + 1 if seed is not None and seed[1].numel() else 0)
    # one stable sort: the cells by group, the skipped ones last
    key = torch.where(group < 0, K, group.long())
    members = torch.sort(key, stable=True)[1].to(torch.int32)
    n_cells = torch.bincount(key, minlength=K + 1)[:K]
    group_ptr = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    torch.cumsum(n_cells, 0, out=group_ptr[1:])
    total = torch.zeros(K + 1, dtype=torch.int64, device=dev).index_add_(0, key, lib)[:K].contiguous()      # integer adds: exact
    if s_total is not None:
        total, n_cells = total + s_total.to(dev), n_cells + s_cells.to(dev)
    over = torch.nonzero((total >= 2 ** 53) | (total < 0))
    if over.numel():
        raise ValueError(f"pool_rows: group {int(over[0])} pools a library size of 2^53 or more (fp64 no longer holds it exactly)")
    out = pool_rows_grouped(rowptr, col, cnt, group_ptr, members, total, n_genes, scale, threshold, seed, cells_per_unit,
                            slab_genes, max_bytes)
    return out + (total, n_cells)


SOUP_MAX_ADD = 2 ** 23              # soup_rows: the most soup reads a cell takes (with a count of 2^23 the sum stays exact in float32)

_SOUP_STATUS = ((_lib.SOUP_BAD_ROWPTR, "rowptr points outside col / cnt, or a unit kept more entries than were counted"),
                (_lib.SOUP_BAD_COL, "a gene id is outside [0, n_genes)"),
                (_lib.SOUP_BAD_ADD, "an n_add is outside [0, 2^23]"))


def soup_rows(rowptr: torch.Tensor, col: torch.Tensor, cnt: torch.Tensor, lib: torch.Tensor, n_add: torch.Tensor, cdf: torch.Tensor,
              n_draws: int, *, row0: int = 0, draw0: int = 0, seed: int = 0, scale: float, threshold: float, slab_genes: int = 0,
              want_cnt: bool = False):
    """``wgnn_soup_rows_count`` / ``wgnn_soup_rows_fill``: every cell's count row with ``n_add`` reads of ambient RNA added to
    it, ``n_draws`` times - contaminated copies of a batch.  ``(rowptr int32 / int64 [B+1], col int32, cnt float32)``: a device
    CSR of raw counts over the bundle's gene ids, every count an integer in [1, 2^23] (``pair_operand_check``); the rows need
    not be sorted.  ``lib`` int64 [B]: each cell's library size, columns outside the bundle included.  ``n_add`` int64 [B]: the
    soup reads a cell takes, each in [0, 2^23].  ``cdf`` int64 [G + 2] (the kernel's uint64: the same bits below 2^63),
    ascending from 0: the soup profile as cumulative weights, bin ``g < G`` = bundle gene ``g``, bin ``G`` = a column outside
    the bundle, ``0 < cdf[-1]`` (checked here with one read-back).

    Unit ``q = r * n_draws + d`` leaves, in ascending gene id, ``float32(log1p(float64(c) / (lib[r] + n_add[r]) * scale))`` for
    every gene with ``c = cnt_r(g) + s(g) > 0`` and a value ``> threshold`` (``>= 0``), ``s`` = the unit's soup reads per gene -
    a pure function of ``(seed, row0 + r, draw0 + d, t)``, read ``t`` the same at every ``n_add`` that reaches it (the contract
    in ``include/wgnn.h``): the bits ``align_rows(..., normalize="lognorm")`` leaves on the contaminated count matrix.
    ``slab_genes``: the kernel's LDS slab width (0 = its default), which changes no bit.  Returns ``(rowptr int64 [B * n_draws
    + 1], col int32, val float32, soup_mapped int32 [B * n_draws])`` on the device - the first three are what ``predict_rows``
    takes, ``soup_mapped`` counts a unit's soup reads that fell on bundle genes - and with ``want_cnt`` a fifth, ``cnt`` int64:
    ``c`` of every kept entry.  The count pass, a ``torch.cumsum``, one read-back of the total to size the outputs, the fill
    pass, and a read-back of the status word - a ``rowptr`` outside ``col``, a gene id outside ``[0, G)`` or an ``n_add`` out of
    range raises ``WgnnError`` (the kernels skip it).  Argument errors are ``ValueError``."""
    dev = _require_cuda(rowptr, col, cnt, lib, n_add, cdf)
    _check_lognorm("soup_rows", scale, threshold)
    rowptr, col, cnt, lib, B, nnz, flags = _count_csr("soup_rows", rowptr, col, cnt, lib)
    D = int(n_draws)
    if n_add.dtype != torch.int64 or tuple(n_add.shape) != (B,):
        raise ValueError(f"soup_rows: n_add must be int64 [{B}]")
    if cdf.dtype != torch.int64 or cdf.dim() != 1 or cdf.shape[0] < 2 or cdf.shape[0] - 2 >= 2 ** 31 - 1:
        raise ValueError("soup_rows: cdf must be an int64 vector [n_genes + 2]")
    if D < 1:
        raise ValueError(f"soup_rows: n_draws = {n_draws} must be >= 1")
    if B * D >= 2 ** 31:
        raise ValueError("soup_rows: B * n_draws >= 2^31 (split the batch or the draws)")
    if int(row0) < 0 or int(draw0) < 0:
        raise ValueError("soup_rows: row0 and draw0 must not be negative")
    if not 0 <= int(slab_genes) <= _lib.SOUP_MAX_SLAB_GENES:
        raise ValueError(f"soup_rows: slab_genes = {slab_genes} must be in [0, {_lib.SOUP_MAX_SLAB_GENES}]")
    G = int(cdf.shape[0]) - 2
    if B and not int(cdf[-1]) > 0:
        raise ValueError("soup_rows: the profile's total weight cdf[-1] must be in (0, 2^63)")
    n_add, cdf = n_add.contiguous(), cdf.contiguous()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    n_out = torch.empty(B * D, dtype=torch.int32, device=dev)
    soup_mapped = torch.empty(B * D, dtype=torch.int32, device=dev)
    head = (_ptr(rowptr), _ptr(col), _ptr(cnt), B, nnz, _ptr(lib), _ptr(n_add), _ptr(cdf), G, D, int(row0), int(draw0),
            int(seed) & (2 ** 64 - 1), float(scale), float(threshold), int(slab_genes))
    _lib.run(dev, "wgnn_soup_rows_count", *head, _ptr(n_out), _ptr(soup_mapped), _ptr(status), flags, _stream(dev))
    out_rowptr, total = _scan(n_out)
    out_col = torch.empty(total, dtype=torch.int32, device=dev)
    out_val = torch.empty(total, dtype=torch.float32, device=dev)
    out_cnt = torch.empty(total, dtype=torch.int64, device=dev) if want_cnt else None
    if total:
        _lib.run(dev, "wgnn_soup_rows_fill", *head, _ptr(out_rowptr), _ptr(out_col), _ptr(out_val), _ptr(out_cnt),
                 _ptr(status), flags, _stream(dev))
    _check_status("soup_rows", int(status), _SOUP_STATUS)
    out = (out_rowptr, out_col, out_val, soup_mapped)
    return out + (out_cnt,) if want_cnt else out


_HOOD_STATUS = ((_lib.HOOD_BAD_INDEX, "a member names a row outside [0, n_rows)"),
                (_lib.HOOD_BAD_ROWPTR, "rowptr points outside col / cnt, hood_ptr is not ascending within [0, n_members], or a unit "
                                       "kept more entries than were counted"),
                (_lib.HOOD_BAD_COL, "a gene id is outside [0, n_genes)"),
                (_lib.HOOD_BAD_SIZE, f"a unit holds more than {_lib.HOOD_MAX_MEMBERS} members"))


def hood_rows(rowptr: torch.Tensor, col: torch.Tensor, cnt: torch.Tensor, lib: torch.Tensor, hood_ptr: torch.Tensor,
              members: torch.Tensor, n_genes: int, scale: float = 1e4, threshold: float = 0.0, slab_genes: int = 0):
    """``wgnn_hood_rows_count`` / ``wgnn_hood_rows_fill``: the count rows of every unit's members pooled into one log-normalised
    row - a cell with its nearest neighbours, one step of kNN smoothing.  ``(rowptr int32 / int64 [B+1], col int32, cnt
    float32)``: a device CSR of raw counts over the bundle's gene ids, every count an integer in [1, 2^23]
    (``pair_operand_check``); the rows need not be sorted.  ``lib`` int64 [B]: each cell's library size, columns outside the
    bundle included.  ``hood_ptr`` int64 [U + 1] (ascending) and ``members`` int32 [M]: unit ``q`` pools the rows
    ``members[hood_ptr[q]:hood_ptr[q + 1]]``, at most 256 of them; the units may overlap, a member listed twice adds twice, and
    a slice ``hood_ptr[q0:q1 + 1]`` next to the same ``members`` is a valid operand.  Making the lists - a kNN search - is the
    caller's.

    Unit ``q`` leaves, in ascending gene id, ``float32(log1p(float64(c) / total * scale))`` for every gene with ``c`` = the
    members' summed count ``> 0`` and a value ``> threshold`` (``>= 0``), ``total`` = the members' summed ``lib`` (the contract
    in ``include/wgnn.h``): integer sums in LDS, exact, the same bits for any order of the members and any ``slab_genes`` (the
    kernel's LDS slab width, 0 = its default).  A unit without a member leaves the empty row.  Returns ``(rowptr int64 [U + 1],
    col int32, val float32, cnt int64)`` on the device; the first three are what ``predict_rows`` takes, ``cnt`` holds the summed
    count of every kept entry.  The count pass, a ``torch.cumsum``, one read-back of the total to size the outputs, the fill
    pass, and a read-back of the status word - a member out of range, a ``rowptr`` outside ``col``, a gene id outside
    ``[0, n_genes)``, a malformed ``hood_ptr`` or a unit of more than 256 members raises ``WgnnError`` (the kernels skip it).
    Argument errors are ``ValueError``."""
    dev = _require_cuda(rowptr, col, cnt, lib, hood_ptr, members)
    _check_lognorm("hood_rows", scale, threshold)
    rowptr, col, cnt, lib, B, nnz, flags = _count_csr("hood_rows", rowptr, col, cnt, lib)
    G = int(n_genes)
    if hood_ptr.dtype != torch.int64 or hood_ptr.dim() != 1 or hood_ptr.shape[0] < 1:
        raise ValueError("hood_rows: hood_ptr must be an int64 vector [n_units + 1]")
    if members.dtype != torch.int32 or members.dim() != 1:
        raise ValueError("hood_rows: members must be an int32 vector")
    U, M = int(hood_ptr.shape[0]) - 1, int(members.shape[0])
    if not 0 <= G < 2 ** 31 or B >= 2 ** 31 or U >= 2 ** 31:
        raise ValueError("hood_rows: n_genes, the rows and the units must each be below 2^31")
    if not 0 <= int(slab_genes) <= _lib.HOOD_MAX_SLAB_GENES:
        raise ValueError(f"hood_rows: slab_genes = {slab_genes} must be in [0, {_lib.HOOD_MAX_SLAB_GENES}]")
    hood_ptr, members = hood_ptr.contiguous(), members.contiguous()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    n_out = torch.empty(U, dtype=torch.int32, device=dev)
    head = (_ptr(rowptr), _ptr(col), _ptr(cnt), B, nnz, _ptr(lib), _ptr(hood_ptr), _ptr(members), U, M, G, float(scale),
            float(threshold), int(slab_genes))
    _lib.run(dev, "wgnn_hood_rows_count", *head, _ptr(n_out), _ptr(status), flags, _stream(dev))
    out_rowptr, total = _scan(n_out)
    out_col = torch.empty(total, dtype=torch.int32, device=dev)
    out_val = torch.empty(total, dtype=torch.float32, device=dev)
    out_cnt = torch.empty(total, dtype=torch.int64, device=dev)
    if total:
        _lib.run(dev, "wgnn_hood_rows_fill", *head, _ptr(out_rowptr), _ptr(out_col), _ptr(out_val), _ptr(out_cnt),
                 _ptr(status), flags, _stream(dev))
    _check_status("hood_rows", int(status), _HOOD_STATUS)
    return out_rowptr, out_col, out_val, out_cnt


def attrib_rows(rowptr: torch.Tensor, col: torch.Tensor, raw: torch.Tensor, table: torch.Tensor, alpha: torch.Tensor,
                bias: torch.Tensor, *, head: Optional[tuple] = None, target: Optional[torch.Tensor] = None,
                self_rows: Optional[torch.Tensor] = None, direction: Optional[torch.Tensor] = None,
                scores: Optional[torch.Tensor] = None, accumulate: bool = False, want_direction: bool = False,
                unsure_threshold: float = 0.0, explicit_self: Optional[bool] = None, check_cols: bool = True):
    """``wgnn_attrib_rows``: per-entry attribution scores of one layer over a batch given as ``predict_rows`` takes it
    (``include/wgnn.h``).  ``H = bias.shape[0]`` valid columns; other widths are zero-padded here.

    Head mode, ``head = (w_head [C, H], b_head [C])`` (the model's last layer): the gather of ``predict_rows`` with the same
    bits, then ``score[j] = u_j <table[g_j], v>`` with ``v = (z > 0) * w_head[t]``.  ``target`` int [B] in ``[0, C)`` (checked
    here with one ``aminmax``) or None = the class ``predict_rows`` picks.  Returns ``(scores f32 [nnz], target int32 [B],
    logit f32 [B], base f32 [B], label int32 [B], v [B, H] | None)``: ``label`` as ``predict_rows`` gives it for
    ``unsure_threshold``, ``v`` only with ``want_direction``.  A head wider than the kernel stages
    in LDS raises ``WgnnError``.

    Direction mode, ``direction [B, H]`` (layers below the last): ``score[j] = u_j <table[g_j], direction[c]>``, written into
    ``scores`` (allocated when None) or added to it with ``accumulate``.  ``explicit_self`` picks the coefficient rule of
    layers with an explicit self term (default: ``self_rows is not None``).  Returns ``scores``."""
    if (head is None) == (direction is None):
        raise WgnnError("attrib_rows takes either head= (last layer) or direction= (layers below it)")
    dev = _require_cuda(rowptr, col, raw, table, alpha, bias, self_rows, target, direction, scores, *(head or ()))
    H = bias.shape[0]
    o = _row_operands("attrib_rows", rowptr, col, raw, table, alpha, H, check_cols)
    B, Hp, flags = o.B, o.Hp, o.flags
    nnz = o.col.shape[0]
    if scores is None:
        if accumulate:
            raise WgnnError("accumulate needs the scores to add to")
        scores = torch.empty(nnz, dtype=torch.float32, device=dev)
    elif scores.dtype != torch.float32 or scores.shape != (nnz,) or not scores.is_contiguous():
        raise WgnnError(f"scores must be a contiguous float32 [{nnz}]")
    if head is None:
        if direction.shape[0] != B or direction.shape[1] < H:
            raise WgnnError(f"direction must be [{B}, >= {H}]")
        direction = _rowmajor(direction.float()) if direction.shape[1] == Hp else _pad_cols(direction[:, :H], Hp)
        if explicit_self is None:
            explicit_self = self_rows is not None
        flags |= (_lib.ATTRIB_ACCUMULATE if accumulate else 0) | (_lib.ATTRIB_EXPLICIT_SELF if explicit_self else 0)
        _lib.run(dev, "wgnn_attrib_rows", *o.c_args, None, None, 0, None, None, 0, None, 0.0, None, _ptr(direction),
                 direction.stride(0), _ptr(scores), None, None, None, None, 0, flags, _stream(dev))
        return scores
    if accumulate:
        raise WgnnError("head mode overwrites the scores")
    w_head, b_head, n_cls = _fused_head(head, Hp, lambda c: WgnnError(
        f"attrib_rows: a [{c}, {Hp}] head does not fit the {HEAD_LDS_BYTES >> 10} KiB the kernel stages in LDS"))
    bias = _pad_cols(bias, Hp)
    self_rows = _self_rows(self_rows, B, B, H, Hp, WgnnError)
    if target is not None:
        if target.shape != (B,):
            raise WgnnError(f"target must hold one class per cell ([{B}])")
        if B:
            lo, hi = torch.aminmax(target)
            if int(lo) < 0 or int(hi) >= n_cls:
                raise WgnnError(f"target class out of range [0, {n_cls}) (min {int(lo)}, max {int(hi)})")
        target = target.to(torch.int32).contiguous()
    target_out = torch.empty(B, dtype=torch.int32, device=dev)
    logit = torch.empty(B, dtype=torch.float32, device=dev)
    base = torch.empty(B, dtype=torch.float32, device=dev)
    label = torch.empty(B, dtype=torch.int32, device=dev)
    v = torch.empty((B, Hp), dtype=torch.float32, device=dev) if want_direction else None
    _lib.run(dev, "wgnn_attrib_rows", *o.c_args, _ptr(bias), _ptr(self_rows),
             self_rows.stride(0) if self_rows is not None else 0, _ptr(w_head), _ptr(b_head), n_cls, _ptr(target),
             float(unsure_threshold), _ptr(label), None, 0, _ptr(scores), _ptr(target_out), _ptr(logit), _ptr(base), _ptr(v),
             Hp if v is not None else 0, flags, _stream(dev))
    return scores, target_out, logit, base, label, (v if v is None or Hp == H else v[:, :H])


def rows_topk(rowptr: torch.Tensor, col: torch.Tensor, scores: torch.Tensor, k: int):
    """``wgnn_rows_topk``: per CSR row the ``k`` (1..64) entries with the largest score, descending, equal scores by the lower
    CSR position.  Returns ``(gene int32 [B, k], score f32 [B, k])``: -1 / 0 where a row has fewer than ``k`` entries."""
    dev = _require_cuda(rowptr, col, scores)
    if not 1 <= int(k) <= 64:
        raise WgnnError(f"rows_topk: k = {k} is outside [1, 64]")
    rowptr, col, scores, B, _, flags = _csr_operand("rows_topk", WgnnError, rowptr, col, scores, "scores")
    gene = torch.empty((B, int(k)), dtype=torch.int32, device=dev)
    top = torch.empty((B, int(k)), dtype=torch.float32, device=dev)
    _lib.run(dev, "wgnn_rows_topk", _ptr(rowptr), _ptr(col), _ptr(scores), B, int(k), _ptr(gene), _ptr(top),
             flags, _stream(dev))
    return gene, top


def group_gene_reduce(rowptr: torch.Tensor, col: torch.Tensor, scores: torch.Tensor, group: torch.Tensor, n_groups: int,
                      n_genes: int, out: Optional[tuple] = None, accumulate: bool = False, check: bool = True):
    """``wgnn_group_gene_reduce``: per (group, gene) the fp64 sum of the f32 ``scores`` of a batch given cell-major as
    ``attrib_rows`` hands it over (``rowptr`` int32 / int64 [B+1], ``col`` int32 gene ids in ``[0, n_genes)``, one score per
    stored entry; a cell lists a gene at most once) and the number of cells behind it.  ``group`` int [B]: a cell's group in
    ``[0, n_groups)``, or -1 = the cell takes no part.

    Returns ``(sum f64 [n_groups, n_genes], count int32 [n_groups, n_genes])`` - ``out`` when given (every element is
    written, the caller does not pre-clear), added to with ``accumulate``.  The batch is re-ordered gene-major by the
    library's stable transpose (``group >= 0`` as its row mask; a stable sort above that kernel's 32 768 columns), then one
    wavefront per gene adds in a fixed order: no atomics, two calls are bit-identical.  ``check``: verify the ranges of
    ``group`` and ``col`` (one ``aminmax`` each and a read-back)."""
    name = "group_gene_reduce"
    dev = _require_cuda(rowptr, col, scores, group, *(out or ()))
    K, G = int(n_groups), int(n_genes)
    if K <= 0 or G <= 0:
        raise WgnnError(f"{name}: n_groups = {K} and n_genes = {G} must be positive")
    rowptr, col, scores, B, nnz, _ = _csr_operand(name, WgnnError, rowptr, col, scores, "scores")
    if nnz >= 2 ** 31:
        raise WgnnError(f"{name}: nnz >= 2^31 (split the batch and accumulate)")
    _group_operand(name, WgnnError, group, B, K, check)
    if check:
        check_gene_ids(col, G)
    if out is None:
        if accumulate:
            raise WgnnError("accumulate needs the tables to add to (out=)")
        out = (torch.empty((K, G), dtype=torch.float64, device=dev), torch.empty((K, G), dtype=torch.int32, device=dev))
    total, count = out
    if total.dtype != torch.float64 or count.dtype != torch.int32 or total.shape != (K, G) or count.shape != (K, G) or \
            not total.is_contiguous() or not count.is_contiguous():
        raise WgnnError(f"out must be contiguous (float64 [{K}, {G}], int32 [{K}, {G}])")
    group = group.to(torch.int32).contiguous()
    t_rowptr, t_cell, t_score = _gene_major(rowptr, col, scores, B, G, group)
    ws, ws_bytes = _workspace(dev, "wgnn_group_gene_reduce_workspace", B, nnz, K, G)     # none today: the partial sums live in LDS
    _lib.run(dev, "wgnn_group_gene_reduce", _ptr(t_rowptr), _ptr(t_cell), _ptr(t_score), _ptr(group), B, K, G,
             _ptr(total), _ptr(count), _ptr(ws), ws_bytes, _lib.MARKERS_ACCUMULATE if accumulate else 0, _stream(dev))
    return total, count


RANK_GENES_MAX_ROWS = 2 ** 20       # wgnn_rank_genes_groups' largest batch: N^3 must fit int64
RANK_GENES_MAX_GROUPS = 4096        # and its most groups


def rank_genes_groups(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, group: torch.Tensor, n_groups: int,
                      n_genes: int, check: bool = True, out: Optional[tuple] = None):
    """``wgnn_rank_genes_groups``: the integer tables of a Wilcoxon rank-sum test of every gene, each group of cells against
    the rest (``include/wgnn.h`` has the definition).  The batch comes cell-major as ``group_gene_reduce`` takes it (``rowptr``
    int32 / int64 [B+1], ``col`` int32 gene ids in ``[0, n_genes)``, ``val`` f32; a cell lists a gene at most once); ``group``
    int32 / int64 [B]: a cell's group in ``[0, n_groups)``, or -1 = the cell takes no part.  ``B <= 2^20``, ``n_groups <= 4096``.

    Returns ``(rank2_sum int64 [K, G], count int32 [K, G], tie_sum int64 [G], group_size int64 [K])``: per (group, gene) the
    doubled tie-averaged ranks of ALL the group's cells added up (a cell that does not list the gene holds +0.0) and the
    group's stored entries, per gene the tie term ``sum(t^3 - t)``, per group its cells.  ``out``: the first three to write
    into - ``rank2_sum`` and ``count`` may be views with unit column stride and a wider row stride; every element of the
    [K, G] / [G] tables is written, nothing else.  The batch is re-ordered gene-major by the library's stable transpose
    (``group >= 0`` as its row mask; a stable sort above that kernel's 32 768 columns), then ranks are counted, not sorted, in
    integers: two calls are bit-identical and the tables do not depend on the order of cells or of a cell's genes.  ``check``:
    verify the ranges of ``group`` and ``col`` (one ``aminmax`` each and a read-back); without it an out-of-range GROUP takes no
    part (an out-of-range gene id is the transpose's to fault on).  Argument errors are ``ValueError``."""
    name = "rank_genes_groups"
    dev = _require_cuda(rowptr, col, val, group, *(out or ()))
    K, G = int(n_groups), int(n_genes)
    if not 1 <= K <= RANK_GENES_MAX_GROUPS:
        raise ValueError(f"{name}: n_groups = {K} must be in [1, {RANK_GENES_MAX_GROUPS}]")
    if G <= 0:
        raise ValueError(f"{name}: n_genes = {G} must be positive")
    rowptr, col, val, B, nnz, _ = _csr_operand(name, ValueError, rowptr, col, val, "val")
    if B > RANK_GENES_MAX_ROWS:
        raise ValueError(f"{name}: {B} cells > 2^20 (the tie term N^3 must fit int64)")
    if nnz >= 2 ** 31:
        raise ValueError(f"{name}: nnz >= 2^31")
    _group_operand(name, ValueError, group, B, K, check)
    if check:
        check_gene_ids(col, G)
    if out is None:
        out = (torch.empty((K, G), dtype=torch.int64, device=dev), torch.empty((K, G), dtype=torch.int32, device=dev),
               torch.empty(G, dtype=torch.int64, device=dev))
    rank2_sum, count, tie_sum = out
    _view_2d(name, ValueError, "out's rank2_sum", rank2_sum, torch.int64, K, G)
    _view_2d(name, ValueError, "out's count", count, torch.int32, K, G)
    if tie_sum.dtype != torch.int64 or tuple(tie_sum.shape) != (G,) or (G > 1 and tie_sum.stride(0) != 1):
        raise ValueError(f"{name}: out's tie_sum must be a dense int64 [{G}]")
    group = group.to(torch.int32).contiguous()
    in_range = (group >= 0) & (group < K)
    group_size = torch.bincount(group[in_range].long(), minlength=K).to(torch.int64)
    t_rowptr, t_cell, t_val = _gene_major(rowptr, col, val, B, G, group)
    ws, ws_bytes = _workspace(dev, "wgnn_rank_genes_groups_workspace", B, nnz, K, G)
    _lib.run(dev, "wgnn_rank_genes_groups", _ptr(t_rowptr), _ptr(t_cell), _ptr(t_val), _ptr(group), _ptr(group_size),
             B, K, G, _ptr(rank2_sum), _ld(rank2_sum, K, G), _ptr(count), _ld(count, K, G), _ptr(tie_sum), _ptr(ws), ws_bytes, 0,
             _stream(dev))
    return rank2_sum, count, tie_sum, group_size


def group_class_reduce(logits: torch.Tensor, label: torch.Tensor, group: torch.Tensor, n_groups: int,
                       out: Optional[tuple] = None, accumulate: bool = False, check: bool = True):
    """``wgnn_group_class_reduce``: per (group, class) the fp64 sum of the cells' softmax probabilities, taken in fp64 from the
    f32 ``logits`` [B, C] that ``predict_rows`` leaves (any row stride ``>= C``), with the votes of its ``label`` int32 /
    int64 [B] (a class id, or -1 = unsure).  ``group`` int32 / int64 [B]: a cell's group in ``[0, n_groups)``, or -1 = the cell
    takes no part.  A cell whose logits hold a NaN or a +inf, or are all -inf, is bad: counted in ``tally[:, 2]`` and in
    nothing else.

    Returns ``(prob_sum f64 [K, C], conf_sum f64 [K], votes int32 [K, C], tally int32 [K, 3])`` with ``tally[k] = (cells that
    took part, cells with label -1, bad cells)`` - ``out`` when given (every element is written, the caller does not
    pre-clear), added to with ``accumulate``.  The batch is re-ordered group-major on the device (a stable sort of the group
    ids, the groups' bounds by a search in the sorted ids: no read-back), then one wavefront per 256-cell chunk of a group
    adds in a fixed order: no atomics, two calls are bit-identical.  ``check``: verify the range of ``group`` (one ``aminmax``
    and a read-back); without it an id outside ``[0, n_groups)`` takes no part."""
    dev = _require_cuda(logits, label, group, *(out or ()))
    K = int(n_groups)
    if K <= 0:
        raise WgnnError(f"group_class_reduce: n_groups = {K} must be positive")
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.shape[1] < 1:
        raise WgnnError("group_class_reduce takes logits float32 [B, C] with C >= 1")
    B, n_cls = logits.shape
    if B >= 2 ** 31:
        raise WgnnError("group_class_reduce: B >= 2^31 (split the batch and accumulate)")
    if label.shape != (B,) or label.dtype not in (torch.int32, torch.int64):
        raise WgnnError(f"label must hold one int32 / int64 class id per cell ([{B}]), got {label.dtype} {tuple(label.shape)}")
    _group_operand("group_class_reduce", WgnnError, group, B, K, check)
    if out is None:
        if accumulate:
            raise WgnnError("accumulate needs the tables to add to (out=)")
        out = (torch.empty((K, n_cls), dtype=torch.float64, device=dev), torch.empty(K, dtype=torch.float64, device=dev),
               torch.empty((K, n_cls), dtype=torch.int32, device=dev), torch.empty((K, 3), dtype=torch.int32, device=dev))
    if len(out) != 4:
        raise WgnnError("out must be (prob_sum, conf_sum, votes, tally)")
    want = ((K, n_cls), torch.float64), ((K,), torch.float64), ((K, n_cls), torch.int32), ((K, 3), torch.int32)
    if any(tuple(o.shape) != s or o.dtype != d or not o.is_contiguous() for o, (s, d) in zip(out, want)):
        raise WgnnError(f"out must be contiguous (float64 [{K}, {n_cls}], float64 [{K}], int32 [{K}, {n_cls}], int32 [{K}, 3])")
    prob_sum, conf_sum, votes, tally = out
    if not _row_strided(logits, B, n_cls):
        logits = logits.contiguous()
    label = label.to(torch.int32).contiguous()
    order, seg_ptr = _group_major(group, K)
    ws, ws_bytes = _workspace(dev, "wgnn_group_class_reduce_workspace", B, K, n_cls)     # K, C >= 1: never empty
    _lib.run(dev, "wgnn_group_class_reduce", _ptr(logits), _ld(logits, B, n_cls), _ptr(label), _ptr(order), _ptr(seg_ptr), B, K,
             n_cls, _ptr(prob_sum), _ptr(conf_sum), _ptr(votes), _ptr(tally), _ptr(ws), ws_bytes,
             _lib.CLUSTERS_ACCUMULATE if accumulate else 0, _stream(dev))
    return prob_sum, conf_sum, votes, tally


_ALIGN_STATUS = ((_lib.ALIGN_BAD_COL, "a CSR entry's column is outside [0, n_cols)"),
                 (_lib.ALIGN_BAD_MAP, "a gene_map value is outside [-1, n_genes)"),
                 (_lib.ALIGN_BAD_ROWPTR, "a row kept more entries than were counted"),
                 (_lib.ALIGN_BAD_VALUE, "a count is negative, NaN or infinite, or the library size of a row that holds counts "
                                        "is not a finite number > 0"))


def _align_operand(name: str, expr, gene_map: torch.Tensor, n_genes: int):
    """The checks ``align_rows`` and ``coverage_rows`` make of their batch: ``(dev, x, ld, rowptr, col, val, B, n_cols, G,
    flags)`` as the C entry points take them (the other form's tensors ``None``)."""
    dense = isinstance(expr, torch.Tensor)
    if not dense and not (isinstance(expr, (tuple, list)) and len(expr) == 3):
        raise WgnnError(f"{name} takes a dense [B, n_cols] tensor or a (rowptr, col, val) triple")
    dev = _require_cuda(gene_map, *((expr,) if dense else expr))
    if gene_map.dtype != torch.int32 or gene_map.dim() != 1 or not gene_map.is_contiguous():
        raise WgnnError("gene_map must be a contiguous int32 vector")
    n_cols, G = int(gene_map.shape[0]), int(n_genes)
    if G <= 0:
        raise WgnnError(f"{name}: n_genes = {G} must be positive")
    x = rowptr = col = val = None
    ld = flags = 0
    if dense:
        x = expr
        if x.dtype != torch.float32 or x.dim() != 2:
            raise WgnnError(f"{name} takes a 2-D float32 matrix, got {x.dtype} with {x.dim()} dimensions")
        if x.shape[1] != n_cols:
            raise WgnnError(f"the matrix has {x.shape[1]} columns, gene_map {n_cols} entries")
        B = int(x.shape[0])
        if not _row_strided(x, B, n_cols):
            raise WgnnError(f"{name} takes row-major rows (unit column stride, row stride >= n_cols)")
        ld = _ld(x, B, n_cols)
    else:
        if not all(t.is_contiguous() for t in expr):          # this batch is refused, not copied
            raise WgnnError(f"{name} takes contiguous rowptr, col and val")
        rowptr, col, val, B, _, flags = _csr_operand(name, WgnnError, *expr, "val")
    return dev, x, ld, rowptr, col, val, B, n_cols, G, flags


def align_rows(expr, gene_map: torch.Tensor, n_genes: int, threshold: float = 0.0, normalize=None, scale: float = 1e4,
               library_size=None, groups=None):
    """``wgnn_align_count`` / ``wgnn_align_fill``: a batch over the caller's gene list as the bundle-vocabulary CSR that
    ``predict_rows`` takes.  ``expr``: a dense float32 ``[B, n_cols]`` device matrix (unit column stride; the row stride is its
    leading dimension) or a device ``(rowptr int32 / int64 [B+1], col int32, val float32)`` triple over the caller's columns.
    ``gene_map`` int32 ``[n_cols]`` on the device: a column's bundle gene id in ``[0, n_genes)``, or -1.

    An entry is kept iff its column maps to a gene and its value is ``> threshold`` (a NaN is dropped); a row's kept entries
    keep their input order and their bits.  Returns ``(rowptr int64 [B+1], col int32, raw float32)`` on the device: the count
    pass, a ``torch.cumsum``, one read-back of the total to size the outputs, the fill pass, and a read-back of the status word -
    a column outside ``[0, n_cols)`` or a map value outside ``[-1, n_genes)`` raises ``WgnnError`` (the kernels skip it).

    ``normalize="lognorm"``: ``expr`` holds raw counts and the values that leave are Seurat's ``LogNormalize``
    (``wgnn_align_count_ln`` / ``wgnn_align_fill_ln``, the contract in ``include/wgnn.h``):
    ``float32(log1p(float64(x) / total * scale))`` with ``total`` the fp64 sum of the cell's WHOLE row, columns outside the
    bundle included; an entry is kept iff its column maps, its count is ``> 0`` and the value is ``> threshold``
    (``threshold >= 0``, else ``ValueError``).  No normalised matrix is stored.  ``library_size``: a ``[B]`` vector (any real
    dtype, made fp64 on the device) that replaces the totals.  A negative, NaN or infinite count on any column, or a library
    size that is not finite and ``> 0`` on a cell that holds a count, raises ``WgnnError``.  Still two host synchronisations.

    ``groups`` (``normalize="lognorm"`` only, else ``ValueError``): ``(col_group int32 [n_cols], group_ptr int32 [n_groups + 1],
    group_cols int32 [n_members])`` on the device - the columns that name one bundle gene, whose counts are added per cell
    before the logarithm (``wgnn_align_count_ln_merge`` / ``wgnn_align_fill_ln_merge``; the contract in ``include/wgnn.h``):
    one entry per cell and gene, at the place of the first member that counts.  ``None``, or tables without a group, run the
    kernels above - a caller without duplicates never runs the merging walk."""
    if normalize not in (None, "lognorm"):
        raise ValueError(f"normalize = {normalize!r}: pass None or \"lognorm\"")
    lognorm = normalize is not None
    if lognorm and not float(threshold) >= 0:
        raise ValueError(f"threshold = {threshold} must be >= 0 when normalising (a dropped entry counts as 0)")
    if lognorm and not (0 < float(scale) < float("inf")):
        raise ValueError(f"scale = {scale} must be positive and finite")
    if not lognorm and library_size is not None:
        raise ValueError("library_size belongs to normalize=\"lognorm\"")
    merge = ()
    if groups is not None:
        col_group, group_ptr, group_cols = groups
        if not lognorm:
            raise ValueError("groups belongs to normalize=\"lognorm\": counts add, log-values do not")
        _require_cuda(gene_map, col_group, group_ptr, group_cols)
        for name, tab in (("col_group", col_group), ("group_ptr", group_ptr), ("group_cols", group_cols)):
            if tab.dtype != torch.int32 or tab.dim() != 1 or not tab.is_contiguous():
                raise WgnnError(f"{name} must be a contiguous int32 vector")
        if col_group.shape[0] != gene_map.shape[0] or group_ptr.shape[0] < 1:
            raise WgnnError(f"col_group has {col_group.shape[0]} entries for {gene_map.shape[0]} columns, group_ptr "
                            f"{group_ptr.shape[0]}")
        if group_ptr.shape[0] > 1:                                 # no group: the walk without merging
            merge = (_ptr(col_group), _ptr(group_ptr), _ptr(group_cols), int(group_ptr.shape[0]) - 1, int(group_cols.shape[0]))
    sfx = "_merge" if merge else ""
    dev, x, ld, rowptr, col, val, B, n_cols, G, flags = _align_operand("align_rows", expr, gene_map, n_genes)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    head = (_ptr(x), ld, _ptr(rowptr), _ptr(col), _ptr(val), B, n_cols, _ptr(gene_map), G, float(threshold))
    if lognorm:
        lib = None
        if library_size is not None:
            lib = library_size if isinstance(library_size, torch.Tensor) else torch.as_tensor(library_size)
            if lib.dim() != 1 or lib.shape[0] != B or lib.is_complex():
                raise ValueError(f"library_size must be a real vector with one entry per cell ({B}), got {tuple(lib.shape)}")
            lib = lib.to(dev).to(torch.float64).contiguous()       # widened on the device
        row_total = torch.empty(B, dtype=torch.float64, device=dev)    # alive until the fill pass has been launched
        ln = (_ptr(row_total), float(scale))                       # the count pass stores the totals, the fill pass reads them
        _lib.run(dev, "wgnn_align_count_ln" + sfx, *head, *merge, _ptr(lib), *ln, _ptr(counts), _ptr(status), flags,
                 _stream(dev))
    else:
        _lib.run(dev, "wgnn_align_count", *head, _ptr(counts), _ptr(status), flags, _stream(dev))
    out_rowptr, total = _scan(counts)
    out_col = torch.empty(total, dtype=torch.int32, device=dev)
    out_raw = torch.empty(total, dtype=torch.float32, device=dev)
    if lognorm:
        _lib.run(dev, "wgnn_align_fill_ln" + sfx, *head, *merge, *ln, _ptr(out_rowptr), _ptr(out_col), _ptr(out_raw),
                 _ptr(status), flags, _stream(dev))
    else:
        _lib.run(dev, "wgnn_align_fill", *head, _ptr(out_rowptr), _ptr(out_col), _ptr(out_raw), _ptr(status), flags,
                 _stream(dev))
    bits = int(status)
    merge_text = ("or a group table (col_group, group_ptr, group_cols) points outside its range",)
    _check_status("align_rows", bits, _ALIGN_STATUS, merge_text if merge and bits & _lib.ALIGN_BAD_MAP else ())
    return out_rowptr, out_col, out_raw


def coverage_rows(expr, gene_map: torch.Tensor, n_genes: int):
    """``wgnn_coverage_rows``: what of a batch over the caller's gene list the bundle's vocabulary sees.  ``expr`` and
    ``gene_map`` as ``align_rows`` takes them (a dense float32 ``[B, n_cols]`` device matrix or a device CSR triple over the
    caller's columns); the batch is only read.  An entry counts iff its value is finite and ``> 0``.

    Returns six device tensors ``(n_expressed int32 [B], n_mapped int32 [B], n_bad int32 [B], total float64 [B],
    total_mapped float64 [B], col_cells int32 [n_cols])``: per cell the counting entries over all columns and over the mapped
    ones, the entries that are negative, NaN or infinite (in no other output), the fp64 sum of the counting values over all
    columns - the very bits ``align_rows(..., normalize="lognorm")`` divides by - and over the mapped ones; per column the
    cells in which it counts.  Two calls give identical bits.  One read-back, of the status word: a column outside
    ``[0, n_cols)`` or a map value outside ``[-1, n_genes)`` raises ``WgnnError`` with ``align_rows``' message."""
    dev, x, ld, rowptr, col, val, B, n_cols, G, flags = _align_operand("coverage_rows", expr, gene_map, n_genes)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    n_expressed, n_mapped, n_bad = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    total, total_mapped = (torch.empty(B, dtype=torch.float64, device=dev) for _ in range(2))
    col_cells = torch.empty(n_cols, dtype=torch.int32, device=dev)       # cleared by the entry point, on the stream
    _lib.run(dev, "wgnn_coverage_rows", _ptr(x), ld, _ptr(rowptr), _ptr(col), _ptr(val), B, n_cols, _ptr(gene_map), G,
             _ptr(n_expressed), _ptr(n_mapped), _ptr(n_bad), _ptr(total), _ptr(total_mapped), _ptr(col_cells),
             _ptr(status), flags, _stream(dev))
    _check_status("coverage_rows", int(status), _ALIGN_STATUS)
    return n_expressed, n_mapped, n_bad, total, total_mapped, col_cells


KNN_MAX_K, KNN_MAX_D, KNN_MAX_SPLITS = _lib.KNN_MAX_K, _lib.KNN_MAX_D, _lib.KNN_MAX_SPLITS      # wgnn_knn_rows' limits
KNN_WORKSPACE_BYTES = 1 << 30       # knn_rows: the [splits, queries of a chunk, k] 64-bit partial lists stay under this


def _knn_rows_operand(name: str, what: str, t: torch.Tensor) -> torch.Tensor:
    """A [n, D] float32 matrix as ``wgnn_knn_rows`` reads it: unit column stride, rows 16-byte aligned, D a multiple of 4
    (zero columns are appended otherwise: they add ``fmaf(0, 0, d)``, which changes no bit)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
        raise ValueError(f"{name}: {what} must be a 2-D float32 tensor")
    if t.shape[1] % 4:
        return _pad_cols(t, -(-t.shape[1] // 4) * 4)
    if t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < t.shape[1] or t.data_ptr() % 16:
        return t.contiguous()
    return t


def knn_rows(x: torch.Tensor, k: int, queries: Optional[torch.Tensor] = None, exclude_self: bool = True, n_splits: int = 0,
             self_offset: int = 0, out: Optional[tuple] = None):
    """``wgnn_knn_rows``: for every query row the ``k`` (1..64) nearest rows of ``x`` [n_c, D] float32 under squared Euclidean
    distance - exact brute force on the device, the [n_q, n_c] distance matrix is never stored (``include/wgnn.h`` has the
    numerics contract: ``t = q[j] - x[j]; d = fmaf(t, t, d)``, j ascending).  ``queries`` [n_q, D] = None: the rows of ``x``
    themselves.  ``exclude_self``: query ``i`` is row ``self_offset + i`` of ``x`` and is left out of its own list (with
    ``queries`` a sub-range of ``x``, pass where it starts); False: no row is left out - a query that is a candidate comes
    first at distance 0.

    Returns ``(idx int32 [n_q, k], d2 f32 [n_q, k])``, ascending under the total order (d2, index): equal distances go to the
    lower index, a NaN distance is never listed, and with fewer than ``k`` candidates the tail holds -1 / +inf.  ``out``: the
    two tensors to write into - views with unit column stride and a wider row stride (the same for both) are taken, nothing
    outside ``[:, :k]`` is written.  ``n_splits`` (0 = chosen from the sizes, else 1..64): how many contiguous candidate ranges
    are scanned side by side and merged; a large ``n_q`` is chunked over query ranges (halved until the partial lists of
    a chunk fit ``KNN_WORKSPACE_BYTES``).  Neither changes a bit, and two calls are bit-identical.  ``D`` (after padding to a multiple of
    4) must be in [4, 1024].  Argument errors are ``ValueError``."""
    name = "knn_rows"
    dev = _require_cuda(x, queries, *(out or ()))
    k, n_splits = int(k), int(n_splits)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"{name}: k = {k} is outside [1, {KNN_MAX_K}]")
    if not 0 <= n_splits <= KNN_MAX_SPLITS:
        raise ValueError(f"{name}: n_splits = {n_splits} is outside [0, {KNN_MAX_SPLITS}] (0 = chosen from the sizes)")
    x = _knn_rows_operand(name, "x", x)
    q = x if queries is None else _knn_rows_operand(name, "queries", queries)
    D, n_q, n_c = int(x.shape[1]), int(q.shape[0]), int(x.shape[0])
    if q.shape[1] != D:
        raise ValueError(f"{name}: queries have {q.shape[1]} columns, x {D}")
    if not 4 <= D <= KNN_MAX_D:
        raise ValueError(f"{name}: D = {D} is outside [4, {KNN_MAX_D}]")
    if n_q >= 2 ** 31 or n_c >= 2 ** 31:
        raise ValueError(f"{name}: n_q and n_c must be below 2^31")
    first = -1
    if exclude_self:
        first = int(self_offset)
        if first < 0 or first + n_q > n_c:
            raise ValueError(f"{name}: exclude_self says query i is row self_offset + i of x: self_offset = {first} with "
                             f"{n_q} queries does not fit {n_c} rows (pass exclude_self=False for queries that are no rows of x)")
    if out is None:
        out = (torch.empty((n_q, k), dtype=torch.int32, device=dev), torch.empty((n_q, k), dtype=torch.float32, device=dev))
    idx, d2 = out
    _view_2d(name, ValueError, "out's idx", idx, torch.int32, n_q, k)
    _view_2d(name, ValueError, "out's d2", d2, torch.float32, n_q, k)
    ld_out = _ld(idx, n_q, k)
    if _ld(d2, n_q, k) != ld_out:
        raise ValueError(f"{name}: out's idx and d2 must share one row stride")
    if n_q == 0:
        return idx, d2
    sizes = lambda n: ("wgnn_knn_workspace_bytes", n, n_c, k, n_splits)
    # chunks of consecutive queries, halved until the partial lists of one chunk ([splits, queries, k] 64-bit keys) fit the budget
    step = n_q
    while _workspace_bytes(*sizes(step)) > KNN_WORKSPACE_BYTES and step > 1:
        step = -(-step // 2)
    have = (None, 0)                                          # one allocation serves every chunk that it is large enough for
    for r0 in range(0, n_q, step):
        r1 = min(n_q, r0 + step)
        ws, ws_bytes = have = _workspace(dev, *sizes(r1 - r0), have=have)
        _lib.run(dev, "wgnn_knn_rows", q.data_ptr() + r0 * q.stride(0) * 4, q.stride(0), r1 - r0, _ptr(x), x.stride(0), n_c,
                 D, k, first + r0 if first >= 0 else -1, n_splits,
                 idx.data_ptr() + r0 * ld_out * 4, d2.data_ptr() + r0 * ld_out * 4, ld_out, _ptr(ws), ws_bytes, 0, _stream(dev))
    return idx, d2


KNN_SEGMENTS_MAX_SEGS, KNN_SEGMENTS_MAX_LIST = _lib.KNN_SEGMENTS_MAX_SEGS, _lib.KNN_SEGMENTS_MAX_LIST      # wgnn_knn_segments' limits

_KNN_SEGMENTS_STATUS = ((_lib.KNN_SEGMENTS_BAD_ORDER, "order names a row outside [0, n_rows)"),)


class SegmentLists(NamedTuple):
    """What ``knn_segments`` returns, on the device.  ``idx`` int32 / ``d2`` f32 [n, n_groups, k]: per row and group the ``k``
    nearest rows of that group, ascending under (d2, row id), the row itself left out, -1 / +inf where the group holds fewer.
    ``merged_idx`` / ``merged_d2`` [n, n_groups * k]: the same entries as one ascending list, the -1 / +inf entries last."""
    idx: torch.Tensor
    d2: torch.Tensor
    merged_idx: torch.Tensor
    merged_d2: torch.Tensor


def knn_segments(x: torch.Tensor, group: torch.Tensor, n_groups: int, k: int, n_splits: int = 0) -> SegmentLists:
    """``wgnn_knn_segments``: for every row of ``x`` [n, D] float32 its ``k`` nearest rows in EACH of ``n_groups`` groups of the
    rows - the lists of a batch-balanced kNN graph - exact brute force on the device in one launch pair, the rows left where
    they are (``include/wgnn.h`` has the contract; the distance is ``knn_rows``' chain, so a pair's distance carries the bits
    ``knn_rows`` gives it).  ``group``: an integer id in ``[0, n_groups)`` per row; an empty group is allowed, anything else is
    a ``ValueError``.  ``n_groups`` in [1, 64], ``k`` in [1, 64], ``n_groups * k <= 64``.

    Returns ``SegmentLists``.  The order within a list and in the merged list is (d2, row id): equal distances go to the lower
    row id, within a group and across groups; a NaN distance is never listed.  The groups reach the kernel as a stable sort of
    the ids (rows ascending within a group) and the groups' bounds, both built on the device.  ``n_splits`` (0 = chosen from
    the sizes, else the sub-ranges of every group's scan, lowered to ``64 // n_groups``) and the chunking of a large ``n`` over
    query ranges (halved until the partial lists of a chunk fit ``KNN_WORKSPACE_BYTES``) change no bit; two calls are
    bit-identical.  ``D`` is zero-padded to a multiple of 4 as ``knn_rows`` does and must then be in [4, 1024].  CPU tensors
    raise ``WgnnError``; argument errors are ``ValueError``."""
    name = "knn_segments"
    dev = _require_cuda(x, group)
    n_groups, k, n_splits = int(n_groups), int(k), int(n_splits)
    if not 1 <= n_groups <= KNN_SEGMENTS_MAX_SEGS or not 1 <= k <= KNN_MAX_K or n_groups * k > KNN_SEGMENTS_MAX_LIST:
        raise ValueError(f"{name}: n_groups = {n_groups} and k = {k} must be in [1, {KNN_SEGMENTS_MAX_SEGS}] and [1, {KNN_MAX_K}] "
                         f"with n_groups * k <= {KNN_SEGMENTS_MAX_LIST}")
    if not 0 <= n_splits <= KNN_MAX_SPLITS:
        raise ValueError(f"{name}: n_splits = {n_splits} is outside [0, {KNN_MAX_SPLITS}] (0 = chosen from the sizes)")
    x = _knn_rows_operand(name, "x", x)
    n, D = int(x.shape[0]), int(x.shape[1])
    if not 4 <= D <= KNN_MAX_D:
        raise ValueError(f"{name}: D = {D} is outside [4, {KNN_MAX_D}]")
    if n >= 2 ** 31:
        raise ValueError(f"{name}: n must be below 2^31")
    if not isinstance(group, torch.Tensor) or group.dtype not in (torch.int32, torch.int64) or tuple(group.shape) != (n,):
        raise ValueError(f"{name}: group must hold one id per row ([{n}]), int32 / int64")
    width = n_groups * k
    idx = torch.empty((n, width), dtype=torch.int32, device=dev)
    d2 = torch.empty((n, width), dtype=torch.float32, device=dev)
    m_idx, m_d2 = torch.empty_like(idx), torch.empty_like(d2)
    out = lambda: SegmentLists(idx.view(n, n_groups, k), d2.view(n, n_groups, k), m_idx, m_d2)
    if n == 0:
        return out()
    lo, hi = torch.aminmax(group)
    if int(lo) < 0 or int(hi) >= n_groups:
        raise ValueError(f"{name}: group id out of range [0, {n_groups}) (min {int(lo)}, max {int(hi)})")
    order, seg_ptr = _group_major(group, n_groups)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    sizes = lambda rows: ("wgnn_knn_segments_workspace_bytes", rows, n, n_groups, k, n_splits)
    # chunks of consecutive queries, halved until the partial lists of one chunk ([units, queries, k] 64-bit keys) fit the budget
    step = n
    while _workspace_bytes(*sizes(step)) > KNN_WORKSPACE_BYTES and step > 1:
        step = -(-step // 2)
    have = (None, 0)                                          # one allocation serves every chunk that it is large enough for
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        ws, ws_bytes = have = _workspace(dev, *sizes(r1 - r0), have=have)
        _lib.run(dev, "wgnn_knn_segments", _ptr(x), x.stride(0), n, D, _ptr(order), _ptr(seg_ptr), n_groups, k, r0, r1 - r0,
                 n_splits, idx.data_ptr() + r0 * width * 4, d2.data_ptr() + r0 * width * 4, width,
                 m_idx.data_ptr() + r0 * width * 4, m_d2.data_ptr() + r0 * width * 4, width, _ptr(status), _ptr(ws), ws_bytes, 0,
                 _stream(dev))
    _check_status(name, int(status), _KNN_SEGMENTS_STATUS)
    return out()


KMEANS_MAX_K = _lib.KMEANS_MAX_K          # wgnn_kmeans_seed's limit
KMEANS_INITS = ("k-means++",)


def kmeans_seed(x: torch.Tensor, n_clusters: int, seed: int = 0):
    """``wgnn_kmeans_seed``: k-means++ seeding of the rows of ``x`` [B, D] float32, every round on the device - ``K`` passes over
    ``x`` and no read-back in between (``include/wgnn.h`` has the contract: the weights are the f32 squared distances to the
    nearest seed so far in ``wgnn_knn_rows``' chain, the draw ``u_r`` a hash of ``(seed, r)``, the fp64 prefix in a fixed
    order).  A row that holds a non-finite value is never chosen.  With fewer DISTINCT valid rows than ``n_clusters`` the
    rounds that find no weight take the lowest-index valid row that is no seed yet.

    Returns ``(seed_row int32 [K], min_d2 f32 [B])``: the chosen rows in the order they were chosen, and every row's squared
    distance to the nearest of them (NaN for an invalid row).  Two calls are bit-identical.  ``n_clusters`` in [1, 4096] and
    at most the number of valid rows (one read-back, before the launches), ``D`` (after zero-padding to a multiple of 4) in
    [4, 1024]; argument errors are ``ValueError``."""
    name = "kmeans_seed"
    dev = _require_cuda(x)
    K = int(n_clusters)
    if not 1 <= K <= KMEANS_MAX_K:
        raise ValueError(f"{name}: n_clusters = {K} is outside [1, {KMEANS_MAX_K}]")
    x = _knn_rows_operand(name, "x", x)
    B, D = int(x.shape[0]), int(x.shape[1])
    if not 4 <= D <= KNN_MAX_D:
        raise ValueError(f"{name}: D = {D} is outside [4, {KNN_MAX_D}]")
    if B >= 2 ** 31:
        raise ValueError(f"{name}: B must be below 2^31")
    n_valid = int(torch.isfinite(x).all(dim=1).sum()) if B else 0
    if K > n_valid:
        raise ValueError(f"{name}: n_clusters = {K}, but only {n_valid} of the {B} rows are finite")
    seed_row = torch.empty(K, dtype=torch.int32, device=dev)
    min_d2 = torch.empty(B, dtype=torch.float32, device=dev)
    ws, ws_bytes = _workspace(dev, "wgnn_kmeans_seed_workspace_bytes", B, K)             # B >= K >= 1 here: never empty
    _lib.run(dev, "wgnn_kmeans_seed", _ptr(x), _ld(x, B, D), B, D, K, int(seed) & (2 ** 64 - 1),
             _ptr(seed_row), _ptr(min_d2), _ptr(ws), ws_bytes, 0, _stream(dev))
    return seed_row, min_d2


def group_rows_reduce(x: torch.Tensor, group: torch.Tensor, n_groups: int, out: Optional[tuple] = None):
    """``wgnn_group_rows_reduce``: per group the fp64 sum of the rows of ``x`` [B, D] float32 (unit column stride, any row stride
    ``>= D``), their number, and the mean.  ``group`` int32 / int64 [B]: a row's group in ``[0, n_groups)``; any other id = the row
    takes no part.  The batch is re-ordered group-major on the device as ``group_class_reduce`` does (a stable sort of the ids,
    the bounds by a search: no read-back); a group's rows are then added in ascending row order, in chunks of 64 and chunk by
    chunk - a fixed order, no atomics, two calls are bit-identical.

    Returns ``(sum f64 [K, D], count int64 [K], mean f32 [K, D])`` - ``out`` when given (``mean`` may have a wider row stride).
    ``mean = float32(sum / count)``; the ``mean`` row of an EMPTY group is not written: with ``out`` it keeps what it held, bit
    for bit, without ``out`` it is zero."""
    dev = _require_cuda(x, group, *(out or ()))
    K = int(n_groups)
    if K <= 0:
        raise ValueError(f"group_rows_reduce: n_groups = {K} must be positive")
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] < 1:
        raise ValueError("group_rows_reduce takes x float32 [B, D] with D >= 1")
    B, D = int(x.shape[0]), int(x.shape[1])
    if B >= 2 ** 31:
        raise ValueError("group_rows_reduce: B >= 2^31")
    _group_operand("group_rows_reduce", ValueError, group, B, K, False,          # any id outside [0, K) is a row that takes no part
                   says=f"group must hold one int32 / int64 id per row ([{B}])")
    if out is None:
        out = (torch.empty((K, D), dtype=torch.float64, device=dev), torch.empty(K, dtype=torch.int64, device=dev),
               torch.zeros((K, D), dtype=torch.float32, device=dev))
    if len(out) != 3:
        raise ValueError("out must be (sum, count, mean)")
    total, count, mean = out
    if tuple(total.shape) != (K, D) or total.dtype != torch.float64 or not total.is_contiguous() or \
            tuple(count.shape) != (K,) or count.dtype != torch.int64 or not count.is_contiguous():
        raise ValueError(f"out must hold contiguous sum float64 [{K}, {D}] and count int64 [{K}]")
    _view_2d("group_rows_reduce", ValueError, "out's mean", mean, torch.float32, K, D)
    if not _row_strided(x, B, D):
        x = x.contiguous()
    order, seg_ptr = _group_major(group, K)
    ws, ws_bytes = _workspace(dev, "wgnn_group_rows_reduce_workspace", B, K, D)          # K, D >= 1: never empty
    _lib.run(dev, "wgnn_group_rows_reduce", _ptr(x), _ld(x, B, D), _ptr(order), _ptr(seg_ptr), B, K, D, _ptr(total), D, _ptr(count),
             _ptr(mean), _ld(mean, K, D), _ptr(ws), ws_bytes, 0, _stream(dev))
    return total, count, mean


class KMeansRows(NamedTuple):
    """What ``kmeans_rows`` returns.  On the device: ``label`` int32 [B] (-1 = a row with a non-finite value), ``d2`` f32 [B] (the
    squared distance to the row's centre as ``wgnn_knn_rows`` leaves it; NaN beside a -1), ``centers`` f32 [K, D], ``size``
    int64 [K], ``seed_row`` int32 [K] (``None`` with an ``init`` array).  On the host: ``n_iter`` (the assignments made inside
    the loop), ``converged`` and ``inertia_trace`` (float64, one entry per assignment: the sum of ``d2`` over labelled rows)."""
    label: torch.Tensor
    d2: torch.Tensor
    centers: torch.Tensor
    size: torch.Tensor
    seed_row: Optional[torch.Tensor]
    n_iter: int
    converged: bool
    inertia_trace: list


def kmeans_rows(x: torch.Tensor, n_clusters: int, init="k-means++", max_iter: int = 100, seed: int = 0) -> KMeansRows:
    """Lloyd's k-means on the rows of ``x`` [B, D] float32, on the device, deterministic::

        C = x[seed_row]                      (kmeans_seed; or the caller's init array [K, D])
        for it in 1 .. max_iter:
            label, d2 = knn_rows(C, 1, queries=x, exclude_self=False);  label = -1 on rows with a non-finite value
            if it > 1 and label == prev: converged; break
            C = group_rows_reduce(x, label).mean  (an empty cluster keeps its row);  prev = label
        if not converged: one more assignment against the final C

    so the labels are always the assignment against the centres that are returned.  The assignment is ``wgnn_knn_rows`` with
    the centres as candidates: the nearest centre under the total order (distance, index) - of two equal centres the lower
    index takes every row and the higher stays empty.  An empty cluster is left where it is (no relocation).  One small
    read-back per iteration (the stop test, and ``d2`` for ``inertia_trace``, summed on the host in fp64).  It stops on an
    unchanged assignment or on ``max_iter``: there is no ``tol``, no ``n_init`` and no mini-batch mode.  A width that is no
    multiple of 4 is zero-padded as ``knn_rows`` does.  CPU tensors raise ``WgnnError``; argument errors are ``ValueError``.
    Returns a ``KMeansRows``."""
    import numpy as np
    name = "kmeans_rows"
    dev = _require_cuda(x)
    K, max_iter = int(n_clusters), int(max_iter)
    if not 1 <= K <= KMEANS_MAX_K:
        raise ValueError(f"{name}: n_clusters = {K} is outside [1, {KMEANS_MAX_K}]")
    if max_iter < 1:
        raise ValueError(f"{name}: max_iter = {max_iter} must be >= 1")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"{name}: x must be a 2-D float32 tensor")
    D = int(x.shape[1])
    xp = _knn_rows_operand(name, "x", x)
    B, Dp = int(xp.shape[0]), int(xp.shape[1])
    if not 4 <= Dp <= KNN_MAX_D:
        raise ValueError(f"{name}: D = {Dp} is outside [4, {KNN_MAX_D}]")
    seed_row = None
    if isinstance(init, str):
        if init not in KMEANS_INITS:
            raise ValueError(f"{name}: init = {init!r}: pass \"k-means++\" or an array [n_clusters, D]")
        seed_row, _ = kmeans_seed(xp, K, seed)
        centers = xp[seed_row.long()].contiguous()
    else:
        c0 = torch.as_tensor(init)
        if c0.dim() != 2 or tuple(c0.shape) != (K, D) or c0.dtype != torch.float32:
            raise ValueError(f"{name}: an init array must be float32 [{K}, {D}], got {c0.dtype} {tuple(c0.shape)}")
        if not bool(torch.isfinite(c0).all()):
            raise ValueError(f"{name}: the init array holds a non-finite value")
        centers = _pad_cols(c0.to(dev), Dp).contiguous().clone() if Dp != D else c0.to(dev).contiguous().clone()
    valid = torch.isfinite(xp).all(dim=1)
    nan = torch.full((), float("nan"), dtype=torch.float32, device=dev)
    minus = torch.full((), -1, dtype=torch.int32, device=dev)
    total = torch.empty((K, Dp), dtype=torch.float64, device=dev)
    count = torch.empty(K, dtype=torch.int64, device=dev)
    trace: list = []

    def assign():
        idx, d2 = knn_rows(centers, 1, queries=xp, exclude_self=False)
        label, d2 = torch.where(valid, idx[:, 0], minus), torch.where(valid, d2[:, 0], nan)
        host = d2.cpu().numpy().astype(np.float64)
        trace.append(float(host[~np.isnan(host)].sum()))
        return label, d2

    prev, converged, n_iter = None, False, 0
    for it in range(1, max_iter + 1):
        label, d2 = assign()
        n_iter = it
        if prev is not None and torch.equal(label, prev):
            converged = True
            break
        group_rows_reduce(xp, label, K, out=(total, count, centers))
        prev = label
    if not converged:
        label, d2 = assign()
    size = torch.bincount(label[label >= 0].long(), minlength=K)
    return KMeansRows(label, d2, centers[:, :D], size, seed_row, n_iter, converged, trace)


SILHOUETTE_MAX_GROUPS, SILHOUETTE_MAX_SPLITS = _lib.SILHOUETTE_MAX_GROUPS, _lib.SILHOUETTE_MAX_SPLITS     # wgnn_silhouette_rows' limits


class SilhouetteRows(NamedTuple):
    """What ``silhouette_rows`` returns, on the device and in the caller's row order: ``a`` f64 [B] (the mean distance to the other
    members of the row's own group; 0 for a singleton), ``b`` f64 [B] (the lowest mean distance to another non-empty group; +inf
    when there is none), ``score`` f64 [B] (``(b - a) / max(a, b)``), ``nearest`` int32 [B] (the group that attains ``b``; -1 when
    there is none) and ``size`` int64 [K] (the participating rows per group).  A row that takes no part holds NaN / NaN / NaN /
    -1."""
    a: torch.Tensor
    b: torch.Tensor
    score: torch.Tensor
    nearest: torch.Tensor
    size: torch.Tensor


def silhouette_rows(x: torch.Tensor, group: torch.Tensor, n_groups: int, n_splits: int = 0) -> SilhouetteRows:
    """``wgnn_silhouette_rows``: the exact silhouette (Rousseeuw 1987) of every row of ``x`` [B, D] float32 under Euclidean
    distance, the groups given - brute force over every ordered pair on the device, O(B^2 D), the [B, B] distance matrix is never
    stored (``include/wgnn.h`` has the numerics contract: ``wgnn_knn_rows``' f32 chain for the squared distance, a correctly rounded
    ``sqrtf``, fp64 sums per (row, group) in a fixed order, fp64 divides).  ``group`` int32 / int64 [B]: a row's group in
    ``[0, n_groups)``; any other id = the row takes no part, and neither does a row that holds a non-finite value (it is no
    member of its group: ``size`` does not count it).

    The rows are gathered group-major once (``B * D * 4`` bytes, a stable sort of the ids and a search for the groups' bounds: no
    read-back), the kernel streams them, and its four outputs are scattered back to the caller's row order.  Conventions: a
    singleton scores 0 (its ``a`` is 0), ``max(a, b) == 0`` scores 0, an empty group is ignored, and with fewer than two non-empty
    groups ``b = +inf``, ``nearest = -1`` and ``score = NaN``.  ``n_splits`` (0 = chosen from the sizes, else 1..64): how many
    workgroup columns share the groups - it changes no bit, and two calls are bit-identical.  A width that is no multiple of 4 is
    zero-padded as ``knn_rows`` does; ``D`` must then be in [4, 1024], ``n_groups`` in [1, 4096].  CPU tensors raise ``WgnnError``;
    argument errors are ``ValueError``.  Returns a ``SilhouetteRows``."""
    name = "silhouette_rows"
    dev = _require_cuda(x, group)
    K, n_splits = int(n_groups), int(n_splits)
    if not 1 <= K <= SILHOUETTE_MAX_GROUPS:
        raise ValueError(f"{name}: n_groups = {K} is outside [1, {SILHOUETTE_MAX_GROUPS}]")
    if not 0 <= n_splits <= SILHOUETTE_MAX_SPLITS:
        raise ValueError(f"{name}: n_splits = {n_splits} is outside [0, {SILHOUETTE_MAX_SPLITS}] (0 = chosen from the sizes)")
    x = _knn_rows_operand(name, "x", x)
    B, D = int(x.shape[0]), int(x.shape[1])
    if not 4 <= D <= KNN_MAX_D:
        raise ValueError(f"{name}: D = {D} is outside [4, {KNN_MAX_D}]")
    if B >= 2 ** 31:
        raise ValueError(f"{name}: B must be below 2^31")
    _group_operand(name, ValueError, group, B, K, False)                # any id outside [0, K) is a row that takes no part
    group = torch.where(torch.isfinite(x).all(dim=1), group, torch.full_like(group, -1))
    order, seg_ptr = _group_major(group, K)
    rows = x[order.long()]                                              # group-major and contiguous: the kernel streams it
    a, b, s = (torch.empty(B, dtype=torch.float64, device=dev) for _ in range(3))
    nearest = torch.empty(B, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace(dev, "wgnn_silhouette_workspace_bytes", B, K, n_splits)
    _lib.run(dev, "wgnn_silhouette_rows", _ptr(rows), D, B, D, _ptr(seg_ptr), K, n_splits, _ptr(a), _ptr(b), _ptr(s), _ptr(nearest),
             _ptr(ws), ws_bytes, 0, _stream(dev))
    back = torch.empty_like(order, dtype=torch.int64)
    back[order.long()] = torch.arange(B, dtype=torch.int64, device=dev)
    return SilhouetteRows(a[back], b[back], s[back], nearest[back], seg_ptr[1:] - seg_ptr[:-1])


SNN_MAX_K = _lib.SNN_MAX_K                # wgnn_snn_weights' limit
SNN_WEIGHTS = ("snn", "unit")
LOUVAIN_WAVE_ROWS, LOUVAIN_BLOCK_ROWS, LOUVAIN_SCRATCH_BLOCKS = _lib.LOUVAIN_WAVE_ROWS, _lib.LOUVAIN_BLOCK_ROWS, _lib.LOUVAIN_SCRATCH_BLOCKS
LOUVAIN_MAX_DEN = 64                      # louvain_graph's resolution is a fraction with a denominator up to this

_LOUVAIN_STATUS = ((_lib.LOUVAIN_UNSORTED, "a row is not strictly ascending in col"),
                   (_lib.LOUVAIN_BAD_COL, "a column is outside [0, n)"),
                   (_lib.LOUVAIN_BAD_ROWPTR, "rowptr does not ascend from 0 to nnz"),
                   (_lib.LOUVAIN_NO_SCRATCH, "a row above block_rows entries met no scratch"),
                   (_lib.LOUVAIN_BAD_LABEL, "a community id is outside [0, n)"),
                   (_lib.LOUVAIN_BAD_WEIGHT, "a weight is negative"))


class SnnGraph(NamedTuple):
    """What ``snn_graph`` returns, on the device: the symmetric CSR of the union graph - ``rowptr`` int64 [B + 1], ``col`` int32
    ascending within a row, ``w`` int32."""
    rowptr: torch.Tensor
    col: torch.Tensor
    w: torch.Tensor


def _list_entries(name, idx):
    """``[B, k]`` neighbour lists (int32 / int64, -1 = none, ``k`` in [1, 64]) checked - one read-back validates the ids - and
    flattened: ``(B, k, src, dst)``, the int64 row and entry of every list position."""
    if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or idx.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: idx must be a 2-D int32 / int64 tensor [B, k]")
    B, k = int(idx.shape[0]), int(idx.shape[1])
    if not 1 <= k <= SNN_MAX_K:
        raise ValueError(f"{name}: k = {k} is outside [1, {SNN_MAX_K}]")
    if B >= 2 ** 31:
        raise ValueError(f"{name}: B must be below 2^31")
    if B:
        lo, hi = torch.aminmax(idx)
        if int(lo) < -1 or int(hi) >= B:
            raise ValueError(f"{name}: a neighbour id is outside [-1, {B}) (min {int(lo)}, max {int(hi)})")
    src = torch.arange(B, dtype=torch.int64, device=idx.device)[:, None].expand(B, k).reshape(-1)
    return B, k, src, idx.reshape(-1).to(torch.int64)


def _union_csr(B, src, dst, return_inverse=False):
    """``(rowptr int64 [B + 1], col int32, inverse | None)``: the symmetric CSR that stores both directions of every pair
    ``(src, dst)`` once - 64-bit keys, sorted and made unique on the device (one read-back sizes the edge list).  ``inverse``: the
    CSR position of ``cat([src -> dst, dst -> src])``'s entries."""
    keys = torch.unique(torch.cat([src * B + dst, dst * B + src]), return_inverse=return_inverse)      # sorted: row-major, columns ascending
    keys, inverse = keys if return_inverse else (keys, None)
    row = torch.div(keys, max(B, 1), rounding_mode="floor")
    col = (keys - row * B).to(torch.int32)
    rowptr = torch.zeros(B + 1, dtype=torch.int64, device=src.device)
    if B:
        torch.cumsum(torch.bincount(row, minlength=B), 0, out=rowptr[1:])
    return rowptr, col, inverse


def snn_graph(idx: torch.Tensor, weights: str = "snn") -> SnnGraph:
    """The union graph of ``[B, k]`` neighbour lists as ``knn_rows`` leaves them (int32 / int64, -1 = none, ``k`` in [1, 64], no
    self entries) as a symmetric integer-weighted CSR on the device: ``{i, j}`` is an edge iff ``j`` is in ``i``'s list or ``i``
    in ``j``'s.  ``weights="snn"``: ``w(i, j) = |N+(i) & N+(j)|`` with ``N+(i) = {i} + list(i)`` - the shared-neighbour count, the
    numerator of Seurat's Jaccard weight, in [1, k + 1] - counted by ``wgnn_snn_weights``; ``"unit"``: every weight is 1.

    The two directions of every listed pair are concatenated as 64-bit keys, sorted and made unique on the device
    (``torch.unique``); the edge lists are never read back (one read-back validates the ids, one sizes the edge list).  An id
    outside [-1, B) is a ``ValueError``; a self entry or a repeated entry is ignored.  Returns an ``SnnGraph``."""
    name = "snn_graph"
    dev = _require_cuda(idx)
    if weights not in SNN_WEIGHTS:
        raise ValueError(f"{name}: weights = {weights!r}: pass one of {', '.join(map(repr, SNN_WEIGHTS))}")
    B, k, src, dst = _list_entries(name, idx)
    idx = idx.contiguous()
    listed = (dst >= 0) & (dst != src)
    rowptr, col, _ = _union_csr(B, src[listed], dst[listed])
    nnz = int(col.shape[0])
    if weights == "unit" or nnz == 0:
        return SnnGraph(rowptr, col, torch.ones(nnz, dtype=torch.int32, device=dev))
    w = torch.empty(nnz, dtype=torch.int32, device=dev)
    _lib.run(dev, "wgnn_snn_weights", _ptr(idx), k, B, k, _ptr(rowptr), _ptr(col), nnz, _ptr(w),
             _lib.SNN_IDX_I64 if idx.dtype == torch.int64 else 0, _stream(dev))
    return SnnGraph(rowptr, col, w)


class LouvainRows(NamedTuple):
    """What ``louvain_graph`` returns.  On the device: ``cluster`` int64 [B] (final ids by descending size, ties by the lowest
    member; -1 for a vertex without an edge) and ``level_labels`` (one int64 [B] per level run: the dendrogram; a
    level's ids are dense, in ascending order of the communities' own ids; the last level merged nothing and repeats the cut).  On the host: ``levels`` (per
    level a dict ``vertices`` / ``communities`` / ``sweeps`` / ``fallback_moves``), ``qnum_trace`` (Python ints, strictly
    increasing: the start, then one entry per kept sweep or fallback move), ``modularity`` (``Qnum / (den M^2)``),
    ``resolution`` (the ``Fraction`` used), ``M`` and ``converged`` (False when a level stopped at ``max_sweeps``)."""
    cluster: torch.Tensor
    level_labels: list
    levels: list
    qnum_trace: list
    modularity: float
    resolution: object
    M: int
    converged: bool


def louvain_resolution(resolution):
    """``Fraction(resolution).limit_denominator(64)``, positive - the value ``louvain_graph`` uses; ``ValueError`` otherwise."""
    from fractions import Fraction
    try:
        frac = Fraction(resolution).limit_denominator(LOUVAIN_MAX_DEN)
    except (TypeError, ValueError, OverflowError, ZeroDivisionError):
        raise ValueError(f"louvain_graph: resolution = {resolution!r} is no finite number") from None
    if frac <= 0:
        raise ValueError(f"louvain_graph: resolution = {resolution!r} must be positive (at least 1/128)")
    return frac


class _GraphRun:
    """What ``louvain_graph`` and ``leiden_graph`` share: the argument checks, a level's state on the device, the apply / modularity
    pair with its one read-back, the moving phase, the aggregation and the final ids."""

    def __init__(self, name, rowptr, col, w, resolution, max_sweeps, wave_rows, block_rows, scratch_blocks):
        self.name = name
        self.dev = dev = _require_cuda(rowptr, col, w)
        max_sweeps, wave_rows, block_rows, scratch_blocks = int(max_sweeps), int(wave_rows), int(block_rows), int(scratch_blocks)
        if max_sweeps < 1:
            raise ValueError(f"{name}: max_sweeps = {max_sweeps} must be >= 1")
        if not 0 <= wave_rows <= LOUVAIN_WAVE_ROWS or not 0 <= block_rows <= LOUVAIN_BLOCK_ROWS or \
                not 1 <= scratch_blocks <= LOUVAIN_SCRATCH_BLOCKS:
            raise ValueError(f"{name}: wave_rows in [0, {LOUVAIN_WAVE_ROWS}], block_rows in [0, {LOUVAIN_BLOCK_ROWS}] and scratch_blocks in "
                             f"[1, {LOUVAIN_SCRATCH_BLOCKS}], got {wave_rows}, {block_rows}, {scratch_blocks}")
        self.rowptr, self.col, self.w, self.B, nnz = _graph_operand(name, rowptr, col, w, "w", torch.int32)
        self.max_sweeps, self.wave_rows, self.block_rows, self.scratch_blocks = max_sweeps, wave_rows, block_rows, scratch_blocks
        self.frac = frac = louvain_resolution(resolution)
        self.num, self.den = num, den = frac.numerator, frac.denominator
        self.M = M = int(w.sum(dtype=torch.int64)) if nnz else 0
        if M * M * max(num, den) >= 2 ** 62:
            raise ValueError(f"{name}: M * M * max(num, den) = {M * M * max(num, den)} >= 2^62 (M = {M}, resolution {frac}): the "
                             "integer gains would not fit 64 bits")
        if self.B and (int(rowptr[0]) != 0 or int(rowptr[-1]) != nnz):
            raise WgnnError(f"{name}: rowptr does not run from 0 to nnz = {nnz}")
        self.ids = torch.arange(self.B, dtype=torch.int64, device=dev)
        self.isolated = rowptr[1:] == rowptr[:-1]
        self.stream = _stream(dev)
        self.stats = torch.zeros(4, dtype=torch.int64, device=dev)
        self.status = _LOUVAIN_STATUS
        self.trace, self.converged, self.first = None, True, True

    def level(self):
        """The state of the level whose graph is ``rowptr`` / ``col`` / ``w``: its rows, degrees, long rows and scratch."""
        dev, name = self.dev, self.name
        self.n, self.nnz = int(self.rowptr.shape[0]) - 1, int(self.col.shape[0])
        n, nnz = self.n, self.nnz
        self.graph = (self.rowptr, self.col, self.w)
        lens = self.rowptr[1:] - self.rowptr[:-1]
        self.row = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), lens, output_size=nnz)
        if self.first and bool((self.row == self.col).any()):
            raise ValueError(f"{name}: the graph holds a self loop")
        self.first = False
        self.deg = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, self.row, self.w.to(torch.int64))
        self.heavy = torch.nonzero(lens > self.wave_rows).reshape(-1).to(torch.int32)
        self.n_heavy = int(self.heavy.shape[0])
        self.n_scratch = min(self.scratch_blocks, int((lens > self.block_rows).sum())) if self.n_heavy else 0
        self.ws, self.ws_bytes = (None, 0)
        if self.n_scratch:                                          # zero on entry; the kernels leave it zero
            self.ws_bytes = _workspace_bytes("wgnn_louvain_sweep_workspace_bytes", n, self.n_scratch)
            self.ws = torch.zeros(self.ws_bytes // 4, dtype=torch.int32, device=dev)

    def routes(self):
        """The operands of the sweep kernels that say which route serves which row."""
        return (_ptr(self.heavy) if self.n_heavy else None, self.n_heavy, self.wave_rows, self.block_rows)

    def scratch(self):
        return (_ptr(self.ws) if self.n_scratch else None, self.ws_bytes, self.n_scratch)

    def measure(self, old, label):
        """tot / size of ``label`` and ``(moved, Qnum)``: apply, modularity and the one read-back."""
        dev, n, graph, stats = self.dev, self.n, self.graph, self.stats
        tot, size = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        _lib.run(dev, "wgnn_louvain_apply", _ptr(old), _ptr(label), _ptr(self.deg), n, _ptr(tot), _ptr(size), _ptr(stats), 0,
                 self.stream)
        _lib.run(dev, "wgnn_louvain_modularity", _ptr(graph[0]), _ptr(graph[1]), _ptr(graph[2]), n, int(graph[1].shape[0]),
                 _ptr(label), _ptr(tot), _ptr(stats), 0, self.stream)
        moved, inside, tot2, status = (int(v) for v in stats.tolist())
        _check_status(self.name, status, self.status)
        return tot, size, moved, self.den * self.M * inside - self.num * tot2

    def sweeps(self, label, tot, size, q0, propose, what):
        """The sweeps of a phase from the labelling ``label`` with its ``tot`` / ``size`` and ``Qnum`` ``q0``, until two in a row
        move nothing or ``max_sweeps``: ``(label, tot, sweeps, fallback moves, the Qnum after every kept step)``.
        ``propose(t, label, tot, size)`` enqueues sweep ``t``'s launches and returns ``(next, gain)``; ``measure`` is the one
        read-back per sweep.  A sweep is kept when ``Qnum`` rose, else discarded for its single best move (largest gain, lowest
        vertex) - ``what`` names that move when it does not raise ``Qnum`` either."""
        t = idle = fallback = 0
        kept = []
        while True:
            if t >= self.max_sweeps:
                self.converged = False
                break
            nxt, gain = propose(t, label, tot, size)
            tot2, size2, moved, q = self.measure(label, nxt)
            t += 1
            if moved == 0:
                idle += 1
                if idle == 2:
                    break
                continue
            idle = 0
            if q > q0:
                label, tot, size = nxt, tot2, size2
            else:                                                   # discarded: the single best move, ties to the lowest vertex
                v = int(torch.nonzero(gain == gain.max()).reshape(-1)[0])
                one = label.clone()
                one[v] = nxt[v]
                tot, size, _, q = self.measure(label, one)
                if q <= q0:
                    raise WgnnError(f"{self.name}: a single {what} move did not raise Qnum ({q0} -> {q}): the graph is not symmetric")
                label = one
                fallback += 1
            q0 = q
            kept.append(q)
        return label, tot, t, fallback, kept

    def move(self, comm):
        """The moving phase of a level from the partition ``comm``: ``(comm, tot, sweeps, fallback moves)``; the trace grows."""
        dev, name, n, nnz = self.dev, self.name, self.n, self.nnz
        rowptr, col, w = self.graph
        tot, size, _, q = self.measure(None, comm)                  # the start's state, and the graph's checks
        if self.trace is None:
            self.trace = [q]
        elif q != self.trace[-1]:                                   # aggregation keeps the partition, so Qnum too
            raise WgnnError(f"{name}: Qnum changed across the aggregation ({self.trace[-1]} -> {q})")

        def propose(t, comm, tot, size):
            nxt = torch.empty(n, dtype=torch.int32, device=dev)
            gain = torch.empty(n, dtype=torch.int64, device=dev)
            _lib.run(dev, "wgnn_louvain_sweep", _ptr(rowptr), _ptr(col), _ptr(w), n, nnz, _ptr(comm), _ptr(self.deg), _ptr(tot),
                     _ptr(size), self.M * self.den, self.num, t, *self.routes(), _ptr(nxt), _ptr(gain), _ptr(self.stats),
                     *self.scratch(), 0, self.stream)
            return nxt, gain

        comm, tot, t, fallback, kept = self.sweeps(comm, tot, size, q, propose, "positive-gain")
        self.trace += kept
        return comm, tot, t, fallback

    def coarsen(self, inv, nc):
        """The next level's graph: the ``nc`` communities ``inv`` (dense ids per vertex) as vertices, their internal weight on
        the diagonal."""
        dev = self.dev
        key, kinv = torch.unique(inv[self.row] * nc + inv[self.col.long()], return_inverse=True)
        self.w = torch.zeros(key.shape[0], dtype=torch.int64, device=dev).index_add_(0, kinv, self.w.to(torch.int64)).to(torch.int32)
        crow = torch.div(key, nc, rounding_mode="floor")
        self.col = (key - crow * nc).to(torch.int32)
        self.rowptr = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(crow, minlength=nc), 0, out=self.rowptr[1:])

    def clusters(self, member):
        """Final ids: by descending size, ties by the lowest member; a vertex without an edge has none."""
        B, dev, ids = self.B, self.dev, self.ids
        on = ~self.isolated
        cluster = torch.full((B,), -1, dtype=torch.int64, device=dev)
        uniq, inv, count = torch.unique(member[on], return_inverse=True, return_counts=True)
        first = torch.full((int(uniq.shape[0]),), B, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, ids[on], "amin")
        order = torch.argsort((B - count) * B + first)
        rank = torch.empty_like(order)
        rank[order] = torch.arange(order.shape[0], dtype=torch.int64, device=dev)
        cluster[on] = rank[inv]
        return cluster


def louvain_graph(rowptr: torch.Tensor, col: torch.Tensor, w: torch.Tensor, resolution=1.0, max_sweeps: int = 256,
                  wave_rows: int = LOUVAIN_WAVE_ROWS, block_rows: int = LOUVAIN_BLOCK_ROWS, scratch_blocks: int = 32) -> LouvainRows:
    """Louvain communities of a symmetric CSR graph with int32 weights and no self loops (``rowptr`` int64 [B + 1], ``col`` int32
    ascending within a row, ``w`` int32 >= 0 - what ``snn_graph`` returns), on the device and in integers (``include/wgnn.h``
    has the contract).  ``resolution`` becomes ``num / den = Fraction(resolution).limit_denominator(64)``; with ``M`` the sum of
    all weights, ``M * M * max(num, den) >= 2^62`` is a ``ValueError`` before any launch - below it every product fits int64.

    A level's local moving is synchronous: sweep ``t`` (``wgnn_louvain_sweep``) lets every vertex pick, from the state before the
    sweep, the best community of its neighbours that lies below its own id (``t`` even) or above (odd) and scores higher than
    staying; ``wgnn_louvain_apply`` / ``wgnn_louvain_modularity`` then give ``Qnum`` of the new assignment, and one read-back of
    four integers decides: kept when ``Qnum`` rose, else discarded for the single best move of the sweep (largest gain, lowest
    vertex).  A level ends after two consecutive sweeps without a move or at ``max_sweeps``; its communities, renumbered densely
    in ascending order of their ids, are the next level's vertices (the aggregation is ``torch.unique`` and an integer
    ``index_add_`` on the device), until a level merges nothing.  No refinement phase (this is Louvain, not Leiden), no random
    restarts.  ``wave_rows`` (<= 128), ``block_rows`` (<= 2048) and ``scratch_blocks`` (1..256) bound the three routes of the sweep
    kernel by row length and change no bit; two calls are bit-identical.  CPU tensors raise ``WgnnError``; argument errors are
    ``ValueError``; a malformed graph (unsorted rows, columns out of range) raises ``WgnnError``.  Returns a ``LouvainRows``."""
    run = _GraphRun("louvain_graph", rowptr, col, w, resolution, max_sweeps, wave_rows, block_rows, scratch_blocks)
    B, dev = run.B, run.dev
    if run.M == 0:
        return LouvainRows(torch.full((B,), -1, dtype=torch.int64, device=dev), [run.ids],
                           [dict(vertices=B, communities=B, sweeps=0, fallback_moves=0)], [0], 0.0, run.frac, 0, True)
    member, levels, level_labels = run.ids, [], []
    while True:
        run.level()
        n = run.n
        comm, _, t, fallback = run.move(torch.arange(n, dtype=torch.int32, device=dev))
        uniq, inv = torch.unique(comm, return_inverse=True)         # dense ids in ascending order of the old ones
        nc = int(uniq.shape[0])
        member = inv[member]
        levels.append(dict(vertices=n, communities=nc, sweeps=t, fallback_moves=fallback))
        level_labels.append(member)
        if nc == n:
            break
        run.coarsen(inv, nc)
    trace = run.trace
    return LouvainRows(run.clusters(member), level_labels, levels, trace, trace[-1] / (run.den * run.M * run.M), run.frac, run.M,
                       run.converged)


class LeidenRows(NamedTuple):
    """What ``leiden_graph`` returns: ``LouvainRows``' fields and ``refined_labels``.  ``level_labels[l]`` is the partition ``P``
    the moving phase of level ``l`` left, per original vertex and dense; one more entry follows when the final cut split a
    community into its connected components (``levels[-1]["split"]`` > 0), and ``cluster`` is the last entry's ids by descending
    size.  ``refined_labels[l]`` is level ``l``'s refined partition (dense, in ascending order of the founders' ids): the next
    level's vertices.  Each ``levels[l]`` adds ``refined`` (how many refined communities), ``refine_sweeps`` and
    ``refine_fallback_moves``; the last adds ``split`` (how many communities the final cut added).  ``qnum_trace`` holds the moving
    phases' entries and the final cut's; the refinement keeps a running value of its own."""
    cluster: torch.Tensor
    level_labels: list
    refined_labels: list
    levels: list
    qnum_trace: list
    modularity: float
    resolution: object
    M: int
    converged: bool


_LEIDEN_STATUS = _LOUVAIN_STATUS + ((_lib.LEIDEN_BAD_PARTITION, "a refined or moved id is outside [0, n), or a refined community's "
                                                                "founder lies in another community"),)


def _leiden_refine(run: _GraphRun, P: torch.Tensor, totP: torch.Tensor):
    """The refinement of one level inside the partition ``P``: ``(ref, sweeps, fallback moves)``.  Per sweep five launches
    (boundary, refine sweep, accept, apply, modularity) and one read-back; the running ``Qnum`` is the loop's own, not the trace's."""
    dev, n, nnz, stats, stream = run.dev, run.n, run.nnz, run.stats, run.stream
    rowptr, col, w = run.graph
    ref = torch.arange(n, dtype=torch.int32, device=dev)
    tot, size, _, q = run.measure(None, ref)
    ext = torch.empty(n, dtype=torch.int64, device=dev)
    kinP = torch.empty(n, dtype=torch.int64, device=dev)

    def propose(r, ref, tot, size):
        prop, nxt = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        gain = torch.empty(n, dtype=torch.int64, device=dev)
        _lib.run(dev, "wgnn_leiden_boundary", _ptr(rowptr), _ptr(col), _ptr(w), n, nnz, _ptr(P), _ptr(ref), _ptr(ext),
                 _ptr(kinP) if r == 0 else None, _ptr(stats), 0, stream)                     # kinP depends on P alone
        _lib.run(dev, "wgnn_leiden_refine_sweep", _ptr(rowptr), _ptr(col), _ptr(w), n, nnz, _ptr(P), _ptr(ref), _ptr(run.deg),
                 _ptr(totP), _ptr(tot), _ptr(size), _ptr(ext), _ptr(kinP), run.M * run.den, run.num, r, *run.routes(), _ptr(prop),
                 _ptr(gain), _ptr(stats), *run.scratch(), 0, stream)
        _lib.run(dev, "wgnn_leiden_accept", _ptr(ref), _ptr(prop), n, _ptr(nxt), _ptr(gain), _ptr(stats), 0, stream)
        return nxt, gain                                            # measure counts the accepted moves again: the one read-back

    ref, _, r, fallback, _ = run.sweeps(ref, tot, size, q, propose, "accepted")
    return ref, r, fallback


def _leiden_components(run: _GraphRun, P: torch.Tensor) -> torch.Tensor:
    """The lowest vertex of every vertex's connected component inside its community of ``P``: min-label propagation over the
    entries whose two ends share a community, on the device, until a round changes nothing (one read-back per round)."""
    same = P[run.row] == P[run.col.long()]
    return _min_labels(run.n, run.row[same], run.col[same].long(), run.dev).to(torch.int32)


def _min_labels(n: int, r: torch.Tensor, c: torch.Tensor, dev) -> torch.Tensor:
    """int64 [n]: the lowest vertex every vertex reaches over the directed entries ``(r, c)`` (both directions stored), by
    min-label propagation in integers until a round changes nothing (one read-back per round)."""
    label = torch.arange(n, dtype=torch.int64, device=dev)
    while True:
        nxt = label.clone().scatter_reduce_(0, r, label[c], "amin")
        if bool((nxt == label).all()):
            return label
        label = nxt


def leiden_graph(rowptr: torch.Tensor, col: torch.Tensor, w: torch.Tensor, resolution=1.0, max_sweeps: int = 256,
                 wave_rows: int = LOUVAIN_WAVE_ROWS, block_rows: int = LOUVAIN_BLOCK_ROWS, scratch_blocks: int = 32) -> LeidenRows:
    """Leiden communities of the graph ``louvain_graph`` takes, on the device and in integers: deterministic and synchronous, no
    floating point and no random number, so two calls and every launch geometry give the same bits (``include/wgnn.h`` and
    DESIGN.md section 3 have the contract).  What it buys over ``louvain_graph`` is that every community is connected; it does
    not claim a higher modularity.

    A level (1) runs ``louvain_graph``'s moving phase from the partition it inherited (singletons at level 0), which leaves
    ``P``; (2) refines: from singletons, a vertex that is alone and well connected to its community of ``P`` proposes the best
    well-connected refined community of its neighbours inside that community (``wgnn_leiden_boundary``,
    ``wgnn_leiden_refine_sweep``), a proposal holds iff the founder of its target stays (``wgnn_leiden_accept``), and a sweep that
    does not raise ``Qnum`` is discarded for its single best accepted move; (3) aggregates by the refined partition, the next
    level starting from the refined communities grouped by ``P``.  A level whose refinement merges nothing ends the run, and the
    last ``P`` is cut into its connected components.  ``max_sweeps`` bounds the moving phase and the refinement of a level each.
    Arguments, refusals and errors are ``louvain_graph``'s.  Returns a ``LeidenRows``."""
    run = _GraphRun("leiden_graph", rowptr, col, w, resolution, max_sweeps, wave_rows, block_rows, scratch_blocks)
    run.status = _LEIDEN_STATUS
    B, dev = run.B, run.dev
    if run.M == 0:
        return LeidenRows(torch.full((B,), -1, dtype=torch.int64, device=dev), [run.ids], [run.ids],
                          [dict(vertices=B, communities=B, sweeps=0, fallback_moves=0, refined=B, refine_sweeps=0,
                                refine_fallback_moves=0, split=0)], [0], 0.0, run.frac, 0, True)
    member, levels, level_labels, refined_labels = run.ids, [], [], []
    comm0 = torch.arange(B, dtype=torch.int32, device=dev)
    while True:
        run.level()
        n = run.n
        P, totP, t, fallback = run.move(comm0)
        ref, r, r_fallback = _leiden_refine(run, P, totP)
        dense_P = torch.unique(P, return_inverse=True)[1]
        uniq, inv = torch.unique(ref, return_inverse=True)          # dense ids in ascending order of the founders' ids
        nc = int(uniq.shape[0])
        levels.append(dict(vertices=n, communities=int(dense_P.max()) + 1, sweeps=t, fallback_moves=fallback, refined=nc,
                           refine_sweeps=r, refine_fallback_moves=r_fallback))
        level_labels.append(dense_P[member])
        refined_labels.append(inv[member])
        if nc == n:
            break
        lowest = torch.full((n,), nc, dtype=torch.int64, device=dev).scatter_reduce_(0, P.long(), inv, "amin")
        comm0 = torch.empty(nc, dtype=torch.int32, device=dev)
        comm0[inv] = lowest[P.long()].to(torch.int32)               # the refined communities of one community of P start together
        member = inv[member]
        run.coarsen(inv, nc)
    trace = run.trace
    parts = _leiden_components(run, P)                              # the final cut: a coarse move can leave a community in pieces
    uniq, dense_parts = torch.unique(parts, return_inverse=True)
    split = int(uniq.shape[0]) - levels[-1]["communities"]
    levels[-1]["split"] = split
    if split:
        _, _, _, q = run.measure(None, parts)
        if q <= trace[-1]:
            raise WgnnError(f"leiden_graph: the cut into connected components did not raise Qnum ({trace[-1]} -> {q})")
        trace.append(q)
        level_labels.append(dense_parts[member])
    return LeidenRows(run.clusters(level_labels[-1]), level_labels, refined_labels, levels, trace,
                      trace[-1] / (run.den * run.M * run.M), run.frac, run.M, run.converged)


FUZZY_MAX_K = _lib.FUZZY_MAX_K            # wgnn_fuzzy_rows' limit
LAYOUT_LANES, LAYOUT_MAX_EPOCHS, LAYOUT_MAX_NEG = _lib.LAYOUT_LANES, _lib.LAYOUT_MAX_EPOCHS, _lib.LAYOUT_MAX_NEG
LAYOUT_A, LAYOUT_B = 1.577, 0.895         # layout_curve(0.1, 1.0), rounded: layout_graph's defaults
LAYOUT_INITS = ("hash",)


class FuzzyGraph(NamedTuple):
    """What ``fuzzy_graph`` returns, on the device: the symmetric CSR of the union graph (``rowptr`` int64 [B + 1], ``col`` int32
    ascending within a row) with UMAP's connectivities ``w`` float32 [nnz] - ``w(i, j)`` and ``w(j, i)`` are the same bits - and the
    per-row ``rho`` / ``sigma`` float64 [B] and ``member`` float32 [B, k] of ``wgnn_fuzzy_rows``."""
    rowptr: torch.Tensor
    col: torch.Tensor
    w: torch.Tensor
    rho: torch.Tensor
    sigma: torch.Tensor
    member: torch.Tensor


def fuzzy_graph(idx: torch.Tensor, d2: torch.Tensor) -> FuzzyGraph:
    """UMAP's fuzzy simplicial set of ``[B, k]`` neighbour lists as ``knn_rows`` leaves them (``idx`` int32 / int64 with -1 = none,
    ``d2`` float32 squared distances with +inf = none; ``k`` in [1, 64]; views into wider rows are taken), on the device
    (``include/wgnn.h`` has the contract).  ``wgnn_fuzzy_rows`` gives every row its ``rho`` (the nearest positive distance), its
    ``sigma`` (64 bisection steps towards ``sum_j exp(-(d_j - rho) / sigma) = log2(k + 1)``, floored at 1e-3 of the row's mean
    distance) and the memberships of its own list; ``wgnn_fuzzy_union`` joins the two directions on ``snn_graph(idx, "unit")``'s
    structure as ``w = a + b - a b``.  Given ``member``, numpy reproduces ``w`` bit for bit; ``member`` itself is within one
    float32 ulp (2^-24 absolute) of a numpy restatement, the two ``exp`` differing in the last bit of a float64.

    Against umap-learn: the bisection never exits early (no 1e-5 tolerance); the floor uses the row's own mean even when
    ``rho = 0`` (umap-learn then takes the mean of all distances); ``local_connectivity`` is fixed at 1 and ``set_op_mix_ratio`` at
    1.  An entry with ``idx >= 0`` and a finite ``d2`` is listed, a self entry among them; an id outside [-1, B) or a negative
    ``d2`` is a ``ValueError``.  Returns a ``FuzzyGraph``."""
    name = "fuzzy_graph"
    dev = _require_cuda(idx, d2)
    B, k, src, dst = _list_entries(name, idx)                                   # rank, dtype, k and the ids
    if not _row_strided(idx, B, k):
        raise ValueError(f"{name}: idx must have unit column stride and a row stride >= {k}")
    _view_2d(name, ValueError, "d2", d2, torch.float32, B, k)
    if B and bool((d2 < 0).any()):
        raise ValueError(f"{name}: d2 holds a negative squared distance")
    listed = (dst >= 0) & (dst != src)
    rowptr, col, _ = _union_csr(B, src[listed], dst[listed])                    # snn_graph(idx, "unit")'s structure
    rho = torch.empty(B, dtype=torch.float64, device=dev)
    sigma = torch.empty(B, dtype=torch.float64, device=dev)
    member = torch.empty((B, k), dtype=torch.float32, device=dev)
    nnz = int(col.shape[0])
    w = torch.empty(nnz, dtype=torch.float32, device=dev)
    flags = _lib.FUZZY_IDX_I64 if idx.dtype == torch.int64 else 0
    _lib.run(dev, "wgnn_fuzzy_rows", _ptr(idx), _ld(idx, B, k), _ptr(d2), _ld(d2, B, k), B, k, math.log2(k + 1), _ptr(rho),
             _ptr(sigma), _ptr(member), flags, _stream(dev))
    _lib.run(dev, "wgnn_fuzzy_union", _ptr(idx), _ld(idx, B, k), _ptr(member), B, k, _ptr(rowptr), _ptr(col), nnz, _ptr(w), flags,
             _stream(dev))
    return FuzzyGraph(rowptr, col, w, rho, sigma, member)


class LayoutRows(NamedTuple):
    """What ``layout_graph`` returns: ``y`` float32 [B, 2] on the device, ``n_epochs`` (the number run) and ``n_fired`` (how many
    times a stored, directed edge fired over all epochs; a Python int)."""
    y: torch.Tensor
    n_epochs: int
    n_fired: int


def layout_curve(min_dist: float = 0.1, spread: float = 1.0):
    """``(a, b)`` of the layout's similarity ``1 / (1 + a d^(2 b))``: the least-squares fit to ``d < min_dist ? 1 :
    exp(-(d - min_dist) / spread)`` on 300 points of [0, 3 spread] that umap-learn's ``find_ab_params`` makes, by
    ``scipy.optimize.curve_fit`` on the host.  ``min_dist`` in [0, spread], ``spread`` > 0, else ``ValueError``."""
    import numpy as np
    from scipy.optimize import curve_fit
    min_dist, spread = float(min_dist), float(spread)
    if not (0.0 < spread < float("inf")) or not 0.0 <= min_dist <= spread:
        raise ValueError(f"layout_curve: spread must be positive and min_dist in [0, spread], got {min_dist}, {spread}")
    xv = np.linspace(0.0, 3.0 * spread, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    (a, b), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2.0 * b)), xv, yv)
    return float(a), float(b)


def layout_epochs(n_cells: int) -> int:
    """umap-learn's default number of epochs: 500 below 10 000 cells, 200 from there on."""
    return 500 if n_cells < 10000 else 200


def layout_graph(rowptr: torch.Tensor, col: torch.Tensor, w: torch.Tensor, init="hash", n_epochs: Optional[int] = None,
                 a: float = LAYOUT_A, b: float = LAYOUT_B, gamma: float = 1.0, n_neg: int = 5, lr: float = 1.0,
                 seed: int = 0) -> LayoutRows:
    """A 2-D layout of a symmetric weighted CSR graph (``rowptr`` int64 [B + 1], ``col`` int32, ``w`` float32 >= 0 - what
    ``fuzzy_graph`` returns) by UMAP's forces applied SYNCHRONOUSLY: every epoch (``wgnn_layout_epoch``, one launch each on the
    current stream, no read-back and no graph capture in between) reads the positions of the epoch before and writes new ones
    into a second buffer, and every vertex's sum runs in a fixed order (``include/wgnn.h`` has the contract) - so two calls give
    the same bits, whatever the grid.  A stored edge fires in ``floor(n_epochs w / max w)`` of the epochs, both its directions in
    the same ones; a firing edge pulls its row's vertex towards the other end and pushes it away from ``n_neg`` vertices drawn
    by a counter hash of ``(seed, epoch, edge, draw)``; the step is ``lr (1 - epoch / n_epochs)``, computed here in float64.

    ``init``: a float32 [B, 2] tensor (copied) or ``"hash"`` - uniform in [-10, 10) from the same hash of ``seed``
    (``wgnn_layout_init``).  ``n_epochs`` = None: 500 below 10 000 vertices, 200 from there on; at most 10 000.  ``a`` / ``b``:
    ``layout_curve``'s (the defaults are its values for ``min_dist`` 0.1, ``spread`` 1); with ``b == 1`` the whole epoch is +, -,
    x, / in float32 and numpy restates it bit for bit, otherwise ``q^b`` is a float64 ``pow`` rounded to float32.  A vertex
    without an edge keeps its position.  One read-back before the loop (``max w`` and the finiteness of ``w`` and ``init``) and one
    after it (``n_fired``).  Not umap-learn's order: there an edge moves both ends at once and later edges see the move.
    A non-finite or negative ``w``, a non-finite ``init`` and every other argument error are ``ValueError``; CPU tensors raise
    ``WgnnError``.  Returns a ``LayoutRows``."""
    name = "layout_graph"
    dev = _require_cuda(rowptr, col, w, init if isinstance(init, torch.Tensor) else None)
    rowptr, col, w, B, nnz = _graph_operand(name, rowptr, col, w, "w", torch.float32)
    n_epochs = layout_epochs(B) if n_epochs is None else int(n_epochs)
    n_neg, seed = int(n_neg), int(seed)
    if not 1 <= n_epochs <= LAYOUT_MAX_EPOCHS:
        raise ValueError(f"{name}: n_epochs = {n_epochs} is outside [1, {LAYOUT_MAX_EPOCHS}]")
    if not 0 <= n_neg <= LAYOUT_MAX_NEG:
        raise ValueError(f"{name}: n_neg = {n_neg} is outside [0, {LAYOUT_MAX_NEG}]")
    if not 0 <= seed < 2 ** 32:
        raise ValueError(f"{name}: seed = {seed} is outside [0, 2^32)")
    a, b, gamma, lr = float(a), float(b), float(gamma), float(lr)
    if not (0.0 < a < float("inf") and 0.0 < b < float("inf") and 0.0 <= gamma < float("inf") and 0.0 < lr < float("inf")):
        raise ValueError(f"{name}: a, b and lr must be positive, gamma not negative, all finite (got {a}, {b}, {gamma}, {lr})")
    stream = _stream(dev)
    if isinstance(init, torch.Tensor):
        if init.dtype != torch.float32 or tuple(init.shape) != (B, 2):
            raise ValueError(f"{name}: init must be a float32 [{B}, 2] tensor or one of {', '.join(map(repr, LAYOUT_INITS))}")
        y = init.contiguous().clone()
    elif isinstance(init, str) and init in LAYOUT_INITS:
        y = torch.empty((B, 2), dtype=torch.float32, device=dev)
        _lib.run(dev, "wgnn_layout_init", _ptr(y), B, seed, 0, stream)
    else:
        raise ValueError(f"{name}: init = {init!r}: pass a float32 [{B}, 2] tensor or one of {', '.join(map(repr, LAYOUT_INITS))}")
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    wmax, wmin, bad_w, bad_y = torch.stack([w.max() if nnz else zero, w.min() if nnz else zero,
                                            (~torch.isfinite(w)).sum().float(), (~torch.isfinite(y)).sum().float()]).tolist()
    if bad_w or wmin < 0:
        raise ValueError(f"{name}: w holds a non-finite or a negative weight")
    if bad_y:
        raise ValueError(f"{name}: init holds a non-finite position")
    if B and (int(rowptr[0]) != 0 or int(rowptr[-1]) != nnz):
        raise ValueError(f"{name}: rowptr does not run from 0 to nnz = {nnz}")
    if B == 0 or nnz == 0 or wmax <= 0:                                         # nothing can fire
        return LayoutRows(y, n_epochs, 0)
    fired = torch.zeros(B, dtype=torch.int64, device=dev)
    other = torch.empty_like(y)
    for n in range(n_epochs):
        _lib.run(dev, "wgnn_layout_epoch", _ptr(rowptr), _ptr(col), _ptr(w), B, nnz, wmax, _ptr(y), _ptr(other), n, n_epochs, a, b,
                 gamma, lr * (1.0 - n / n_epochs), n_neg, seed, _ptr(fired), 0, stream)
        y, other = other, y
    return LayoutRows(y, n_epochs, int(fired.sum()))


GEODESIC_LANES, GEODESIC_MAX_BLOCKS = _lib.GEODESIC_LANES, _lib.GEODESIC_MAX_BLOCKS
GROUP_EDGES_MAX_GROUPS = 4096             # group_edges' most groups: a [K, K] int64 table

_GEODESIC_STATUS = ((_lib.GEODESIC_UNSORTED, "a row is not strictly ascending in col"),
                    (_lib.GEODESIC_BAD_COL, "a column is outside [0, n)"),
                    (_lib.GEODESIC_BAD_ROWPTR, "rowptr does not ascend from 0 to nnz"),
                    (_lib.GEODESIC_BAD_LENGTH, "a length is negative, infinite or NaN"))


class DistanceGraph(NamedTuple):
    """What ``distance_graph`` returns, on the device: the symmetric CSR of the union graph - ``rowptr`` int64 [B + 1], ``col`` int32
    ascending within a row (``snn_graph``'s structure) - and ``length`` float32 [nnz], the Euclidean length of every stored edge;
    ``length(i, j)`` and ``length(j, i)`` are the same bits."""
    rowptr: torch.Tensor
    col: torch.Tensor
    length: torch.Tensor


def distance_graph(idx: torch.Tensor, d2: torch.Tensor) -> DistanceGraph:
    """The union graph of ``[B, k]`` neighbour lists with their distances as edge lengths: ``idx`` int32 / int64 (-1 = none) and
    ``d2`` float32 squared distances as ``knn_rows`` leaves them, ``k`` in [1, 64]; ``{i, j}`` is an edge iff one lists the other -
    ``snn_graph``'s keys and ``torch.unique``, so the structure is ``snn_graph``'s exactly - and ``length = sqrt(d2)`` of the listed
    direction.  ``knn_rows`` gives ``d(i, j)`` and ``d(j, i)`` the same bits; where a caller's two directions differ, the smaller
    one is kept, so the result never depends on an order.

    The root is float32 and correctly rounded - the bits of ``np.sqrt(np.float32(d2))``: it is taken in float64 and rounded once
    more, which cannot differ (the root of a 24-bit number lies at least 2^-51, relatively, from every midpoint of two float32
    values, beyond the last bit of a float64), however the framework's float32 ``sqrt`` was built (measured on an MI355X: the
    same bits on 4 000 000 values).  Framework ops only; one read-back
    validates the ids and the distances, one sizes the edge list.  An id outside [-1, B) and a negative, NaN or infinite ``d2`` on a
    listed entry are ``ValueError`` (a self entry is not listed); CPU tensors raise ``WgnnError``.  Returns a ``DistanceGraph``."""
    name = "distance_graph"
    dev = _require_cuda(idx, d2)
    B, k, src, dst = _list_entries(name, idx)
    if not isinstance(d2, torch.Tensor) or d2.dtype != torch.float32 or tuple(d2.shape) != (B, k):
        raise ValueError(f"{name}: d2 must be a float32 [{B}, {k}] tensor")
    listed = (dst >= 0) & (dst != src)
    sq = d2.reshape(-1)[listed]
    if bool((~((sq >= 0) & (sq < float("inf")))).any()):
        raise ValueError(f"{name}: d2 holds a negative, NaN or infinite squared distance on a listed entry")
    rowptr, col, inverse = _union_csr(B, src[listed], dst[listed], return_inverse=True)
    root = torch.sqrt(sq.to(torch.float64)).to(torch.float32)
    length = torch.full((int(col.shape[0]),), float("inf"), dtype=torch.float32, device=dev)
    length.scatter_reduce_(0, inverse, torch.cat([root, root]), "amin")
    return DistanceGraph(rowptr, col, length)


class GeodesicRows(NamedTuple):
    """What ``geodesic_rows`` returns.  On the device: ``dist`` float32 [B] (+inf = not reached) and ``pred`` int32 [B] (the
    neighbour the distance came through; -1 = a root or not reached).  On the host: ``rounds`` (how many rounds changed
    something), ``converged`` (False when ``max_rounds`` cut the run before a round changed nothing) and ``reached`` (the number of
    vertices with a finite distance, the roots included)."""
    dist: torch.Tensor
    pred: torch.Tensor
    rounds: int
    converged: bool
    reached: int


def _geodesic_roots(name, roots, B, dev):
    """``roots`` - an int, or a 1-D sequence / tensor of ints - as a sorted, unique int64 tensor on ``dev``, checked."""
    if isinstance(roots, torch.Tensor):
        if roots.dtype not in (torch.int32, torch.int64) or roots.dim() > 1:
            raise ValueError(f"{name}: roots must be an int or a 1-D int32 / int64 tensor / sequence")
        r = roots.reshape(-1).to(device=dev, dtype=torch.int64)
    else:
        import numpy as np
        arr = np.asarray(roots)
        if arr.dtype.kind not in "iu" or arr.ndim > 1:
            raise ValueError(f"{name}: roots must be an int or a 1-D sequence of ints, got {roots!r}")
        r = torch.as_tensor(arr.reshape(-1).astype(np.int64), device=dev)
    if r.numel() == 0:
        raise ValueError(f"{name}: the root set is empty")
    lo, hi = torch.aminmax(r)
    if int(lo) < 0 or int(hi) >= B:
        raise ValueError(f"{name}: a root is outside [0, {B}) (min {int(lo)}, max {int(hi)})")
    return torch.unique(r)


def geodesic_rows(rowptr: torch.Tensor, col: torch.Tensor, length: torch.Tensor, roots, max_rounds: Optional[int] = None,
                  check_every: int = 8, grid_blocks: int = 0) -> GeodesicRows:
    """The geodesic (shortest-path) distance of every vertex of a graph to the nearest of ``roots``, by a SYNCHRONOUS Bellman-Ford
    in float32 on the device.  ``rowptr`` int64 [B + 1], ``col`` int32 ascending within a row and ``length`` float32 >= 0 - what
    ``distance_graph`` returns: both directions of every edge are stored.  ``roots``: an int, or a 1-D int sequence / tensor.

    From ``dist = 0`` at the roots and ``+inf`` elsewhere, every round (``wgnn_geodesic_round``, ``include/wgnn.h`` has the
    contract) reads the state before it and gives every vertex ``min_u float32(dist[u] + length(u, v))`` under the total order
    (candidate, u) when that is STRICTLY below what it has - one individually rounded add per stored entry, two buffers, no
    atomics on the state - so numpy restates the run round by round and two calls give the same bits.  The fixed point is the
    float32 distance a heap Dijkstra with the same add finds; against float64 it differs by one rounding per hop.

    ``check_every`` rounds are enqueued at a time, each with its own counter, and read back together; a round past the fixed
    point is the identity, so the extra rounds change no bit.  ``max_rounds`` (None = ``B``) caps the rounds RUN - the last batch
    is cut to it - and a run that was still changing when it hit the cap returns the state after exactly ``max_rounds`` rounds with
    ``converged=False``.  ``grid_blocks`` (0 = from ``B``) caps the grid and changes no bit.  O(rounds x nnz): ``rounds`` is the hop
    diameter from the roots, up to ``B - 1`` on a chain.

    A malformed graph (unsorted row, column out of range, bad ``rowptr``, a negative / infinite / NaN length) raises ``WgnnError``
    from the kernel's status word; an out-of-range or empty root set and every other argument error are ``ValueError``; CPU
    tensors raise ``WgnnError``.  Returns a ``GeodesicRows``."""
    name = "geodesic_rows"
    dev = _require_cuda(rowptr, col, length, roots if isinstance(roots, torch.Tensor) else None)
    rowptr, col, length, B, nnz = _graph_operand(name, rowptr, col, length, "length", torch.float32)
    max_rounds = B if max_rounds is None else int(max_rounds)
    check_every, grid_blocks = int(check_every), int(grid_blocks)
    if max_rounds < 0:
        raise ValueError(f"{name}: max_rounds = {max_rounds} must not be negative")
    if check_every < 1:
        raise ValueError(f"{name}: check_every = {check_every} must be >= 1")
    if not 0 <= grid_blocks <= GEODESIC_MAX_BLOCKS:
        raise ValueError(f"{name}: grid_blocks = {grid_blocks} is outside [0, {GEODESIC_MAX_BLOCKS}] (0 = from B)")
    dist = torch.full((B,), float("inf"), dtype=torch.float32, device=dev)
    dist[_geodesic_roots(name, roots, B, dev)] = 0.0
    pred = torch.full((B,), -1, dtype=torch.int32, device=dev)
    stream = _stream(dev)
    dist2, pred2 = torch.empty_like(dist), torch.empty_like(pred)
    slots = torch.empty(check_every + 1, dtype=torch.int64, device=dev)        # one counter per round of a batch, then the status
    status = slots.data_ptr() + 8 * check_every
    done, rounds, converged = 0, 0, B == 0
    while not converged and done < max_rounds:
        batch = min(check_every, max_rounds - done)
        slots.zero_()
        for t in range(batch):
            _lib.run(dev, "wgnn_geodesic_round", _ptr(rowptr), _ptr(col), _ptr(length), B, nnz, _ptr(dist), _ptr(pred), _ptr(dist2),
                     _ptr(pred2), slots.data_ptr() + 8 * t, status, grid_blocks, 0, stream)
            dist, dist2, pred, pred2 = dist2, dist, pred2, pred
        counts = slots.tolist()
        _check_status(name, counts[check_every], _GEODESIC_STATUS)
        done += batch
        changed = sum(1 for c in counts[:batch] if c)
        rounds += changed
        converged = changed < batch                # a round that changed nothing: the fixed point, and every later round is the identity
    reached = int(torch.isfinite(dist).sum()) if B else 0
    return GeodesicRows(dist, pred, rounds, converged, reached)


class GroupEdges(NamedTuple):
    """What ``group_edges`` returns, on the device: ``edges`` int64 [K, K] - ``edges[a, b]`` = the number of list entries that lead
    from a cell of group ``a`` to a cell of group ``b`` - and ``size`` int64 [K], the cells per group."""
    edges: torch.Tensor
    size: torch.Tensor


def group_edges(idx: torch.Tensor, group: torch.Tensor, n_groups: int) -> GroupEdges:
    """The directed kNN graph counted by group: ``idx`` [B, k] int32 / int64 neighbour lists (-1 = none, ``k`` in [1, 64]) and
    ``group`` int32 / int64 [B], a cell's group in ``[0, n_groups)`` or -1 = it takes no part.
    ``edges[a, b] = #{(i, j) : j in list(i), group[i] = a, group[j] = b}`` - an entry with either end at -1 does not count (``knn_rows``
    lists no cell in its own list; a self entry given all the same counts on the diagonal) - and ``size[a]`` = the number of cells of group ``a``; both int64, one integer ``bincount`` of
    ``group[i] * K + group[j]`` each (the coarsening idiom of ``louvain_graph``): exact, whatever the order.  ``n_groups`` in
    [1, 4096].  An id outside [-1, B) and a group outside [-1, n_groups) are ``ValueError``; CPU tensors raise ``WgnnError``."""
    name = "group_edges"
    _require_cuda(idx, group)
    K = int(n_groups)
    if not 1 <= K <= GROUP_EDGES_MAX_GROUPS:
        raise ValueError(f"{name}: n_groups = {K} is outside [1, {GROUP_EDGES_MAX_GROUPS}]")
    B, _, src, dst = _list_entries(name, idx)
    _group_operand(name, ValueError, group, B, K, True)
    g = group.to(torch.int64)
    listed = dst >= 0
    ga, gb = g[src[listed]], g[dst[listed]]
    both = (ga >= 0) & (gb >= 0)
    edges = torch.bincount(ga[both] * K + gb[both], minlength=K * K).reshape(K, K)
    size = torch.bincount(g[g >= 0], minlength=K)
    return GroupEdges(edges, size)


DIFFUSION_LANES, DIFFUSION_MAX_BLOCKS, DIFFUSION_MAX_COMPS = _lib.DIFFUSION_LANES, _lib.DIFFUSION_MAX_BLOCKS, _lib.DIFFUSION_MAX_COMPS
LANCZOS_CHUNK, LANCZOS_MAX_STEPS, LANCZOS_BREAKDOWN = _lib.LANCZOS_CHUNK, _lib.LANCZOS_MAX_STEPS, _lib.LANCZOS_BREAKDOWN
LANCZOS_BASIS_BYTES = 4 << 30             # lanczos_graph: the basis [steps + 1, B] float64 stays under this

_DIFFUSION_STATUS = ((_lib.DIFFUSION_UNSORTED, "a row is not strictly ascending in col"),
                     (_lib.DIFFUSION_BAD_COL, "a column is outside [0, n)"),
                     (_lib.DIFFUSION_BAD_ROWPTR, "rowptr does not ascend from 0 to nnz"),
                     (_lib.DIFFUSION_BAD_WEIGHT, "a weight is negative, infinite or NaN"))


def _check_grid(name, grid_blocks) -> int:
    grid_blocks = int(grid_blocks)
    if not 0 <= grid_blocks <= DIFFUSION_MAX_BLOCKS:
        raise ValueError(f"{name}: grid_blocks = {grid_blocks} is outside [0, {DIFFUSION_MAX_BLOCKS}] (0 = from B)")
    return grid_blocks


def graph_components(rowptr: torch.Tensor, col: torch.Tensor) -> torch.Tensor:
    """The connected components of a symmetric CSR graph (``rowptr`` int64 [B + 1], ``col`` int32; both directions of every edge
    stored), on the device: int64 [B], the lowest vertex of every vertex's component - min-label propagation with framework ops,
    in integers, one read-back per round and as many rounds as the longest shortest path to a component's lowest vertex.  A
    ``rowptr`` that does not ascend from 0 to ``nnz`` or a column outside [0, B) is a ``ValueError`` (one read-back); CPU tensors
    raise ``WgnnError``."""
    name = "graph_components"
    dev = _require_cuda(rowptr, col)
    if rowptr.dim() != 1 or rowptr.dtype != torch.int64 or rowptr.shape[0] < 1 or col.dim() != 1 or col.dtype != torch.int32:
        raise ValueError(f"{name}: rowptr int64 [B + 1] and col int32 [nnz] are expected")
    B, nnz = int(rowptr.shape[0]) - 1, int(col.shape[0])
    deg = rowptr[1:] - rowptr[:-1]
    bad = torch.stack([rowptr[0] != 0, rowptr[-1] != nnz, (deg < 0).any(), ((col < 0) | (col >= B)).any()]).tolist()
    if any(bad):
        raise ValueError(f"{name}: rowptr does not ascend from 0 to nnz = {nnz}, or a column is outside [0, {B})")
    row = torch.repeat_interleave(torch.arange(B, dtype=torch.int64, device=dev), deg)
    return _min_labels(B, row, col.long(), dev)


class DiffusionOperator(NamedTuple):
    """What ``diffusion_operator`` returns, on the device, float64: ``t`` [nnz] - the density-normalised symmetric transition
    matrix on the graph's own structure, ``t(i, j)`` and ``t(j, i)`` the same bits - and the per-row ``q`` (the sum of the row's
    weights) and ``z`` (the root of the sum of the row's ``w / (q_i q_j)``) [B]; an empty row has ``q = z = 0``."""
    t: torch.Tensor
    q: torch.Tensor
    z: torch.Tensor


def diffusion_operator(rowptr: torch.Tensor, col: torch.Tensor, w: torch.Tensor, grid_blocks: int = 0) -> DiffusionOperator:
    """scanpy's density-normalised symmetric transition matrix of a symmetric weighted CSR graph (``rowptr`` int64 [B + 1], ``col``
    int32 ascending within a row, ``w`` float32 >= 0 - what ``fuzzy_graph`` returns), in float64 on the device: ``q_i = sum_j w_ij``,
    ``K_ij = w_ij / (q_i q_j)``, ``z_i = sqrt(sum_j K_ij)``, ``t_ij = K_ij / (z_i z_j)`` (``include/wgnn.h`` has the contract) -
    ``neighbors.Neighbors.compute_transitions(density_normalize=True)``'s ``transitions_sym``.  Every row sum runs in
    ``wgnn_layout_epoch``'s order and every operation is rounded on its own, so numpy restates it bit for bit and the grid
    (``grid_blocks``, 0 = from ``B``) changes nothing; an entry with ``w == 0`` gives ``t = +0.0``.  The matrix has the eigenvalue 1
    with the eigenvector ``z`` on every connected component.  Three launches and one read-back (the status word): a malformed
    graph (unsorted row, column out of range, bad ``rowptr``, a negative / infinite / NaN weight) raises ``WgnnError``; every
    argument error is a ``ValueError``; CPU tensors raise ``WgnnError``.  Returns a ``DiffusionOperator``."""
    name = "diffusion_operator"
    dev = _require_cuda(rowptr, col, w)
    rowptr, col, w, B, nnz = _graph_operand(name, rowptr, col, w, "w", torch.float32)
    grid_blocks = _check_grid(name, grid_blocks)
    stream = _stream(dev)
    q, z = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)
    t = torch.zeros(nnz, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int64, device=dev)
    graph = (_ptr(rowptr), _ptr(col), _ptr(w), B, nnz)
    _lib.run(dev, "wgnn_diffusion_degree", *graph, None, _ptr(q), _ptr(status), grid_blocks, 0, stream)
    _lib.run(dev, "wgnn_diffusion_degree", *graph, _ptr(q), _ptr(z), _ptr(status), grid_blocks, 0, stream)
    _lib.run(dev, "wgnn_diffusion_weights", *graph, _ptr(q), _ptr(z), _ptr(t), _ptr(status), grid_blocks, 0, stream)
    _check_status(name, int(status), _DIFFUSION_STATUS)
    return DiffusionOperator(t, q, z)


class LanczosRows(NamedTuple):
    """What ``lanczos_graph`` returns.  On the device, float64: ``V`` [m + 1, B] - the basis, a vector per contiguous row, ``V[0]``
    the deflated ``z mask / ||z mask||`` and the rows past ``n_run`` zero - and ``alpha`` / ``beta`` [m] (``alpha[j - 1]`` is step
    ``j``'s diagonal entry, ``beta[j - 1]`` the norm it left; zero past ``n_run``).  On the host: ``n_run`` (the steps run: ``m =
    min(n_steps, cells of the mask - 1)`` unless the run broke down), ``breakdown`` (a norm fell to 2^-26 or below: the Krylov
    space is exhausted) and ``n_cells`` (the cells of the mask)."""
    V: torch.Tensor
    alpha: torch.Tensor
    beta: torch.Tensor
    n_run: int
    breakdown: bool
    n_cells: int


def lanczos_steps(n_cells: int) -> int:
    """``lanczos_graph``'s default number of steps: 128 below 10 000 cells, 256 from there on (the float64 prototype's figures in
    profiles/resident_diffmap.md: 128 steps leave the 15 leading eigenvalues of a 20 000-cell graph at 4e-11, 256 at 5e-15)."""
    return 128 if n_cells < 10000 else 256


def lanczos_graph(rowptr: torch.Tensor, col: torch.Tensor, t: torch.Tensor, z: torch.Tensor, mask: torch.Tensor,
                  n_steps: Optional[int] = None, seed: int = 0, check_every: int = 16, grid_blocks: int = 0) -> LanczosRows:
    """A Lanczos iteration with full re-orthogonalisation and a fixed number of steps on the symmetric matrix ``t`` float64 [nnz]
    over the CSR ``rowptr`` int64 [B + 1] / ``col`` int32 (``diffusion_operator``'s), restricted to the cells of ``mask`` bool [B] -
    a union of connected components - with the known eigenvector ``z`` float64 [B] of eigenvalue 1 deflated, on the device
    (``include/wgnn.h`` has the contracts).  ``V[0] = z mask / ||z mask||``; ``V[1]`` starts from a counter hash of ``(seed, i)`` in
    [-1, 1), zero outside the mask, orthogonalised against ``V[0]`` twice and normalised.  Step ``j = 1 .. m``: ``w = T V[j]``
    (``wgnn_lanczos_apply``); ``c = V[0 .. j] w`` with ``alpha_j = c[j]`` (``wgnn_lanczos_dots``); ``w -= V[r] c[r]``, ``r`` ascending
    (``wgnn_lanczos_update``); dots and update once more (classical Gram-Schmidt twice); ``beta_j = ||w||``; ``V[j + 1] = w /
    beta_j`` (``wgnn_lanczos_scale``; not formed after the last step).  ``m = min(n_steps, cells of the mask - 1)``; ``n_steps`` =
    None: 128 below 10 000 cells, 256 from there on; at most 1024.  Every sum runs in a stated order and every operation is
    rounded on its own, so numpy restates the run bit for bit, two calls give the same bits and ``grid_blocks`` (0 = from ``B``)
    changes none; a row outside the mask stays exactly zero.

    The run ends after the first step that leaves ``beta_j <= 2^-26`` (``breakdown``).  ``beta`` stays on the device: the norm that
    finds it sets a halt word there, every launch enqueued behind it finds the word and does nothing, and the host reads the
    word once per ``check_every`` steps - no read-back inside a step.  Ten launches a step.  The basis takes ``(m + 1) B`` float64;
    more than ``LANCZOS_BASIS_BYTES`` is a ``ValueError``, as every argument error; a malformed graph raises ``WgnnError`` from
    the status word; CPU tensors raise ``WgnnError``.  Returns a ``LanczosRows``."""
    name = "lanczos_graph"
    dev = _require_cuda(rowptr, col, t, z, mask)
    rowptr, col, t, B, nnz = _graph_operand(name, rowptr, col, t, "t", torch.float64)
    if z.dtype != torch.float64 or tuple(z.shape) != (B,) or mask.dtype != torch.bool or tuple(mask.shape) != (B,):
        raise ValueError(f"{name}: z float64 [{B}] and mask bool [{B}] are expected")
    n_steps = lanczos_steps(B) if n_steps is None else int(n_steps)
    seed, check_every, grid_blocks = int(seed), int(check_every), _check_grid(name, grid_blocks)
    if not 1 <= n_steps <= LANCZOS_MAX_STEPS:
        raise ValueError(f"{name}: n_steps = {n_steps} is outside [1, {LANCZOS_MAX_STEPS}]")
    if not 0 <= seed < 2 ** 32:
        raise ValueError(f"{name}: seed = {seed} is outside [0, 2^32)")
    if check_every < 1:
        raise ValueError(f"{name}: check_every = {check_every} must be >= 1")
    n_c = int(mask.sum()) if B else 0
    m = max(0, min(n_steps, n_c - 1))
    if (m + 1) * B * 8 > LANCZOS_BASIS_BYTES:
        raise ValueError(f"{name}: the basis [{m + 1}, {B}] float64 takes {(m + 1) * B * 8} bytes, above LANCZOS_BASIS_BYTES = "
                         f"{LANCZOS_BASIS_BYTES}: lower n_steps")
    V = torch.zeros((m + 1, B), dtype=torch.float64, device=dev)
    alpha, beta = torch.zeros(m, dtype=torch.float64, device=dev), torch.zeros(m, dtype=torch.float64, device=dev)
    if n_c == 0:
        return LanczosRows(V, alpha, beta, 0, False, 0)
    stream = _stream(dev)
    z, mask8 = z.contiguous(), mask.to(torch.uint8).contiguous()
    w, w1 = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
    c, nrm = torch.empty(m + 1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    words = torch.zeros(2, dtype=torch.int64, device=dev)                      # the halt word, then the status
    halt, status = words.data_ptr(), words.data_ptr() + 8
    ws_bytes = int(_lib.lib().wgnn_lanczos_dots_workspace_bytes(B, m + 1))
    ws = torch.empty(max(1, ws_bytes // 8), dtype=torch.float64, device=dev)
    row = lambda j: V.data_ptr() + 8 * B * j

    def ortho(n_rows, vec, keep=None):                                          # classical Gram-Schmidt, twice
        for k in (keep, None):
            _lib.run(dev, "wgnn_lanczos_dots", _ptr(V), B, n_rows, _ptr(vec), B, _ptr(c), k, halt, 1, _ptr(ws), ws_bytes, grid_blocks,
                     0, stream)
            _lib.run(dev, "wgnn_lanczos_update", _ptr(V), B, n_rows, _ptr(c), _ptr(vec), B, halt, grid_blocks, 0, stream)

    def norm(vec, keep, tag):
        _lib.run(dev, "wgnn_lanczos_dots", None, 0, 1, _ptr(vec), B, _ptr(nrm), keep, halt, tag, _ptr(ws), ws_bytes, grid_blocks,
                 _lib.LANCZOS_NORM, stream)

    def scale(vec, by, j):
        _lib.run(dev, "wgnn_lanczos_scale", _ptr(vec), by, row(j), B, halt, grid_blocks, 0, stream)

    _lib.run(dev, "wgnn_lanczos_init", _ptr(z), _ptr(mask8), B, seed, _ptr(w), _ptr(w1), 0, stream)
    norm(w, None, -1)
    scale(w, _ptr(nrm), 0)
    if m >= 1:
        ortho(1, w1)
        norm(w1, None, -1)
        scale(w1, _ptr(nrm), 1)
    done, halted, bits = 0, 0, 0
    while True:
        batch = min(check_every, m - done)
        for j in range(done + 1, done + batch + 1):
            _lib.run(dev, "wgnn_lanczos_apply", _ptr(rowptr), _ptr(col), _ptr(t), B, nnz, row(j), _ptr(w), halt, status, grid_blocks, 0,
                     stream)
            ortho(j + 1, w, alpha.data_ptr() + 8 * (j - 1))
            norm(w, beta.data_ptr() + 8 * (j - 1), j)
            if j < m:
                scale(w, beta.data_ptr() + 8 * (j - 1), j + 1)
        done += batch
        halted, bits = words.tolist()
        _check_status(name, bits, _DIFFUSION_STATUS)
        if halted or done >= m:
            break
    n_run = m if not halted else max(0, halted)                                 # -1: a start vector had no norm
    return LanczosRows(V, alpha, beta, n_run, bool(halted), n_c)


def lanczos_ritz(alpha, beta, n: int):
    """The host step between ``lanczos_graph`` and ``basis_combine``, in numpy: ``(theta [n], S [n, n], residual [n])`` of the
    ``n x n`` tridiagonal with diagonal ``alpha[:n]`` and off-diagonal ``beta[:n - 1]`` by ``numpy.linalg.eigh`` on the dense
    matrix - the Ritz values descending (ties by ``eigh``'s position), ``S``'s columns in that order, and the residual estimate
    ``|beta[n - 1] S[n - 1, c]|`` of every Ritz pair.  ``alpha`` / ``beta``: arrays or tensors with at least ``n`` entries."""
    import numpy as np
    to_host = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    a, b, n = to_host(alpha).astype(np.float64), to_host(beta).astype(np.float64), int(n)
    if n < 0 or a.ndim != 1 or b.ndim != 1 or len(a) < n or len(b) < n:
        raise ValueError(f"lanczos_ritz: alpha and beta must hold at least n = {n} entries")
    if n == 0:
        return np.zeros(0), np.zeros((0, 0)), np.zeros(0)
    theta, S = np.linalg.eigh(np.diag(a[:n]) + np.diag(b[:n - 1], 1) + np.diag(b[:n - 1], -1))
    order = np.argsort(-theta, kind="stable")
    return theta[order], np.ascontiguousarray(S[:, order]), np.abs(b[n - 1] * S[n - 1, order])


def basis_combine(V: torch.Tensor, S) -> torch.Tensor:
    """The Ritz vectors of a Lanczos run on the device: ``Y`` float64 [B, 1 + n_cols] with ``Y[:, 0] = V[0]`` and ``Y[i, c] =
    sum_{j = 1 .. m} V[j, i] S[j - 1, c - 1]``, ``j`` ascending, every product and add rounded on its own (``wgnn_basis_combine``;
    row-local, so numpy restates it bit for bit).  ``V`` float64 [>= m + 1, B] (``lanczos_graph``'s), ``S`` float64 [m, n_cols] -
    columns of ``lanczos_ritz``'s, a numpy array or a tensor - with ``n_cols`` <= 63.  Then every column but the first is given
    the sign that makes its entry of largest magnitude (the lowest cell among equal ones) positive, with framework ops: a
    multiplication by +-1."""
    import numpy as np
    name = "basis_combine"
    dev = _require_cuda(V)
    S = torch.as_tensor(np.ascontiguousarray(S, dtype=np.float64) if not isinstance(S, torch.Tensor) else S, device=dev)
    if V.dim() != 2 or V.dtype != torch.float64 or S.dim() != 2 or S.dtype != torch.float64:
        raise ValueError(f"{name}: V float64 [m + 1, B] and S float64 [m, n_cols] are expected")
    (m, n_cols), B = S.shape, int(V.shape[1])
    if V.shape[0] < m + 1 or m > LANCZOS_MAX_STEPS or n_cols >= DIFFUSION_MAX_COMPS:
        raise ValueError(f"{name}: S [{m}, {n_cols}] does not fit V {tuple(V.shape)} (at most {LANCZOS_MAX_STEPS} steps, "
                         f"{DIFFUSION_MAX_COMPS - 1} columns)")
    V, S = V.contiguous(), S.contiguous()
    Y = torch.zeros((B, n_cols + 1), dtype=torch.float64, device=dev)
    _lib.run(dev, "wgnn_basis_combine", _ptr(V), B, m, _ptr(S) if n_cols else None, n_cols, n_cols, _ptr(Y), n_cols + 1, B, 0,
             _stream(dev))
    if B and n_cols:
        mag = Y[:, 1:].abs()
        cells = torch.arange(B, device=dev)[:, None].expand(B, n_cols)
        first = torch.where(mag == mag.max(dim=0).values, cells, B).min(dim=0).values.clamp(max=B - 1)   # a NaN column: any cell
        Y[:, 1:] *= torch.where(Y[first, torch.arange(1, n_cols + 1, device=dev)] < 0, -1.0, 1.0)
    return Y


def diffusion_distance(Y: torch.Tensor, g, roots) -> torch.Tensor:
    """Diffusion pseudotime's distance on the device: ``d_i = min over roots r of sqrt(sum_{l = 1 .. n_dcs - 1} (g_l (Y[r, l] -
    Y[i, l]))^2)``, float64 [B], the sum sequential in ``l`` and every operation rounded on its own (``wgnn_diffusion_distance``;
    numpy restates it bit for bit).  ``Y`` float64 [B, >= n_dcs] (``basis_combine``'s; column 0 is not read), ``g`` float64
    [n_dcs] - ``lambda_l / (1 - lambda_l)``, computed by the caller; ``n_dcs`` in [2, 64] - and ``roots`` as ``geodesic_rows``
    takes them.  A NaN coordinate gives a NaN distance."""
    import numpy as np
    name = "diffusion_distance"
    dev = _require_cuda(Y, roots if isinstance(roots, torch.Tensor) else None)
    g = torch.as_tensor(np.ascontiguousarray(g, dtype=np.float64) if not isinstance(g, torch.Tensor) else g, device=dev)
    if Y.dim() != 2 or Y.dtype != torch.float64 or g.dim() != 1 or g.dtype != torch.float64:
        raise ValueError(f"{name}: Y float64 [B, n] and g float64 [n_dcs] are expected")
    B, n_dcs = int(Y.shape[0]), int(g.shape[0])
    if not 2 <= n_dcs <= min(DIFFUSION_MAX_COMPS, int(Y.shape[1])):
        raise ValueError(f"{name}: n_dcs = {n_dcs} is outside [2, {min(DIFFUSION_MAX_COMPS, int(Y.shape[1]))}]")
    r = _geodesic_roots(name, roots, B, dev)
    Y, g = Y.contiguous(), g.contiguous()
    d = torch.empty(B, dtype=torch.float64, device=dev)
    _lib.run(dev, "wgnn_diffusion_distance", _ptr(Y), int(Y.shape[1]), B, _ptr(g), n_dcs, _ptr(r), int(r.shape[0]), _ptr(d), 0,
             _stream(dev))
    return d


HARMONY_MAX_K, HARMONY_MAX_BATCHES, HARMONY_MAX_D, HARMONY_MAX_BLOCKS = (_lib.HARMONY_MAX_K, _lib.HARMONY_MAX_BATCHES, _lib.HARMONY_MAX_D,
                                                                         _lib.HARMONY_MAX_BLOCKS)      # the wgnn_harmony_* limits
HARMONY_MAX_GRID = 1 << 16


def _f64(name, what, t, shape):
    """``t`` checked as a contiguous float64 tensor of ``shape`` (``None`` entries are free); returns it."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != len(shape) or not t.is_contiguous() or \
            any(s is not None and int(n) != s for n, s in zip(t.shape, shape)):
        want = ", ".join("*" if s is None else str(s) for s in shape)
        raise ValueError(f"{name}: {what} must be a contiguous float64 tensor [{want}]")
    return t


def _harmony_sizes(name, B=None, K=None, S=None, D=None, n_blocks=None, grid_blocks=0):
    for what, v, lo, hi in (("B", B, 1, 2 ** 31 - 1), ("K", K, 1, HARMONY_MAX_K), ("S", S, 1, HARMONY_MAX_BATCHES),
                            ("D", D, 1, HARMONY_MAX_D), ("n_blocks", n_blocks, 1, HARMONY_MAX_BLOCKS),
                            ("grid_blocks", grid_blocks, 0, HARMONY_MAX_GRID)):
        if v is not None and not lo <= int(v) <= hi:
            raise ValueError(f"{name}: {what} = {int(v)} is outside [{lo}, {hi}]")


def _harmony_batch(name, batch, B):
    if not isinstance(batch, torch.Tensor) or batch.dtype != torch.int32 or tuple(batch.shape) != (B,) or not batch.is_contiguous():
        raise ValueError(f"{name}: batch must be a contiguous int32 tensor [{B}]")
    return batch


def harmony_scores(U: torch.Tensor, Y: torch.Tensor, sigma: float, want_dot: bool = False):
    """``wgnn_harmony_scores``: ``(dot | None, dist, e)`` float64 [B, K] of the unit rows ``U`` [B, D] against the unit centres
    ``Y`` [K, D] (both float64): ``dot_ik = sum_j U_ij Y_kj`` (``j`` ascending, a product and an add each), ``dist = 2 (1 - dot)``,
    ``e_ik = exp(-dist_ik / sigma - max_k(-dist_ik / sigma))``.  ``dot`` and ``dist`` are numpy's bits."""
    name = "harmony_scores"
    U, Y = _f64(name, "U", U, (None, None)), _f64(name, "Y", Y, (None, None))
    (B, D), K = U.shape, int(Y.shape[0])
    if Y.shape[1] != D:
        raise ValueError(f"{name}: Y has {Y.shape[1]} columns, U {D}")
    _harmony_sizes(name, B=B, K=K, D=D)
    if not (float(sigma) > 0 and math.isfinite(float(sigma))):
        raise ValueError(f"{name}: sigma = {sigma} must be positive and finite")
    dev = _require_cuda(U, Y)
    dot = torch.empty((B, K), dtype=torch.float64, device=dev) if want_dot else None
    dist, e = torch.empty((B, K), dtype=torch.float64, device=dev), torch.empty((B, K), dtype=torch.float64, device=dev)
    _lib.run(dev, "wgnn_harmony_scores", _ptr(U), D, _ptr(Y), D, B, D, K, float(sigma), _ptr(dot), _ptr(dist), _ptr(e), 0,
             _stream(dev))
    return dot, dist, e


def harmony_assign_block(e: torch.Tensor, batch: torch.Tensor, n_batches: int, n_blocks: int, q: int, R: torch.Tensor,
                         pen: Optional[torch.Tensor] = None, workspace: Optional[tuple] = None, grid_blocks: int = 0) -> tuple:
    """``wgnn_harmony_assign_block``: the rows ``q, q + n_blocks, ...`` of ``R`` float64 [B, K] become ``e * pen[:, b_i]``
    divided by its sum over ``k`` (ascending); ``pen`` float64 [K, S] = None: ones.  No other row of ``R`` is written.  Returns
    the workspace ``(tensor, n_bytes)`` that now holds the block's chunk tables - ``harmony_fold``'s first argument, and what to
    pass back as ``workspace`` for the next block.  ``grid_blocks`` (0 = chosen) changes no bit."""
    name = "harmony_assign_block"
    e = _f64(name, "e", e, (None, None))
    B, K = e.shape
    S, n_blocks, q = int(n_batches), int(n_blocks), int(q)
    _harmony_sizes(name, B=B, K=K, S=S, n_blocks=n_blocks, grid_blocks=grid_blocks)
    if not 0 <= q < n_blocks:
        raise ValueError(f"{name}: q = {q} is outside [0, {n_blocks})")
    _f64(name, "R", R, (B, K))
    _harmony_batch(name, batch, B)
    if pen is not None:
        _f64(name, "pen", pen, (K, S))
    dev = _require_cuda(e, batch, R, pen)
    ws, ws_bytes = _workspace(dev, "wgnn_harmony_assign_workspace_bytes", B, K, S, n_blocks, have=workspace or (None, 0))
    _lib.run(dev, "wgnn_harmony_assign_block", _ptr(e), _ptr(batch), _ptr(pen), B, K, S, n_blocks, q, _ptr(R), _ptr(ws), ws_bytes,
             int(grid_blocks), 0, _stream(dev))
    return ws, ws_bytes


def harmony_fold(T: torch.Tensor, Pr: torch.Tensor, theta: Optional[torch.Tensor], n_rows: int, q_store: int = -1, q_skip: int = -1,
                 workspace: Optional[tuple] = None, want_pen: bool = True, out: Optional[tuple] = None):
    """``wgnn_harmony_fold``, one workgroup: with ``q_store >= 0`` the table ``T[q_store]`` of ``T`` float64 [n_blocks, K, S] is
    retaken from the chunk tables that ``harmony_assign_block`` left in ``workspace``; then ``O`` = the sum of ``T`` without block
    ``q_skip`` (-1: of all), ``E = rowsum(O) * Pr`` and ``pen = pow((E + 1) / (O + 1), theta)``.  Returns ``(O, E, pen | None)``
    float64 [K, S] - ``out`` when given."""
    name = "harmony_fold"
    T = _f64(name, "T", T, (None, None, None))
    n_blocks, K, S = T.shape
    _harmony_sizes(name, B=n_rows, K=K, S=S, n_blocks=n_blocks)
    _f64(name, "Pr", Pr, (S,))
    if want_pen:
        _f64(name, "theta", theta, (S,))
    q_store, q_skip = int(q_store), int(q_skip)
    if not -1 <= q_store < n_blocks or not -1 <= q_skip < n_blocks:
        raise ValueError(f"{name}: q_store = {q_store} and q_skip = {q_skip} must be in [-1, {n_blocks})")
    if q_store >= 0 and workspace is None:
        raise ValueError(f"{name}: q_store needs the workspace that harmony_assign_block returned")
    dev = _require_cuda(T, Pr, theta)
    if out is None:
        out = tuple(torch.empty((K, S), dtype=torch.float64, device=dev) for _ in range(3 if want_pen else 2))
    O, E = _f64(name, "out's O", out[0], (K, S)), _f64(name, "out's E", out[1], (K, S))
    pen = _f64(name, "out's pen", out[2], (K, S)) if want_pen else None
    ws, ws_bytes = workspace if q_store >= 0 else (None, 0)
    _lib.run(dev, "wgnn_harmony_fold", _ptr(ws), ws_bytes, int(n_rows), _ptr(T), _ptr(Pr), _ptr(theta) if want_pen else None, K, S,
             n_blocks, q_store, q_skip, _ptr(O), _ptr(E), _ptr(pen), 0, _stream(dev))
    return O, E, pen


def weighted_group_reduce(X: torch.Tensor, R: torch.Tensor, group: Optional[torch.Tensor], n_groups: int,
                          out: Optional[tuple] = None, major: Optional[tuple] = None, grid_blocks: int = 0):
    """``wgnn_weighted_group_reduce``: ``(M float64 [K, S, D], n float64 [K, S])`` with ``M[k, s] = sum of R[i, k] * X[i]`` and
    ``n[k, s] = sum of R[i, k]`` over the rows ``i`` of group ``s`` - ``X`` float64 [B, D], ``R`` float64 [B, K], ``group`` int32 /
    int64 [B] in ``[0, S)`` (any other id = the row takes no part; ``None`` with ``S = 1``: every row).  The rows of a group are
    added in ascending order, in chunks of 256 and chunk by chunk, every product and add rounded on its own: numpy's bits, and
    two calls are bit-identical.  ``major``: ``_group_major(group, S)`` where the caller already has it; ``grid_blocks`` (0 =
    chosen) changes no bit."""
    name = "weighted_group_reduce"
    X, R = _f64(name, "X", X, (None, None)), _f64(name, "R", R, (None, None))
    (B, D), K, S = X.shape, int(R.shape[1]), int(n_groups)
    if R.shape[0] != B:
        raise ValueError(f"{name}: R has {R.shape[0]} rows, X {B}")
    _harmony_sizes(name, B=B, K=K, S=S, D=D, grid_blocks=grid_blocks)
    if group is None and major is None and S != 1:
        raise ValueError(f"{name}: without group, n_groups must be 1")
    dev = _require_cuda(X, R, group)
    if major is None:
        if group is None:
            group = torch.zeros(B, dtype=torch.int32, device=dev)
        _group_operand(name, ValueError, group, B, S, False, says=f"{name}: group must hold one int32 / int64 id per row ([{B}])")
        major = _group_major(group, S)
    order, seg_ptr = major
    if out is None:
        out = (torch.empty((K, S, D), dtype=torch.float64, device=dev), torch.empty((K, S), dtype=torch.float64, device=dev))
    M, n = _f64(name, "out's M", out[0], (K, S, D)), _f64(name, "out's n", out[1], (K, S))
    ws, ws_bytes = _workspace(dev, "wgnn_weighted_group_reduce_workspace_bytes", B, K, S, D)
    _lib.run(dev, "wgnn_weighted_group_reduce", _ptr(X), D, _ptr(R), _ptr(order), _ptr(seg_ptr), B, D, K, S, _ptr(M), _ptr(n),
             _ptr(ws), ws_bytes, int(grid_blocks), 0, _stream(dev))
    return M, n


def harmony_objective(R: torch.Tensor, dist: torch.Tensor, batch: torch.Tensor, O: torch.Tensor, E: torch.Tensor,
                      theta: torch.Tensor, sigma: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``wgnn_harmony_objective``: float64 [4] on the device - harmonypy's objective ``sum R dist + sigma sum R log R + sigma sum
    R theta log((O + 1) / (E + 1))`` and its three sums (the last two before ``sigma``), rows in chunks of 256."""
    name = "harmony_objective"
    R = _f64(name, "R", R, (None, None))
    B, K = R.shape
    _f64(name, "dist", dist, (B, K))
    O = _f64(name, "O", O, (K, None))
    S = int(O.shape[1])
    _harmony_sizes(name, B=B, K=K, S=S)
    _f64(name, "E", E, (K, S)), _f64(name, "theta", theta, (S,))
    _harmony_batch(name, batch, B)
    if not (float(sigma) > 0 and math.isfinite(float(sigma))):
        raise ValueError(f"{name}: sigma = {sigma} must be positive and finite")
    dev = _require_cuda(R, dist, batch, O, E, theta)
    out = torch.empty(4, dtype=torch.float64, device=dev) if out is None else _f64(name, "out", out, (4,))
    ws, ws_bytes = _workspace(dev, "wgnn_harmony_objective_workspace_bytes", B)
    _lib.run(dev, "wgnn_harmony_objective", _ptr(R), _ptr(dist), _ptr(batch), _ptr(O), _ptr(E), _ptr(theta), B, K, S, float(sigma),
             _ptr(out), _ptr(ws), ws_bytes, 0, _stream(dev))
    return out


def harmony_apply(Z0: torch.Tensor, R: Optional[torch.Tensor] = None, W: Optional[torch.Tensor] = None,
                  batch: Optional[torch.Tensor] = None, out: Optional[tuple] = None, grid_blocks: int = 0):
    """``wgnn_harmony_apply``: ``(Zc, U)`` float64 [B, D] with ``Zc_i = Z0_i - sum_k R[i, k] W[k, b_i]`` (``k`` ascending) and
    ``U_i = Zc_i / sqrt(sum_j Zc_ij^2)`` (``j`` ascending) - ``W`` float64 [K, S, D].  Without ``R``: ``(Z0, unit(Z0))``.  numpy's
    bits; a zero row gives NaN."""
    name = "harmony_apply"
    Z0 = _f64(name, "Z0", Z0, (None, None))
    B, D = Z0.shape
    K = S = 1
    if R is not None:
        R = _f64(name, "R", R, (B, None))
        K = int(R.shape[1])
        W = _f64(name, "W", W, (K, None, D))
        S = int(W.shape[1])
        _harmony_batch(name, batch, B)
    _harmony_sizes(name, B=B, K=K, S=S, D=D, grid_blocks=grid_blocks)
    dev = _require_cuda(Z0, R, W, batch)
    if out is None:
        out = (torch.empty((B, D), dtype=torch.float64, device=dev) if R is not None else Z0,
               torch.empty((B, D), dtype=torch.float64, device=dev))
    Zc, U = _f64(name, "out's Zc", out[0], (B, D)), _f64(name, "out's U", out[1], (B, D))
    _lib.run(dev, "wgnn_harmony_apply", _ptr(Z0), D, _ptr(R), _ptr(W) if R is not None else None,
             _ptr(batch) if R is not None else None, B, D, K, S, _ptr(Zc) if R is not None else None, _ptr(U), int(grid_blocks), 0,
             _stream(dev))
    return Zc, U


def harmony_ridge(M: torch.Tensor, n: torch.Tensor, lamb: float) -> torch.Tensor:
    """``W`` float64 [K, S, D]: the ridge offsets of harmonypy's ``moe_correct_ridge`` from the moments ``M`` [K, S, D] and ``n``
    [K, S] in closed form (the system has an arrow shape; the intercept is dropped)::

        w0_k = (sum_s lamb M_ks / (n_ks + lamb)) / (sum_s lamb n_ks / (n_ks + lamb));    W_ks = (M_ks - n_ks w0_k) / (n_ks + lamb)

    with float64 framework operations, one rounding each, the sums sequential with ``s`` ascending from 0: numpy's bits."""
    K, S, D = M.shape
    lamb = float(lamb)
    num, den = torch.zeros((K, D), dtype=torch.float64, device=M.device), torch.zeros(K, dtype=torch.float64, device=M.device)
    for s in range(S):
        nl = n[:, s] + lamb
        num = num + (M[:, s] * lamb) / nl[:, None]
        den = den + (n[:, s] * lamb) / nl
    w0 = num / den[:, None]
    W = torch.empty_like(M)
    for s in range(S):
        W[:, s] = (M[:, s] - n[:, s, None] * w0) / (n[:, s] + lamb)[:, None]
    return W


class HarmonyRows(NamedTuple):
    """What ``harmony_rows`` returns.  On the device, float64: ``coords`` [B, D] (the corrected rows), ``R`` [B, K] (the soft
    cluster memberships), ``centers`` [K, D] (unit rows), ``O`` / ``E`` [K, S] (observed and expected cluster-by-batch mass).  On
    the host: ``objective`` (one value per round, the seeding's first), ``objective_cluster`` (every clustering iteration's),
    ``inner_iters`` (clustering iterations per round), ``n_iter`` (rounds) and ``converged``."""
    coords: torch.Tensor
    R: Optional[torch.Tensor]
    centers: Optional[torch.Tensor]
    O: Optional[torch.Tensor]
    E: Optional[torch.Tensor]
    objective: list
    objective_cluster: list
    inner_iters: list
    n_iter: int
    converged: bool


def harmony_default_clusters(n_cells: int) -> int:
    """Harmony's default number of clusters: ``min(round(B / 30), 100)``, at least 1."""
    return max(1, min(int(round(n_cells / 30.0)), 100))


def harmony_rows(x: torch.Tensor, batch: torch.Tensor, n_batches: int, n_clusters: Optional[int] = None, theta=2.0,
                 sigma: float = 0.1, lamb: float = 1.0, n_blocks: int = 20, max_iter: int = 10, max_iter_cluster: int = 20,
                 epsilon_cluster: float = 1e-5, epsilon: float = 1e-4, seed: int = 0) -> HarmonyRows:
    """Harmony (Korsunsky et al. 2019) on the rows of ``x`` [B, D] float32 with one batch id per row (``batch`` int32 / int64 in
    ``[0, n_batches)``; an empty batch is allowed), on the device, in float64, deterministic::

        Z0 = f64(x);  U = unit(Z0);  Y = unit(f64(kmeans_rows(f32(U), K, seed=seed, max_iter=25).centers))
        scores;  R = softmax(-dist / sigma) block by block;  objective
        for round in 1 .. max_iter:
            for it in 1 .. max_iter_cluster:
                Y = unit(sum_i R_ik U_i);  scores;  for q in 0 .. n_blocks - 1: re-assign block q under pen_q;  objective
                stop from it = 4 on when (old - new) / |old| < epsilon_cluster, old / new the sums of the previous / latest 3 values
            M, n = moments of Z0 under R per (cluster, batch);  W = harmony_ridge(M, n, lamb);  Zc = Z0 - sum_k R_ik W[k, b_i];  U = unit(Zc)
            stop when (obj[-2] - obj[-1]) / |obj[-2]| < epsilon on the rounds' last objectives

    Block ``q`` is the cells ``i`` with ``i mod n_blocks == q`` - a fixed stride where the published algorithm draws a random
    order - and ``pen_q = pow((E + 1) / (O + 1), theta)`` is taken from the tables WITHOUT block ``q``, recomputed as a sum of the
    other blocks' tables (``include/wgnn.h``; ``tests/harmony_reference.py`` restates every step).  One 8-byte read-back per
    clustering iteration.  ``theta`` is a scalar or one value per batch.  ``n_clusters`` defaults to ``min(round(B / 30), 100)``.
    With ``n_batches == 1`` the correction is zero by algebra: ``f64(x)`` is returned unchanged, without iterating.

    A row that holds a non-finite value or has a zero norm raises ``ValueError`` naming how many; so does a batch id outside
    ``[0, n_batches)``.  A centre of zero norm, or an objective that is no finite number, raises ``WgnnError``.  Argument errors
    are ``ValueError``; CPU tensors raise ``WgnnError``.  Returns a ``HarmonyRows``."""
    import numpy as np
    name = "harmony_rows"
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"{name}: x must be a 2-D float32 tensor")
    B, D = int(x.shape[0]), int(x.shape[1])
    S = int(n_batches)
    K = harmony_default_clusters(B) if n_clusters is None else int(n_clusters)
    if B < 1:
        raise ValueError(f"{name}: x holds no row")
    if not 1 <= -(-D // 4) * 4 <= KNN_MAX_D:
        raise ValueError(f"{name}: D = {D} is outside [1, {KNN_MAX_D}]")
    if not 1 <= K <= HARMONY_MAX_K:
        raise ValueError(f"{name}: n_clusters = {K} is outside [1, {HARMONY_MAX_K}]")
    if K > B:
        raise ValueError(f"{name}: n_clusters = {K}, but there are only {B} rows")
    if not 1 <= S <= HARMONY_MAX_BATCHES:
        raise ValueError(f"{name}: n_batches = {S} is outside [1, {HARMONY_MAX_BATCHES}]")
    if not 1 <= int(n_blocks) <= HARMONY_MAX_BLOCKS:
        raise ValueError(f"{name}: n_blocks = {n_blocks} is outside [1, {HARMONY_MAX_BLOCKS}]")
    n_blocks = int(n_blocks)
    th = np.asarray(theta, np.float64)
    if th.ndim > 1 or (th.ndim == 1 and th.shape[0] != S) or not np.all(np.isfinite(th)) or np.any(th < 0):
        raise ValueError(f"{name}: theta must be a finite scalar >= 0 or one such value per batch ([{S}])")
    th = np.ascontiguousarray(np.broadcast_to(th, (S,)))
    for what, v in (("sigma", sigma), ("lamb", lamb)):
        if not (float(v) > 0 and math.isfinite(float(v))):
            raise ValueError(f"{name}: {what} = {v} must be positive and finite")
    for what, v in (("epsilon_cluster", epsilon_cluster), ("epsilon", epsilon)):
        if not float(v) >= 0:
            raise ValueError(f"{name}: {what} = {v} must be >= 0")
    if int(max_iter) < 1 or int(max_iter_cluster) < 1:
        raise ValueError(f"{name}: max_iter and max_iter_cluster must be >= 1")
    if not isinstance(batch, torch.Tensor) or batch.dtype not in (torch.int32, torch.int64) or tuple(batch.shape) != (B,):
        raise ValueError(f"{name}: batch must hold one int32 / int64 id per row ([{B}])")
    dev = _require_cuda(x, batch)
    lo, hi = torch.aminmax(batch)
    if int(lo) < 0 or int(hi) >= S:
        raise ValueError(f"{name}: batch id out of range [0, {S}) (min {int(lo)}, max {int(hi)})")
    n_bad = int((~torch.isfinite(x).all(dim=1)).sum())
    if n_bad:
        raise ValueError(f"{name}: {n_bad} of the {B} rows hold a non-finite value")
    Z0 = x.to(torch.float64).contiguous()
    if S == 1:
        return HarmonyRows(Z0, None, None, None, None, [], [], [], 0, True)
    _, U = harmony_apply(Z0)
    n_zero = int((~torch.isfinite(U).all(dim=1)).sum())
    if n_zero:
        raise ValueError(f"{name}: {n_zero} of the {B} rows have a zero norm")
    batch = batch.to(torch.int32).contiguous()
    theta_d, sigma, lamb = torch.as_tensor(th, device=dev), float(sigma), float(lamb)
    Pr = (torch.bincount(batch.long(), minlength=S).to(torch.float64) / float(B)).contiguous()
    _, Y = harmony_apply(kmeans_rows(U.to(torch.float32), K, seed=seed, max_iter=25).centers.to(torch.float64).contiguous())
    if not bool(torch.isfinite(Y).all()):
        raise WgnnError(f"{name}: a seeded centre has a zero norm")
    R = torch.empty((B, K), dtype=torch.float64, device=dev)
    T = torch.zeros((n_blocks, K, S), dtype=torch.float64, device=dev)
    tables = tuple(torch.empty((K, S), dtype=torch.float64, device=dev) for _ in range(3))       # O, E, pen
    M1, n1 = torch.empty((K, 1, D), dtype=torch.float64, device=dev), torch.empty((K, 1), dtype=torch.float64, device=dev)
    MS, nS = torch.empty((K, S, D), dtype=torch.float64, device=dev), torch.empty((K, S), dtype=torch.float64, device=dev)
    Zc, obj = torch.empty_like(Z0), torch.empty(4, dtype=torch.float64, device=dev)
    all_rows = (torch.arange(B, dtype=torch.int32, device=dev), torch.tensor([0, B], dtype=torch.int64, device=dev))
    by_batch = _group_major(batch, S)
    trace: list = []

    def sweep(e, first):
        ws = None
        if not first:
            harmony_fold(T, Pr, theta_d, B, q_skip=0, out=tables)
        for q in range(n_blocks):
            ws = harmony_assign_block(e, batch, S, n_blocks, q, R, pen=None if first else tables[2], workspace=ws)
            last = q + 1 == n_blocks
            harmony_fold(T, Pr, theta_d, B, q_store=q, q_skip=-1 if last or first else q + 1, workspace=ws, out=tables)

    def cluster_step(first=False):
        _, dist, e = harmony_scores(U, Y, sigma)
        sweep(e, first)
        value = float(harmony_objective(R, dist, batch, tables[0], tables[1], theta_d, sigma, out=obj)[0])
        if not math.isfinite(value):
            raise WgnnError(f"{name}: the objective is {value}: a centre of zero norm or a cluster without weight")
        trace.append(value)

    cluster_step(first=True)
    outer, inner, converged = [trace[-1]], [], False
    for _ in range(int(max_iter)):
        for it in range(1, int(max_iter_cluster) + 1):
            weighted_group_reduce(U, R, None, 1, out=(M1, n1), major=all_rows)
            harmony_apply(M1.view(K, D), out=(M1.view(K, D), Y))
            cluster_step()
            if it >= 4:
                old, new = sum(trace[-4:-1]), sum(trace[-3:])
                if (old - new) / abs(old) < float(epsilon_cluster):
                    break
        inner.append(it)
        outer.append(trace[-1])
        weighted_group_reduce(Z0, R, None, S, out=(MS, nS), major=by_batch)
        harmony_apply(Z0, R, harmony_ridge(MS, nS, lamb).contiguous(), batch, out=(Zc, U))
        if (outer[-2] - outer[-1]) / abs(outer[-2]) < float(epsilon):
            converged = True
            break
    return HarmonyRows(Zc, R, Y, tables[0], tables[1], outer, trace, inner, len(inner), converged)
