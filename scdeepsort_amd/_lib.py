"""ctypes binding of the C ABI declared in ``include/wgnn.h``.

The product path has NO CPU fallback: if ``libwgnn_hip.so`` is missing the
import of :func:`lib` raises, and every wrapper raises on a non-zero return.
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from pathlib import Path

LIB_PATH = Path(__file__).resolve().parent / "libwgnn_hip.so"

# error codes / enums (mirror include/wgnn.h)
SRC_IS_GENE, DST_IS_GENE, NO_ALPHA = 0, 1, 2
F32, F16 = 0, 1
PLAN_TALL = 1 << 16                # tile-plan geometry bit OR-ed into `block_rows` (include/wgnn.h WGNN_PLAN_TALL, 0.2.4)
FLAG_RELU, FLAG_NO_MEAN, FLAG_NO_SELF, FLAG_SELF_COMPACT, FLAG_ROWPTR_I64, FLAG_SRC_PRESCALED, FLAG_OUT_SCALE_ALPHA = 1, 2, 4, 8, 16, 32, 64
ATTRIB_ACCUMULATE, ATTRIB_EXPLICIT_SELF = 256, 512     # wgnn_attrib_rows' own flag bits (include/wgnn.h)
MARKERS_ACCUMULATE = 256           # wgnn_group_gene_reduce's flag bit (include/wgnn.h)
CLUSTERS_ACCUMULATE = 256          # wgnn_group_class_reduce's flag bit (include/wgnn.h)
STABILITY_ACCUMULATE = 256         # wgnn_predict_rows_dropout's flag bit (include/wgnn.h)
THIN_ACCUMULATE = 256              # wgnn_predict_rows_thin's flag bit (include/wgnn.h)
ALIGN_BAD_COL, ALIGN_BAD_MAP, ALIGN_BAD_ROWPTR, ALIGN_BAD_VALUE = 1, 2, 4, 8     # wgnn_align_*'s status bits (include/wgnn.h)
PAIR_BAD_INDEX, PAIR_UNSORTED, PAIR_BAD_ROWPTR = 1, 2, 4     # wgnn_pair_rows_*'s status bits (include/wgnn.h)
POOL_BAD_INDEX, POOL_BAD_ROWPTR, POOL_BAD_COL = 1, 2, 4     # wgnn_pool_rows_*'s status bits (include/wgnn.h)
POOL_MAX_CELLS_PER_UNIT, POOL_MAX_SLAB_GENES = 256, 16384    # wgnn_pool_rows_accumulate's unit geometry limits (include/wgnn.h)
SOUP_BAD_ROWPTR, SOUP_BAD_COL, SOUP_BAD_ADD = 1, 2, 4     # wgnn_soup_rows_*'s status bits (include/wgnn.h)
SOUP_MAX_SLAB_GENES = 16384        # wgnn_soup_rows_*'s widest LDS slab (include/wgnn.h)
HOOD_BAD_INDEX, HOOD_BAD_ROWPTR, HOOD_BAD_COL, HOOD_BAD_SIZE = 1, 2, 4, 8     # wgnn_hood_rows_*'s status bits (include/wgnn.h)
HOOD_MAX_MEMBERS, HOOD_MAX_SLAB_GENES = 256, 16384     # wgnn_hood_rows_*'s largest unit and widest LDS slab (include/wgnn.h)
KNN_MAX_K, KNN_MAX_D, KNN_MAX_SPLITS = 64, 1024, 64    # wgnn_knn_rows' limits (include/wgnn.h)
KNN_SEGMENTS_MAX_SEGS, KNN_SEGMENTS_MAX_LIST, KNN_SEGMENTS_BAD_ORDER = 64, 64, 1     # wgnn_knn_segments' limits and status bit (include/wgnn.h)
KMEANS_MAX_K = 4096                # wgnn_kmeans_seed's limit (include/wgnn.h); its D limits are wgnn_knn_rows'
SILHOUETTE_MAX_GROUPS, SILHOUETTE_MAX_SPLITS = 4096, 64      # wgnn_silhouette_rows' limits (include/wgnn.h); D as wgnn_knn_rows
SNN_MAX_K, SNN_IDX_I64 = 64, 256   # wgnn_snn_weights' limit and flag (include/wgnn.h)
LOUVAIN_UNSORTED, LOUVAIN_BAD_COL, LOUVAIN_BAD_ROWPTR, LOUVAIN_NO_SCRATCH, LOUVAIN_BAD_LABEL, LOUVAIN_BAD_WEIGHT = 1, 2, 4, 8, 16, 32
LEIDEN_BAD_PARTITION = 64          # the bit the wgnn_leiden_* entries add to the WGNN_LOUVAIN_* status bits (include/wgnn.h)
LOUVAIN_WAVE_ROWS, LOUVAIN_BLOCK_ROWS, LOUVAIN_SCRATCH_BLOCKS = 128, 2048, 256      # wgnn_louvain_sweep's largest routes (include/wgnn.h)
FUZZY_MAX_K, FUZZY_IDX_I64 = 64, 256       # wgnn_fuzzy_rows' / wgnn_fuzzy_union's limit and flag (include/wgnn.h)
LAYOUT_LANES, LAYOUT_MAX_EPOCHS, LAYOUT_MAX_NEG = 16, 10000, 64      # wgnn_layout_epoch's sum order and limits (include/wgnn.h)
GEODESIC_UNSORTED, GEODESIC_BAD_COL, GEODESIC_BAD_ROWPTR, GEODESIC_BAD_LENGTH = 1, 2, 4, 8      # wgnn_geodesic_round's status bits
GEODESIC_LANES, GEODESIC_MAX_BLOCKS = 16, 8192     # wgnn_geodesic_round's lanes per row and largest grid (include/wgnn.h)
DIFFUSION_UNSORTED, DIFFUSION_BAD_COL, DIFFUSION_BAD_ROWPTR, DIFFUSION_BAD_WEIGHT = 1, 2, 4, 8    # the wgnn_diffusion_* / wgnn_lanczos_apply status bits
DIFFUSION_LANES, DIFFUSION_MAX_BLOCKS, DIFFUSION_MAX_COMPS = 16, 8192, 64      # the row sum's lanes, the largest grid, the most components
LANCZOS_CHUNK, LANCZOS_MAX_STEPS, LANCZOS_NORM, LANCZOS_BREAKDOWN = 256, 1024, 256, 2.0 ** -26    # wgnn_lanczos_*'s dot order, limit, flag and halt bound
HARMONY_MAX_K, HARMONY_MAX_BATCHES, HARMONY_MAX_D, HARMONY_MAX_BLOCKS = 256, 64, 1024, 64      # the wgnn_harmony_* limits (include/wgnn.h)
HARMONY_T_CHUNK, HARMONY_W_CHUNK, HARMONY_OBJ_CHUNK = 64, 256, 256     # ... and the chunks that are part of their sums' orders
ABI_MAJOR = 2              # include/wgnn.h WGNN_VERSION / 100
ABI_MIN = 206                      # 0.2.1: shared-pair marks in tile-plan entries; 0.2.2: WGNN_FLAG_OUT_SCALE_ALPHA (gnn.GNN sets it); 0.2.3: fused training glue; 0.2.5: even-padded plan segments

_vp, _i32, _i64, _u32, _int = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_int

SIGNATURES = {
    "wgnn_version": (C.c_int, []),
    "wgnn_last_error_string": (C.c_char_p, [C.c_int]),
    "wgnn_agg_workspace_bytes": (C.c_int, [_i64, _i64, _i32, _int, _int, _vp, _vp]),
    "wgnn_plan_build_host": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "wgnn_plan_build_host_i64": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "wgnn_agg_fwd": (C.c_int, [_vp, _vp, _vp, _vp, _int, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                               _vp, _i64, _vp, _i64, _i32, _int, _int, _u32,
                               _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "wgnn_agg_fwd_tiled": (C.c_int, [_vp, _vp, _int, _i32, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp,
                                     _vp, _i64, _vp, _i64, _i32, _u32, _vp, _vp, _i32, _i32, _vp, _vp, _i64,
                                     _vp, _i64, _vp, _i64, _vp]),
    "wgnn_agg_bwd_src_tiled": (C.c_int, [_vp, _int, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _int, _i64, _i32,
                                         _vp, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "wgnn_agg_bwd_alpha_tiled": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i32,
                                           _vp, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "wgnn_agg_bwd_src": (C.c_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _i64, _vp, _i64,
                                   _vp, _i64, _vp, _int, _i64, _i32,
                                   _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "wgnn_agg_bwd_alpha": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp,
                                     _i64, _i32, _u32, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "wgnn_normalize_rows": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "wgnn_normalize_rows_i64": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "wgnn_sample_rows": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, C.c_uint64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wgnn_linear_fwd": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _u32, _vp]),
    "wgnn_linear_fwd_ex": (C.c_int, [_vp, _int, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _u32, _vp]),
    # additive exports (the version stays 206): the two-operand loader of the same GEMM and its row coefficients
    "wgnn_linear_mix_fwd": (C.c_int, [_vp, _i64, _vp, _vp, _int, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64,
                                      _i64, _i32, _i32, _u32, _vp]),
    "wgnn_mix_coeffs": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i64, _vp]),
    "wgnn_linear_wgrad_workspace": (C.c_int, [_i64, _i32, _i32, _vp, _vp]),
    "wgnn_linear_wgrad": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _int, _vp, _i64, _vp]),
    "wgnn_agg_bwd_prepare_workspace": (C.c_int, [_i64, _i32, _vp]),
    "wgnn_agg_bwd_prepare": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _int, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp,
                                       _i64, _i32, _vp, _i64, _vp]),
    "wgnn_ce_sum_workspace": (C.c_int, [_i64, _vp]),
    "wgnn_ce_sum_fwd_bwd": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _vp]),
    "wgnn_tile_plan_count": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "wgnn_csr_transpose_workspace": (C.c_int, [_i64, _i32, _vp, _vp]),
    "wgnn_csr_transpose_count": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i64, _vp, _vp, _vp]),
    "wgnn_csr_transpose_fill": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _vp]),
    "wgnn_tile_plan_fill": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "wgnn_agg_linear_relu_fwd": (C.c_int, [_vp, _vp, _vp, _vp, _int, _i32, _vp, _i64, _vp, _i64, _vp, _vp,
                                           _i64, _i32, _u32, _vp, _i64, _vp, _i64, _vp, _i64, _vp,
                                           _vp, _i64, _vp, _i32, _u32, _vp, _i64, _vp]),
    # additive export (the version stays 206): looked up by name like every other entry
    "wgnn_predict_rows": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _i64,
                                    _vp, _vp, _i32, C.c_float, _vp, _i64, _vp, _vp, _u32, _vp]),
    "wgnn_attrib_rows": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64,
                                   _vp, _vp, _i32, _vp, C.c_float, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _u32, _vp]),
    "wgnn_rows_topk": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _u32, _vp]),
    "wgnn_group_gene_reduce_workspace": (C.c_int, [_i64, _i64, _i32, _i32, _vp]),
    "wgnn_group_gene_reduce": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _u32, _vp]),
    "wgnn_group_class_reduce_workspace": (C.c_int, [_i64, _i32, _i32, _vp]),
    "wgnn_group_class_reduce": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _u32, _vp]),
    "wgnn_predict_rows_dropout": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64,
                                            _i32, _i64, _i32, C.c_uint64, C.c_double, _vp, _i64,
                                            _vp, _vp, _i32, C.c_float, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_predict_rows_thin": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64,
                                         _vp, C.c_double, C.c_float,
                                         _i32, _i64, _i32, C.c_uint64, C.c_double, _vp, _i64,
                                         _vp, _vp, _i32, C.c_float, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_predict_rows_panels": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64,
                                           _vp, _i32, _vp, _i64, C.c_double, C.c_float, _vp, _i64,
                                           _vp, _vp, _i32, C.c_float, _vp, _i64, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_align_count": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _i32, C.c_float, _vp, _vp, _u32, _vp]),
    "wgnn_align_fill": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _i32, C.c_float, _vp, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_align_count_ln": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _i32, C.c_float, _vp, _vp, C.c_double, _vp, _vp,
                                      _u32, _vp]),
    "wgnn_align_fill_ln": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _i32, C.c_float, _vp, C.c_double, _vp, _vp, _vp, _vp,
                                     _u32, _vp]),
    "wgnn_align_count_ln_merge": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _i32, C.c_float, _vp, _vp, _vp, _i32, _i32,
                                            _vp, _vp, C.c_double, _vp, _vp, _u32, _vp]),
    "wgnn_align_fill_ln_merge": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _i32, C.c_float, _vp, _vp, _vp, _i32, _i32,
                                           _vp, C.c_double, _vp, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_coverage_rows": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_pair_rows_count": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, C.c_double, C.c_float, _vp, _vp, _u32, _vp]),
    "wgnn_pair_rows_fill": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, C.c_double, C.c_float, _vp, _vp, _vp, _vp,
                                      _u32, _vp]),
    "wgnn_pool_rows_accumulate": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _i32, _vp, _u32, _vp]),
    "wgnn_pool_rows_count": (C.c_int, [_vp, _i64, _vp, _i64, _i32, C.c_double, C.c_float, _vp, _vp, _vp]),
    "wgnn_pool_rows_fill": (C.c_int, [_vp, _i64, _vp, _i64, _i32, C.c_double, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wgnn_soup_rows_count": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _i64, _i32, C.c_uint64, C.c_double,
                                       C.c_float, _i32, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_soup_rows_fill": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _i64, _i32, C.c_uint64, C.c_double,
                                      C.c_float, _i32, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_hood_rows_count": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _i32, C.c_double, C.c_float, _i32,
                                       _vp, _vp, _u32, _vp]),
    "wgnn_hood_rows_fill": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _i32, C.c_double, C.c_float, _i32,
                                      _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_rank_sets_rows": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp, _i64, _vp, _i64, _u32, _vp]),
    "wgnn_rank_genes_groups_workspace": (C.c_int, [_i64, _i64, _i32, _i32, _vp]),
    "wgnn_rank_genes_groups": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _u32, _vp]),
    "wgnn_knn_workspace_bytes": (C.c_int, [_i64, _i64, _i32, _i32, _vp]),
    "wgnn_knn_rows": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _u32, _vp]),
    "wgnn_knn_segments_workspace_bytes": (C.c_int, [_i64, _i64, _i32, _i32, _i32, _vp]),
    "wgnn_knn_segments": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _vp, _i32, _i32, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _i64,
                                    _vp, _vp, _i64, _u32, _vp]),
    "wgnn_kmeans_seed_workspace_bytes": (C.c_int, [_i64, _i32, _vp]),
    "wgnn_kmeans_seed": (C.c_int, [_vp, _i64, _i64, _i32, _i32, C.c_uint64, _vp, _vp, _vp, _i64, _u32, _vp]),
    "wgnn_group_rows_reduce_workspace": (C.c_int, [_i64, _i32, _i32, _vp]),
    "wgnn_group_rows_reduce": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _u32, _vp]),
    "wgnn_silhouette_workspace_bytes": (C.c_int, [_i64, _i32, _i32, _vp]),
    "wgnn_silhouette_rows": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _u32, _vp]),
    "wgnn_snn_weights": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _u32, _vp]),
    "wgnn_louvain_sweep_workspace_bytes": (C.c_int, [_i64, _i32, _vp]),
    "wgnn_louvain_sweep": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i32, _i32, _i32,
                                     _vp, _vp, _vp, _vp, _i64, _i32, _u32, _vp]),
    "wgnn_louvain_apply": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_louvain_modularity": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_leiden_boundary": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_leiden_refine_sweep": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i32,
                                           _i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _u32, _vp]),
    "wgnn_leiden_accept": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_fuzzy_rows": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i32, C.c_double, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_fuzzy_union": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _u32, _vp]),
    "wgnn_layout_init": (C.c_int, [_vp, _i64, _u32, _u32, _vp]),
    "wgnn_layout_epoch": (C.c_int, [_vp, _vp, _vp, _i64, _i64, C.c_float, _vp, _vp, _i32, _i32, C.c_float, C.c_float, C.c_float,
                                    C.c_float, _i32, _u32, _vp, _u32, _vp]),
    "wgnn_geodesic_round": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _u32, _vp]),
    "wgnn_diffusion_degree": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i32, _u32, _vp]),
    "wgnn_diffusion_weights": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _u32, _vp]),
    "wgnn_lanczos_init": (C.c_int, [_vp, _vp, _i64, _u32, _vp, _vp, _u32, _vp]),
    "wgnn_lanczos_apply": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _u32, _vp]),
    "wgnn_lanczos_dots_workspace_bytes": (_i64, [_i64, _i32]),
    "wgnn_lanczos_dots": (C.c_int, [_vp, _i64, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _u32, _vp]),
    "wgnn_lanczos_update": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _i64, _vp, _i32, _u32, _vp]),
    "wgnn_lanczos_scale": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _i32, _u32, _vp]),
    "wgnn_basis_combine": (C.c_int, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64, _i64, _u32, _vp]),
    "wgnn_diffusion_distance": (C.c_int, [_vp, _i64, _i64, _vp, _i32, _vp, _i32, _vp, _u32, _vp]),
    "wgnn_harmony_scores": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, C.c_double, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_harmony_assign_workspace_bytes": (C.c_int, [_i64, _i32, _i32, _i32, _vp]),
    "wgnn_harmony_assign_block": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _i64, _i32, _u32, _vp]),
    "wgnn_harmony_fold": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _u32, _vp]),
    "wgnn_weighted_group_reduce_workspace_bytes": (C.c_int, [_i64, _i32, _i32, _i32, _vp]),
    "wgnn_weighted_group_reduce": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _i32, _u32, _vp]),
    "wgnn_harmony_objective_workspace_bytes": (C.c_int, [_i64, _vp]),
    "wgnn_harmony_objective": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, C.c_double, _vp, _vp, _i64, _u32, _vp]),
    "wgnn_harmony_apply": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _i32, _u32, _vp]),
}


class WgnnError(RuntimeError):
    pass


@lru_cache(maxsize=1)
def lib() -> C.CDLL:
    if not LIB_PATH.exists():
        raise WgnnError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Build it with `python -m scdeepsort_amd.build` or `__graft_entry__.build()`.")
    dll = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(dll, name)          # AttributeError here = header/ABI drift
        fn.restype, fn.argtypes = res, args
    if dll.wgnn_version() // 100 != ABI_MAJOR or dll.wgnn_version() < ABI_MIN:
        raise WgnnError(f"{LIB_PATH} speaks ABI {dll.wgnn_version()}, this binding needs major version {ABI_MAJOR}, "
                        f"at least {ABI_MIN}: rebuild it")
    return dll


def call(device, name: str, *args) -> int:
    """Invoke a kernel-launching entry point with ``device`` current: the library launches on the stream it is given and
    keeps per-device kernel attributes keyed by hipGetDevice(), so the caller's current device must be the one that owns
    the tensors / stream (matters as soon as a process drives more than one GPU or gpu_id != 0)."""
    import torch
    with torch.cuda.device(device):
        return getattr(lib(), name)(*args)


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().wgnn_last_error_string(rc).decode()
        raise WgnnError(f"{what} failed: {msg} (code {rc})")


def run(device, name: str, *args) -> None:
    """``call`` then ``check``: the entry is named once."""
    check(call(device, name, *args), name)
