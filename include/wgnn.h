/*
 * wgnn.h - C ABI of the MI355X (gfx950) weighted-GNN aggregation library
 *          (libwgnn_hip.so, built from scdeepsort_amd/csrc/).
 *
 * This is the drop-in boundary for scDeepSort's hot path.  The reference has no
 * FFI of its own; the operator boundary it replaces is the Python call
 *
 *     nf.block_compute(i, self.message_func, fn.mean('m', 'neigh'), layer)
 *                                                  (reference models/gnn.py:65)
 *
 * i.e. per-edge message  m_e = h[src]*alpha[k(e)]*w_e   (models/gnn.py:47-56),
 * mean over in-edges incl. the self-loop  [DGL 0.4.3 fn.mean], then
 * NodeUpdate = Linear + ReLU  (models/gnn.py:18-25), plus autograd's backward of
 * the same (train.py:84) and the graph-operand normalisation
 * normalize_weight (utils/preprocess_internal.py:15-23).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory unless the
 *     parameter name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - functions enqueue work on `stream` and return immediately: they never
 *     synchronise, never allocate persistent memory, never throw; they are
 *     re-entrant across streams, threads and devices (scratch is passed in by
 *     the caller; the only library state - "dynamic-LDS limit already raised"
 *     marks - is kept per device in atomics).  The CURRENT device
 *     (hipGetDevice) must be the one that owns `stream` and the pointers;
 *   - return value: 0 = ok, negative = WGNN_ERR_* (see wgnn_last_error_string);
 *   - CSR is destination-major: row r lists the in-edges of destination r,
 *     `col` = source index, `val` = normalised edge weight.  Self-loops are
 *     IMPLICIT (weight 1, added by the kernels), matching the reference's
 *     "normalise, then add self-loops" order (preprocess_internal.py:211-214).
 *   - feature matrices are row-major with a leading dimension in ELEMENTS;
 *     D and every ld must be multiples of 4 (16-byte rows for f32).
 */
#ifndef WGNN_H_
#define WGNN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WGNN_VERSION 206           /* 0.2.x - INCOMPATIBLE with 0.1.x binders: `neigh_sum` was inserted before `n_out` in
                                      wgnn_agg_fwd / wgnn_agg_fwd_tiled (0.1.1, should have been a major bump then - a 0.1.0
                                      caller would pass n_out in a pointer slot); 0.2.0 adds int64 row pointers
                                      (WGNN_FLAG_ROWPTR_I64, wgnn_normalize_rows_i64), WGNN_FLAG_SRC_PRESCALED and
                                      wgnn_linear_fwd_ex.  Binders must check wgnn_version() / 100 == 2.
                                      0.2.1: tile-plan entries may mark shared pairs (see wgnn_agg_fwd_tiled); a 0.2.0
                                      library would misread the marks, so a plan that carries them needs >= 201.
                                      0.2.2: WGNN_FLAG_OUT_SCALE_ALPHA (an older library ignores the bit: callers that set it
                                      need >= 202).  0.2.3: wgnn_agg_bwd_prepare, wgnn_ce_sum_fwd_bwd; wgnn_agg_bwd_src_tiled
                                      takes col_scale == NULL (pre-scaled gradient rows).  0.2.4: WGNN_PLAN_TALL (tall tile
                                      plans: 8 waves x 49 rows),
                                      wgnn_tile_plan_count / wgnn_tile_plan_fill.  0.2.5: a tile-plan segment with an odd number
                                      of entries is ALWAYS padded to even (0.2.4: only when shared pairs follow), so its size
                                      depends on its entry count alone: wgnn_tile_plan_count no longer reports pair counts
                                      (`seg_pairs` is ignored, may be NULL) and wgnn_tile_plan_fill takes the padded offsets;
                                      the aggregation kernels read either layout.  0.2.6: wgnn_csr_transpose_* (additive). */

/* Tile-plan geometry, OR-ed into the `block_rows` argument of wgnn_agg_fwd_tiled / wgnn_agg_bwd_src_tiled /
 * wgnn_agg_bwd_alpha_tiled (0.2.4; an older library rejects the bit with WGNN_ERR_PLAN): the plan was built for the TALL tile -
 * 8 waves x 49 destination rows = 392 item slots per tile, seg_ptr with 8 segments per (tile, block), 6-bit slot fields in the
 * entries - instead of 16 waves x 16 rows = 256 item slots, 16 segments, 4-bit slots. */
#define WGNN_PLAN_TALL (1 << 16)

/* error codes */
#define WGNN_OK                 0
#define WGNN_ERR_BAD_ARG       -1  /* NULL pointer / negative size / bad enum             */
#define WGNN_ERR_ALIGNMENT     -2  /* D or ld not a multiple of 4, or pointer not 16-B aligned */
#define WGNN_ERR_UNSUPPORTED   -3  /* dtype / width combination not built                  */
#define WGNN_ERR_WORKSPACE     -4  /* workspace too small                                  */
#define WGNN_ERR_LAUNCH        -5  /* hipLaunch / hipMemsetAsync failed                    */
#define WGNN_ERR_PLAN          -6  /* plan blob malformed or built for another CSR         */

/* which end of an edge is the gene (selects the alpha index rule, gnn.py:49-53) */
#define WGNN_SRC_IS_GENE  0   /* gene->cell edges: k(e) = source gene id   (gnn.py:51); rows are cells  */
#define WGNN_DST_IS_GENE  1   /* cell->gene edges: k(e) = dest   gene id   (gnn.py:52); rows are genes  */
#define WGNN_NO_ALPHA     2   /* plain weighted sum (cell-feature build, preprocess_internal.py:197-199;
                                 multi-GPU partial sums)                                                 */

/* element types of feature matrices */
#define WGNN_F32 0
#define WGNN_F16 1            /* storage only; accumulation is always fp32 */

/* flags for wgnn_agg_fwd */
#define WGNN_FLAG_RELU     1u   /* out = max(out, 0) after bias (NodeUpdate activation, gnn.py:21-22)      */
#define WGNN_FLAG_NO_MEAN  2u   /* skip the 1/(deg+1) division (partial sums that are all-reduced first)  */
#define WGNN_FLAG_NO_SELF  4u   /* skip the self-loop term                                                */
#define WGNN_FLAG_SELF_COMPACT 8u /* h_self holds one row per OUTPUT SLOT (h_self[i]) instead of per CSR row (h_self[r]);
                                     used with row_ids for seed mini-batches (train.py:71-81)                */
#define WGNN_FLAG_ROWPTR_I64 16u  /* `rowptr` points to int64_t[R+1] (scipy / torch CSR of large matrices) instead of int32_t[R+1].
                                     SURVEY 8b: "rowptr[R+1] i32 or i64".  The kernels read rowptr only for the inv_deg == NULL
                                     fallback (row length); non-zero OFFSETS stay 32-bit (plan items), so an operand still has
                                     < 2^31 non-zeros per GPU (see wgnn_plan_build_host_i64)                    */
#define WGNN_FLAG_SRC_PRESCALED 32u /* wgnn_agg_fwd_tiled, WGNN_SRC_IS_GENE: h_src already holds alpha[s]*h[s] (written by
                                     wgnn_linear_fwd_ex's scaled output); no scale pass, src_scratch may be NULL */

#define WGNN_FLAG_OUT_SCALE_ALPHA 64u /* wgnn_agg_fwd / wgnn_agg_fwd_tiled, WGNN_DST_IS_GENE (rows are genes): the finished row
                                     (after mean / self-loop / bias / ReLU) is multiplied by alpha[row] once more, i.e. the
                                     output is the NEXT layer's alpha-folded gene table, (h*alpha) of gnn.py:54, ready for
                                     WGNN_FLAG_SRC_PRESCALED - used when nothing else reads the unscaled gene rows (the
                                     layer below a cells-only last layer).  Forward entries only                */

int         wgnn_version(void);
const char* wgnn_last_error_string(int code);

/* Bytes of caller-provided scratch one aggregation call needs (the library never allocates):
 *   *partials_bytes    = n_partials * D * 4                      (long-row / column-split partial sums)
 *   *src_scratch_bytes = n_src * D * 4 for the tiled kernels that fold a per-row factor into the source table
 *                        (wgnn_agg_fwd_tiled with WGNN_SRC_IS_GENE, wgnn_agg_bwd_src_tiled's g_scratch), else 0. */
int wgnn_agg_workspace_bytes(int64_t n_partials, int64_t n_src, int32_t D, int alpha_mode, int tiled,
                             int64_t* partials_bytes, int64_t* src_scratch_bytes);

/* ---------------------------------------------------------------------------
 * Execution plan: splits long rows into fixed-size chunks so that a hub gene
 * with ~C in-edges does not serialise on one wavefront.  Built once per CSR
 * (host side, from a host copy of rowptr) and uploaded by the caller.
 *
 *   items_host : int32[4 * n_items]  {row_slot, nnz_begin, nnz_end, partial_slot | -1}
 *   long_host  : int32[4 * n_long]   {row_slot, first_partial_slot, n_partials, 0}
 * `row_slot` indexes row_ids (or is the row itself when row_ids == NULL).
 * Call once with items_host == NULL to obtain the counts.
 * ------------------------------------------------------------------------- */
int wgnn_plan_build_host(const int32_t* rowptr_host, const int32_t* row_ids_host, int64_t n_rows,
                         int32_t chunk_nnz,
                         int32_t* items_host, int32_t* long_host,
                         int64_t* n_items, int64_t* n_long, int64_t* n_partials);

/* Same, from a 64-bit row-pointer array (scipy / torch CSR of large matrices).  The kernels address non-zeros with
 * 32-bit offsets (items hold {begin, end} as int32; col/val of 2^31 edges would be 17 GB per direction): when
 * rowptr_host[r+1] > INT32_MAX for any planned row this returns WGNN_ERR_UNSUPPORTED - the caller shards the cell
 * axis (one CSR per GPU / per shard) so that every shard stays below 2^31 non-zeros. */
int wgnn_plan_build_host_i64(const int64_t* rowptr_host, const int32_t* row_ids_host, int64_t n_rows,
                             int32_t chunk_nnz,
                             int32_t* items_host, int32_t* long_host,
                             int64_t* n_items, int64_t* n_long, int64_t* n_partials);

/* ---------------------------------------------------------------------------
 * K1  forward:  replaces message_func + fn.mean (+ optional bias/ReLU epilogue)
 *               (models/gnn.py:47-56,65 and :20-22)
 *
 *   for each output slot i (row r = row_ids ? row_ids[i] : i):
 *     SRC_IS_GENE: out[i] = ( sum_j val_j*alpha[col_j]*h_src[col_j] + alpha[self_idx]*h_self[r] ) * inv_deg[r]
 *     DST_IS_GENE: out[i] = ( alpha[r]*sum_j val_j*h_src[col_j]    + alpha[self_idx]*h_self[r] ) * inv_deg[r]
 *     NO_ALPHA   : out[i] = ( sum_j val_j*h_src[col_j] [+ h_self[r]] ) * inv_deg[r]
 *   then  out[i] += bias (if bias) ; out[i] = relu(out[i]) (if WGNN_FLAG_RELU).
 *   inv_deg == NULL  =>  1/(rowptr[r+1]-rowptr[r]+1)   (in-degree counts the self-loop).
 *   self_idx is gene_num+1 for cell rows and gene_num for gene rows (gnn.py:42,49,53).
 *
 *   items/long_rows come from wgnn_plan_build_host (device copies).  `partials`
 *   must hold n_partials*D floats (may be NULL when n_long == 0).
 *   neigh_sum (optional, f32 [n_out, D] contiguous, NULL to skip): receives sum_j val_j*[alpha[col_j]*]h_src[col_j] per
 *   slot BEFORE the row factor / self-loop / mean / bias / ReLU.  Training saves it for DST_IS_GENE rows: the
 *   gradient of alpha[r] is then inv_deg[r]*<g[r], neigh_sum[r]> - a row dot product instead of a second pass over the
 *   edges (K3).
 * ------------------------------------------------------------------------- */
int wgnn_agg_fwd(const void* rowptr /* int32_t[R+1]; int64_t[R+1] with WGNN_FLAG_ROWPTR_I64 */, const int32_t* col, const float* val,
                 const float* alpha, int alpha_mode, int32_t self_idx,
                 const void* h_src, int64_t ld_src,
                 const void* h_self, int64_t ld_self,
                 const int32_t* row_ids, const float* inv_deg, const float* bias,
                 void* out, int64_t ld_out, float* neigh_sum,
                 int64_t n_out, int32_t D, int dtype_in, int dtype_out, uint32_t flags,
                 const int32_t* items, int64_t n_items,
                 const int32_t* long_rows, int64_t n_long,
                 float* partials, int64_t n_partials,
                 void* stream);

/* ---------------------------------------------------------------------------
 * K1t forward, LDS-streamed variant of K1 (same arithmetic, same outputs) for D <= 256, f32,
 *     h_src contiguous (leading dimension == D).  One 1024-thread workgroup per TILE of up to 256
 *     destination rows (16 waves x 16 rows); the source table is streamed through LDS in blocks of
 *     `block_rows` rows.  The tile plan is a re-ordering of the CSR (built once per graph):
 *
 *   tile_hdr   : int32[n_tiles * 2]        {col_begin, col_end} = source range the tile reduces over
 *   tile_items : int32[n_tiles * 256 * 4]  per tile, wave-major: {row_slot | -1 (padding), -, -, partial_slot | -1};
 *                                          a wave's 16 slots are filled from slot 0.  LOADER WAVES: the leading waves of a tile
 *                                          whose slot 0 is empty own no rows - the kernel makes them issue the tile's whole
 *                                          global->LDS stream while the other waves only compute (a plan that gives every
 *                                          wave rows keeps all 16 waves streaming their share; same results either way)
 *   entries    : int32[n_entries * 2]      {meta, weight (f32 bits)}, grouped by (tile, block, wave) segment;
 *                                          block = (col - col_begin) / block_rows.  meta = dst_slot_in_wave << 8 (bits 8..13) |
 *                                          src_row_in_block (bits 0..7), any order inside a segment, plus optionally
 *                                          SHARED PAIRS: two entries of a segment on the same source row may be marked
 *                                          (bit 31 on both, the first also carrying the second's slot in bits 16..21);
 *                                          the kernel then stages that source row once for both.  Marked pairs must be the
 *                                          LAST entries of their segment and start at an even offset from the segment's
 *                                          begin (pad the unmarked run with a zero-weight copy of its last entry; bit 30
 *                                          marks such a filler for tools, kernels ignore it).  n_entries = nnz + fillers.
 *   seg_ptr    : int32[n_tiles*nblk_max*16 + 1]  entry offsets per (tile, block, wave)
 *   block_rows : source rows per LDS block the plan was built for (16..255; 2*block_rows*D*4 B <= 160 KiB,
 *                at D == 256 minus 4 KiB for the per-wave weight strips, i.e. <= 78)
 *   long_rows / partials as in wgnn_agg_fwd (every row of a column-split plan is a "long row").
 *   src_scratch: float[n_src * D], required for WGNN_SRC_IS_GENE: alpha is folded into the source rows
 *                once ((h*alpha), gnn.py:54) instead of once per edge.
 * ------------------------------------------------------------------------- */
int wgnn_agg_fwd_tiled(const void* rowptr /* int32_t[R+1] | int64_t[R+1] (WGNN_FLAG_ROWPTR_I64) | NULL with inv_deg */, const float* alpha, int alpha_mode, int32_t self_idx,
                       const float* h_src, int64_t n_src, float* src_scratch,
                       const float* h_self, int64_t ld_self,
                       const int32_t* row_ids, const float* inv_deg, const float* bias,
                       float* out, int64_t ld_out, float* neigh_sum, int64_t n_out, int32_t D, uint32_t flags,
                       const int32_t* entries, const int32_t* seg_ptr, int32_t nblk_max, int32_t block_rows,
                       const int32_t* tile_items, const int32_t* tile_hdr, int64_t n_tiles,
                       const int32_t* long_rows, int64_t n_long, float* partials, int64_t n_partials,
                       void* stream);

/* ---------------------------------------------------------------------------
 * K2  backward w.r.t. the source rows (autograd of K1, train.py:84):
 *     runs over the TRANSPOSED structure (row s lists the destinations r that s feeds,
 *     t_val = the same normalised weights re-ordered).
 *
 *     SRC_IS_GENE: T[s] = sum_r t_val*inv_deg[r]*g[r];  dh_src[s] (+)= alpha[s]*T[s];
 *                  dalpha[s] (+)= <h_src[s], T[s]>      (if dalpha && h_src)
 *     DST_IS_GENE: dh_src[s] (+)= sum_r t_val*alpha[r]*inv_deg[r]*g[r]
 *     NO_ALPHA   : dh_src[s] (+)= sum_r t_val*inv_deg[r]*g[r]
 *   `accumulate` != 0 adds into dh_src instead of overwriting.
 *   inv_deg is REQUIRED here (it belongs to the destination rows).
 * ------------------------------------------------------------------------- */
int wgnn_agg_bwd_src(const int32_t* t_rowptr, const int32_t* t_col, const float* t_val,
                     const float* alpha, int alpha_mode,
                     const float* inv_deg_dst,
                     const float* g, int64_t ld_g,
                     const float* h_src, int64_t ld_src,
                     float* dh_src, int64_t ld_dh, float* dalpha, int accumulate,
                     int64_t n_src, int32_t D,
                     const int32_t* items, int64_t n_items,
                     const int32_t* long_rows, int64_t n_long,
                     float* partials, int64_t n_partials,
                     void* stream);

/* ---------------------------------------------------------------------------
 * K3  backward w.r.t. alpha for DST_IS_GENE rows and for the self-loop scalars:
 *     dalpha_row[i]  = inv_deg[r] * < g[i], sum_j val_j*h_src[col_j] >       (DST_IS_GENE only, else untouched)
 *     dself_row[i]   = inv_deg[r] * < g[i], h_self[r] >                      (per-row partial of dalpha[self_idx])
 *   The caller adds dalpha_row into dalpha[r] and sums dself_row into dalpha[self_idx].
 * ------------------------------------------------------------------------- */
int wgnn_agg_bwd_alpha(const int32_t* rowptr, const int32_t* col, const float* val,
                       const float* inv_deg, const int32_t* row_ids,
                       const float* g, int64_t ld_g,
                       const float* h_src, int64_t ld_src,
                       const float* h_self, int64_t ld_self,
                       float* dalpha_row, float* dself_row,
                       int64_t n_out, int32_t D, uint32_t flags,   /* WGNN_FLAG_SELF_COMPACT only */
                       const int32_t* items, int64_t n_items,
                       const int32_t* long_rows, int64_t n_long,
                       float* partials, int64_t n_partials,
                       void* stream);

/* ---------------------------------------------------------------------------
 * K2t / K3t  LDS-streamed variants of K2 / K3 (D <= 256, f32, contiguous rows), same tile-plan layout as K1t.
 *   K2t runs over the tile plan of the TRANSPOSED structure; `col_scale[r]` = inv_deg[r] (x alpha[r] for
 *   WGNN_DST_IS_GENE) is folded into the gradient rows once (g_scratch: float[n_dst*D]); col_scale == NULL (0.2.3): `g`
 *   already carries that factor (written so by wgnn_agg_bwd_prepare) and is read as the source table, no scale pass.
 *   K3t runs over the forward structure's tile plan.
 * ------------------------------------------------------------------------- */
int wgnn_agg_bwd_src_tiled(const float* alpha, int alpha_mode, const float* col_scale,
                           const float* g, int64_t n_dst, float* g_scratch,
                           const float* h_src, int64_t ld_src, float* dh_src, int64_t ld_dh, float* dalpha,
                           int accumulate, int64_t n_src, int32_t D,
                           const int32_t* entries, const int32_t* seg_ptr, int32_t nblk_max, int32_t block_rows,
                           const int32_t* tile_items, const int32_t* tile_hdr, int64_t n_tiles,
                           const int32_t* long_rows, int64_t n_long, float* partials, int64_t n_partials,
                           void* stream);
int wgnn_agg_bwd_alpha_tiled(const float* inv_deg, const float* g, int64_t ld_g,
                             const float* h_src, const float* h_self, int64_t ld_self,
                             float* dalpha_row, float* dself_row, int64_t n_out, int32_t D,
                             const int32_t* entries, const int32_t* seg_ptr, int32_t nblk_max, int32_t block_rows,
                             const int32_t* tile_items, const int32_t* tile_hdr, int64_t n_tiles,
                             const int32_t* long_rows, int64_t n_long, float* partials, int64_t n_partials,
                             void* stream);

/* ---------------------------------------------------------------------------
 * K4  graph-operand normalisation: normalize_weight (preprocess_internal.py:15-23)
 *     val_out[j] = deg_r * val_in[j] / sum_{j in row r} val_in[j]      for rows with >= 1 entry
 *     inv_deg[r] = 1 / (deg_r + 1)                                     (if inv_deg != NULL)
 * ------------------------------------------------------------------------- */
int wgnn_normalize_rows(const int32_t* rowptr, const float* val_in, float* val_out, float* inv_deg,
                        int64_t n_rows, void* stream);
/* the same over a 64-bit row-pointer array ("rowptr[R+1] i32 or i64") */
int wgnn_normalize_rows_i64(const int64_t* rowptr, const float* val_in, float* val_out, float* inv_deg,
                            int64_t n_rows, void* stream);

/* ---------------------------------------------------------------------------
 * K5  seeded neighbour subsampling (train.py:37-40,71-78: NeighborSampler(expand_factor = num_neighbors,
 *     neighbor_type = 'in')): for each of n_rows destination rows (row_ids or 0..n_rows-1) draw min(k, deg + 1) of its
 *     deg + 1 in-edges - the deg CSR entries plus the unit self-loop the reference's graph holds explicitly
 *     (preprocess_internal.py:213-214) - uniformly without replacement.  Output in ELL form (static shapes):
 *       out_col / out_val [n_rows * k] : row i owns [i*k, i*k + out_cnt[i]) (drawn real edges, parent col / val)
 *       out_cnt  [n_rows]              : number of real edges drawn
 *       out_self [n_rows]              : 1.0 where the self-loop was among the draws
 *       out_inv  [n_rows]              : 1 / (number of drawn edges)   - fn.mean's divisor
 *     Random numbers = hash(seed, *step, stream_id, row, draw): `step` is a DEVICE counter the caller advances on the
 *     stream (a captured hipGraph therefore draws a new sample at every replay); no state is read back.  k <= 256.
 *
 * The draw law (pinned bit for bit by tests/sample_reference.py).  All integer arithmetic in uint64 with wrap-around; mix32 is
 * the upper half of the splitmix64 finaliser, as the dropout block below defines it.
 *     K_STEP = 0xD6E8FEB86659FD93,  K_STREAM = 0xA24BAED4963EE407,  K_ROW = 0x9FB21C651E98DF25,  K_DRAW = 0xC2B2AE3D27D4EB4F
 *   For slot s:  r = row_ids ? row_ids[s] : s,  b = rowptr[r],  deg = rowptr[r + 1] - b,  m = deg + 1 candidates: candidate
 *   x < deg is the CSR entry b + x, candidate deg is the self-loop.
 *     m <= k : the chosen list is 0, 1, .., deg.
 *     m >  k : Robert Floyd's algorithm on hashed draws,
 *         base = seed ^ (step[0] * K_STEP) ^ ((uint32)stream_id * K_STREAM) ^ ((uint64)(int64)r * K_ROW)
 *         for i = 0 .. k-1:   j = m - k + i,   h = mix32(base + i * K_DRAW),   t = (h * (j + 1)) >> 32        (t in [0, j])
 *                             x_i = j if t is among x_0 .. x_{i-1}, otherwise t
 *       The key holds the ROW r, not the slot: a row repeated in row_ids gets the same list in every slot.
 *   Output, the x_i != deg in order of i (DRAW order, the self-loop taken out, nothing sorted):
 *     out_col / out_val [s*k + 0 ..) = col[b + x_i] / val[b + x_i], val copied bit for bit;  out_cnt[s] = their number;
 *     out_self[s] = 1.0f iff some x_i == deg, else 0.0f;  out_inv[s] = 1.0f / max(1, out_cnt + out_self) in float32
 *     (a correctly rounded division).  The slots [s*k + out_cnt[s], (s+1)*k) are NOT written.
 *   Pure consequences: out_cnt + out_self == min(k, m); every k-subset of the m candidates is equally likely over the keys;
 *   for an operand whose longest row has L entries, k' = min(k, L + 1) gives the lists of k in every row.
 *   Errors, before any launch: WGNN_ERR_BAD_ARG (a missing operand other than row_ids, n_rows < 0, k <= 0),
 *   WGNN_ERR_UNSUPPORTED (k > 256); n_rows == 0 is WGNN_OK and writes nothing; wgnn_last_error_string names the check.
 *   row_ids is not checked against the operand's row count (the entry is not given it).
 * ------------------------------------------------------------------------- */
int wgnn_sample_rows(const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* row_ids,
                     int64_t n_rows, int32_t k, uint64_t seed, const int64_t* step, int32_t stream_id,
                     int32_t* out_col, float* out_val, int32_t* out_cnt, float* out_self, float* out_inv,
                     void* stream);

/* ---------------------------------------------------------------------------
 * Dense half of a layer on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, an fmaf chain in k order):
 *     out[M, N] = act( x[M, K] . w[N, K]^T + bias[N] )
 * = NodeUpdate.forward's `activation(fc_neigh(neigh))` (models/gnn.py:18-25; w / bias in nn.Linear's layout) and the
 * classifier head `linear(h)` (models/gnn.py:66-67).  flags: WGNN_FLAG_RELU or 0.  K, ld_x, ld_w multiples of 4,
 * x / w 16-byte aligned; M, N arbitrary.  bias may be NULL.  Makes the ABI self-sufficient for one whole layer.
 * ------------------------------------------------------------------------- */
/* Extended form (0.2.0):
 *   x_dtype WGNN_F32 | WGNN_F16: fp16-STORED features (BASELINE cfg5) are widened in registers on their way into LDS - fp16-
 *     rounded inputs, fp32 multiply-accumulate, no fp32 copy of x in HBM (x 8-byte aligned then);
 *   row_scale / out_scaled (both or neither): out_scaled[m, :] = row_scale[m] * out[m, :], written from the same
 *     accumulators.  With row_scale = alpha[0:G] this is the alpha-folded gene table (h*alpha, models/gnn.py:54) that
 *     wgnn_agg_fwd_tiled takes under WGNN_FLAG_SRC_PRESCALED - no separate scale pass.  `out` may be NULL then. */
int wgnn_linear_fwd_ex(const void* x, int x_dtype, int64_t ld_x, const float* w, int64_t ld_w, const float* bias,
                       float* out, int64_t ld_out, const float* row_scale, float* out_scaled, int64_t ld_out_scaled,
                       int64_t M, int32_t N, int32_t K, uint32_t flags, void* stream);
int wgnn_linear_fwd(const float* x, int64_t ld_x, const float* w, int64_t ld_w, const float* bias,
                    float* out, int64_t ld_out, int64_t M, int32_t N, int32_t K, uint32_t flags, void* stream);

/* Two-operand loader (additive exports, WGNN_VERSION stays 206): the same product with its A operand formed on the way into
 * LDS from two row tables and two per-row coefficient vectors, in exactly this order of operations:
 *     a[m, k]  = fmaf(c2[m], x2[m, k], c1[m] * x1[m, k])       (c1 * x1 rounded to fp32 first, then ONE fused multiply-add)
 *     out      = act(a . w^T + bias),   out_scaled[m, :] = row_scale[m] * out[m, :]      (either output may be NULL, as above)
 * No [M, K] intermediate goes through HBM.  It serves layer 1's genes<-cells rows from a cached feature sum S = A_gc . X_c
 * (the aggregation is linear and alpha[r] is a per-DESTINATION factor on that side, so sum_c w_rc (X_c W^T)[c] = (S W^T)[r]):
 *     x1 = S, x2 = X_g, c1[r] = alpha[r] * inv_deg[r], c2[r] = alpha[G] * inv_deg[r]
 * The coefficients are two [M] vectors (not alpha / inv_deg / self_idx folded into the entry: the product then stays a plain
 * function of its operands); wgnn_mix_coeffs writes both in one small launch.
 * x1: fp32, 16-byte aligned; x2: WGNN_F32 (16-byte aligned) or WGNN_F16 (8-byte aligned, widened by the loader that
 * wgnn_linear_fwd_ex uses); K, ld_x1, ld_x2, ld_w multiples of 4; ld_* >= K (inputs) / N (outputs); M, N arbitrary; flags as
 * wgnn_linear_fwd_ex. */
int wgnn_linear_mix_fwd(const float* x1, int64_t ld_x1, const float* c1, const void* x2, int x2_dtype, int64_t ld_x2,
                        const float* c2, const float* w, int64_t ld_w, const float* bias,
                        float* out, int64_t ld_out, const float* row_scale, float* out_scaled, int64_t ld_out_scaled,
                        int64_t M, int32_t N, int32_t K, uint32_t flags, void* stream);
/* c1[i] = alpha[i] * inv_deg[i], c2[i] = alpha[self_idx] * inv_deg[i] for i in [0, n). */
int wgnn_mix_coeffs(const float* alpha, int32_t self_idx, const float* inv_deg, float* c1, float* c2, int64_t n, void* stream);

/* Weight gradient of the same Linear (autograd of fc_neigh / linear, train.py:84):
 *     dW[N, K] (+)= sum_m g[m, N] * x[m, K]
 * The node axis M (1e5 at cfg3) is the reduction: it is cut into n_slabs slabs whose partial [N, K] products are folded in
 * fixed order (deterministic).  Query n_slabs / workspace bytes with wgnn_linear_wgrad_workspace; N, K, ld_g, ld_x
 * multiples of 4. */
int wgnn_linear_wgrad_workspace(int64_t M, int32_t N, int32_t K, int64_t* n_slabs, int64_t* bytes);
int wgnn_linear_wgrad(const float* g, int64_t ld_g, const float* x, int64_t ld_x, float* dW, int64_t ld_dw,
                      int64_t M, int32_t N, int32_t K, int accumulate, float* workspace, int64_t n_slabs, void* stream);

/* ---------------------------------------------------------------------------
 * One reference layer on a block in the reference's literal order (SURVEY 8b's optional "fused variant" - here a COMPOSED
 * entry: two launches through the caller's neigh_scratch, see DESIGN.md section 8 for why the fusion itself does not pay):
 *     neigh = nf.block_compute(i, message_func, fn.mean('m','neigh'))   (models/gnn.py:47-56,65)  = wgnn_agg_fwd (f32)
 *     out   = relu(fc_neigh(neigh))                                      (models/gnn.py:18-25)     = wgnn_linear_fwd
 * Arguments up to n_partials as wgnn_agg_fwd (f32 in/out, no bias, agg_flags without WGNN_FLAG_RELU);
 * neigh_scratch: float[n_out * D] (caller-owned); W: float[H, ld_w] (nn.Linear layout), bias: float[H] or NULL;
 * lin_flags: WGNN_FLAG_RELU or 0; out: float[n_out, ld_out].
 * ------------------------------------------------------------------------- */
int wgnn_agg_linear_relu_fwd(const void* rowptr /* as wgnn_agg_fwd */, const int32_t* col, const float* val,
                             const float* alpha, int alpha_mode, int32_t self_idx,
                             const float* h_src, int64_t ld_src, const float* h_self, int64_t ld_self,
                             const int32_t* row_ids, const float* inv_deg,
                             int64_t n_out, int32_t D, uint32_t agg_flags,
                             const int32_t* items, int64_t n_items, const int32_t* long_rows, int64_t n_long,
                             float* partials, int64_t n_partials,
                             float* neigh_scratch,
                             const float* W, int64_t ld_w, const float* bias, int32_t H, uint32_t lin_flags,
                             float* out, int64_t ld_out, void* stream);

/* ---------------------------------------------------------------------------
 * Fused glue of the training step (0.2.3; reference train.py:80-87 through torch autograd).
 *
 * wgnn_agg_bwd_prepare: everything the backward of ONE aggregation pass derives from the upstream gradient, in one read of it
 * (full passes: one gradient row per CSR row, f32):
 *     g             = gout * (out > 0)              out = the saved forward output (NodeUpdate's ReLU, gnn.py:21-22) or NULL
 *     g_scaled[r]   = inv_deg[r] * (alpha[r] for WGNN_DST_IS_GENE) * g[r]      float[n_rows, D]: K2t's source table (col_scale NULL)
 *     dh_self[r]    = alpha[self_idx] * inv_deg[r] * g[r]                       gradient of the self rows (alpha = 1 for WGNN_NO_ALPHA)
 *     dalpha_row[r] = inv_deg[r] * < g[r], neigh_sum[r] >                       neigh_sum: the raw sums K1 saved (float[n_rows, D])
 *     dself_row[r]  = inv_deg[r] * < g[r], h_self[r] >                          the caller sums it into dalpha[self_idx]
 *     dbias[c]      = sum_r g[r, c]                                              block partials in `workspace`, folded in fixed order
 *   Any of g_scaled / dh_self / dalpha_row / dself_row / dbias may be NULL.  inv_deg NULL = 1.  D <= 1024, multiples of 4.
 *   workspace: wgnn_agg_bwd_prepare_workspace floats (needed for dbias only).
 *
 * wgnn_ce_sum_fwd_bwd: CrossEntropyLoss(reduction='sum') (train.py:36) over float logits[n_rows, n_classes] and int64 labels:
 *     *loss_sum = sum_r ( logsumexp(logits[r]) - logits[r, labels[r]] ) ;  dlogits[r] = softmax(logits[r]) - onehot(labels[r])
 *   (dlogits may be NULL).  workspace: wgnn_ce_sum_workspace floats.  Deterministic (fixed-order folds, no atomics).
 *   A label of -100 (torch's default ignore_index) contributes 0 to the loss and a zero dlogits row, as in the framework call
 *   this replaces.  Any other label outside [0, n_classes) - tested on the 64-bit value - is never used as an index: its
 *   row's loss term and dlogits row are NaN (the framework call raises a device-side assertion; a kernel that never
 *   synchronises cannot, NaN is its loud answer).  expf / logf, not the fast intrinsics.
 * ------------------------------------------------------------------------- */
int wgnn_agg_bwd_prepare_workspace(int64_t n_rows, int32_t D, int64_t* floats);
int wgnn_agg_bwd_prepare(const float* gout, int64_t ld_gout, const float* out, int64_t ld_out,
                         const float* inv_deg, const float* alpha, int alpha_mode, int32_t self_idx,
                         float* g_scaled, const float* h_self, int64_t ld_self, float* dh_self, int64_t ld_dh,
                         const float* neigh_sum, float* dalpha_row, float* dself_row, float* dbias,
                         int64_t n_rows, int32_t D, float* workspace, int64_t workspace_floats, void* stream);
int wgnn_ce_sum_workspace(int64_t n_rows, int64_t* floats);
int wgnn_ce_sum_fwd_bwd(const float* logits, int64_t ld_logits, const int64_t* labels, int64_t n_rows, int32_t n_classes,
                        float* loss_sum, float* dlogits, int64_t ld_dlogits, float* workspace, int64_t workspace_floats,
                        void* stream);

/* ---------------------------------------------------------------------------
 * Tile-plan construction on the device (0.2.4, revised 0.2.5).  `entries` / `seg_ptr` of a tile plan (see wgnn_agg_fwd_tiled) from
 * the CSR and the row -> (tile, wave, slot) assignment, without a sort: one wavefront per (tile, wave), lane = destination slot,
 * steps through its <= 64 destination rows (their non-zeros are sorted by column) along the tile's source range.  Two passes:
 *   wgnn_tile_plan_count : seg_total[s] = entries of segment s  (s = (tile * nblk_max + block) * waves + wave; array
 *                          zero-initialised by the caller; every lane counts along its own row, no group walk)
 *   caller               : seg_ptr = exclusive prefix sum of seg_total + (seg_total & 1)   [n_seg + 1 offsets]
 *   wgnn_tile_plan_fill  : entries[seg_ptr[s] .. seg_ptr[s + 1]) = [unshared][pad, iff the count is odd][shared pairs]: the walk in
 *                          lock step (wave minimum of the pending columns -> ballot = the group on that source row) writes the
 *                          unshared entries upwards from the segment's start and the pairs downwards from its end
 *   seg_pairs : ignored since 0.2.5 (may be NULL)
 *   slot_vrow : int32[n_row_tiles * waves * rpw]   virtual row of (row tile, wave, slot) | -1
 *   vrow_*    : per virtual row: CSR row, part j, parts k  (the row's non-zeros j, j + k, j + 2k, ...; k = 1: the whole row)
 *   flat_t    : int32[n_tiles]  row tile of the tile launched at position f;  tile_hdr as in wgnn_agg_fwd_tiled
 *   waves x rpw : 16 x 16 or 8 x 49 (WGNN_PLAN_TALL); block_rows: source rows per LDS block (<= 255)
 * Deterministic, no atomics, no allocation; col / rowptr are int32 (an operand holds < 2^31 non-zeros per GPU).
 * ------------------------------------------------------------------------- */
int wgnn_tile_plan_count(const int32_t* rowptr, const int32_t* col, const int32_t* slot_vrow,
                         const int32_t* vrow_row, const int32_t* vrow_part, const int32_t* vrow_k,
                         const int32_t* flat_t, const int32_t* tile_hdr, int64_t n_tiles, int32_t waves, int32_t rpw,
                         int32_t nblk_max, int32_t block_rows, int32_t* seg_total, int32_t* seg_pairs, void* stream);
int wgnn_tile_plan_fill(const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* slot_vrow,
                        const int32_t* vrow_row, const int32_t* vrow_part, const int32_t* vrow_k,
                        const int32_t* flat_t, const int32_t* tile_hdr, int64_t n_tiles, int32_t waves, int32_t rpw,
                        int32_t nblk_max, int32_t block_rows, const int32_t* seg_total, const int32_t* seg_pairs,
                        const int32_t* seg_ptr, int32_t* entries, void* stream);

/* ---------------------------------------------------------------------------
 * Stable CSR transpose on the device (0.2.6): the gene-major copy of the (cells x genes) expression CSR - every stored value
 * gives a cell->gene AND a gene->cell edge (preprocess_internal.py:170-173), and normalize_weight is per destination (:17-23), so
 * the genes<-cells direction needs the RAW values re-ordered by gene, cells ascending inside a gene - without a sort: an entry's
 * place in its gene's row is the number of earlier cells that express the gene (per-chunk LDS histograms, a prefix over the
 * chunks, then every chunk walks its cells in order).  Deterministic; n_cols <= 32768 (else WGNN_ERR_UNSUPPORTED: the caller
 * sorts).  Precondition: a row lists a column at most once.
 *   wgnn_csr_transpose_workspace : n_chunks and the byte size of `counts` (int32 [n_chunks * n_cols]) for an operand
 *   wgnn_csr_transpose_count     : counts[chunk][col], t_count[col] = entries of column col (rows with row_keep[r] == 0 dropped;
 *                                  row_keep == NULL keeps every row)
 *   caller                       : t_rowptr[0] = 0, t_rowptr[c + 1] = t_rowptr[c] + t_count[c]
 *   wgnn_csr_transpose_fill      : t_col[t_rowptr[c] ..) = the rows that list column c, ascending; t_val their values
 *                                  (overwrites `counts`)
 * ------------------------------------------------------------------------- */
int wgnn_csr_transpose_workspace(int64_t n_rows, int32_t n_cols, int64_t* n_chunks, int64_t* bytes);
int wgnn_csr_transpose_count(const int32_t* rowptr, const int32_t* col, const uint8_t* row_keep, int64_t n_rows, int32_t n_cols,
                             int64_t n_chunks, int32_t* counts, int32_t* t_count, void* stream);
int wgnn_csr_transpose_fill(const int32_t* rowptr, const int32_t* col, const float* val, const uint8_t* row_keep, int64_t n_rows,
                            int32_t n_cols, int64_t n_chunks, int32_t* counts, const int32_t* t_rowptr, int32_t* t_col, float* t_val,
                            void* stream);

/* ---------------------------------------------------------------------------
 * Resident prediction (additive export, WGNN_VERSION stays 206: the binding looks the symbol up by name, and a caller that
 * needs it checks for the symbol, not for a version).  One layer of a trained model over a batch of B TEST cells, against
 * gene-side tables that are constants of the bundle: test cells get gene->cell edges only (reference preprocess.py:184-187)
 * and PCA is fitted on the support cells, so a test cell's output depends on its own expression row alone.  No plan, no
 * graph: one wavefront per cell (grid-stride), deterministic (fixed-order folds, no atomics).
 *
 *   rowptr [B+1] (int32, or int64 with WGNN_FLAG_ROWPTR_I64), col int32 gene ids in [0, n_genes), raw f32: the RAW
 *   (unnormalised) expression values of the batch.  deg = row length, S = sum of the row's raw values:
 *     self_rows == NULL (layer 1):  z = sum_j x_j (alpha[g_j] deg / S + alpha[G+1] / (S + 1e-6)) table[g_j] / (deg + 1) + bias
 *                                   (table = gene_feat . W1^T; the second term is the self-loop on the cell feature
 *                                   rownorm(X) . gene_feat, preprocess.py:201-204, folded through W1)
 *     self_rows != NULL:            z = (sum_j alpha[g_j] deg x_j / S table[g_j] + alpha[G+1] self_rows[c]) / (deg + 1) + bias
 *                                   (table = h_{l-1}[genes] . W_l^T, self_rows = h_{l-1}[cell] . W_l^T)
 *   An empty row has z = bias (+ alpha[G+1] self_rows[c]).  h = ReLU(z).
 *   table [n_genes, ld_table], H valid columns, H % 4 == 0, H <= 256 (else WGNN_ERR_ALIGNMENT / _UNSUPPORTED: the caller
 *   zero-pads other widths); alpha [n_genes + 2]; bias [H].
 *   Without a head (w_head == NULL): out [B, ld_out] = h.
 *   With a head w_head [C, H] (contiguous), b_head [C]; C * H * 4 <= 64 KiB (staged in LDS once per workgroup; else
 *   WGNN_ERR_UNSUPPORTED - run the head as a GEMM):
 *     logits [B, ld_logits] = h . w_head^T + b_head     (may be NULL)
 *     max_prob [B]          = 1 / sum_j exp(logits_j - max_j logits_j)         (softmax maximum, predict.py:78-80)
 *     label [B]             = argmax (lowest index among equal maxima), or -1 when max_prob < unsure_threshold
 *                             (the caller passes float32(unsure_rate / C), the comparison of predict.py:83)
 *   flags: WGNN_FLAG_ROWPTR_I64 or 0.  B < 2^31.  wgnn_last_error_string(code), asked on the same thread right after a failing
 *   call, names the check that failed.
 * ------------------------------------------------------------------------- */
int wgnn_predict_rows(const void* rowptr, const int32_t* col, const float* raw, int64_t n_rows,
                      const float* table, int64_t ld_table, int32_t n_genes, int32_t H,
                      const float* alpha, const float* bias, const float* self_rows, int64_t ld_self,
                      float* out, int64_t ld_out,
                      const float* w_head, const float* b_head, int32_t n_classes, float unsure_threshold,
                      float* logits, int64_t ld_logits, int32_t* label, float* max_prob,
                      uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Per-cell gene attribution on the resident tables (additive exports, WGNN_VERSION stays 206).  For one test cell with the
 * ReLU pattern m_l = (z_l > 0) fixed, the target logit is linear in the cell's per-gene message weights
 *     u_j = x_j (alpha[g_j] deg / S + alpha[G+1] / (S + 1e-6)) / (deg + 1)      self-loop from the row (layer 1)
 *     u_j = alpha[g_j] (deg x_j / S) / (deg + 1)                                explicit-self layers (l >= 2)
 * and splits exactly: logit_t = sum_j phi_j + base, phi_j = sum_l u_{l,j} <T_l[g_j], v_l>, base = bh[t] + sum_l <v_l, b_l>, with
 *     v_L = m_L * Wh[t] ,   v_{l-1} = m_{l-1} * (W_l^T v_l) * alpha[G+1] / (deg + 1)         (the caller's small [B, H] step).
 *
 * wgnn_attrib_rows, one wavefront per cell, deterministic (no atomics, fixed fold order).  rowptr / col / raw / table / alpha /
 * n_genes / H / ld_table as wgnn_predict_rows (H % 4 == 0, H <= 256).  score f32 [nnz], in the CSR order of the batch.
 *   Head mode (w_head != NULL, direction == NULL; the model's last layer): bias, self_rows, w_head [C, H], b_head, C as
 *     wgnn_predict_rows with a head (C * H * 4 <= 64 KiB).  The gather is wgnn_predict_rows' own, operation for operation: the
 *     logits and the arg max carry the bits of that call.  target int32 [B] or NULL (= the arg max, lowest index among equal
 *     maxima, also for a cell wgnn_predict_rows would label -1); the caller checks 0 <= target < C (the kernel clamps).
 *       target_out [B] = t,  logit_out [B] = logit_t,  base_out [B] = b_head[t] + <v, bias>,  score[j] = u_j <table[g_j], v>
 *       dir_out [B, ld_dir_out] = v = (z > 0) * w_head[t]    (may be NULL)
 *       label_out [B] = wgnn_predict_rows' label for unsure_threshold (arg max, or -1; whatever `target` says; may be NULL)
 *     With self_rows the logit also holds alpha[G+1] <self_rows[c], v> / (deg + 1): the share the layers below split further.
 *   Direction mode (w_head == NULL, direction [B, ld_dir] given; layers below the last): score[j] = u_j <table[g_j], direction[c]>,
 *     added to score[j] with WGNN_ATTRIB_ACCUMULATE (a row is owned by one wave).  WGNN_ATTRIB_EXPLICIT_SELF selects the
 *     second coefficient rule.  bias, self_rows, the head and the *_out arrays are ignored.
 *   flags: WGNN_FLAG_ROWPTR_I64 | WGNN_ATTRIB_ACCUMULATE | WGNN_ATTRIB_EXPLICIT_SELF (the last two in direction mode only).
 *
 * wgnn_rows_topk: per row of a CSR with f32 scores the k (1..64) entries with the largest score, descending, equal scores by
 * the lower CSR position: gene_out int32 [B, k] = their col (-1 where the row has fewer than k entries), score_out f32 [B, k]
 * (0 there).  One wavefront per row, deterministic, `score` is only read.  flags: WGNN_FLAG_ROWPTR_I64 or 0.
 * ------------------------------------------------------------------------- */
#define WGNN_ATTRIB_ACCUMULATE 256
#define WGNN_ATTRIB_EXPLICIT_SELF 512
int wgnn_attrib_rows(const void* rowptr, const int32_t* col, const float* raw, int64_t n_rows,
                     const float* table, int64_t ld_table, int32_t n_genes, int32_t H,
                     const float* alpha, const float* bias, const float* self_rows, int64_t ld_self,
                     const float* w_head, const float* b_head, int32_t n_classes, const int32_t* target,
                     float unsure_threshold, int32_t* label_out, const float* direction, int64_t ld_dir,
                     float* score, int32_t* target_out, float* logit_out, float* base_out,
                     float* dir_out, int64_t ld_dir_out, uint32_t flags, void* stream);
int wgnn_rows_topk(const void* rowptr, const int32_t* col, const float* score, int64_t n_rows, int32_t k,
                   int32_t* gene_out, float* score_out, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Per-group gene tables (additive exports, WGNN_VERSION stays 206): the reduction over cells behind
 * api.ResidentPredictor.markers.  For a batch of B cells with one f32 score per stored (cell, gene) entry (wgnn_attrib_rows'
 * `score`) and one group id per cell,
 *     sum   f64   [n_groups, n_genes] : sum[k, g]   = sum over the cells i with group[i] == k that list g of score[i, g]
 *     count int32 [n_groups, n_genes] : count[k, g] = number of those cells
 * wgnn_group_gene_reduce takes the batch GENE-MAJOR: t_rowptr int32 [n_genes + 1], t_cell int32 (the cells that list gene g,
 * ascending, in [0, n_rows)), t_score f32 in the same order - wgnn_csr_transpose_count / _fill with the scores as values (or a
 * stable sort by gene above that kernel's 32 768 columns).  Precondition as there: a cell lists a gene at most once.
 * group int32 [n_rows]: in [0, n_groups), or -1 = the cell takes no part (cells the transpose already dropped may be absent).
 * An entry whose cell id or group id is out of range takes no part either (callers check their operands; never a fault).
 *   One wavefront per gene, per-lane private fp64 / int32 bins in LDS (64 lanes x up to 85 groups per pass, more groups =
 *   more passes over the gene's run), an xor butterfly over the lanes at the end of the run.  f32 terms, fp64 accumulation, no
 *   atomics; the order of a bin's additions depends on the operand alone: two launches are bit-identical.  n_groups <= 2^20, no
 *   limit on n_genes beyond int32.  B = 0 is a valid batch (t_cell / t_score / group may be NULL then).
 *   flags: WGNN_MARKERS_ACCUMULATE - add to what sum / count hold (a cohort streamed in batches); without it EVERY element of
 *   both outputs is written, zeros included (the caller does not pre-clear).
 *   workspace: wgnn_group_gene_reduce_workspace bytes, caller-owned (0 for the present route, whose partial sums never leave
 *   LDS; `workspace` may then be NULL).  Errors: WGNN_ERR_BAD_ARG (NULL sum / count / t_rowptr, n_groups <= 0, n_genes <= 0,
 *   n_rows outside [0, 2^31), unknown flag), WGNN_ERR_UNSUPPORTED, WGNN_ERR_ALIGNMENT, WGNN_ERR_WORKSPACE;
 *   wgnn_last_error_string names the check.
 * ------------------------------------------------------------------------- */
#define WGNN_MARKERS_ACCUMULATE 256
int wgnn_group_gene_reduce_workspace(int64_t n_rows, int64_t nnz, int32_t n_groups, int32_t n_genes, int64_t* bytes);
int wgnn_group_gene_reduce(const int32_t* t_rowptr, const int32_t* t_cell, const float* t_score, const int32_t* group,
                           int64_t n_rows, int32_t n_groups, int32_t n_genes, double* sum, int32_t* count,
                           void* workspace, int64_t workspace_bytes, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Per-group class tables (additive exports, WGNN_VERSION stays 206): the reduction over cells behind
 * api.ResidentPredictor.annotate - one cell type per CLUSTER from what wgnn_predict_rows leaves on the device.  For a batch of
 * B cells with logits f32 [n_rows, ld_logits] (ld_logits >= n_classes = C; columns beyond C are never read), label int32
 * [n_rows] (wgnn_predict_rows' label: a class id, or -1 = unsure) and K groups, per cell in fp64 from the f32 logits
 *     m = max_j l_j,  e_j = exp((double)l_j - (double)m),  Z = sum_j e_j,  p_j = e_j / Z,  conf = max_j p_j = 1 / Z
 * and a cell is BAD if its logits hold a NaN or a +inf or are all -inf (a -inf next to finite logits is fine: p_j = 0).  Over
 * the cells of group k that are not bad:
 *     prob_sum f64   [K, C] : sum of p_ij                  conf_sum f64 [K] : sum of conf_i
 *     votes    int32 [K, C] : cells with label == j        tally int32 [K, 3] : {cells that take part, cells with label -1,
 *                                                                              bad cells}; a bad cell counts in tally[k][2] only
 * so tally[k][0] == sum_j votes[k][j] + tally[k][1].
 * The batch comes GROUP-MAJOR: seg_ptr int64 [K + 1] (non-decreasing, 0 <= seg_ptr[0], seg_ptr[K] <= n_rows), order int32
 * [seg_ptr[K]] with the ids of the cells of group k, ascending, in order[seg_ptr[k] .. seg_ptr[k + 1]); cells that take no part
 * are absent.  An order entry outside [0, n_rows) or whose label is outside [-1, C) takes no part; a seg_ptr value outside
 * [0, min(seg_ptr[K], n_rows)] is clamped into it: malformed operands never fault.  n_rows == 0 or seg_ptr[K] == 0 is valid
 * (logits / label / order may be NULL then, the outputs are still written; with one of them NULL no cell takes part).
 *   A group's run is cut into chunks of 256 cells (a constant of the kernel, not of the device), one wavefront per chunk, lanes
 *   laid out (cell slot, class); per-cell max and Z by an xor butterfly, per-lane private fp64 sums, an xor butterfly over the
 *   cell slots, one partial per chunk in the workspace; a second kernel adds a group's partials in ascending chunk order.  No
 *   atomics of any kind; the order of a bin's additions depends on the operand alone: two launches are bit-identical whatever
 *   the grid.  No limit on C beyond int32 (C > 64 walks the classes 64 at a time).
 *   flags: WGNN_CLUSTERS_ACCUMULATE - add the batch to what the four outputs hold; without it EVERY element of all four is
 *   written, zeros included (the caller does not pre-clear).
 *   workspace: wgnn_group_class_reduce_workspace bytes, caller-owned, 8-byte aligned.
 *   Errors, before any launch: WGNN_ERR_BAD_ARG (a NULL output or seg_ptr, K <= 0, C <= 0, ld_logits < C, n_rows outside
 *   [0, 2^31), unknown flag), WGNN_ERR_ALIGNMENT (prob_sum / conf_sum / seg_ptr / workspace not 8-byte, the others not 4-byte
 *   aligned), WGNN_ERR_WORKSPACE, WGNN_ERR_UNSUPPORTED (sizes whose workspace is beyond 2^63 bytes); wgnn_last_error_string
 *   names the check.  Whether logits / label / order are missing while
 *   seg_ptr[K] > 0 is not visible to the host without a read-back: wrappers check it.
 * ------------------------------------------------------------------------- */
#define WGNN_CLUSTERS_ACCUMULATE 256
int wgnn_group_class_reduce_workspace(int64_t n_rows, int32_t n_groups, int32_t n_classes, int64_t* bytes);
int wgnn_group_class_reduce(const float* logits, int64_t ld_logits, const int32_t* label,
                            const int32_t* order, const void* seg_ptr /* int64_t[n_groups+1] */,
                            int64_t n_rows, int32_t n_groups, int32_t n_classes,
                            double* prob_sum, double* conf_sum, int32_t* votes, int32_t* tally,
                            void* workspace, int64_t workspace_bytes, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Calls re-drawn under gene dropout (additive export, WGNN_VERSION stays 206): the kernel behind
 * api.ResidentPredictor.stability.  One layer of wgnn_predict_rows for every (cell, draw) pair of a batch, a draw being the
 * cell with a random subset of its stored entries kept.  rowptr / col / raw / table / ld_table / n_genes / H / alpha / bias /
 * w_head / b_head / n_classes / unsure_threshold exactly as wgnn_predict_rows takes them (H % 4 == 0, H <= 256, C * H * 4 <=
 * 64 KiB, WGNN_FLAG_ROWPTR_I64); an out-of-range gene id is the caller's to check, as there.
 *
 * Which entries are kept.  The mask is a pure function of (seed, cell, draw, gene id) - no generator state.  All arithmetic
 * in uint64 with wrap-around; mix32 is the upper half of the splitmix64 finaliser:
 *     mix32(x):  x += 0x9E3779B97F4A7C15;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;  x = (x ^ (x >> 27)) * 0x94D049BB133111EB;
 *                x ^= x >> 31;  return (uint32)(x >> 32)
 *     cell = row0 + r,  draw = draw0 + d,  g = col[j]                      (r in [0, n_rows), d in [0, n_draws))
 *     key  = seed ^ (cell * 0x9FB21C651E98DF25) ^ (draw * 0xD6E8FEB86659FD93)
 *     u    = mix32(key + g * 0xC2B2AE3D27D4EB4F)
 *     kept iff (uint64)u < T,   T = (uint64)floor(keep * 4294967296.0)      (computed on the host, here)
 *   keep == 1 keeps every entry, keep == 0 none.  The mask follows the GENE, not the entry's position: a cell's mask is the
 *   same in whatever order its genes are stored.  row0 / draw0 (>= 0) let a caller split a batch by cells or by draws and get
 *   the same masks.  keep outside [0, 1], NaN included: WGNN_ERR_BAD_ARG.
 *
 * What a draw computes: wgnn_predict_rows' formula over the kept entries only - deg' = their number, S' = their f32 sum, z by
 * the layer-1 rule (self_rows == NULL) or the explicit-self rule, with the gather and the fold order of wgnn_predict_rows; a
 * masked entry has weight 0 (selected, not multiplied).  A draw that keeps nothing - or whose kept values sum to exactly 0,
 * where wgnn_predict_rows would divide 0 by 0 - is an empty row, z = bias (+ alpha[G+1] self_rows): never a NaN.  With
 * keep == 1 a draw's output, label and max_prob carry THE BITS of wgnn_predict_rows on the same batch.
 *
 * Without a head (w_head == NULL; the layers below the last): out [n_rows * n_draws, ld_out], row r * n_draws + d = ReLU(z) of
 * that draw; self_rows, when given, is indexed the same way, [n_rows * n_draws, ld_self] - a deeper model runs
 * wgnn_linear_fwd between the launches and every draw carries its own mask through every layer.
 * With a head, reduced over the draws of a cell on the device:
 *     votes    int32 [n_rows, ld_votes], ld_votes >= C : draws whose label (wgnn_predict_rows' rule for unsure_threshold) is j
 *     unsure   int32 [n_rows] : draws labelled -1
 *     empty    int32 [n_rows] : draws that kept no entry (still counted in votes / unsure by the label they get)
 *     conf_sum f64   [n_rows] : the draws' f32 max_prob added in fp64 in ascending draw order
 *     draw_label int32 [n_rows, n_draws], draw_prob f32 [n_rows, n_draws] : per draw; either may be NULL
 *   so sum_j votes[r][j] + unsure[r] == n_draws per call.  WGNN_STABILITY_ACCUMULATE (head only): add this call's draws to
 *   what the four tables hold (conf_sum continues the running sum: 32 draws, then 32 more with draw0 = 32, leave the bits of
 *   64 at once); without it EVERY element of the four is written, zeros included.  Columns of votes beyond C are not touched.
 *
 * One workgroup per cell, its 8 waves take draws d, d + 8, ...; the kept entries of a 64-entry chunk are compacted to the low
 * lanes (the identity permutation when nothing is masked) so masked entries load no table row; the draws' results are
 * tallied in LDS.  No atomics of any kind, one addition order whatever the grid: two launches are bit-identical.
 * n_rows * n_draws < 2^31.  Errors, before any launch: WGNN_ERR_BAD_ARG (a missing operand, n_draws < 1, n_rows * n_draws >=
 * 2^31, negative row0 / draw0, keep outside [0, 1], a head without votes / unsure / empty / conf_sum, ld_votes < C, an unknown
 * flag), WGNN_ERR_ALIGNMENT (H % 4, leading dimensions, pointers), WGNN_ERR_UNSUPPORTED (H > 256, a head beyond 64 KiB);
 * wgnn_last_error_string names the check.
 * ------------------------------------------------------------------------- */
#define WGNN_STABILITY_ACCUMULATE 256
int wgnn_predict_rows_dropout(const void* rowptr, const int32_t* col, const float* raw, int64_t n_rows,
                              const float* table, int64_t ld_table, int32_t n_genes, int32_t H,
                              const float* alpha, const float* bias, const float* self_rows, int64_t ld_self,
                              int32_t n_draws, int64_t row0, int32_t draw0, uint64_t seed, double keep,
                              float* out, int64_t ld_out,
                              const float* w_head, const float* b_head, int32_t n_classes, float unsure_threshold,
                              int32_t* votes, int64_t ld_votes, int32_t* unsure, int32_t* empty, double* conf_sum,
                              int32_t* draw_label, float* draw_prob, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Calls re-drawn under READ-LEVEL THINNING (additive export, WGNN_VERSION stays 206): the kernel behind
 * api.ResidentPredictor.stability(thin="reads").  wgnn_predict_rows_dropout drops whole genes of the normalised values; this
 * entry re-sequences the cell at a share `keep` of its depth: `raw` holds COUNTS (f32 integers in [1, 2^24]; anything else
 * counts as no read), every read survives with probability keep, low-count genes drop out first, and the library size the
 * logarithm divides by shrinks with the reads.  No thinned matrix is stored.  Every operand of wgnn_predict_rows_dropout is
 * taken as there; further: rest int64 [n_rows] = the cell's reads in columns OUTSIDE the bundle (negative counts as 0), scale
 * (Seurat's scale.factor, > 0) and threshold (>= 0) of wgnn_align_count_ln.
 *
 * Which reads are kept.  mix32, key(seed, cell, draw) and T = (uint64)floor(keep * 4294967296.0) are the dropout block's;
 * mix64(x) is the same splitmix64 finaliser returning all 64 bits, so mix32(x) == (uint32)(mix64(x) >> 32).  All in uint64
 * with wrap-around:
 *     ek = mix64(key + g * 0xC2B2AE3D27D4EB4F)                                   (K_GENE, g = col[j])
 *     read i in [0, c) of the entry (cell, g, count c) is kept iff (uint64)mix32(ek + i * 0xA0761D6478BD642F) < T     (K_READ)
 *     c' = the number of kept reads of the entry;   rest' = the same over rest[r] reads with g = n_genes
 *   Pure consequences of the hash: c' is Binomial(c, T / 2^32); the result does not depend on the order of a cell's genes;
 *   levels are nested (a read kept at 0.25 is kept at 0.5); row0 / draw0 split a batch by cells or draws without changing a bit.
 *   keep == 1 keeps every read, keep == 0 none.
 *
 * The draw's values.  total' = sum over the cell's entries of c' + rest' (an integer), and
 *     v' = float( log1p( double(c') / double(total') * scale ) )
 *   in fp64 with contraction off: the function wgnn_align_count_ln evaluates (one definition in the source, csrc/
 *   wgnn_align_rows.h).  An entry TAKES PART iff c' > 0 && v' > threshold.
 * The draw's layer.  The participating entries, in row order, form a row of wgnn_predict_rows: deg' = their number, S' = their
 *   f32 sum, the same weights (selected to 0 for a draw whose S' is 0), the same gather and fold, then - with a head - the
 *   head, label rule and tallies of wgnn_predict_rows_dropout.  The arithmetic order is wgnn_predict_rows' on that compacted
 *   row, so a draw carries the bits wgnn_predict_rows leaves on the materialised draw run through wgnn_align_count_ln / _fill_ln
 *   (one more column holding rest'), and with keep == 1 THE BITS of wgnn_predict_rows on the lognorm-aligned batch, whatever
 *   the threshold.  A draw with nothing left - total' == 0 included - is the empty row (z = bias (+ alpha[G+1] self_rows)) and
 *   counts in `empty`.
 *
 * Outputs as wgnn_predict_rows_dropout (out without a head; votes / unsure / empty / conf_sum / draw_label / draw_prob with
 * one, WGNN_THIN_ACCUMULATE as WGNN_STABILITY_ACCUMULATE), and per pair, in either mode, either may be NULL:
 *     draw_reads   int32 [n_rows, n_draws] : total' (the caller keeps a cell's reads below 2^31; a larger value saturates)
 *     draw_entries int32 [n_rows, n_draws] : deg'
 *
 * One workgroup per cell, its 8 waves take the draws.  The hash costs O(reads): c' is computed once per (cell, draw) and the
 * surviving entries are kept in a per-wave stash in LDS (1024 entries) for the later sweeps; of a draw that outgrows it the
 * tail is recomputed.  Entries with c >= 16, and rest, are thinned by the whole wave, 64 reads per step.  No atomics of any
 * kind, vector stores only, one addition order whatever the grid: two launches are bit-identical.
 * Errors, before any launch: those of wgnn_predict_rows_dropout, and WGNN_ERR_BAD_ARG for rest NULL, scale not positive and
 * finite, threshold < 0 or NaN; WGNN_ERR_ALIGNMENT for rest not 8-byte, draw_reads / draw_entries not 4-byte aligned.
 * ------------------------------------------------------------------------- */
#define WGNN_THIN_ACCUMULATE 256
int wgnn_predict_rows_thin(const void* rowptr, const int32_t* col, const float* raw, int64_t n_rows,
                           const float* table, int64_t ld_table, int32_t n_genes, int32_t H,
                           const float* alpha, const float* bias, const float* self_rows, int64_t ld_self,
                           const int64_t* rest, double scale, float threshold,
                           int32_t n_draws, int64_t row0, int32_t draw0, uint64_t seed, double keep,
                           float* out, int64_t ld_out,
                           const float* w_head, const float* b_head, int32_t n_classes, float unsure_threshold,
                           int32_t* votes, int64_t ld_votes, int32_t* unsure, int32_t* empty, double* conf_sum,
                           int32_t* draw_label, float* draw_prob, int32_t* draw_reads, int32_t* draw_entries,
                           uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Batch alignment (additive exports, WGNN_VERSION stays 206): a batch over the CALLER's gene list made into the clean
 * bundle-vocabulary CSR that wgnn_predict_rows / wgnn_attrib_rows / wgnn_group_gene_reduce take - the device counterpart of the
 * column selection, `> threshold` and COO -> CSR of api._read_test_csr (reference preprocess.py:160-161, 173-178).  It runs
 * BEFORE those kernels because their deg and S are the row length and row sum over the bundle's genes only.
 *
 * Two passes over the same row walk, one wavefront per row (grid-stride), wave ballots for the slots: no atomics on the data
 * path, no LDS, two launches are bit-identical.
 *   wgnn_align_count: row_count int32 [B] = kept entries per row.
 *   wgnn_align_fill : out_rowptr int64 [B + 1] = the exclusive scan of row_count (the caller's; out_rowptr[B] = the total),
 *                     out_col int32 [total] bundle gene ids, out_raw f32 [total].
 * Input, one of two forms (the other's pointers NULL):
 *   dense: x f32 [B, ld] row-major, n_cols valid columns, ld >= n_cols (elements; the last row needs n_cols of them).  Rows that
 *          are 16-byte aligned (x and gene_map 16-byte aligned, ld % 4 == 0) are read 16 bytes per lane.
 *   CSR  : rowptr [B + 1] (int32, or int64 with WGNN_FLAG_ROWPTR_I64), col int32 in [0, n_cols), val f32 - the caller's columns.
 * gene_map int32 [n_cols]: the bundle id in [0, n_genes) of a column, or -1 = not in the bundle.  threshold f32.
 * Semantics, exact: entry (r, j) with value v is kept iff gene_map[j] >= 0 && v > threshold (a NaN is dropped; an explicit CSR
 * entry at or below the threshold too).  A row's kept entries leave in their INPUT order (stable) as (gene_map[j], v), v's bits
 * untouched - wgnn_predict_rows sums a row in CSR order.  Nothing is sorted or merged: a gene listed twice stays listed twice.
 * Malformed operands never fault: a CSR entry with col outside [0, n_cols) is not looked up, a gene_map value outside
 * [-1, n_genes) is not stored, a slot past out_rowptr[r + 1] is not written; each such entry is skipped and ORs its bit into
 * *status (int32, device memory, zeroed by the caller; required).  All address arithmetic is 64-bit (B * ld may exceed 2^31);
 * B < 2^31, a row keeps < 2^31 entries.  B = 0 and n_cols = 0 are valid (x / gene_map may be NULL then).
 * Errors: WGNN_ERR_BAD_ARG (status NULL, both or neither input form, ld < n_cols, n_genes <= 0, negative sizes, a missing
 * output, unknown flag), WGNN_ERR_ALIGNMENT (out_rowptr not 8-byte, x / val / gene_map not 4-byte aligned);
 * wgnn_last_error_string names the check.
 * ------------------------------------------------------------------------- */
#define WGNN_ALIGN_BAD_COL    1   /* status bit: a CSR entry's col was outside [0, n_cols)            */
#define WGNN_ALIGN_BAD_MAP    2   /* status bit: a gene_map value was outside [-1, n_genes)           */
#define WGNN_ALIGN_BAD_ROWPTR 4   /* status bit: out_rowptr left a row less room than it keeps (fill) */
#define WGNN_ALIGN_BAD_VALUE  8   /* status bit: a count was negative / NaN / infinite, or a library size unusable (_ln) */
int wgnn_align_count(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                     int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold,
                     int32_t* row_count, int32_t* status, uint32_t flags, void* stream);
int wgnn_align_fill(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                    int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold,
                    const int64_t* out_rowptr, int32_t* out_col, float* out_raw, int32_t* status,
                    uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Log-normalising alignment (additive exports, WGNN_VERSION stays 206): the same walk over RAW COUNTS, leaving what Seurat's
 * NormalizeData defaults ("LogNormalize", reference pre-process.R:33) make of them - the values the model was trained on.
 * For a batch of B cells over the caller's n_cols columns holding counts x[r, j]:
 *
 *   total[r] = sum over ALL j of double(x[r, j])          (columns outside the bundle included; fp64, fixed order)
 *   v[r, j]  = float( log1p( double(x[r, j]) / total[r] * scale ) )          (fp64 throughout, Seurat's operation order)
 *   entry (r, j) is kept  iff  gene_map[j] >= 0  &&  x[r, j] > 0  &&  v[r, j] > threshold
 *
 * The total is taken BEFORE the vocabulary filter, as the reference does (it normalises at pre-process.R:33 and drops unknown
 * symbols at :61): aligning first and normalising second gives another library size and other values.  Kept entries leave as
 * (gene_map[j], v[r, j]) in the row's input order, exactly as wgnn_align_fill orders them.  scale > 0 (Seurat: 10000);
 * threshold >= 0 is required (an entry that is not stored counts as 0).  A row whose total is 0 keeps nothing and no division
 * is made for it (its malformed columns and map values are still reported).  Counts need not be integers; a -0.0 is a zero.  No normalised matrix is stored: v is evaluated inside the
 * COUNT and the FILL walk by the same instructions, in fp64, and only for candidates (mapped column, x > 0).
 *   wgnn_align_count_ln: wgnn_align_count, and total double [B] (written).  The walk reads a row twice: first every column
 *                        into the total (dense: the row's n_cols columns; CSR: the row's stored entries, col is not read) - a
 *                        lane adds its entries in ascending position, the wave's 64 partial sums fold in a fixed butterfly: no
 *                        atomics, two launches are bit-identical - then the keep test.  library_size (double [B], or NULL): the
 *                        caller's own depths, which replace the sum on every row that holds a count > 0 (for a caller who has
 *                        already subset the genes); a value that is <= 0 or not finite on such a row is reported and the row's
 *                        total is 0.  The summing read also finds, on EVERY column, the counts that are negative, NaN or
 *                        infinite: such a count poisons the total whether or not its column maps, so it is left out and
 *                        WGNN_ALIGN_BAD_VALUE is raised in *status (as the other bits: never a fault, skip and report).
 *   wgnn_align_fill_ln : wgnn_align_fill over the totals wgnn_align_count_ln stored.
 * Every other argument, operand form, status bit and error as wgnn_align_count / _fill.  Further errors: WGNN_ERR_BAD_ARG
 * (threshold < 0 or NaN, scale not positive and finite, total NULL), WGNN_ERR_ALIGNMENT (total / library_size not 8-byte aligned).
 * ------------------------------------------------------------------------- */
int wgnn_align_count_ln(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                        int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold,
                        const double* library_size, double* total, double scale, int32_t* row_count, int32_t* status,
                        uint32_t flags, void* stream);
int wgnn_align_fill_ln(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                       int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold,
                       const double* total, double scale, const int64_t* out_rowptr, int32_t* out_col, float* out_raw,
                       int32_t* status, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Merging log-normalising alignment (additive exports, WGNN_VERSION stays 206): wgnn_align_count_ln / _fill_ln for a gene list
 * in which several columns name ONE bundle gene (several Ensembl ids of a symbol, a symbol and its synonym).  The counts of
 * such columns are added per cell BEFORE the logarithm - counts add, log-values do not.
 * A GROUP is the set of columns that name one bundle gene, when there are two or more of them (its MEMBERS; all carry the same
 * gene_map value).  The caller describes the groups by three int32 device tables:
 *   col_group  [n_cols]       : the group of column j in [0, n_groups), or -1 for a column that is alone in its gene;
 *   group_ptr  [n_groups + 1] : group s has the members group_cols[group_ptr[s] .. group_ptr[s + 1]);
 *   group_cols [n_members]    : member columns, ascending within a group.
 * For cell r and a group with gene g:
 *   total[r]  is unchanged - the fp64 sum over ALL of the caller's columns, members like any other; library_size replaces it.
 *   c = the fp64 sum of double(x[r, j]) over the members that COUNT (finite and > 0), added in the row's input order:
 *       ascending column for a dense row, ascending position for a CSR row (whatever the column ids say);
 *   v = float( log1p( c / total[r] * scale ) ), the operation order of wgnn_align_count_ln;
 *   ONE entry (g, v) is kept iff c > 0 && v > threshold - a group may pass a positive threshold jointly - and it sits where the
 *   FIRST counting member sits in the row's input order; every later member leaves nothing.
 * A column that is alone behaves exactly as in wgnn_align_count_ln / _fill_ln, and a row in which no group has two counting
 * members leaves bit for bit what those leave.  COUNT and FILL take the same decisions by the same instructions; no atomics on
 * the data path, two launches are bit-identical.  A CSR row may hold any number of member entries (beyond 256 counting ones the
 * walk searches the row's own entries instead of a list in LDS: slower, the same result).
 * Both operand forms, every argument, status bit and error as wgnn_align_count_ln / _fill_ln; a negative, NaN or infinite
 * count on a member raises WGNN_ALIGN_BAD_VALUE like on any column.  Malformed tables never fault: a col_group value outside
 * [-1, n_groups) (the column is then alone), a group_ptr range outside [0, n_members] (clamped) and a member outside
 * [0, n_cols) (skipped) raise WGNN_ALIGN_BAD_MAP (the CSR form finds a row's members by col_group alone and does not read
 * group_ptr / group_cols).  Rows are read 16 bytes per lane when col_group is 16-byte aligned too.
 * n_groups == 0 runs wgnn_align_count_ln / _fill_ln themselves (the tables may be NULL then).  Further errors: WGNN_ERR_BAD_ARG
 * (n_groups or n_members negative, a table NULL), WGNN_ERR_ALIGNMENT (a table not 4-byte aligned).
 * ------------------------------------------------------------------------- */
int wgnn_align_count_ln_merge(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                              int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold,
                              const int32_t* col_group, const int32_t* group_ptr, const int32_t* group_cols,
                              int32_t n_groups, int32_t n_members, const double* library_size, double* total, double scale,
                              int32_t* row_count, int32_t* status, uint32_t flags, void* stream);
int wgnn_align_fill_ln_merge(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                             int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold,
                             const int32_t* col_group, const int32_t* group_ptr, const int32_t* group_cols,
                             int32_t n_groups, int32_t n_members, const double* total, double scale,
                             const int64_t* out_rowptr, int32_t* out_col, float* out_raw, int32_t* status,
                             uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Vocabulary coverage (additive export, WGNN_VERSION stays 206): how much of a batch over the CALLER's gene list the bundle
 * sees - what wgnn_align_count / _fill drop without a word.  The operand is wgnn_align_count's, in the same two forms (dense
 * x / ld, or CSR rowptr / col / val with WGNN_FLAG_ROWPTR_I64), with gene_map [n_cols] and n_genes; it is only read.
 * An entry COUNTS iff its value is finite and > 0 (the candidates of wgnn_align_count_ln: a 0, a -0.0, a NaN, a negative and
 * an infinite value do not count).  A column is MAPPED iff gene_map[j] >= 0.
 * Per row r (all [n_rows]):
 *   n_expressed int32 : counting entries over ALL of the caller's columns (CSR: all the row's stored entries).
 *   n_mapped    int32 : those on mapped columns.
 *   total       double: the sum of the counting values over all columns - bit for bit the total wgnn_align_count_ln stores
 *                       for the same operand without library_size (the same code: a lane adds its entries in ascending
 *                       position, the wave's 64 partial sums fold in a fixed butterfly).
 *   total_mapped double: the same sum over the mapped columns only, in the same fixed order.
 *   n_bad       int32 : entries that are negative, NaN or infinite.  They are counted here and are in no other output; this
 *                       is a diagnostic, no status bit is raised for them.
 * Per caller column j:
 *   col_cells int32 [n_cols]: rows in which column j counts (written in full: cleared on the stream, then raised).
 * No floating-point atomics: the sums have a fixed order; the column counts are integer atomics (one per workgroup and column
 * for the dense form, whose columns are walked a second time by column-owning threads; one per counting entry for the CSR
 * form).  Two launches on the same operand give identical bits in every output.  Any n_cols.
 * Malformed operands never fault and raise wgnn_align's bits in *status (int32, device memory, zeroed by the caller; required):
 * a CSR entry with col outside [0, n_cols) is not looked up - it stays one of the row's stored entries (n_expressed, total, as
 * in wgnn_align_count_ln's total) but is unmapped and in no column's count - WGNN_ALIGN_BAD_COL; a gene_map value outside
 * [-1, n_genes) counts as unmapped, WGNN_ALIGN_BAD_MAP.  B = 0 and n_cols = 0 are valid.
 * Errors, before any launch: WGNN_ERR_BAD_ARG (status NULL, both or neither input form, ld < n_cols, the i64 flag on the dense
 * form, n_genes <= 0, negative sizes, a missing output, unknown flag), WGNN_ERR_ALIGNMENT (total / total_mapped not 8-byte,
 * x / val / gene_map / an int32 output not 4-byte aligned); wgnn_last_error_string names the check.
 * ------------------------------------------------------------------------- */
int wgnn_coverage_rows(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                       int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes,
                       int32_t* n_expressed, int32_t* n_mapped, int32_t* n_bad, double* total, double* total_mapped,
                       int32_t* col_cells, int32_t* status, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Pair rows (additive exports, WGNN_VERSION stays 206): two cells' COUNT rows merged into the log-normalised row of their sum -
 * a synthetic doublet, the operand of api.ResidentPredictor.doublets.  The merged rows are written out as a CSR that
 * wgnn_predict_rows takes unchanged; the scheme is wgnn_align_count_ln / _fill_ln's: count, the caller's exclusive scan, fill.
 * Operand: a bundle-vocabulary CSR of raw counts - rowptr [n_rows + 1] (int32, or int64 with WGNN_FLAG_ROWPTR_I64), col int32,
 * cnt f32, nnz = the length of col / cnt - whose EVERY ROW IS STRICTLY ASCENDING in col (so a gene occurs once per row), every
 * count an integer in [1, 2^23] (the caller's check; the f32 sum of two counts is then exact).  lib int64 [n_rows]: a cell's
 * library size, ALL its reads, those in columns outside the bundle included.  a, b int32 [n_pairs]: the pairs' rows.
 * scale > 0 (Seurat's scale.factor), threshold >= 0.  For pair q, with A = a[q] and B = b[q]:
 *
 *   total = double(lib[A] + lib[B])
 *   for every gene g in the union of the two rows:  c = cnt_A(g) + cnt_B(g)        (a missing entry counts 0)
 *   v = float( log1p( double(c) / total * scale ) )      - lognorm() of csrc/wgnn_align_rows.h, the ONE definition that
 *                                                          wgnn_align_count_ln and wgnn_predict_rows_thin evaluate
 *   the entry (g, v) leaves  iff  c > 0 && v > threshold;  entries leave in ascending g.
 *
 * So a merged row carries THE BITS wgnn_align_count_ln / _fill_ln leave on the two cells' summed count row (one more column
 * holding their reads outside the bundle), and a self pair (A == B, allowed) the bits of the cell's own lognorm-aligned row:
 * 2c / 2T == c / T exactly.  total == 0 gives the empty row.
 *   wgnn_pair_rows_count: n_out int32 [n_pairs] = the entries pair q leaves.
 *   wgnn_pair_rows_fill : out_rowptr int64 [n_pairs + 1] = the exclusive scan of n_out (the caller's), out_col int32 and
 *                         out_val f32 [out_rowptr[n_pairs]].
 * One wavefront per pair (grid-stride); COUNT and FILL are the same walk - a merge path over the two sorted rows, 64 merged
 * positions per step, each lane finding its element by a binary search on its diagonal (ties: A's element first; B's equal
 * element is the duplicate, added to A's and dropped) - so they agree on every decision.  Wave ballots give the slots: no
 * atomics on the data path, no LDS, vector stores only; a slot depends on the pair alone, so two launches are bit-identical
 * and splitting the pair list changes no bit.
 * Malformed operands never fault; each is skipped and ORs its bit into *status (int32, device memory, zeroed by the caller;
 * required): a pair with A or B outside [0, n_rows) leaves the empty row, WGNN_PAIR_BAD_INDEX; a row that is found not strictly
 * ascending, WGNN_PAIR_UNSORTED (what leaves for its pairs is unspecified, every read stays inside the two rows); a row range
 * outside [0, nnz] (the empty row) or a slot at or past out_rowptr[q + 1] (not written), WGNN_PAIR_BAD_ROWPTR.
 * n_rows < 2^31, n_pairs < 2^31, a merged row keeps < 2^31 entries.  n_pairs = 0 is valid.
 * Errors, before any launch: WGNN_ERR_BAD_ARG (status NULL, a missing operand or output, a negative size, n_pairs >= 2^31, scale
 * not positive and finite, threshold < 0 or NaN, an unknown flag), WGNN_ERR_ALIGNMENT (lib / out_rowptr / an int64 rowptr not
 * 8-byte, any other operand not 4-byte aligned); wgnn_last_error_string names the check.
 * ------------------------------------------------------------------------- */
#define WGNN_PAIR_BAD_INDEX  1   /* status bit: a[q] or b[q] was outside [0, n_rows)                              */
#define WGNN_PAIR_UNSORTED   2   /* status bit: a row was not strictly ascending in col                           */
#define WGNN_PAIR_BAD_ROWPTR 4   /* status bit: a row range outside [0, nnz], or out_rowptr left a pair less room */
int wgnn_pair_rows_count(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                         const int64_t* lib, const int32_t* a, const int32_t* b, int64_t n_pairs, double scale,
                         float threshold, int32_t* n_out, int32_t* status, uint32_t flags, void* stream);
int wgnn_pair_rows_fill(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                        const int64_t* lib, const int32_t* a, const int32_t* b, int64_t n_pairs, double scale,
                        float threshold, const int64_t* out_rowptr, int32_t* out_col, float* out_val, int32_t* status,
                        uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Pool rows (additive exports, WGNN_VERSION stays 206): the COUNT rows of all cells of a group - a cluster, a sample, a metacell -
 * added into one pooled count row per group, and that row log-normalised against the group's pooled library size: the operand
 * of api.ResidentPredictor.pseudobulk.  Two steps: ACCUMULATE adds cells into a dense integer table, FINISH turns the table
 * into a CSR that wgnn_predict_rows takes unchanged (count, the caller's exclusive scan, fill, as wgnn_pair_rows_*).
 *
 * wgnn_pool_rows_accumulate
 * Operand: a bundle-vocabulary CSR of raw counts - rowptr [n_rows + 1] (int32, or int64 with WGNN_FLAG_ROWPTR_I64), col int32,
 * cnt f32, nnz = the length of col / cnt.  Every count is an integer in [1, 2^23] (the caller's check; any other value is
 * left out without a word).  Rows need NOT be sorted, and a gene listed twice in a row adds twice.
 * group_ptr int64 [n_groups + 1], ascending, and members int32 [n_rows]: the cells of group k are
 * members[group_ptr[k] : group_ptr[k + 1]] (one stable sort of the cells' group ids gives both; the member buffer always holds
 * n_rows entries, of which [group_ptr[0], group_ptr[n_groups]) are read, so a slice group_ptr + k0 of a longer list is a valid
 * operand next to the same members).  acc uint64 [n_groups, ld_acc], ld_acc >= n_genes: zeroed or pre-seeded by the caller;
 *
 *   acc[k][g] += sum over the members r of group k, over the entries j of row r with col[j] == g, of uint64(cnt[j])
 *
 * columns [n_genes, ld_acc) are never touched.  All sums are integers: the result is exact and the same bits in every order - two
 * launches, any split of the group list, any permutation of the cells.
 * Work unit: (group k, a run of at most cells_per_unit consecutive members, a slab of at most slab_genes genes); the runs are
 * cut at multiples of cells_per_unit of the POSITION in the member list counted from group_ptr[0] (so the number of units is
 * known without reading group_ptr back) and at the groups' ends; a big group is thus spread over n / cells_per_unit workgroups,
 * a workgroup whose window of positions holds several small groups takes them one after the other.  One workgroup per (window,
 * slab), grid-stride: it zeroes a uint32 LDS slab, its waves walk the unit's rows (one wave per row, entries outside the slab
 * skipped by comparison, so a row is read once per slab), LDS integer atomics take the counts - cells_per_unit <= 256 and
 * 256 x 2^23 < 2^31, no overflow - and only the NON-ZERO slab entries go to acc, one 64-bit global atomic add each.
 * cells_per_unit: 0 = the default (64), at most 256.  slab_genes: 0 = the default (16384: 64 KiB of the CU's 160 KiB LDS, two
 * workgroups per CU), at most 16384; a slab is never wider than n_genes.
 *
 * wgnn_pool_rows_count / wgnn_pool_rows_fill
 * total int64 [n_groups]: the groups' summed library sizes, ALL reads, those outside the bundle included, each < 2^53.
 * scale > 0, threshold >= 0.  For group k, g ascending:
 *
 *   c = acc[k][g];   v = float( log1p( double(c) / double(total[k]) * scale ) )   - lognorm() of csrc/wgnn_align_rows.h in its
 *                                                        form that takes the count as a double (a pooled count may exceed 2^24)
 *   the entry leaves  iff  c > 0 && v > threshold;   total[k] <= 0 gives the empty row.
 *
 *   count: n_out int32 [n_groups] = the entries group k leaves.
 *   fill : out_rowptr int64 [n_groups + 1] = the exclusive scan of n_out (the caller's), out_col int32, out_val f32 and - may be
 *          NULL - out_cnt int64 [out_rowptr[n_groups]]: gene, value and c of every kept entry.
 * So wherever every c <= 2^24 a pooled row carries THE BITS wgnn_align_count_ln / _fill_ln leave on the group's summed count row
 * (one more column holding the reads outside the bundle), a group of two the bits of wgnn_pair_rows_*, a group of one the bits
 * of the cell's own lognorm-aligned row.  One wavefront per group row (grid-stride), 64 genes per step, wave ballots give the
 * slots; COUNT and FILL are the same walk.  No atomics, vector stores only.
 *
 * Malformed operands never fault; each is skipped and ORs its bit into *status (int32, device memory, zeroed by the caller;
 * required): a member outside [0, n_rows), WGNN_POOL_BAD_INDEX; a row range outside [0, nnz], a group_ptr that is not ascending
 * or leaves [0, n_rows] (what is added for the groups around it is unspecified, every read stays inside the operands), a slot at
 * or past out_rowptr[k + 1] (not written), WGNN_POOL_BAD_ROWPTR; a gene id outside [0, n_genes), WGNN_POOL_BAD_COL.
 * n_rows, n_groups, n_genes < 2^31.  n_groups = 0 and n_rows = 0 are valid.
 * Errors, before any launch: WGNN_ERR_BAD_ARG (status NULL, a missing operand or output, a negative size, a size >= 2^31,
 * ld_acc < n_genes, cells_per_unit outside [0, 256], slab_genes outside [0, 16384] - a wider slab does not fit the LDS budget -,
 * scale not positive and finite, threshold < 0 or NaN, an unknown flag), WGNN_ERR_ALIGNMENT (group_ptr / acc / total /
 * out_rowptr / out_cnt / an int64 rowptr not 8-byte, any other operand not 4-byte aligned); wgnn_last_error_string names the
 * check.
 * ------------------------------------------------------------------------- */
#define WGNN_POOL_BAD_INDEX  1   /* status bit: a member was outside [0, n_rows)                                      */
#define WGNN_POOL_BAD_ROWPTR 2   /* status bit: a row range outside [0, nnz], a malformed group_ptr, or too little room */
#define WGNN_POOL_BAD_COL    4   /* status bit: a gene id was outside [0, n_genes)                                    */
#define WGNN_POOL_MAX_CELLS_PER_UNIT 256
#define WGNN_POOL_MAX_SLAB_GENES     16384
int wgnn_pool_rows_accumulate(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                              const int64_t* group_ptr, const int32_t* members, int64_t n_groups, int32_t n_genes,
                              uint64_t* acc, int64_t ld_acc, int32_t cells_per_unit, int32_t slab_genes, int32_t* status,
                              uint32_t flags, void* stream);
int wgnn_pool_rows_count(const uint64_t* acc, int64_t ld_acc, const int64_t* total, int64_t n_groups, int32_t n_genes,
                         double scale, float threshold, int32_t* n_out, int32_t* status, void* stream);
int wgnn_pool_rows_fill(const uint64_t* acc, int64_t ld_acc, const int64_t* total, int64_t n_groups, int32_t n_genes,
                        double scale, float threshold, const int64_t* out_rowptr, int32_t* out_col, float* out_val,
                        int64_t* out_cnt, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------
 * Soup rows (additive exports, WGNN_VERSION stays 206): a cell's COUNT row with reads of AMBIENT RNA - the "soup", free-floating
 * transcripts every droplet captures besides its cell - drawn from a batch-wide profile and added to it, and the contaminated row
 * log-normalised against the contaminated library size: the operand of api.ResidentPredictor.ambient.  The scheme is
 * wgnn_pair_rows_*'s: count, the caller's exclusive scan, fill; the output is a CSR that wgnn_predict_rows takes unchanged.
 * Operand: a bundle-vocabulary CSR of raw counts - rowptr [n_rows + 1] (int32, or int64 with WGNN_FLAG_ROWPTR_I64), col int32,
 * cnt f32, nnz = the length of col / cnt.  Every count is an integer in [1, 2^23] (the caller's check; any other value is left
 * out without a word, as in pool rows).  Rows need NOT be sorted, and a gene listed twice in a row adds twice (a gene's summed
 * count stays below 2^32).  lib int64 [n_rows]: a cell's library size, ALL its reads, those in columns outside the bundle
 * included.  n_add int64 [n_rows]: the soup reads added to the cell, each in [0, 2^23] (the caller makes it of its contamination
 * level).  cdf uint64 [n_genes + 2], ascending, cdf[0] = 0: the soup profile as cumulative weights - bin g < n_genes is bundle
 * gene g, bin n_genes is "a column outside the bundle", W = cdf[n_genes + 1] with 0 < W < 2^63.  n_draws >= 1; row0, draw0 >= 0;
 * seed; scale > 0 (Seurat's scale.factor), threshold >= 0.
 *
 * Unit q = r * n_draws + d is cell r, draw d.  With key and mix64 of the dropout block and K_READ of the thinning block, in
 * uint64 with wrap-around:
 *
 *   sk   = mix64(key(seed, row0 + r, draw0 + d) + K_SOUP)       K_SOUP = 0x94D049BB133111EB (a stream of its own)
 *   u_t  = mix64(sk + t * K_READ)                                t in [0, n_add[r])
 *   x_t  = the high 64 bits of the 128-bit product u_t * W       (exact, in [0, W))
 *   bin_t = the k with cdf[k] <= x_t < cdf[k + 1]                (a bin of width zero is never drawn)
 *   s(g) = #{t : bin_t == g},  s_rest = #{t : bin_t == n_genes}
 *   c(g) = cnt_r(g) + s(g);    total = double(lib[r] + n_add[r])
 *   v    = float( log1p( double(c) / total * scale ) )           - lognorm() of csrc/wgnn_align_rows.h in its form that takes the
 *                                                                  count as a double, the ONE definition, as pool rows
 *   the entry (g, v) leaves  iff  c > 0 && v > threshold;  entries leave in ascending g;  total <= 0 gives the empty row.
 *
 * Pure consequences of the hash: s is Multinomial(n_add, widths / W) up to the 2^-64 grain of x_t; the result does not depend
 * on the order of a cell's genes; levels are NESTED - read t is the same read at every n_add that reaches it, so the reads added
 * at a contamination of 5 % are a subset of those added at 10 %; row0 / draw0 split a batch by cells (rowptr + r0, lib + r0,
 * n_add + r0, row0 = r0) or by draws without changing a bit; n_add == 0 gives the bits wgnn_align_count_ln / _fill_ln leave on
 * the cell's own row.  So a unit carries THE BITS of the aligned, log-normalised, host-materialised contaminated count row (one
 * more column holding lib - sum(cnt) + s_rest).
 *   wgnn_soup_rows_count: n_out int32 [n_rows * n_draws] = the entries unit q leaves; soup_mapped int32 [n_rows * n_draws] (may be
 *                         NULL) = n_add - s_rest, the soup reads that fell on bundle genes.
 *   wgnn_soup_rows_fill : out_rowptr int64 [n_rows * n_draws + 1] = the exclusive scan of n_out (the caller's), out_col int32,
 *                         out_val f32 and - may be NULL - out_cnt int64 [out_rowptr[n_rows * n_draws]]: gene, value and c of
 *                         every kept entry.
 * One workgroup per unit (grid-stride).  The genes are cut into slabs of slab_genes (0 = the default, 16384: 64 KiB of uint32, two
 * workgroups per CU; at most 16384; never wider than n_genes); per slab the workgroup zeroes a uint32 LDS slab, adds the cell's own
 * entries and the unit's reads with LDS integer atomics (what lies outside the slab is skipped by comparison, so every further
 * slab hashes the reads again) and sweeps the slab 64 genes per wave step; wave ballots give the slots.  A read's bin is searched
 * in two levels: a table of every 2^sh-th boundary of cdf in LDS (sh >= 6, at most 512 entries), then sh probes of cdf itself.
 * COUNT and FILL are the same walk, so they agree on every decision.  All sums are integers: exact whatever the order, two
 * launches are bit-identical.  No floating-point atomics, no global atomics on the data path, vector stores only.
 * Malformed operands never fault; each ORs its bit into *status (int32, device memory, zeroed by the caller; required): a row
 * range outside [0, nnz] (the unit leaves the empty row) or a slot at or past out_rowptr[q + 1] (not written; with out_col or
 * out_val NULL every slot is such a slot), WGNN_SOUP_BAD_ROWPTR; a gene id outside [0, n_genes) (the entry is skipped),
 * WGNN_SOUP_BAD_COL; an n_add outside [0, 2^23] (the unit is treated as 0 reads), WGNN_SOUP_BAD_ADD.  A cdf that is not
 * ascending gives unspecified draws, but every read stays inside the operands.
 * n_rows, n_rows * n_draws < 2^31, n_genes < 2^31 - 1.  n_rows = 0 is a valid no-op.
 * Errors, before any launch: WGNN_ERR_BAD_ARG (status NULL, a missing operand or output, a negative size, a size >= 2^31,
 * n_rows * n_draws >= 2^31, n_draws < 1, row0 or draw0 negative, scale not positive and finite, threshold < 0 or NaN, slab_genes
 * outside [0, 16384], an unknown flag), WGNN_ERR_ALIGNMENT (lib / n_add / cdf / out_rowptr / out_cnt / an int64 rowptr not
 * 8-byte, any other operand not 4-byte aligned); wgnn_last_error_string names the check.
 * ------------------------------------------------------------------------- */
#define WGNN_SOUP_BAD_ROWPTR 1   /* status bit: a row range outside [0, nnz], or out_rowptr left a unit less room */
#define WGNN_SOUP_BAD_COL    2   /* status bit: a gene id was outside [0, n_genes)                                */
#define WGNN_SOUP_BAD_ADD    4   /* status bit: an n_add was outside [0, 2^23]                                    */
#define WGNN_SOUP_MAX_SLAB_GENES 16384
int wgnn_soup_rows_count(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                         const int64_t* lib, const int64_t* n_add, const uint64_t* cdf, int32_t n_genes, int32_t n_draws,
                         int64_t row0, int32_t draw0, uint64_t seed, double scale, float threshold, int32_t slab_genes,
                         int32_t* n_out, int32_t* soup_mapped, int32_t* status, uint32_t flags, void* stream);
int wgnn_soup_rows_fill(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                        const int64_t* lib, const int64_t* n_add, const uint64_t* cdf, int32_t n_genes, int32_t n_draws,
                        int64_t row0, int32_t draw0, uint64_t seed, double scale, float threshold, int32_t slab_genes,
                        const int64_t* out_rowptr, int32_t* out_col, float* out_val, int64_t* out_cnt, int32_t* status,
                        uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Hood rows (additive exports, WGNN_VERSION stays 206): every unit's COUNT rows POOLED - a cell's row added to the rows of its
 * neighbours, the caller's kNN lists - and the pooled row log-normalised against the pooled library size: one step of kNN
 * smoothing, the operand of api.ResidentPredictor.smooth.  The scheme is wgnn_pair_rows_*'s: count, the caller's exclusive scan,
 * fill; the output is a CSR that wgnn_predict_rows takes unchanged.  Where wgnn_pool_rows_accumulate pools DISJOINT groups into a
 * dense uint64 [n_groups, n_genes] table - n_rows x n_genes x 8 bytes with one group per cell -, the units here may overlap and
 * their sums never leave the LDS.
 * Operand: the count CSR of the pool-rows and soup-rows blocks - rowptr [n_rows + 1] (int32, or int64 with
 * WGNN_FLAG_ROWPTR_I64), col int32, cnt f32, nnz = the length of col / cnt.  Every count is an integer in [1, 2^23] (the caller's
 * check; any other value is left out without a word).  Rows need NOT be sorted, and a gene listed twice in a row adds twice.
 * lib int64 [n_rows]: a cell's library size, ALL its reads, those in columns outside the bundle included, each >= 0.
 * hood_ptr int64 [n_units + 1], ascending, and members int32 [n_members]: unit q pools the rows
 * members[hood_ptr[q] : hood_ptr[q + 1]].  The indices refer to the whole member list, so hood_ptr + q0 (with n_units - q0) is a
 * valid operand for a slice of the units next to the same members.  A member listed twice adds twice, counts and library size.
 * scale > 0 (Seurat's scale.factor), threshold >= 0.  For unit q, g ascending:
 *
 *   c(g)  = sum over the unit's members r, over the entries j of row r with col[j] == g, of uint64(cnt[j])
 *   total = double( sum over the members of lib[r] )               (an int64 sum; the caller keeps it below 2^53: a double holds it)
 *   v     = float( log1p( double(c) / total * scale ) )            - lognorm() of csrc/wgnn_align_rows.h in its form that takes the
 *                                                                    count as a double, the ONE definition, as pool rows
 *   the entry (g, v) leaves  iff  c > 0 && v > threshold;  total <= 0, or a unit without a member, gives the empty row.
 *
 * A unit holds at most WGNN_HOOD_MAX_MEMBERS = 256 members: 256 x 2^23 = 2^31 fits the uint32 counter of a gene; where rows list
 * a gene twice, keeping a gene's summed count in a unit below 2^32 is the caller's condition, as in the soup block.  All sums are
 * integers, so the result does not depend on the order of the members, of a row's entries or of the slabs; two launches are
 * bit-identical.  A unit of one carries THE BITS wgnn_align_count_ln / _fill_ln leave on the cell's own row (one more column
 * holding the reads outside the bundle), a unit of two the bits of wgnn_pair_rows_*, a list of units that partitions the cells
 * the bits of wgnn_pool_rows_*.
 *   wgnn_hood_rows_count: n_out int32 [n_units] = the entries unit q leaves.
 *   wgnn_hood_rows_fill : out_rowptr int64 [n_units + 1] = the exclusive scan of n_out (the caller's), out_col int32, out_val f32
 *                         and - may be NULL - out_cnt int64 [out_rowptr[n_units]]: gene, value and c of every kept entry.
 * One workgroup of 8 waves per unit (grid-stride).  The members are checked once and their row ranges staged in LDS.  The genes
 * are cut into slabs of slab_genes (0 = the default, 16384: 64 KiB of uint32, two workgroups per CU; at most 16384; never wider
 * than n_genes); per slab the workgroup zeroes a uint32 LDS slab, its waves take the member rows (one wave per row, lanes over its
 * entries; what lies outside the slab is skipped by comparison, so with n_genes > slab_genes a row is read once per slab), LDS
 * integer atomics take the counts, and the slab is swept 64 genes per wave step; wave ballots and the folded per-wave counts give
 * the slots.  COUNT and FILL are the same walk, so they agree on every decision; at threshold == 0 && scale >= 1 every c > 0 is
 * kept and the counting walk skips the logarithm.  No floating-point atomics, no global atomics on the data path, vector stores
 * only.
 * Malformed operands never fault; each is skipped and ORs its bit into *status (int32, device memory, zeroed by the caller;
 * required): a member outside [0, n_rows) (that member is skipped, counts and library size), WGNN_HOOD_BAD_INDEX; a member's row
 * range outside [0, nnz] (that member is skipped), a hood_ptr range that descends or leaves [0, n_members] (the unit leaves the
 * empty row), a slot at or past out_rowptr[q + 1] (not written; with out_col or out_val NULL every slot is such a slot),
 * WGNN_HOOD_BAD_ROWPTR; a gene id outside [0, n_genes) (the entry is skipped), WGNN_HOOD_BAD_COL; more than 256 members (the unit
 * leaves the empty row), WGNN_HOOD_BAD_SIZE.
 * n_rows, n_units, n_genes < 2^31.  n_units = 0 is a valid no-op; n_rows = 0 is valid too (rowptr, lib, col and cnt may then be
 * NULL): every unit leaves the empty row, and a member it lists is WGNN_HOOD_BAD_INDEX.
 * Errors, before any launch: WGNN_ERR_BAD_ARG (status NULL, a missing operand or output, a negative size, a size >= 2^31, scale
 * not positive and finite, threshold < 0 or NaN, slab_genes outside [0, 16384], an unknown flag), WGNN_ERR_ALIGNMENT (lib /
 * hood_ptr / out_rowptr / out_cnt / an int64 rowptr not 8-byte, any other operand not 4-byte aligned); wgnn_last_error_string
 * names the entry and the check.
 * ------------------------------------------------------------------------- */
#define WGNN_HOOD_BAD_INDEX  1   /* status bit: a member was outside [0, n_rows)                                          */
#define WGNN_HOOD_BAD_ROWPTR 2   /* status bit: a row range outside [0, nnz], a malformed hood_ptr range, or too little room */
#define WGNN_HOOD_BAD_COL    4   /* status bit: a gene id was outside [0, n_genes)                                        */
#define WGNN_HOOD_BAD_SIZE   8   /* status bit: a unit held more than WGNN_HOOD_MAX_MEMBERS members                       */
#define WGNN_HOOD_MAX_MEMBERS    256
#define WGNN_HOOD_MAX_SLAB_GENES 16384
int wgnn_hood_rows_count(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                         const int64_t* lib, const int64_t* hood_ptr, const int32_t* members, int64_t n_units,
                         int64_t n_members, int32_t n_genes, double scale, float threshold, int32_t slab_genes,
                         int32_t* n_out, int32_t* status, uint32_t flags, void* stream);
int wgnn_hood_rows_fill(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                        const int64_t* lib, const int64_t* hood_ptr, const int32_t* members, int64_t n_units,
                        int64_t n_members, int32_t n_genes, double scale, float threshold, int32_t slab_genes,
                        const int64_t* out_rowptr, int32_t* out_col, float* out_val, int64_t* out_cnt, int32_t* status,
                        uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Calls on GIVEN gene subsets (additive export, WGNN_VERSION stays 206): the kernel behind api.ResidentPredictor.panels, the
 * third member of the family of wgnn_predict_rows_dropout (a mask drawn per gene) and wgnn_predict_rows_thin (reads drawn).
 * One layer of wgnn_predict_rows for every (cell, panel) pair of a batch; no sub-matrix is stored.  Every operand of
 * wgnn_predict_rows is taken as there (H % 4 == 0, H <= 256, a head of C * H * 4 <= 64 KiB, WGNN_FLAG_ROWPTR_I64); further:
 *     member   uint64 [n_genes] : bit p of member[g] = gene g belongs to panel p (one 8-byte load beside col[j] answers for
 *                                 all panels of the launch); bits at or above n_panels are ignored
 *     n_panels in [1, 64]
 *     lib      int64 [n_rows, ld_lib] or NULL, ld_lib >= n_panels; with it scale (> 0, finite) and threshold (>= 0)
 * A pair is (r, p); its row in out, self_rows, logits, label, max_prob and entries is r * n_panels + p.  A deeper model runs
 * wgnn_linear_fwd between the launches; the mask is applied again in every layer.
 *
 * Values mode (lib == NULL).  The kept entries of pair (r, p) are the row's entries whose gene is in panel p, in row order,
 *   their values as given.
 * Counts mode (lib != NULL).  raw holds COUNTS; lib[r, p] = the cell's reads inside panel p over ALL the caller's columns
 *   (the host computes it; panel columns outside the bundle count).  An entry takes part iff its gene is in the panel, its
 *   count is countable (finite and > 0) and
 *     v' = float( log1p( double(count) / double(lib[r, p]) * scale ) )  >  threshold
 *   - the function wgnn_align_count_ln evaluates (one definition in the source, csrc/wgnn_align_rows.h).  lib[r, p] <= 0 gives
 *   the empty row.
 * The pair's layer.  The kept / participating entries form a row of wgnn_predict_rows: deg' = their number, S' = their f32
 *   sum, the same weights, gather, fold order, head, softmax maximum and label rule.  A pair that keeps nothing is the empty
 *   row, z = bias (+ alpha[G+1] self_rows); where the kept values sum to exactly 0 the weights are selected to 0 and never
 *   divided.  The arithmetic order is wgnn_predict_rows' on the COMPACTED row (a kept entry's position in the compacted row
 *   decides its lane in the S' sum and its lane group and step in the gather), so in values mode every pair carries THE BITS
 *   wgnn_predict_rows leaves on the materialised sub-row (out, logits, label, max_prob), and in counts mode those it leaves
 *   on wgnn_align_count_ln / _fill_ln of the count matrix with the non-panel columns zeroed.
 *
 * Outputs.  Without a head: out [n_rows * n_panels, ld_out] = ReLU(z).  With one: label int32 and max_prob f32
 * [n_rows, n_panels] (required), logits [n_rows * n_panels, ld_logits] (may be NULL).  In either mode entries int32
 * [n_rows, n_panels] = deg' (may be NULL).  There are no tallies across panels.
 *
 * One workgroup per cell, its 8 waves take the panels; a pair's kept entries sit in a per-wave stash in LDS (1024 entries), of
 * a pair that outgrows it the tail is tested again.  No atomics of any kind, vector stores only, one addition order whatever
 * the grid: two launches are bit-identical.
 * Errors, before any launch: WGNN_ERR_BAD_ARG (a missing operand, member included; n_panels outside [1, 64]; n_rows * n_panels
 * >= 2^31; with lib: ld_lib < n_panels, scale not positive and finite, threshold < 0 or NaN; a head without label or max_prob;
 * no head and no out; an unknown flag), WGNN_ERR_ALIGNMENT (H % 4, leading dimensions, pointers - member and lib 8-byte),
 * WGNN_ERR_UNSUPPORTED (H > 256, a head beyond 64 KiB); wgnn_last_error_string names the check.
 * ------------------------------------------------------------------------- */
int wgnn_predict_rows_panels(const void* rowptr, const int32_t* col, const float* raw, int64_t n_rows,
                             const float* table, int64_t ld_table, int32_t n_genes, int32_t H,
                             const float* alpha, const float* bias, const float* self_rows, int64_t ld_self,
                             const uint64_t* member, int32_t n_panels,
                             const int64_t* lib, int64_t ld_lib, double scale, float threshold,
                             float* out, int64_t ld_out,
                             const float* w_head, const float* b_head, int32_t n_classes, float unsure_threshold,
                             float* logits, int64_t ld_logits, int32_t* label, float* max_prob, int32_t* entries,
                             uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Rank-based scores of GIVEN gene sets (additive export, WGNN_VERSION stays 206): the kernel behind
 * api.ResidentPredictor.signatures - UCell's signature score (Andreatta & Carmona 2021), a Mann-Whitney U of the set's ranks
 * inside the cell's own row.  The batch is a CSR over the bundle's gene ids as wgnn_predict_rows takes it (rowptr int32, or int64
 * with WGNN_FLAG_ROWPTR_I64; col; val f32), a row of fewer than 2^31 entries; further:
 *     member   uint64 [n_genes] : bit p of member[g] = gene g belongs to set p - wgnn_predict_rows_panels' word; bits at or
 *                                 above n_sets are ignored
 *     n_sets   in [1, 64]
 *     max_rank in [1, 2^30]     : UCell's maxRank; ranks past it all count as max_rank + 1
 * The definition, for one cell r (deg stored entries) and one set p - all of it integer arithmetic:
 *   Order.  Stored entries are ordered by their f32 value, descending, compared on the order-preserving integer key of the
 *     f32 bits: all bits flipped for a value whose sign bit is set, only the sign bit flipped otherwise.  That is one total
 *     order over every bit pattern (NaNs and signed zeros included); on finite values it is the numeric order, -0.0 below +0.0.
 *   Doubled mid-rank of a stored entry j.  gt_j = #{i : key_i > key_j}, eq_j = #{i : key_i == key_j} (j itself included),
 *     R2_j = 2 * gt_j + eq_j + 1: twice the tie-averaged rank, rank 1 = the highest value.
 *   Cap.  R2c_j = min(R2_j, 2 * (max_rank + 1)).
 *   Outputs.  rank2_sum[r, p] int64 = the sum of R2c_j over the stored entries whose gene is in set p; present[r, p] int32 =
 *     the number of those entries.  Both are [n_rows, ld_*], ld_* >= n_sets; columns >= n_sets are left untouched.
 *   The genes that are not stored all tie below every stored entry, R2_zero = deg + 1 + n_genes; with n_p = the set's size the
 *     HOST finishes  two_u = rank2_sum + (n_p - present) * min(deg + 1 + n_genes, 2 * (max_rank + 1)) - n_p * (n_p + 1)  and
 *     score = 1 - two_u / (2 * n_p * max_rank)  in fp64 (UCell's 1 - U / (n * maxRank)); the kernel does not see n_p.
 * An entry whose gene id is outside [0, n_genes) belongs to no set and is never used as an index; as a stored value it still
 * takes part in the other entries' ranks.  A gene listed twice in a row counts twice, as two stored entries.
 *
 * One workgroup per cell: the row's keys are staged in LDS (16 384 keys, 64 KiB, at most - a longer row's tail is read from
 * global memory), the set members are compacted into a stash of 512 entries (a row with more members runs in passes), and a
 * member's rank is COUNTED against the staged keys - nothing is sorted.  Integers only, no atomics, vector stores only: the
 * result is independent of the grid, the slab width, the pass structure and the order of the entries within a row, and two
 * launches are bit-identical.
 * Errors, before any launch: WGNN_ERR_BAD_ARG (a missing operand; n_rows outside [0, 2^31); n_sets outside [1, 64]; max_rank
 * outside [1, 2^30]; n_genes <= 0; ld_sum or ld_present < n_sets; an unknown flag), WGNN_ERR_ALIGNMENT (member or rank2_sum not
 * 8-byte aligned; rowptr not aligned to its entries; col, val or present not 4-byte aligned); wgnn_last_error_string names the
 * check.  n_rows == 0 is a no-op.
 * ------------------------------------------------------------------------- */
int wgnn_rank_sets_rows(const void* rowptr, const int32_t* col, const float* val, int64_t n_rows, int32_t n_genes,
                        const uint64_t* member, int32_t n_sets, int32_t max_rank,
                        int64_t* rank2_sum, int64_t ld_sum, int32_t* present, int64_t ld_present,
                        uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Wilcoxon rank-sum tables per (group, gene) (additive exports, WGNN_VERSION stays 206): the kernel behind
 * api.ResidentPredictor.rank_genes - every gene tested for each group of cells against the rest (Mann-Whitney U with the tie
 * correction; scanpy's rank_genes_groups(method="wilcoxon"), presto).  The operand is the batch GENE-MAJOR exactly as
 * wgnn_group_gene_reduce takes it (t_rowptr int32 [n_genes + 1], t_cell, t_val f32), group int32 [n_rows] with -1 = the cell
 * takes no part, and group_size int64 [n_groups] = the histogram of group over [0, n_groups).  All of it is integer arithmetic:
 *   Taking part.  The cells with group[i] in [0, n_groups); N = their number = the sum of group_size, N_k = group_size[k].
 *   Values.  For gene g a participating cell that does not list g holds the implicit value +0.0f.  Values are ordered by
 *     wgnn_rank_sets_rows' order-preserving key of the f32 bits, ASCENDING: one total order over every bit pattern, the numeric
 *     order on finite values with -0.0 below +0.0.  n_g = the participating stored entries of g, z = N - n_g implicit zeros.
 *   Doubled mid-rank.  R2_j = 2 * #{less} + #{equal, j included} + 1 over all N values of the gene, rank 1 = the lowest.  For a
 *     stored entry the z implicit zeros count as "less" when its key is above key(+0.0f) and as "equal" when it equals that key.
 *     An implicit zero has R2_0 = 2 * #{stored below +0.0f} + t0 + 1 with t0 = z + #{stored equal to +0.0f}.
 *   Outputs, EVERY element written (the caller does not pre-clear); rank2_sum and count are [n_groups, ld_*], ld_* >= n_genes,
 *   columns >= n_genes are left untouched:
 *     rank2_sum int64 [k, g] = the sum of R2 over ALL cells of group k: its stored entries and its (N_k - count[k, g]) zeros
 *     count     int32 [k, g] = the stored entries of group k
 *     tie_sum   int64 [g]    = the sum over the gene's tie groups of t^3 - t (= the sum over its N values of eq^2 - 1)
 *   The HOST finishes in fp64, with n1 = N_k and n2 = N - n1:  U = (rank2_sum - n1 * (n1 + 1)) / 2,  mu = n1 * n2 / 2,
 *     var = n1 * n2 / 12 * ((N + 1) - tie_sum / (N * (N - 1))),  z = (U - mu) / sqrt(var),  auc = U / (n1 * n2).
 * An entry whose cell id is outside [0, n_rows) or whose group is outside [0, n_groups) takes no part - in no rank and not in
 * count; it is never used as an index and never faults.  group_size is trusted: one that is not the histogram of group gives
 * other numbers, not a fault.
 *
 * Nothing is sorted: a work unit is (gene, block of 512 stored entries); the gene's keys stream through an LDS slab of at most
 * 16 384 keys and every lane counts "less" and "equal" for the entry it owns; a long gene is many units.  Units meet in integer
 * LDS atomics and 64-bit integer global atomic adds - integer addition commutes, so the result is independent of the grid, the
 * chunking and the order of cells, and two launches are bit-identical.  A first pass clears the outputs and counts n_g per
 * gene, a last one adds the implicit zeros' terms.
 *   workspace: wgnn_rank_genes_groups_workspace bytes (8-byte aligned, caller-owned; about 24 bytes per gene, nothing per entry;
 *   not read for n_rows == 0).
 * Errors, before any launch: WGNN_ERR_BAD_ARG (a missing operand; n_rows outside [0, 2^20], so that N^3 fits int64; n_groups
 * outside [1, 4096]; n_genes <= 0; ld_sum or ld_count < n_genes; any flag bit - none is defined), WGNN_ERR_WORKSPACE,
 * WGNN_ERR_ALIGNMENT (rank2_sum, tie_sum, group_size or workspace not 8-byte aligned; another operand not 4-byte aligned);
 * wgnn_last_error_string names the check.  n_rows == 0 is a valid batch: the tables come back zero.
 * ------------------------------------------------------------------------- */
int wgnn_rank_genes_groups_workspace(int64_t n_rows, int64_t nnz, int32_t n_groups, int32_t n_genes, int64_t* bytes);
int wgnn_rank_genes_groups(const int32_t* t_rowptr, const int32_t* t_cell, const float* t_val, const int32_t* group,
                           const int64_t* group_size, int64_t n_rows, int32_t n_groups, int32_t n_genes,
                           int64_t* rank2_sum, int64_t ld_sum, int32_t* count, int64_t ld_count, int64_t* tie_sum,
                           void* workspace, int64_t workspace_bytes, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Exact k nearest neighbours of dense rows (additive exports, WGNN_VERSION stays 206): the kernel behind
 * api.ResidentPredictor.knn.  Brute force over every ordered (query, candidate) pair, O(n_q * n_c * D); the [n_q, n_c] distance
 * matrix is never stored, and symmetry is not exploited.
 *     Q [n_q, ld_q] f32, X [n_c, ld_x] f32 : queries and candidates, D valid columns each; they may be one buffer
 *     self_offset                          : query i IS candidate self_offset + i and is left out of its own list; -1 = no
 *                                            candidate is left out
 *     n_splits                             : the candidate rows are scanned in this many contiguous ranges (0 = chosen from n_q
 *                                            and n_c so that a small batch still fills the chip); it changes no bit
 *     idx int32 [n_q, ld_out], d2 f32 [n_q, ld_out] : the first k columns of a row are written, the others left untouched
 * Numerics.  The squared Euclidean distance is taken in difference form, one chain per pair:
 *     d = 0;  for j = 0 .. D-1 ascending:  t = q[j] - x[j] (one f32 rounding);  d = fmaf(t, t, d)
 *   with no re-association across the kernel's slabs of D.  Hence d >= +0; d2(i, j) and d2(j, i) carry the same bits (t is
 *   negated, t * t is not changed); every term is non-negative, so against the exact distance of the f32 rows the error is
 *   bounded RELATIVE TO d: |d - exact| <= gamma * exact, gamma = (D + 3) u / (1 - (D + 3) u), u = 2^-24.  (The norm form
 *   |q|^2 + |x|^2 - 2 q.x is not used: its error scales with the norms and re-orders exactly the closest neighbours.)
 * Selection.  Per query the k candidates smallest under the total order (d2, candidate index), ascending: equal distances go
 *   to the lower index.  A candidate whose distance is NaN is never selected (+inf is a distance like any other).  With fewer
 *   than k selectable candidates the tail holds idx = -1 and d2 = +inf.  The order is total, so the result does not depend on
 *   the grid, the tiles, n_splits or the order in which lanes find candidates; two launches are bit-identical.  LDS atomics
 *   claim staging slots and nothing else; there are no global atomics.
 * A workgroup holds 64 queries and streams tiles of 64 candidates x 16 columns through LDS; a lane owns 4 x 4 pairs.  Per query
 * the k best keys (bits(d2) << 32 | index) stay sorted in LDS; a finished distance is compared with the k-th, survivors are
 * staged and merged by rank, a wavefront per list, when a staging list fills.  LDS per workgroup: 34 KiB + 512 * (k | 1) bytes.
 *   workspace: wgnn_knn_workspace_bytes(n_q, n_c, k, n_splits) bytes, 8-byte aligned, caller-owned: [splits, n_q, k] 64-bit keys
 *   that a second kernel merges under the same order; 0 bytes (workspace may be NULL) when the scan is not split.
 * Errors, before any launch: WGNN_ERR_BAD_ARG (n_q or n_c outside [0, 2^31); n_splits outside [0, 64]; ld_out < k; self_offset
 * below -1 or self_offset + n_q > n_c; any flag bit - none is defined; a missing operand), WGNN_ERR_UNSUPPORTED (k outside
 * [1, 64], as wgnn_rows_topk; D outside [4, 1024]), WGNN_ERR_ALIGNMENT (D, ld_q or ld_x not a multiple of 4 or ld < D; Q or X
 * not 16-byte, idx or d2 not 4-byte, workspace not 8-byte aligned), WGNN_ERR_WORKSPACE; wgnn_last_error_string names the check.
 * n_q == 0 returns WGNN_OK without a launch.
 * ------------------------------------------------------------------------- */
int wgnn_knn_workspace_bytes(int64_t n_q, int64_t n_c, int32_t k, int32_t n_splits, int64_t* bytes);
int wgnn_knn_rows(const float* Q, int64_t ld_q, int64_t n_q, const float* X, int64_t ld_x, int64_t n_c,
                  int32_t D, int32_t k, int64_t self_offset, int32_t n_splits,
                  int32_t* idx, float* d2, int64_t ld_out, void* workspace, int64_t workspace_bytes,
                  uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Exact k nearest neighbours per SEGMENT of the rows (additive exports, WGNN_VERSION stays 206): the search behind
 * ops.knn_segments / api.ResidentPredictor.bbknn, a batch-balanced kNN graph.  Every query row lists its k nearest rows in
 * each of n_segs segments of the same matrix; brute force, O(n_q * n_rows * D), nothing of the distance matrix is stored.
 *     X [n_rows, ld_x] f32          : the rows, D valid columns, under wgnn_knn_rows' alignment rules; they stay in the
 *                                     caller's order
 *     order int32 [n_rows]          : the row ids segment-major
 *     seg_ptr int64 [n_segs + 1]    : segment s holds the candidates order[seg_ptr[s] .. seg_ptr[s+1]); a segment may be empty
 *     q_first, n_q                  : the queries are the rows q_first .. q_first + n_q - 1 of X
 *     n_segs in [1, 64], k in [1, 64], n_segs * k <= 64
 *     n_splits                      : every segment's candidate tiles are scanned in this many contiguous sub-ranges; 0 = chosen
 *                                     from n_q, n_rows and n_segs so that a small batch still fills the chip; a value above
 *                                     64 / n_segs is lowered to that (a query tile has at most 64 work units); it changes no bit
 *     idx int32, d2 f32 [n_q, ld_out]  : the BLOCKED lists, ld_out >= n_segs * k: columns s*k .. s*k+k-1 hold segment s's list,
 *                                     ascending, with a tail of -1 / +inf; the other columns of a row are left untouched
 *     merged_idx, merged_d2 [n_q, ld_merged] : optional (both or neither; ld_merged >= n_segs * k): the same n_segs * k entries
 *                                     as ONE ascending list, the -1 / +inf entries last
 *     status int32 [1] on the device: bits are OR-ed in, the caller clears it
 * Numerics are wgnn_knn_rows': d = 0; for j = 0 .. D-1 ascending: t = q[j] - x[j]; d = fmaf(t, t, d), one chain per pair, so
 *   a distance carries the bits wgnn_knn_rows gives that pair.  Selection is on the key (bits(d2) << 32 | ORIGINAL row id): the
 *   low word is order[c], not the position c, so equal distances go to the lower row id within a block and, in the merged list,
 *   across blocks.  A query is left out of the list of the segment that holds it (order[c] == q); a NaN distance is never
 *   listed.  The order is total: the result is a function of the operands alone, not of the grid, n_splits or lane timing.
 *   Atomics claim LDS staging slots and OR into the status word, nothing else.
 * A work unit is (64-query tile, segment, sub-range): it streams its candidates in tiles of 64 through LDS, rows loaded by id
 * through `order`, a lane owning 4 x 4 pairs as in wgnn_knn_rows, the last tile of a segment ending at seg_ptr[s+1]; it leaves k
 * sorted keys per query in the workspace.  A second kernel, a wavefront per query and a lane per unit, pops the smallest head
 * n_segs * k times under a quota of k per segment and writes each pop at its rank in both layouts.
 * Malformed operands are safe: seg_ptr is clamped into [0, n_rows] (and to ascend); an order id outside [0, n_rows) is skipped
 * and sets WGNN_KNN_SEGMENTS_BAD_ORDER.  (An id listed twice is searched twice; a list may then name it twice.)
 *   workspace: wgnn_knn_segments_workspace_bytes(n_q, n_rows, n_segs, k, n_splits) = n_segs * splits * n_q * k * 8 bytes,
 *   8-byte aligned, caller-owned.
 * Errors, before any launch, with wgnn_knn_rows' codes: WGNN_ERR_BAD_ARG (n_q or n_rows outside [0, 2^31); n_splits outside
 * [0, 64]; ld_out or ld_merged < n_segs * k; one of merged_idx / merged_d2 without the other; q_first < 0 or q_first + n_q >
 * n_rows; any flag bit - none is defined; a missing operand), WGNN_ERR_UNSUPPORTED (k or n_segs outside [1, 64]; n_segs * k >
 * 64; D outside [4, 1024]), WGNN_ERR_ALIGNMENT (D or ld_x not a multiple of 4 or ld_x < D; X not 16-byte, seg_ptr or workspace
 * not 8-byte, another operand not 4-byte aligned), WGNN_ERR_WORKSPACE; wgnn_last_error_string names the check.  n_q == 0 returns
 * WGNN_OK without a launch.
 * ------------------------------------------------------------------------- */
#define WGNN_KNN_SEGMENTS_MAX_SEGS  64   /* the most segments                                                          */
#define WGNN_KNN_SEGMENTS_MAX_LIST  64   /* the largest n_segs * k: a query's whole list                                */
#define WGNN_KNN_SEGMENTS_BAD_ORDER  1   /* status bit: an order id outside [0, n_rows): the candidate is skipped        */
int wgnn_knn_segments_workspace_bytes(int64_t n_q, int64_t n_rows, int32_t n_segs, int32_t k, int32_t n_splits, int64_t* bytes);
int wgnn_knn_segments(const float* X, int64_t ld_x, int64_t n_rows, int32_t D,
                      const int32_t* order, const int64_t* seg_ptr, int32_t n_segs, int32_t k,
                      int64_t q_first, int64_t n_q, int32_t n_splits,
                      int32_t* idx, float* d2, int64_t ld_out,
                      int32_t* merged_idx, float* merged_d2, int64_t ld_merged,
                      int32_t* status, void* workspace, int64_t workspace_bytes, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * k-means++ seeding of dense rows, every round on the device (additive exports, WGNN_VERSION stays 206): the seeding of
 * ops.kmeans_rows / api.ResidentPredictor.kmeans.  The assignment of a Lloyd step is wgnn_knn_rows with k = 1.
 *     X [n_rows, ld_x] f32 : the rows, D valid columns
 *     seed_row int32 [K]   : the chosen rows in the order they were chosen (-1 from the round on in which no valid row was left)
 *     min_d2 f32 [n_rows]  : a row's squared distance to the nearest of the K seeds (0 for a seed); NaN for an invalid row
 * A row is VALID iff all its D values are finite; an invalid row has weight 0 in every round and is never chosen.
 * Round r = 0 .. K-1:
 *     w_i = 0 for an invalid row; else 1 in round 0, and min_d2[i] against the seeds 0 .. r-1 later: the f32 distance in
 *           wgnn_knn_rows' chain,  d = 0;  for j = 0 .. D-1 ascending:  t = x[j] - c[j];  d = fmaf(t, t, d),  the minimum over the
 *           seeds so far (exactly 0 for a seed and for every copy of one), widened to fp64
 *     u_r = (mix64(mix64(seed) + r) >> 11) * 2^-53 in [0, 1), mix64 the splitmix64 finaliser (x += 0x9E3779B97F4A7C15;
 *           x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;  x = (x ^ x >> 27) * 0x94D049BB133111EB;  x ^ x >> 31), sums modulo 2^64
 *     the prefix, ALL in fp64 and in this order - a constant of the kernel, it does not depend on the grid: the rows are cut
 *           into chunks of 256 consecutive rows;  S_c = the weights of chunk c added in row order from 0.0;  C_0 = 0.0,
 *           C_{c+1} = C_c + S_c;  T = C_{n_chunks};  the inclusive prefix of row i of chunk c is  P_i = C_c + s_i  with s_i the
 *           weights of the chunk's rows up to and including i added in row order from 0.0  (P is non-decreasing)
 *     t = u_r * T (one rounding); the seed is the lowest i with P_i > t - a row of positive weight.  Should rounding give
 *           t >= T, the last row with w > 0 is taken.
 *     T == 0 (fewer distinct valid rows than rounds): the lowest-index valid row that is no seed yet; -1 when there is none
 *           (the caller's to refuse: the kernel cannot see it without a read-back).
 * Two launches per round and one closing pass, all on `stream`, no read-back in between: a pass over X (a workgroup per chunk,
 * a lane per row) lowers min_d2 against the newest seed - read through seed_row in device memory - and leaves the chunk sums; a
 * one-workgroup kernel walks them and the chosen chunk and stores the next seed.  No atomics, vector stores only: two
 * launches are bit-identical.  Squared distances that overflow f32 are outside the contract (never a fault).
 *   workspace: wgnn_kmeans_seed_workspace_bytes(n_rows, K) bytes, 8-byte aligned, caller-owned (8 bytes per chunk, 4 per row).
 * Errors, before any launch: WGNN_ERR_BAD_ARG (n_rows outside [1, 2^31); any flag bit - none is defined; a missing operand),
 * WGNN_ERR_UNSUPPORTED (K outside [1, 4096]: the cost is O(K n_rows D); D outside [4, 1024]), WGNN_ERR_ALIGNMENT (D or ld_x not a
 * multiple of 4 or ld_x < D; X not 16-byte, seed_row or min_d2 not 4-byte, workspace not 8-byte aligned), WGNN_ERR_WORKSPACE;
 * wgnn_last_error_string names the check.
 * ------------------------------------------------------------------------- */
int wgnn_kmeans_seed_workspace_bytes(int64_t n_rows, int32_t K, int64_t* bytes);
int wgnn_kmeans_seed(const float* X, int64_t ld_x, int64_t n_rows, int32_t D, int32_t K, uint64_t seed,
                     int32_t* seed_row, float* min_d2, void* workspace, int64_t workspace_bytes,
                     uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Per-group fp64 sums of dense f32 rows (additive exports, WGNN_VERSION stays 206): the update of a Lloyd step.
 *     X [n_rows, ld_x] f32 : the rows, D valid columns
 *     order int32 [n_rows], seg_ptr int64 [n_groups + 1] : the batch GROUP-MAJOR, as wgnn_group_class_reduce takes it - the
 *           rows of group k, ascending, in order[seg_ptr[k] .. seg_ptr[k+1]).  seg_ptr is clamped into [0, n_rows] and an entry
 *           of `order` outside [0, n_rows) takes no part (it is not counted either): a malformed operand never faults.
 *     sum f64 [n_groups, ld_sum], count int64 [n_groups] : every element of the first D columns is written
 *     mean f32 [n_groups, ld_mean], optional : (float)(sum / (double)count), one fp64 divide and one rounding; the row of a
 *           group with count == 0 is NOT written - what the caller had there stays, bit for bit
 * Addition order, part of the contract: a group's run is cut into chunks of 64 members; within a chunk the rows are added
 * sequentially in run order from 0.0, one fp64 accumulator per column; a second kernel adds a group's chunk partials
 * sequentially in chunk order from 0.0.  No atomics: the result depends on the operand alone, never on the grid.
 *   workspace: wgnn_group_rows_reduce_workspace(n_rows, n_groups, D) bytes, 8-byte aligned, caller-owned
 *   ((n_rows / 64 + n_groups) chunk partials of D doubles and one int32).
 * Errors, before any launch: WGNN_ERR_BAD_ARG (sum, count or seg_ptr missing; n_rows outside [0, 2^31); n_groups <= 0; D <= 0;
 * ld_x, ld_sum or ld_mean < D; any flag bit - none is defined), WGNN_ERR_UNSUPPORTED (D > 65536; a workspace beyond 2^63
 * bytes), WGNN_ERR_ALIGNMENT (sum, count, seg_ptr or workspace not 8-byte, X, order or mean not 4-byte aligned),
 * WGNN_ERR_WORKSPACE; wgnn_last_error_string names the check.  X or order NULL, or n_rows == 0: every group is empty.
 * ------------------------------------------------------------------------- */
int wgnn_group_rows_reduce_workspace(int64_t n_rows, int32_t n_groups, int32_t D, int64_t* bytes);
int wgnn_group_rows_reduce(const float* X, int64_t ld_x, const int32_t* order, const void* seg_ptr, int64_t n_rows,
                           int32_t n_groups, int32_t D, double* sum, int64_t ld_sum, int64_t* count,
                           float* mean, int64_t ld_mean, void* workspace, int64_t workspace_bytes,
                           uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Exact silhouette of dense rows under Euclidean distance (additive exports, WGNN_VERSION stays 206): the kernel behind
 * ops.silhouette_rows / api.ResidentPredictor.silhouette (Rousseeuw 1987).  Brute force over every ordered pair of rows,
 * O(n^2 D); the [n, n] distance matrix is never stored, and symmetry is not exploited.
 *     X [n, ld_x] f32        : the rows GROUP-MAJOR, D valid columns: group k holds the rows seg_ptr[k] .. seg_ptr[k+1] - 1
 *     seg_ptr int64 [K + 1]  : the groups' bounds; rows at positions >= seg_ptr[K] take no part - neither as queries nor as
 *                              candidates.  seg_ptr is clamped into [0, n]: a malformed operand never faults.
 *     n_splits               : the groups are dealt to this many workgroup columns (0 = chosen from n and K so that a small
 *                              batch still fills the chip); it changes no bit
 *     a, b, s f64 [n], nearest int32 [n] : per row, at its group-major position; every element is written
 * Definition, for a participating row i of group g (n_c = the members of group c):
 *     d2(i, j)  wgnn_knn_rows' chain:  d2 = 0;  for c = 0 .. D-1 ascending:  t = x_i[c] - x_j[c];  d2 = fmaf(t, t, d2)   (f32)
 *     d(i, j) = sqrtf(d2(i, j)), correctly rounded (f32);  d(i, i) = +0.0 exactly, so the row itself needs no exclusion
 *     S(i, c) = the fp64 sum of d(i, j) over the members j of group c, in the order below
 *     a(i)    = S(i, g) / (n_g - 1);  0.0 when n_g == 1
 *     b(i)    = the minimum over the non-empty groups c != g of S(i, c) / n_c  (one fp64 divide each)
 *     nearest(i) = the group that attains b(i) under the total order (mean, group id): of equal means the lower id
 *     s(i)    = (b - a) / max(a, b);  0.0 when n_g == 1 or max(a, b) == 0 (scikit-learn's conventions)
 *     with no other non-empty group: b = +inf, nearest = -1, s = NaN (also for a singleton)
 *   A row that takes no part gets a = b = s = NaN and nearest = -1.
 * Addition order of S(i, c), part of the contract and a constant of the kernel - it depends on neither the grid nor n_splits:
 *   the member at position p of its group (p = 0 for the row at seg_ptr[c]) goes to partial (p % 64) / 4; each of the 16 partials
 *   is summed sequentially in ascending p from 0.0; the 16 partials are then added as a balanced tree, partial u with partial
 *   u ^ 1, the results with those at u ^ 2, then u ^ 4, then u ^ 8.  (A group's members are cut into candidate tiles of 64 from
 *   the group's own start, a lane owns four consecutive candidates and carries one partial per query across the tiles; the 16
 *   lanes of a query meet in an xor butterfly.  A position past the group's end adds a selected +0.0.)
 * A workgroup of 256 threads holds 64 queries and streams the candidate tiles x 16 columns through 17 KiB of LDS; a lane owns
 * 4 x 4 pairs.  No atomics: two launches are bit-identical.  Distances that overflow f32 are outside the contract (never a
 * fault), and so are rows with a non-finite value (the caller leaves them out of the groups).
 *   workspace: wgnn_silhouette_workspace_bytes(n, K, n_splits) bytes, 8-byte aligned, caller-owned: the splits' group ranges
 *   and per split and row (S_own, best mean, its group), 20 bytes, which a second kernel merges under the same order; 0 bytes
 *   (workspace may be NULL) when the groups are not split.  Whole groups are dealt, in contiguous ranges balanced by their
 *   number of candidate tiles: one dominant group bounds the balance.
 * Errors, before any launch: WGNN_ERR_BAD_ARG (n outside [0, 2^31); n_splits outside [0, 64]; any flag bit - none is defined;
 * a missing operand), WGNN_ERR_UNSUPPORTED (K outside [1, 4096]; D outside [4, 1024]), WGNN_ERR_ALIGNMENT (D or ld_x not a
 * multiple of 4 or ld_x < D; X not 16-byte, seg_ptr, a, b, s or workspace not 8-byte, nearest not 4-byte aligned),
 * WGNN_ERR_WORKSPACE; wgnn_last_error_string names the check.  n == 0 returns WGNN_OK without a launch.
 * ------------------------------------------------------------------------- */
int wgnn_silhouette_workspace_bytes(int64_t n, int32_t K, int32_t n_splits, int64_t* bytes);
int wgnn_silhouette_rows(const float* X, int64_t ld_x, int64_t n, int32_t D, const void* seg_ptr, int32_t K,
                         int32_t n_splits, double* a, double* b, double* s, int32_t* nearest,
                         void* workspace, int64_t workspace_bytes, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Graph clusters in integers (additive exports, WGNN_VERSION stays 206): the kernels behind ops.snn_graph / ops.louvain_graph /
 * api.ResidentPredictor.louvain.  No floating point anywhere: every value is an int32 / int64 and every decision a comparison
 * of 64-bit integers, so neither the order of the integer atomics below nor the grid changes a bit.
 *
 * wgnn_snn_weights - the shared-neighbour weights of a kNN union graph.
 *     idx [n, ld_idx] int32 (int64 with WGNN_SNN_IDX_I64), k <= 64 valid columns: row i's neighbour list, -1 = none; an entry
 *         outside [0, n), the row itself and a repeated entry count as none
 *     rowptr int64 [n + 1], col int32 [nnz] : the symmetric CSR of the union graph ({i, j} is an edge iff one lists the other)
 *     w int32 [nnz] : w(i, j) = |N+(i) & N+(j)| with N+(i) = {i} + list(i) - at least 1 on a union edge, at most k + 1
 *   A wavefront takes a row, a lane an entry of its list; for every stored neighbour j the lanes load j's list and count.
 *
 * One sweep of a synchronous Louvain on a symmetric CSR with int32 weights (a diagonal entry = the internal weight of the
 * community a coarse vertex came from; it counts in deg and is skipped for kin).  resolution = num / den, M = the sum of all
 * stored weights, m_den = M * den; the caller guarantees M * M * max(num, den) < 2^62, below which no product here overflows.
 *   wgnn_louvain_sweep: every vertex v reads comm / tot / size as they were before the sweep.  kin[C] = the sum of w(v, u)
 *     over the neighbours u != v with comm[u] = C;
 *         score(C) = kin[C] * m_den - num * deg[v] * (tot[C] - (C == own ? deg[v] : 0))
 *     C != own is admissible iff (sweep even: C < own; odd: C > own), not (size[own] == 1 and size[C] == 1 and C > own), and
 *     score(C) > score(own) (kin[own] = 0 without a neighbour there).  next[v] = the admissible C that is best under (higher
 *     score, lower id), else comm[v]; gain[v] = score(next) - score(own), 0 for a vertex that stays.
 *     Rows of at most wave_rows (<= 128) entries are served by a wavefront and an LDS table of 256 slots keyed by the community
 *     id; the others are listed in heavy int32 [n_heavy]: up to block_rows (<= 2048) entries by a workgroup and an LDS table of
 *     4096 slots, beyond by a workgroup and its own dense int32 scratch [n] in `workspace`
 *     (wgnn_louvain_sweep_workspace_bytes(n, scratch_blocks): scratch_blocks <= 256 such workgroups; ZERO on entry, zero again
 *     on return).  wave_rows, block_rows and scratch_blocks change no bit.
 *   wgnn_louvain_apply: tot[c] = the sum of deg over label == c, size[c] = their number (both zeroed first; 64-bit integer
 *     atomics), stats[0] = how many vertices have old_label != label (0 with old_label NULL); stats[1], stats[2] = 0.
 *   wgnn_louvain_modularity: stats[1] += IN, the stored weight whose two ends share a label, the diagonal included;
 *     stats[2] += the sum of tot[c]^2.  Qnum = den * M * IN - num * stats[2];  Q = Qnum / (den * M^2).
 *   stats int64 [4]: [moved, IN, sum tot^2, status].  status is only ever OR-ed into (the caller zeroes it):
 * ------------------------------------------------------------------------- */
#define WGNN_SNN_IDX_I64          256   /* wgnn_snn_weights' flag: idx holds int64                                   */
#define WGNN_LOUVAIN_UNSORTED       1   /* a row is not strictly ascending in col                                    */
#define WGNN_LOUVAIN_BAD_COL        2   /* a column outside [0, n)                                                   */
#define WGNN_LOUVAIN_BAD_ROWPTR     4   /* rowptr does not ascend from 0 to nnz                                      */
#define WGNN_LOUVAIN_NO_SCRATCH     8   /* a row above block_rows entries met no scratch (scratch_blocks == 0)       */
#define WGNN_LOUVAIN_BAD_LABEL     16   /* a label / community id outside [0, n)                                     */
#define WGNN_LOUVAIN_BAD_WEIGHT    32   /* a negative weight                                                         */
/* Errors, before any launch: WGNN_ERR_BAD_ARG (a missing operand; n outside [0, 2^31); a negative nnz, sweep, n_heavy or
 * workspace size; ld_idx < k; m_den or num < 1; scratch_blocks outside [0, 256]; an unknown flag), WGNN_ERR_UNSUPPORTED (k outside
 * [1, 64]; wave_rows outside [0, 128]; block_rows outside [0, 2048]), WGNN_ERR_ALIGNMENT (64-bit operands not 8-byte, 32-bit
 * ones not 4-byte aligned), WGNN_ERR_WORKSPACE; wgnn_last_error_string names the check.  What only the entries of the graph can
 * show - unsorted rows, columns out of range - is reported through the status word by wgnn_louvain_modularity, and no kernel
 * reads or writes out of bounds on such a graph. */
int wgnn_snn_weights(const void* idx, int64_t ld_idx, int64_t n, int32_t k, const int64_t* rowptr, const int32_t* col,
                     int64_t nnz, int32_t* w, uint32_t flags, void* stream);
int wgnn_louvain_sweep_workspace_bytes(int64_t n, int32_t scratch_blocks, int64_t* bytes);
int wgnn_louvain_sweep(const int64_t* rowptr, const int32_t* col, const int32_t* w, int64_t n, int64_t nnz,
                       const int32_t* comm, const int64_t* deg, const int64_t* tot, const int32_t* size,
                       int64_t m_den, int64_t num, int32_t sweep, const int32_t* heavy, int32_t n_heavy,
                       int32_t wave_rows, int32_t block_rows, int32_t* next, int64_t* gain, int64_t* stats,
                       void* workspace, int64_t workspace_bytes, int32_t scratch_blocks, uint32_t flags, void* stream);
int wgnn_louvain_apply(const int32_t* old_label, const int32_t* label, const int64_t* deg, int64_t n, int64_t* tot,
                       int32_t* size, int64_t* stats, uint32_t flags, void* stream);
int wgnn_louvain_modularity(const int64_t* rowptr, const int32_t* col, const int32_t* w, int64_t n, int64_t nnz,
                            const int32_t* label, const int64_t* tot, int64_t* stats, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * The refinement of a deterministic, synchronous, integer Leiden (additive exports, WGNN_VERSION stays 206): the kernels that
 * ops.leiden_graph / api.ResidentPredictor.leiden add to the Louvain ones above.  Graph, resolution, M, m_den, deg, the guard
 * M * M * max(num, den) < 2^62 and the total orders are wgnn_louvain_sweep's; no floating point, no random number.
 *     P   int32 [n] : the partition the moving phase left (ids in [0, n)); totP int64 [n] = the sum of deg over P == c
 *     ref int32 [n] : the refined partition inside P.  A refined community's id is the id of the vertex that founded it, so
 *         P[ref[v]] == P[v]; the refinement starts from ref = identity.  tot / size int64 / int32 [n]: wgnn_louvain_apply's of ref
 *   wgnn_leiden_boundary: kinP[v] = the sum of w(v, u) over the stored u != v with P[u] == P[v] (kinP may be NULL: not wanted);
 *     ext[S] = the sum of w(u, x) over the stored off-diagonal entries with ref[u] == S, P[x] == P[u] and ref[x] != S (zeroed
 *     first; one 64-bit integer atomic per row).
 *   wgnn_leiden_refine_sweep: every vertex reads the state before the sweep.  v MAY MOVE iff size[ref[v]] == 1 and
 *         kinP[v] * m_den >= num * deg[v] * (totP[P[v]] - deg[v])
 *     kin[S] = the sum of w(v, u) over u != v with P[u] == P[v] and ref[u] == S;  score(S) = kin[S] * m_den - num * deg[v] * tot[S].
 *     S != ref[v] is admissible iff (sweep even: S < ref[v]; odd: S > ref[v]),
 *         ext[S] * m_den >= num * tot[S] * (totP[P[v]] - tot[S])
 *     and score(S) > 0.  prop[v] = the admissible S that is best under (higher score, lower id), gain[v] = its score; a vertex
 *     that may not move or has no admissible S leaves prop[v] = ref[v], gain[v] = 0.  ext, tot and kinP are at most M, so every
 *     product stays below 2^62.  heavy, wave_rows, block_rows, the workspace (wgnn_louvain_sweep_workspace_bytes; ZERO on entry,
 *     zero again on return) and scratch_blocks are wgnn_louvain_sweep's: the same tables, the same three routes, no bit changed.
 *   wgnn_leiden_accept: next[v] = prop[v] iff prop[prop[v]] == prop[v] - the vertex whose id is the target's label stays at
 *     home - else next[v] = ref[v] and gain[v] = 0.  stats[0] = how many vertices have next != ref (set, not added to).  An
 *     accepted target keeps every member it had and every vertex that joins it is adjacent to one of them, so a refined
 *     community is connected.  Runs behind the sweep on the same stream with no read-back between them.
 *   stats int64 [4] as above; the status word takes the WGNN_LOUVAIN_* bits and
 * ------------------------------------------------------------------------- */
#define WGNN_LEIDEN_BAD_PARTITION  64   /* a ref / P id outside [0, n), or a ref label whose founder lies in another P-community */
/* Errors, before any launch: as for the Louvain entries.  No kernel reads or writes out of bounds on a malformed graph or
 * partition: an id outside [0, n) is skipped and reported. */
int wgnn_leiden_boundary(const int64_t* rowptr, const int32_t* col, const int32_t* w, int64_t n, int64_t nnz,
                         const int32_t* P, const int32_t* ref, int64_t* ext, int64_t* kinP, int64_t* stats,
                         uint32_t flags, void* stream);
int wgnn_leiden_refine_sweep(const int64_t* rowptr, const int32_t* col, const int32_t* w, int64_t n, int64_t nnz,
                             const int32_t* P, const int32_t* ref, const int64_t* deg, const int64_t* totP,
                             const int64_t* tot, const int32_t* size, const int64_t* ext, const int64_t* kinP,
                             int64_t m_den, int64_t num, int32_t sweep, const int32_t* heavy, int32_t n_heavy,
                             int32_t wave_rows, int32_t block_rows, int32_t* prop, int64_t* gain, int64_t* stats,
                             void* workspace, int64_t workspace_bytes, int32_t scratch_blocks, uint32_t flags, void* stream);
int wgnn_leiden_accept(const int32_t* ref, const int32_t* prop, int64_t n, int32_t* next, int64_t* gain, int64_t* stats,
                       uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * The fuzzy kNN graph and a synchronous 2-D layout (additive exports, WGNN_VERSION stays 206): the kernels behind
 * ops.fuzzy_graph / ops.layout_graph / api.ResidentPredictor.umap.  Every floating-point operation named here is rounded on its
 * own (no fused multiply-add), every sum runs in the stated order and nothing depends on the grid: two calls give the same bits.
 *
 * wgnn_fuzzy_rows - the memberships of each row's own neighbour list (UMAP's smooth kNN distances, local_connectivity = 1).
 *     idx [n, ld_idx] int32 (int64 with WGNN_FUZZY_IDX_I64) and d2 [n, ld_d2] float32, k <= 64 valid columns, as wgnn_knn_rows
 *         leaves them; an entry is LISTED iff idx >= 0 and d2 is finite
 *     target = log2(k + 1), passed by the host
 *   Per row: d_j = sqrtf(d2_j) in float32, all that follows in float64.  rho = the smallest d_j > 0 (0 without one);
 *   x_j = d_j - rho;  p(s) = the sum over the listed j, in list order, of (x_j > 0 ? exp(-x_j / s) : 1).  From lo = 0, hi = inf,
 *   s = 1, exactly 64 times: p(s) > target ? (hi = s, s = (lo + hi) / 2) : (lo = s, s = hi == inf ? 2 s : (lo + hi) / 2).  Then
 *   sigma = max(s, 1e-3 * mean_j d_j) (the mean over the listed entries, summed in list order) and
 *   member_j = (float)(x_j > 0 ? exp(-x_j / sigma) : 1) for a listed entry, 0 for another.
 *     rho, sigma float64 [n]; member float32 [n, k] (dense).  A row with nothing listed: rho = sigma = 0, members 0.
 *
 * wgnn_fuzzy_union - the weights of the symmetric union graph (set_op_mix_ratio = 1).
 *     rowptr int64 [n + 1], col int32 [nnz]: the union CSR (ops.snn_graph's); idx / member as above
 *   For the stored edge (i, c): p = member[i, t] at the first t with idx[i, t] == c (0 without one), q the same with i and c
 *   swapped;  w = (p + q) - p * q, three float32 operations - so w(i, c) and w(c, i) are the same bits.  A column outside [0, n)
 *   gives 0.
 *
 * wgnn_layout_init - the "hash" start: y[t] = ((float)(h >> 40) * 2^-24) * 20 - 10 in float32, in [-10, 10), with
 *     h = mix64(mix64(((u64)seed << 32) | 0xFFFFFFFF) + t) for t = 2 * vertex + component (mix64: the splitmix64 finaliser).
 *
 * wgnn_layout_epoch - epoch `epoch` of n_epochs: reads y_in, writes y_out (another buffer), float32 [n, 2].
 *   The directed edge at CSR position e of vertex i, other end j:  r = w[e] / wmax;  it FIRES iff
 *   floorf((float)(epoch + 1) * r) != floorf((float)epoch * r) - both directions of an undirected edge in the same epochs.
 *   A firing edge adds, in this order, with dx = y_i - y_j, q = dx0 * dx0 + dx1 * dx1 and qb = q^b:
 *     the attraction, if q > 0:  c = (((-2 * a) * b) * qb / q) / (1 + a * qb);  g = clamp(c * dx, -4, 4) per component
 *     for s = 0 .. n_neg - 1 a repulsion from vertex t = ((h >> 32) * n) >> 32,
 *       h = mix64(mix64(((u64)seed << 32) | epoch) + e * n_neg + s), if t != i and (dx = y_i - y_t) q > 0:
 *       c = ((2 * gamma) * b) / ((0.001f + q) * (1 + a * qb));  g = clamp(c * dx, -4, 4)
 *   An edge that does not fire adds nothing (no negatives either).  qb = q itself when b == 1.0f, else
 *   (float)pow((double)q, (double)b).  WGNN_LAYOUT_LANES lanes serve a vertex: lane (e - rowptr[i]) % 16 adds its edges' terms in
 *   e order to its partial G (from +0), and the partials fold by halves (lane l += lane l + 8, then 4, 2, 1).
 *   y_out_i = y_i + alpha * G_i (one multiply, one add per component); a vertex without a stored edge copies its position.
 *   fired int64 [n] (optional): fired[i] += the number of i's edges that fired.  No atomics, no workspace.
 * ------------------------------------------------------------------------- */
#define WGNN_FUZZY_IDX_I64        256   /* wgnn_fuzzy_rows' / wgnn_fuzzy_union's flag: idx holds int64               */
#define WGNN_LAYOUT_LANES          16   /* lanes per vertex: part of wgnn_layout_epoch's sum order                   */
#define WGNN_LAYOUT_MAX_EPOCHS  10000   /* (float)epoch is exact far beyond; the schedule is the caller's            */
#define WGNN_LAYOUT_MAX_NEG        64
/* Errors, before any launch: WGNN_ERR_BAD_ARG (a missing operand; n outside [0, 2^31); a negative nnz; ld < k; a target, wmax, a,
 * b, gamma or alpha that is not finite, target or wmax not positive; epoch outside [0, n_epochs), n_epochs outside [1, 10000];
 * n_neg outside [0, 64]; y_out == y_in; an unknown flag), WGNN_ERR_UNSUPPORTED (k outside [1, 64]), WGNN_ERR_ALIGNMENT (64-bit
 * operands and the positions not 8-byte, 32-bit ones not 4-byte aligned); wgnn_last_error_string names the check.  No kernel reads
 * or writes out of bounds on a malformed graph: rowptr is clamped to [0, nnz] and a column outside [0, n) is skipped. */
int wgnn_fuzzy_rows(const void* idx, int64_t ld_idx, const float* d2, int64_t ld_d2, int64_t n, int32_t k, double target,
                    double* rho, double* sigma, float* member, uint32_t flags, void* stream);
int wgnn_fuzzy_union(const void* idx, int64_t ld_idx, const float* member, int64_t n, int32_t k, const int64_t* rowptr,
                     const int32_t* col, int64_t nnz, float* w, uint32_t flags, void* stream);
int wgnn_layout_init(float* y, int64_t n, uint32_t seed, uint32_t flags, void* stream);
int wgnn_layout_epoch(const int64_t* rowptr, const int32_t* col, const float* w, int64_t n, int64_t nnz, float wmax,
                      const float* y_in, float* y_out, int32_t epoch, int32_t n_epochs, float a, float b, float gamma,
                      float alpha, int32_t n_neg, uint32_t seed, int64_t* fired, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Geodesic distances on a graph (additive export, WGNN_VERSION stays 206): the kernel behind ops.geodesic_rows /
 * api.ResidentPredictor.pseudotime - one round of a SYNCHRONOUS Bellman-Ford over float32 edge lengths.  The only floating-point
 * operation is one float32 add per stored entry, rounded on its own; everything else is a comparison.  Nothing depends on the
 * grid or on the order of the threads: two calls give the same bits, and numpy restates a round exactly.
 *     rowptr int64 [n + 1], col int32 [nnz] strictly ascending within a row, length float32 [nnz] >= 0 and finite: a CSR that
 *         stores both directions of every edge (ops.distance_graph's); row v lists the u that can hand v a distance
 *     dist_in float32 [n] (+inf = not reached), pred_in int32 [n] (-1 = a root or not reached): the state before the round
 *     dist_out, pred_out : the state after it - other buffers than dist_in / pred_in (the caller swaps them: ping-pong)
 *   For every vertex v:  cand(u) = dist_in[u] + length(u, v) in float32 for every stored neighbour u whose dist_in[u] is finite;
 *   best = the least under the total order (cand, u).  If best.cand < dist_in[v] (strictly) then dist_out[v] = best.cand and
 *   pred_out[v] = best.u, else both are copied.  A vertex that is reached never loses its predecessor to an equal candidate, and
 *   a round at the fixed point is the identity.
 *   *changed (int64) += the number of vertices the round improved (one 64-bit integer atomic per wavefront that has any: the
 *   caller hands every round of a batch its own zeroed slot and reads them back together); *status (int64) is only ever OR-ed
 *   into (the caller zeroes it) with the bits below.  No atomic touches dist or pred.
 *   WGNN_GEODESIC_LANES lanes serve a row - lane l its entries l, l + 16, ... - and fold their partial minima by halves; rows are
 *   taken in a grid-stride loop by min(grid_blocks, ceil(n / 16)) workgroups of 256 (grid_blocks == 0: at most
 *   WGNN_GEODESIC_MAX_BLOCKS).  The minimum of a total order is associative and commutative: neither changes a bit.
 * ------------------------------------------------------------------------- */
#define WGNN_GEODESIC_LANES        16   /* lanes per row                                                             */
#define WGNN_GEODESIC_MAX_BLOCKS 8192   /* the largest grid                                                          */
#define WGNN_GEODESIC_UNSORTED      1   /* a row is not strictly ascending in col                                    */
#define WGNN_GEODESIC_BAD_COL       2   /* a column outside [0, n): the entry is skipped                             */
#define WGNN_GEODESIC_BAD_ROWPTR    4   /* rowptr does not ascend from 0 to nnz: the row is clamped to [0, nnz]      */
#define WGNN_GEODESIC_BAD_LENGTH    8   /* a negative, infinite or NaN length: the entry is skipped                  */
/* Errors, before any launch: WGNN_ERR_BAD_ARG (a missing operand; n outside [0, 2^31); a negative nnz; grid_blocks outside
 * [0, 8192]; dist_out == dist_in or pred_out == pred_in; any flag bit - none is defined), WGNN_ERR_ALIGNMENT (rowptr, changed or
 * status not 8-byte, the others not 4-byte aligned); wgnn_last_error_string names the check.  n == 0 returns WGNN_OK without a
 * launch.  No kernel reads or writes out of bounds on a malformed graph. */
int wgnn_geodesic_round(const int64_t* rowptr, const int32_t* col, const float* length, int64_t n, int64_t nnz,
                        const float* dist_in, const int32_t* pred_in, float* dist_out, int32_t* pred_out,
                        int64_t* changed, int64_t* status, int32_t grid_blocks, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * The diffusion operator of a graph and a Lanczos iteration on it (additive exports, WGNN_VERSION stays 206): the kernels behind
 * ops.diffusion_operator / ops.lanczos_graph / ops.basis_combine / ops.diffusion_distance and api.ResidentPredictor.diffmap / dpt.
 * All arithmetic is float64; every operation named here is rounded on its own (no fused multiply-add), every sum runs in the
 * stated order and nothing depends on the grid: two calls give the same bits, and numpy restates every entry exactly.
 *     rowptr int64 [n + 1], col int32 [nnz] strictly ascending within a row: a CSR that stores both directions of every edge
 *         (ops.fuzzy_graph's), with w float32 [nnz] >= 0 and finite, or t float64 [nnz] >= 0 and finite
 *   A ROW SUM is wgnn_layout_epoch's: WGNN_DIFFUSION_LANES lanes serve a row, lane l adds the row's entries l, l + 16, ... in
 *   order from +0.0, and the partials fold by halves (lane l += lane l + 8, then 4, 2, 1).
 *   A DOT of two vectors of n elements: chunks of WGNN_LANCZOS_CHUNK consecutive elements; within a chunk element s gives one
 *   rounded product (+0.0 past n) and the 256 values fold by halves (p[s] += p[s + 128], then 64, ..., 1); the chunks' values are
 *   added in ascending chunk order from +0.0.
 *
 * wgnn_diffusion_degree  - q == null: out_i = the row sum of (double)w_ij.  With q float64 [n]: out_i = sqrt(row sum of K_ij),
 *     K_ij = (double)w_ij / (q_i * q_j); an entry with w == 0 adds +0.0 without a division.  An empty row gives 0.
 * wgnn_diffusion_weights - t_ij = K_ij / (z_i * z_j) with z float64 [n], +0.0 where w == 0: scanpy's density-normalised symmetric
 *     transition matrix.  Both products are commutative, so t_ij and t_ji are the same bits.
 * wgnn_lanczos_init      - w0_i = mask_i ? z_i : 0 and w1_i = mask_i ? ((double)(h >> 11) * 2^-53) * 2 - 1 : 0, in [-1, 1), with
 *     h = mix64(mix64(((u64)seed << 32) | 0xFFFFFFFE) + i) (wgnn_layout_init's hash, its own key word); mask uint8 [n].
 * wgnn_lanczos_apply     - y_i = the row sum of t_ij * x_j (each product rounded); y another buffer than x.
 * wgnn_lanczos_dots      - c[r] = the dot of V[r, :] and w for r = 0 .. n_rows - 1; V float64 [n_rows, ld], a basis vector per
 *     row.  A workgroup takes a chunk for all rows; workspace holds one float64 per (chunk, row)
 *     (wgnn_lanczos_dots_workspace_bytes).  *keep (optional) = c[n_rows - 1].  With WGNN_LANCZOS_NORM: V is null, n_rows 1, and
 *     c[0] = sqrt(the dot of w with itself); if that is not above WGNN_LANCZOS_BREAKDOWN (a NaN is not) *halt = tag.
 * wgnn_lanczos_update    - w_i = w_i - V[r, i] * c[r] for r = 0 .. n_rows - 1 ascending (a product and a subtraction each).
 * wgnn_lanczos_scale     - v_i = w_i / *beta (a division; beta float64 on the device).
 *   halt (int64 on the device, optional; 0 = running): apply, dots, update and scale return at once, writing nothing, when they
 *   find it set - a step enqueued behind a breakdown is inert - and only a norm sets it.  No read-back is needed inside a step.
 * wgnn_basis_combine     - Y[i, 0] = V[0, i];  Y[i, c] = sum_{j = 1 .. m} V[j, i] * S[j - 1, c - 1] for c = 1 .. n_cols, j ascending
 *     from +0.0 (a product and an add each); S float64 [m, lds] and Y float64 [n, ldy] on the device.
 * wgnn_diffusion_distance - d_i = min over the roots r of sqrt(sum_{l = 1 .. n_dcs - 1} (g_l * (Y[r, l] - Y[i, l]))^2), l
 *     ascending from +0.0; roots int64 [n_roots], one outside [0, n) is skipped; a NaN distance stays.  g float64 [n_dcs].
 *
 *   *status (int64) is only ever OR-ed into (the caller zeroes it) with the bits below, by degree, weights and apply; no other
 *   atomic is used.  No kernel reads or writes out of bounds on a malformed graph: a row is clamped to [0, nnz], a column
 *   outside [0, n) and a bad weight are skipped (weights writes +0.0 there).
 * ------------------------------------------------------------------------- */
#define WGNN_DIFFUSION_LANES        16   /* lanes per row: part of the row sum's order                                */
#define WGNN_DIFFUSION_MAX_BLOCKS 8192   /* the largest grid                                                          */
#define WGNN_DIFFUSION_MAX_COMPS    64   /* the most components (the stationary one included)                         */
#define WGNN_DIFFUSION_UNSORTED      1   /* a row is not strictly ascending in col                                    */
#define WGNN_DIFFUSION_BAD_COL       2   /* a column outside [0, n): the entry is skipped                             */
#define WGNN_DIFFUSION_BAD_ROWPTR    4   /* rowptr does not ascend from 0 to nnz: the row is clamped to [0, nnz]      */
#define WGNN_DIFFUSION_BAD_WEIGHT    8   /* a negative, infinite or NaN w or t: the entry is skipped                  */
#define WGNN_LANCZOS_CHUNK         256   /* elements per chunk: part of the dot's order                               */
#define WGNN_LANCZOS_MAX_STEPS    1024   /* V holds at most 1025 rows                                                 */
#define WGNN_LANCZOS_NORM          256   /* wgnn_lanczos_dots' flag: the norm of w                                    */
#define WGNN_LANCZOS_BREAKDOWN 0x1p-26   /* a norm at or below this halts the run                                     */
/* Errors, before any launch: WGNN_ERR_BAD_ARG (a missing operand; n outside [0, 2^31); a negative nnz; grid_blocks outside
 * [0, 8192]; ld < n; n_rows outside [1, 1025]; m outside [0, 1024]; n_cols outside [0, 63]; n_dcs outside [2, 64]; n_roots < 1;
 * tag == 0; an output that is, or lies inside, an input; an unknown flag), WGNN_ERR_WORKSPACE (a workspace smaller than asked
 * for), WGNN_ERR_ALIGNMENT (64-bit operands not 8-byte, 32-bit ones not 4-byte aligned); wgnn_last_error_string names the check.
 * n == 0 returns WGNN_OK without a launch. */
int wgnn_diffusion_degree(const int64_t* rowptr, const int32_t* col, const float* w, int64_t n, int64_t nnz, const double* q,
                          double* out, int64_t* status, int32_t grid_blocks, uint32_t flags, void* stream);
int wgnn_diffusion_weights(const int64_t* rowptr, const int32_t* col, const float* w, int64_t n, int64_t nnz, const double* q,
                           const double* z, double* t, int64_t* status, int32_t grid_blocks, uint32_t flags, void* stream);
int wgnn_lanczos_init(const double* z, const uint8_t* mask, int64_t n, uint32_t seed, double* w0, double* w1, uint32_t flags,
                      void* stream);
int wgnn_lanczos_apply(const int64_t* rowptr, const int32_t* col, const double* t, int64_t n, int64_t nnz, const double* x,
                       double* y, const int64_t* halt, int64_t* status, int32_t grid_blocks, uint32_t flags, void* stream);
int64_t wgnn_lanczos_dots_workspace_bytes(int64_t n, int32_t n_rows);
int wgnn_lanczos_dots(const double* V, int64_t ld, int32_t n_rows, const double* w, int64_t n, double* c, double* keep,
                      int64_t* halt, int64_t tag, void* workspace, int64_t workspace_bytes, int32_t grid_blocks,
                      uint32_t flags, void* stream);
int wgnn_lanczos_update(const double* V, int64_t ld, int32_t n_rows, const double* c, double* w, int64_t n,
                        const int64_t* halt, int32_t grid_blocks, uint32_t flags, void* stream);
int wgnn_lanczos_scale(const double* w, const double* beta, double* v, int64_t n, const int64_t* halt, int32_t grid_blocks,
                       uint32_t flags, void* stream);
int wgnn_basis_combine(const double* V, int64_t ld, int32_t m, const double* S, int64_t lds, int32_t n_cols, double* Y,
                       int64_t ldy, int64_t n, uint32_t flags, void* stream);
int wgnn_diffusion_distance(const double* Y, int64_t ldy, int64_t n, const double* g, int32_t n_dcs, const int64_t* roots,
                            int32_t n_roots, double* d, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Harmony (Korsunsky et al. 2019) on dense rows (additive exports, WGNN_VERSION stays 206): the kernels behind ops.harmony_rows
 * and api.ResidentPredictor.harmony.  All arithmetic is float64; every operation named here is rounded on its own (no fused
 * multiply-add), every sum runs in the stated order, which the data alone fix: nothing depends on the grid, there is no atomic,
 * two calls give the same bits, and numpy restates every entry (bit for bit where no exp / pow / log takes part).
 *     B cells, D columns, K clusters, S batches;  b_i int32 in [0, S): a cell's batch;  unit(z) = z / sqrt(sum_j z_j^2), j ascending
 *     U = unit(Z0) [B, D];  Y [K, D] unit centres;  R, dist, e [B, K] contiguous;  T [n_blocks, K, S];  O, E, pen [K, S];
 *     M [K, S, D], n [K, S];  Pr_s = N_s / B;  theta [S];  block q = { i : i mod n_blocks == q }, member m of it is cell q + m n_blocks
 *
 * wgnn_harmony_scores        - dot_ik = sum_j U_ij Y_kj (a product and an add each, j ascending from +0.0), dist_ik = 2 (1 - dot_ik),
 *     a_ik = -dist_ik / sigma, e_ik = exp(a_ik - max_k a_ik).  dot is optional.
 * wgnn_harmony_assign_block  - for the members of block q: t_ik = e_ik * pen[k, b_i] (pen == null: t = e), R_ik = t_ik / sum_k t_ik
 *     with k ascending from +0.0.  It also leaves, in the workspace, one [K, S] table per chunk of WGNN_HARMONY_T_CHUNK members:
 *     P[c, k, s] = the sum of R_ik over the chunk's members with b_i = s, members ascending from +0.0.
 * wgnn_harmony_fold          - one workgroup.  q_store >= 0: T[q_store] = sum_c P[c], c ascending from +0.0 (an empty block: +0.0).
 *     Then O = sum of T[q'] over q' != q_skip, q' ascending from +0.0 (q_skip = -1: over all), E_ks = (sum_s O_ks) * Pr_s with s
 *     ascending, and, where pen is given, pen_ks = pow((E_ks + 1) / (O_ks + 1), theta_s).  The sum without a block replaces
 *     Harmony's remove-and-add-back of a block, which drifts.
 * wgnn_weighted_group_reduce - M[k, s, :] = sum of R_ik * X_i over the rows of group s and n[k, s] = the sum of R_ik (a product and
 *     an add each).  order int32 [B] / seg_ptr int64 [S + 1]: the rows group-major, ascending within a group.  A group's rows are
 *     cut into chunks of WGNN_HARMONY_W_CHUNK, a chunk is added in order from +0.0, then the chunks in order from +0.0.  With S = 1
 *     and X = U these are the centres before unit().
 * wgnn_harmony_objective     - out[1] = sum R_ik dist_ik, out[2] = sum R_ik log R_ik (0 where R_ik = 0), out[3] = sum R_ik (theta_b
 *     log((O_kb + 1) / (E_kb + 1))) with b = b_i; out[0] = (out[1] + sigma out[2]) + sigma out[3].  A row adds its terms k ascending,
 *     WGNN_HARMONY_OBJ_CHUNK consecutive rows are added in row order, then the chunks in order, each from +0.0.
 * wgnn_harmony_apply         - Zc_i = Z0_i - sum_k R_ik W[k, b_i, :] (k ascending from +0.0) and U_i = unit(Zc_i).  R == null:
 *     U_i = unit(Z0_i) alone (Zc, W and batch are not read).  A zero row gives NaN: the caller checks.
 *   A batch id outside [0, S) reads nothing out of bounds: the cell gets pen = 1, no correction, and takes no part in T or the
 *   objective (ops refuses such ids before any launch).
 * ------------------------------------------------------------------------- */
#define WGNN_HARMONY_MAX_K        256   /* clusters                                                                   */
#define WGNN_HARMONY_MAX_BATCHES   64   /* batches                                                                    */
#define WGNN_HARMONY_MAX_D       1024   /* columns                                                                    */
#define WGNN_HARMONY_MAX_BLOCKS    64   /* blocks of a sweep                                                          */
#define WGNN_HARMONY_T_CHUNK       64   /* members per partial table: part of T's order                               */
#define WGNN_HARMONY_W_CHUNK      256   /* rows per partial moment: part of M's and n's order                         */
#define WGNN_HARMONY_OBJ_CHUNK    256   /* rows per partial objective: part of its order                              */
/* Errors, before any launch: WGNN_ERR_BAD_ARG (a missing operand; n_rows outside [1, 2^31); sigma not positive and finite; q,
 * q_store or q_skip outside its range; ld < D; grid_blocks outside [0, 65536]; an unknown flag), WGNN_ERR_UNSUPPORTED (K outside
 * [1, 256], S outside [1, 64], D outside [1, 1024], n_blocks outside [1, 64]), WGNN_ERR_WORKSPACE (a workspace smaller than asked
 * for), WGNN_ERR_ALIGNMENT (64-bit operands not 8-byte, 32-bit ones not 4-byte aligned); wgnn_last_error_string names the check. */
int wgnn_harmony_scores(const double* U, int64_t ld_u, const double* Y, int64_t ld_y, int64_t n_rows, int32_t D, int32_t K,
                        double sigma, double* dot, double* dist, double* e, uint32_t flags, void* stream);
int wgnn_harmony_assign_workspace_bytes(int64_t n_rows, int32_t K, int32_t S, int32_t n_blocks, int64_t* bytes);
int wgnn_harmony_assign_block(const double* e, const int32_t* batch, const double* pen, int64_t n_rows, int32_t K, int32_t S,
                              int32_t n_blocks, int32_t q, double* R, void* workspace, int64_t workspace_bytes,
                              int32_t grid_blocks, uint32_t flags, void* stream);
int wgnn_harmony_fold(const void* workspace, int64_t workspace_bytes, int64_t n_rows, double* T, const double* Pr,
                      const double* theta, int32_t K, int32_t S, int32_t n_blocks, int32_t q_store, int32_t q_skip, double* O,
                      double* E, double* pen, uint32_t flags, void* stream);
int wgnn_weighted_group_reduce_workspace_bytes(int64_t n_rows, int32_t K, int32_t S, int32_t D, int64_t* bytes);
int wgnn_weighted_group_reduce(const double* X, int64_t ld_x, const double* R, const int32_t* order, const void* seg_ptr,
                               int64_t n_rows, int32_t D, int32_t K, int32_t S, double* M, double* n, void* workspace,
                               int64_t workspace_bytes, int32_t grid_blocks, uint32_t flags, void* stream);
int wgnn_harmony_objective_workspace_bytes(int64_t n_rows, int64_t* bytes);
int wgnn_harmony_objective(const double* R, const double* dist, const int32_t* batch, const double* O, const double* E,
                           const double* theta, int64_t n_rows, int32_t K, int32_t S, double sigma, double* out,
                           void* workspace, int64_t workspace_bytes, uint32_t flags, void* stream);
int wgnn_harmony_apply(const double* Z0, int64_t ld_z, const double* R, const double* W, const int32_t* batch, int64_t n_rows,
                       int32_t D, int32_t K, int32_t S, double* Zc, double* U, int32_t grid_blocks, uint32_t flags,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WGNN_H_ */
