// wgnn_align.hip - wgnn_align_count / wgnn_align_fill: a batch over the CALLER's gene list (a dense [B, n_cols] matrix or a CSR
// over the caller's columns) made into the clean bundle-vocabulary CSR the resident kernels take (api.ResidentPredictor.align).
//
//   entry (r, j) with value v is kept  iff  gene_map[j] >= 0  &&  v > threshold          (api._read_test_csr's comparison: a NaN
//   is dropped), and leaves as (gene_map[j], v) - the same bits - in the row's INPUT order.
//
// Why before the kernels and not inside their gather: deg and S of wgnn_predict_rows are the row length and the row sum over
// the bundle's genes only (reference preprocess.py:160-161 drops the other columns first), and that kernel sums a row in CSR
// order - so the selection is stable and the values are copied, never recomputed.
//
// Layout: one wavefront per row, grid-stride over the batch (as wgnn_predict_rows).  A step takes 64 consecutive entries, one
// per lane; the keep mask is one wave ballot, the row's count grows by its popcount and a kept lane's slot is the running base
// plus the popcount of the mask below the lane (v_mbcnt).  COUNT and FILL are the same walk: count stores base at the end of the
// row, fill starts base at out_rowptr[r] (the exclusive scan of the counts) and stores (gene, value) at the slot.  No atomics on
// the data path, no LDS, a slot depends on the row alone: two launches are bit-identical.
// Dense rows are the bandwidth-bound case (the whole matrix is read in both passes).  With 16-byte aligned rows (x and gene_map
// 16-byte aligned, ld % 4 == 0) a lane takes 4 consecutive columns per load, kVecAhead such loads of x and of gene_map in flight:
// the slot of (lane, component c) is base + the kept entries of lower lanes (four mbcnt, one per component's ballot) + the kept
// lower components of the lane itself - lane-major, component-minor, which IS column order.  Other dense operands and the CSR
// form take one entry per lane and load, kAhead in flight; the CSR form's gene_map[col] is a dependent gather (L2: the map is
// n_cols * 4 bytes).
// Never a fault: a CSR entry whose col is outside [0, n_cols) is not looked up, a gene_map value outside [-1, n_genes) is not
// stored; both are skipped and raise a bit in the caller's status word (an ordinary global atomic OR, off the data path).
//
// Log-normalising walk (wgnn_align_count_ln / wgnn_align_fill_ln, the LN instantiation of the same kernel): the operand holds
// raw counts, total[r] is the fp64 sum of the caller's WHOLE row, and a candidate - a mapped column
// with a finite count > 0 - becomes v = float(log1p(double(x) / total * scale)) before the keep test `v > threshold`; what is
// no candidate becomes 0 and fails that test (threshold >= 0).  log1p in fp64 costs on the order of a hundred instructions a
// wave, and a dense row is mostly zeros: the candidates of the 256 entries a wave holds in flight are packed into consecutive
// slots of a 1 KB LDS slab (ballot + mbcnt, as the output slots), evaluated 64 at a time by consecutive lanes, and read back -
// one round where a lane-per-column evaluation would take four.  COUNT and FILL run the same instructions on the same slab
// order, so they agree on every keep decision.  The total: COUNT reads the row twice - first every column into the sum (a lane
// adds its columns in ascending order, the 64 partial sums fold in a fixed butterfly; no atomics), storing it for FILL, then the
// walk.  Measured once against a launch of its own for the totals (profiles/resident_lognorm.md): no difference in kernel time
// that the run resolves (the normalising walk is bound by its fp64 arithmetic), so the launch was saved.  The summing read sees every column, so it is where a count that is negative, NaN or infinite is
// skipped and reported (WGNN_ALIGN_BAD_VALUE).

#include <math.h>
#include "wgnn_common.h"
#include "wgnn_align_rows.h"

namespace {
using namespace wgnn;

constexpr int kAWaves = 8;                    // waves per workgroup, as the predict kernel
constexpr int kABlock = 64 * kAWaves;
constexpr int kAMaxBlocks = 1024;             // 256 CUs x 4 workgroups: grid-stride beyond that
// kAhead / kVecAhead (steps in flight per wave) and the FORM_* operand forms: wgnn_align_rows.h

struct AArgs {
    const float* x; long ld;                                   // dense
    const void* rowptr; const int* col; const float* val;      // CSR over the caller's columns
    long n_rows; int n_cols;
    const int* gene_map; int n_genes; float thr;
    int* row_count;                                            // COUNT
    const long long* out_rowptr; int* out_col; float* out_raw; // FILL
    int* status;
    const double* total; double scale;                         // LN: the row totals (FILL reads them), Seurat's scale.factor
    const double* lib; double* total_out;                      // LN COUNT: the caller's library sizes (or null), the totals it stores
};

// keep test of one entry; `on` = the lane holds an entry of the row.  A map value outside [-1, n_genes) is reported, not kept.
__device__ __forceinline__ bool keep_entry(const AArgs& a, bool on, int g, float v, unsigned& bad) {
    if (on && (g < -1 || g >= a.n_genes)) { bad |= WGNN_ALIGN_BAD_MAP; return false; }
    return on && g >= 0 && v > a.thr;
}

// FILL's store.  out_rowptr that is not the scan of COUNT's result over the same operand would send a slot past the row's
// room: such an entry is dropped and reported, never written.
__device__ __forceinline__ void put(const AArgs& a, long s, long room, int g, float v, unsigned& bad) {
    if (s < room) { a.out_col[s] = g; a.out_raw[s] = v; }
    else bad |= WGNN_ALIGN_BAD_ROWPTR;
}

// LN: the definition's value is lognorm() of wgnn_align_rows.h (wgnn_predict_rows_thin evaluates the same function)

// LN: the wave's candidates among the 4 entries per lane it holds (c[k]) become their log-normalised values, every other entry
// 0.  Candidates are packed into the wave's slab (k-major, lane-minor), consecutive lanes evaluate consecutive slots, and each
// candidate reads its slot back; the fences order the slab's writes and reads among the lanes of this one wave.
__device__ __forceinline__ void lognorm_group(float* slab, int lane, float (&x)[4], const bool (&c)[4], double total, double scale) {
    int pos[4], n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long m = __ballot(c[k]);
        pos[k] = n + below(m);
        n += __popcll(m);
    }
    if (n == 0) {                                                // wave-uniform: no candidate, the slab is not touched
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = 0.f;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (c[k]) slab[pos[k]] = x[k];                           // pos < n <= 256
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < n; i += 64) slab[i] = lognorm(slab[i], total, scale);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = c[k] ? slab[pos[k]] : 0.f;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// LN COUNT: the fp64 sum of row r over ALL its columns (CSR: all its stored entries), the same bits in every lane.  Fixed order: a
// lane adds its entries in ascending position, then the 64 partial sums fold in a butterfly (both operands of every add are
// the same pair in both lanes) - row_visit / wave_fold of wgnn_align_rows.h, which wgnn_coverage_rows shares.  With library
// sizes, a row that holds a count takes the caller's value instead - a value that is not finite and > 0 is reported and the
// row's total is 0 (the row keeps nothing).
template <int FORM, typename TPtr>
__device__ __forceinline__ double row_total(const AArgs& a, long r, int lane, unsigned& bad) {
    double acc = 0.0;
    row_visit<FORM, TPtr>(a, r, lane, [&](long, bool, float v) { add_count(acc, v, bad); });
    acc = wave_fold(acc);
    if (a.lib && acc > 0.0) {                                  // wave-uniform
        const double size = a.lib[r];
        if (size > 0.0 && size < __builtin_inf()) acc = size;
        else { bad |= WGNN_ALIGN_BAD_VALUE; acc = 0.0; }
    }
    return acc;
}

template <int FORM, bool FILL, bool LN, typename TPtr>
__global__ void __launch_bounds__(kABlock) align_rows_kernel(const AArgs a) {
    const int lane = threadIdx.x & 63;
    const long stride = (long)gridDim.x * kAWaves;
    unsigned bad = 0;
    for (long r = (long)blockIdx.x * kAWaves + (threadIdx.x >> 6); r < a.n_rows; r += stride) {      // wave-uniform
        long base = FILL ? (long)a.out_rowptr[r] : 0;
        const long first = base;
        const long room = FILL ? (long)a.out_rowptr[r + 1] : 0;      // a slot at or past it is not written (see `bad`)
        double total = 0.0;
        bool live = true;                                            // LN: the row has a total > 0 (wave-uniform); else it has
        float* slab = nullptr;                                       // no candidate - nothing divided, nothing kept - and the walk
                                                                     // below only reports malformed columns and map values
        if constexpr (LN) {
            __shared__ float s_slab[kAWaves][256];                   // the wave's candidates, packed (lognorm_group)
            slab = s_slab[threadIdx.x >> 6];
            if constexpr (!FILL) {                                   // the row's first read: every column into the total
                total = row_total<FORM, TPtr>(a, r, lane, bad);
                if (lane == 0) a.total_out[r] = total;
            } else total = a.total[r];
            live = total > 0.0;
        }
        if constexpr (FORM == FORM_DENSE_V4) {
            const float* xr = a.x + (size_t)r * a.ld;
            for (long j0 = 0; j0 < a.n_cols; j0 += 256 * kVecAhead) {
                float4 v[kVecAhead];
                int4 g[kVecAhead];
#pragma unroll
                for (int u = 0; u < kVecAhead; ++u) {
                    const long j = j0 + u * 256 + lane * 4;
                    if (j + 3 < a.n_cols) {                          // whole quad inside the row: one 16-byte load each
                        v[u] = ld4(xr + j);
                        g[u] = *reinterpret_cast<const int4*>(a.gene_map + j);
                    } else {                                         // the row's last quad (or past it): per element, guarded
                        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                        g[u] = make_int4(-1, -1, -1, -1);
                        if (j < a.n_cols)     { v[u].x = xr[j];     g[u].x = a.gene_map[j]; }
                        if (j + 1 < a.n_cols) { v[u].y = xr[j + 1]; g[u].y = a.gene_map[j + 1]; }
                        if (j + 2 < a.n_cols) { v[u].z = xr[j + 2]; g[u].z = a.gene_map[j + 2]; }
                    }
                }
                if constexpr (LN) {                                  // counts -> values; what is no candidate -> 0
#pragma unroll
                    for (int u = 0; u < kVecAhead; ++u) {
                        float x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                        const bool c[4] = {live && g[u].x >= 0 && countable(x[0]), live && g[u].y >= 0 && countable(x[1]),
                                           live && g[u].z >= 0 && countable(x[2]), live && g[u].w >= 0 && countable(x[3])};
                        lognorm_group(slab, lane, x, c, total, a.scale);
                        v[u] = make_float4(x[0], x[1], x[2], x[3]);
                    }
                }
#pragma unroll
                for (int u = 0; u < kVecAhead; ++u) {                // columns past n_cols carry map -1: never kept, never reported
                    const bool k0 = keep_entry(a, true, g[u].x, v[u].x, bad), k1 = keep_entry(a, true, g[u].y, v[u].y, bad);
                    const bool k2 = keep_entry(a, true, g[u].z, v[u].z, bad), k3 = keep_entry(a, true, g[u].w, v[u].w, bad);
                    const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1), m2 = __ballot(k2), m3 = __ballot(k3);
                    if constexpr (FILL) {
                        long s = base + below(m0) + below(m1) + below(m2) + below(m3);
                        if (k0) { put(a, s, room, g[u].x, v[u].x, bad); ++s; }
                        if (k1) { put(a, s, room, g[u].y, v[u].y, bad); ++s; }
                        if (k2) { put(a, s, room, g[u].z, v[u].z, bad); ++s; }
                        if (k3) put(a, s, room, g[u].w, v[u].w, bad);
                    }
                    base += __popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3);
                }
            }
        } else {
            long b = 0, e = a.n_cols;
            const float* vals = a.x + (FORM == FORM_DENSE ? (size_t)r * a.ld : 0);
            if constexpr (FORM == FORM_CSR) {
                const TPtr* rp = reinterpret_cast<const TPtr*>(a.rowptr);
                b = rp[r]; e = rp[r + 1];
                vals = a.val;
            }
            for (long j0 = b; j0 < e; j0 += 64 * kAhead) {
                float v[kAhead];
                int g[kAhead];
                bool on[kAhead];
#pragma unroll
                for (int u = 0; u < kAhead; ++u) {
                    const long j = j0 + u * 64 + lane;
                    on[u] = j < e;
                    v[u] = on[u] ? vals[j] : 0.f;
                    if constexpr (FORM == FORM_CSR) g[u] = on[u] ? a.col[j] : 0;       // the caller's column, mapped below
                    else g[u] = on[u] ? a.gene_map[j] : -1;
                }
                if constexpr (FORM == FORM_CSR) {
#pragma unroll
                    for (int u = 0; u < kAhead; ++u) {
                        const bool in = (unsigned)g[u] < (unsigned)a.n_cols;            // outside: no lookup, reported, skipped
                        if (on[u] && !in) bad |= WGNN_ALIGN_BAD_COL;
                        on[u] = on[u] && in;
                        g[u] = on[u] ? a.gene_map[g[u]] : -1;
                    }
                }
                if constexpr (LN) {                                  // counts -> values; what is no candidate -> 0
                    static_assert(kAhead == 4, "lognorm_group takes 4 entries per lane");
                    const bool c[4] = {live && on[0] && g[0] >= 0 && countable(v[0]), live && on[1] && g[1] >= 0 && countable(v[1]),
                                       live && on[2] && g[2] >= 0 && countable(v[2]), live && on[3] && g[3] >= 0 && countable(v[3])};
                    lognorm_group(slab, lane, v, c, total, a.scale);
                }
#pragma unroll
                for (int u = 0; u < kAhead; ++u) {
                    const bool k = keep_entry(a, on[u], g[u], v[u], bad);
                    const unsigned long long m = __ballot(k);
                    if constexpr (FILL) {
                        if (k) put(a, base + below(m), room, g[u], v[u], bad);
                    }
                    base += __popcll(m);
                }
            }
        }
        if constexpr (!FILL) {
            if (lane == 0) a.row_count[r] = (int)(base - first);
        }
    }
    if (bad) atomicOr(a.status, (int)bad);                     // malformed operands only
}

template <int FORM, bool FILL, bool LN>
int launch(const AArgs& a, bool i64, hipStream_t st) {
    const long want = (a.n_rows + kAWaves - 1) / kAWaves;
    const unsigned nb = (unsigned)(want < kAMaxBlocks ? want : kAMaxBlocks);
    if (i64) hipLaunchKernelGGL((align_rows_kernel<FORM, FILL, LN, long long>), dim3(nb), dim3(kABlock), 0, st, a);
    else hipLaunchKernelGGL((align_rows_kernel<FORM, FILL, LN, int>), dim3(nb), dim3(kABlock), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : WGNN_ERR_LAUNCH;
}

}  // namespace

// the checks COUNT and FILL share, then the launch; fn names the entry point in the error detail.  LN: the log-normalising walk
// (COUNT stores the row totals in total_out, FILL reads them from total).
template <bool FILL, bool LN>
static int align_run(const char* fn, const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                     int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold,
                     int32_t* row_count, const int64_t* out_rowptr, int32_t* out_col, float* out_raw, int32_t* status,
                     uint32_t flags, void* stream, const double* total = nullptr, double scale = 0.0,
                     double* total_out = nullptr, const double* library_size = nullptr) {
    auto fail = [fn](int code, const char* what) { return wgnn::fail(code, fn, what); };
    wgnn::error_clear();
    if (!status) return fail(WGNN_ERR_BAD_ARG, "status is required");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [0, 2^31)");
    if (n_cols < 0) return fail(WGNN_ERR_BAD_ARG, "n_cols must not be negative");
    if (n_genes <= 0) return fail(WGNN_ERR_BAD_ARG, "n_genes must be positive");
    if (flags & ~WGNN_FLAG_ROWPTR_I64) return fail(WGNN_ERR_BAD_ARG, "only WGNN_FLAG_ROWPTR_I64 is a valid flag");
    if ((x != nullptr) == (rowptr != nullptr) && n_rows > 0 && (x || n_cols > 0))
        return fail(WGNN_ERR_BAD_ARG, "pass either x (dense) or rowptr / col / val (CSR)");
    const bool dense = rowptr == nullptr;
    if (dense && (flags & WGNN_FLAG_ROWPTR_I64)) return fail(WGNN_ERR_BAD_ARG, "WGNN_FLAG_ROWPTR_I64 belongs to the CSR form");
    if (dense && x && ld < n_cols) return fail(WGNN_ERR_BAD_ARG, "ld must be >= n_cols");
    if (n_cols > 0 && !gene_map) return fail(WGNN_ERR_BAD_ARG, "gene_map is required");
    if (!FILL && n_rows > 0 && !row_count) return fail(WGNN_ERR_BAD_ARG, "row_count is required");
    if (FILL && n_rows > 0 && !out_rowptr) return fail(WGNN_ERR_BAD_ARG, "out_rowptr is required");
    if (FILL && !wgnn::aligned8(out_rowptr)) return fail(WGNN_ERR_ALIGNMENT, "out_rowptr must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(val) | reinterpret_cast<uintptr_t>(gene_map)) & 3u)
        return fail(WGNN_ERR_ALIGNMENT, "x, val and gene_map must be 4-byte aligned");
    if (LN) {
        if (!(threshold >= 0.f)) return fail(WGNN_ERR_BAD_ARG, "threshold must be >= 0 when normalising");
        if (!(scale > 0.0 && scale < HUGE_VAL)) return fail(WGNN_ERR_BAD_ARG, "scale must be positive and finite");
        if (n_rows > 0 && !(FILL ? total != nullptr : total_out != nullptr)) return fail(WGNN_ERR_BAD_ARG, "total is required");
        if (!wgnn::aligned8(total) || !wgnn::aligned8(total_out) || !wgnn::aligned8(library_size))
            return fail(WGNN_ERR_ALIGNMENT, "total and library_size must be 8-byte aligned");
    }
    if (n_rows == 0) return WGNN_OK;
    AArgs a{};
    a.x = x; a.ld = ld; a.rowptr = rowptr; a.col = col; a.val = val; a.n_rows = n_rows; a.n_cols = n_cols;
    a.gene_map = gene_map; a.n_genes = n_genes; a.thr = threshold;
    a.row_count = row_count; a.out_rowptr = reinterpret_cast<const long long*>(out_rowptr); a.out_col = out_col; a.out_raw = out_raw;
    a.status = status; a.total = total; a.scale = scale; a.total_out = total_out; a.lib = library_size;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc;
    if (!dense) rc = launch<FORM_CSR, FILL, LN>(a, flags & WGNN_FLAG_ROWPTR_I64, st);
    else if (wgnn::aligned16(x) && wgnn::aligned16(gene_map) && ld % 4 == 0) rc = launch<FORM_DENSE_V4, FILL, LN>(a, false, st);
    else rc = launch<FORM_DENSE, FILL, LN>(a, false, st);
    return rc == WGNN_OK ? rc : fail(rc, "HIP launch failed");
}

extern "C" int wgnn_align_count(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                                int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold,
                                int32_t* row_count, int32_t* status, uint32_t flags, void* stream) {
    return align_run<false, false>("wgnn_align_count", x, ld, rowptr, col, val, n_rows, n_cols, gene_map, n_genes, threshold,
                                   row_count, nullptr, nullptr, nullptr, status, flags, stream);
}

extern "C" int wgnn_align_fill(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                               int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold,
                               const int64_t* out_rowptr, int32_t* out_col, float* out_raw, int32_t* status,
                               uint32_t flags, void* stream) {
    return align_run<true, false>("wgnn_align_fill", x, ld, rowptr, col, val, n_rows, n_cols, gene_map, n_genes, threshold,
                                  nullptr, out_rowptr, out_col, out_raw, status, flags, stream);
}

extern "C" int wgnn_align_count_ln(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                                   int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold,
                                   const double* library_size, double* total, double scale, int32_t* row_count, int32_t* status,
                                   uint32_t flags, void* stream) {
    return align_run<false, true>("wgnn_align_count_ln", x, ld, rowptr, col, val, n_rows, n_cols, gene_map, n_genes, threshold,
                                  row_count, nullptr, nullptr, nullptr, status, flags, stream, nullptr, scale, total, library_size);
}

extern "C" int wgnn_align_fill_ln(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                                  int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold,
                                  const double* total, double scale, const int64_t* out_rowptr, int32_t* out_col, float* out_raw,
                                  int32_t* status, uint32_t flags, void* stream) {
    return align_run<true, true>("wgnn_align_fill_ln", x, ld, rowptr, col, val, n_rows, n_cols, gene_map, n_genes, threshold,
                                 nullptr, out_rowptr, out_col, out_raw, status, flags, stream, total, scale);
}
