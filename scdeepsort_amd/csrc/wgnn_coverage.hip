// wgnn_coverage.hip - wgnn_coverage_rows: how much of a batch over the CALLER's gene list the bundle's vocabulary sees
// (api.ResidentPredictor.coverage).  It reads the operand wgnn_align_count takes and writes, per row, the counting entries and
// their fp64 sum over all columns and over the mapped ones, and the entries that are no counts at all; per caller column, the
// rows in which it counts.  An entry counts iff countable() of wgnn_align_rows.h: finite and > 0.
//
// Layout, two walks:
//   rows    - one wavefront per row, grid-stride (as the align kernels).  The walk IS row_visit of wgnn_align_rows.h, the one
//             wgnn_align_count_ln's total comes out of: a lane adds its entries in ascending position into two fp64 partial sums
//             (all columns / mapped columns) and three integer counts, wave_fold folds the sums in the fixed butterfly.  total is
//             therefore the very bits align stores, and no sum ever meets an atomic.  The CSR form also raises col_cells here:
//             one integer global atomic per counting entry (its column is only known per entry; the adds spread over n_cols
//             addresses).
//   columns - dense form only: a thread owns a column (four with 16-byte rows), a workgroup 256 of them, and walks the rows of
//             its slabs (kSlabRows rows, kRowsAhead loads in flight; consecutive threads read consecutive addresses), counting in
//             a register; one integer global atomic per (workgroup, column) that saw a count.  Nothing per entry, no LDS
//             histogram, so any n_cols.  The price is a second read of the matrix.
// Integer addition does not depend on order, the fp64 sums have a fixed one: two launches give identical bits.
// Never a fault: a CSR col outside [0, n_cols) is not looked up (its value still belongs to the row's stored entries: it is in
// n_expressed / total as it is in align's total, and in no column's count), a gene_map value outside [-1, n_genes) counts as
// unmapped; both raise their bit in the caller's status word.

#include <string.h>
#include "wgnn_common.h"
#include "wgnn_align_rows.h"

namespace {
using namespace wgnn;

constexpr int kCWaves = 8;                    // waves per workgroup of the row walk, as the align kernels
constexpr int kCBlock = 64 * kCWaves;
constexpr int kCMaxBlocks = 1024;             // 256 CUs x 4 workgroups: grid-stride beyond that
constexpr int kColBlock = 256;                // threads per workgroup of the column walk
constexpr int kSlabRows = 32;                 // rows a workgroup of the column walk takes at a time
constexpr int kRowsAhead = 4;                 // row loads in flight per thread there
constexpr int kMaxSlabBlocks = 2048;          // grid.y of the column walk: slab-stride beyond that

struct CArgs {
    const float* x; long ld;                                   // dense
    const void* rowptr; const int* col; const float* val;      // CSR over the caller's columns
    long n_rows; int n_cols;
    const int* gene_map; int n_genes;
    int* n_expressed; int* n_mapped; int* n_bad;               // [n_rows]
    double* total; double* total_mapped;                       // [n_rows]
    int* col_cells;                                            // [n_cols], zeroed before the launch
    int* status;
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int FORM, typename TPtr>
__global__ void __launch_bounds__(kCBlock) coverage_rows_kernel(const CArgs a) {
    const int lane = threadIdx.x & 63;
    const long stride = (long)gridDim.x * kCWaves;
    unsigned bad = 0;
    for (long r = (long)blockIdx.x * kCWaves + (threadIdx.x >> 6); r < a.n_rows; r += stride) {      // wave-uniform
        double all = 0.0, mapped = 0.0;
        int n_all = 0, n_map = 0, n_bad = 0;
        row_visit<FORM, TPtr>(a, r, lane, [&](long j, bool on, float v) {
            if (!on) return;
            int g;
            if constexpr (FORM == FORM_CSR) {
                const int c = a.col[j];
                const bool in = (unsigned)c < (unsigned)a.n_cols;         // outside: no lookup, reported
                if (!in) bad |= WGNN_ALIGN_BAD_COL;
                g = in ? a.gene_map[c] : -1;
                if (in && countable(v)) atomicAdd(a.col_cells + c, 1);
            } else g = a.gene_map[j];
            if (g < -1 || g >= a.n_genes) { bad |= WGNN_ALIGN_BAD_MAP; g = -1; }
            unsigned no_count = 0;
            add_count(all, v, no_count);                                  // align's own add: the same sum
            const bool counts = countable(v), in_bundle = counts && g >= 0;
            if (in_bundle) mapped += (double)v;
            n_all += counts ? 1 : 0;
            n_map += in_bundle ? 1 : 0;
            n_bad += no_count ? 1 : 0;
        });
        all = wave_fold(all);
        mapped = wave_fold(mapped);
        n_all = wave_sum(n_all); n_map = wave_sum(n_map); n_bad = wave_sum(n_bad);
        if (lane == 0) {
            a.total[r] = all; a.total_mapped[r] = mapped;
            a.n_expressed[r] = n_all; a.n_mapped[r] = n_map; a.n_bad[r] = n_bad;
        }
    }
    if (bad) atomicOr(a.status, (int)bad);                     // malformed operands only
}

// dense: the rows in which each column counts.  W = columns per thread (4: 16-byte loads, x 16-byte aligned and ld % 4 == 0).
template <int W>
__global__ void __launch_bounds__(kColBlock) coverage_cols_kernel(const CArgs a) {
    const long j = ((long)blockIdx.x * kColBlock + threadIdx.x) * W;
    if (j >= a.n_cols) return;
    const bool whole = j + W <= a.n_cols;                      // W == 4: all four columns inside the row
    int n[W] = {};
    const long n_slabs = (a.n_rows + kSlabRows - 1) / kSlabRows;
    for (long slab = blockIdx.y; slab < n_slabs; slab += gridDim.y) {
        const long r0 = slab * kSlabRows;
        const long r1 = r0 + kSlabRows < a.n_rows ? r0 + kSlabRows : a.n_rows;
        for (long r = r0; r < r1; r += kRowsAhead) {
            float v[kRowsAhead][W];
#pragma unroll
            for (int u = 0; u < kRowsAhead; ++u) {
                const float* p = a.x + (size_t)(r + u) * a.ld + j;
#pragma unroll
                for (int c = 0; c < W; ++c) v[u][c] = 0.f;
                if (r + u < r1) {
                    if constexpr (W == 4) {
                        if (whole) { const float4 q = ld4(p); v[u][0] = q.x; v[u][1] = q.y; v[u][2] = q.z; v[u][3] = q.w; }
                        else {
#pragma unroll
                            for (int c = 0; c < W; ++c) if (j + c < a.n_cols) v[u][c] = p[c];
                        }
                    } else v[u][0] = p[0];
                }
            }
#pragma unroll
            for (int u = 0; u < kRowsAhead; ++u)
#pragma unroll
                for (int c = 0; c < W; ++c) n[c] += countable(v[u][c]) ? 1 : 0;
        }
    }
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (n[c]) atomicAdd(a.col_cells + j + c, n[c]);        // j + c < n_cols: a column past the row loaded zeros only
}

template <int FORM>
int launch_rows(const CArgs& a, bool i64, hipStream_t st) {
    const long want = (a.n_rows + kCWaves - 1) / kCWaves;
    const unsigned nb = (unsigned)(want < kCMaxBlocks ? want : kCMaxBlocks);
    if (i64) hipLaunchKernelGGL((coverage_rows_kernel<FORM, long long>), dim3(nb), dim3(kCBlock), 0, st, a);
    else hipLaunchKernelGGL((coverage_rows_kernel<FORM, int>), dim3(nb), dim3(kCBlock), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : WGNN_ERR_LAUNCH;
}

template <int W>
int launch_cols(const CArgs& a, hipStream_t st) {
    const long per_block = (long)kColBlock * W;
    const long bx = (a.n_cols + per_block - 1) / per_block;
    const long n_slabs = (a.n_rows + kSlabRows - 1) / kSlabRows;
    const long by = n_slabs < kMaxSlabBlocks ? n_slabs : kMaxSlabBlocks;
    hipLaunchKernelGGL((coverage_cols_kernel<W>), dim3((unsigned)bx, (unsigned)by), dim3(kColBlock), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : WGNN_ERR_LAUNCH;
}

}  // namespace

extern "C" int wgnn_coverage_rows(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                                  int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes,
                                  int32_t* n_expressed, int32_t* n_mapped, int32_t* n_bad, double* total, double* total_mapped,
                                  int32_t* col_cells, int32_t* status, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_coverage_rows", what); };
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
    if (n_rows > 0 && !(n_expressed && n_mapped && n_bad && total && total_mapped))
        return fail(WGNN_ERR_BAD_ARG, "n_expressed, n_mapped, n_bad, total and total_mapped are required");
    if (n_cols > 0 && !col_cells) return fail(WGNN_ERR_BAD_ARG, "col_cells is required");
    if (!wgnn::aligned8(total) || !wgnn::aligned8(total_mapped))
        return fail(WGNN_ERR_ALIGNMENT, "total and total_mapped must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(val) | reinterpret_cast<uintptr_t>(gene_map) |
         reinterpret_cast<uintptr_t>(n_expressed) | reinterpret_cast<uintptr_t>(n_mapped) | reinterpret_cast<uintptr_t>(n_bad) |
         reinterpret_cast<uintptr_t>(col_cells)) & 3u)
        return fail(WGNN_ERR_ALIGNMENT, "x, val, gene_map and the int32 outputs must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_cols > 0 && hipMemsetAsync(col_cells, 0, (size_t)n_cols * sizeof(int32_t), st) != hipSuccess)
        return fail(WGNN_ERR_LAUNCH, "clearing col_cells failed");
    if (n_rows == 0) return WGNN_OK;
    CArgs a{};
    a.x = x; a.ld = ld; a.rowptr = rowptr; a.col = col; a.val = val; a.n_rows = n_rows; a.n_cols = n_cols;
    a.gene_map = gene_map; a.n_genes = n_genes;
    a.n_expressed = n_expressed; a.n_mapped = n_mapped; a.n_bad = n_bad; a.total = total; a.total_mapped = total_mapped;
    a.col_cells = col_cells; a.status = status;
    int rc;
    const bool rows16 = wgnn::aligned16(x) && ld % 4 == 0;
    if (!dense) rc = launch_rows<FORM_CSR>(a, flags & WGNN_FLAG_ROWPTR_I64, st);
    else if (rows16 && wgnn::aligned16(gene_map)) rc = launch_rows<FORM_DENSE_V4>(a, false, st);
    else rc = launch_rows<FORM_DENSE>(a, false, st);
    if (rc == WGNN_OK && dense && n_cols > 0) rc = rows16 ? launch_cols<4>(a, st) : launch_cols<1>(a, st);
    return rc == WGNN_OK ? rc : fail(rc, "HIP launch failed");
}
