// wgnn_pool.hip - wgnn_pool_rows_accumulate / wgnn_pool_rows_count / wgnn_pool_rows_fill: the count rows of all cells of a group
// (a cluster, a sample, a metacell) added into one pooled row per group and that row log-normalised against the pooled library
// size - a pseudobulk profile (api.ResidentPredictor.pseudobulk).  The contract is the pool-rows block of include/wgnn.h.
//
// ACCUMULATE.  The operand is a bundle-vocabulary CSR of raw integer counts, the groups come as (group_ptr, members).  The member
// list is cut into WINDOWS of cells_per_unit positions counted from group_ptr[0]; a work item is (window, slab of slab_genes
// genes), one workgroup per item, grid-stride.  A window that lies inside one big group is one unit of that group - a cluster of
// 50 000 cells is spread over 50 000 / cells_per_unit workgroups -, a window that holds several small groups takes them one after
// the other, each as a unit of its own: a unit is always (group, at most cells_per_unit consecutive members, slab).  Cutting at
// positions, not at each group's own start, makes the number of items a function of n_rows alone: no read-back of group_ptr, no
// pre-pass that lists units.  Per unit the workgroup zeroes a uint32 LDS slab, its waves walk the unit's rows (one wave per row,
// 64 entries per step, entries outside the slab skipped by comparison), LDS integer atomics take the counts
// (256 cells x 2^23 < 2^31: no overflow) and the NON-ZERO slab entries leave with one 64-bit global atomic add each.  Integer
// sums: exact, the same bits in every order.
//
// FINISH.  One wavefront per group row, grid-stride; COUNT and FILL are the same walk over the n_genes accumulators, 4 x 64 per
// step (the 4 loads are issued before the first is used), a wave ballot of the keep test gives the slots.  No atomics.
//
// Never a fault: a member outside [0, n_rows), a row range outside [0, nnz], a gene id outside [0, n_genes), a group_ptr that is
// not ascending or leaves [0, n_rows], a slot past out_rowptr[k + 1] are skipped and reported in the status word (an ordinary
// global atomic OR, off the data path).  Every member position read lies in [group_ptr[0], group_ptr[n_groups]) within
// [0, n_rows), every accumulator row in [0, n_groups), whatever group_ptr holds in between.

#include <math.h>
#include "wgnn_align_rows.h"             // lognorm, below
#include "wgnn_build_rows.h"

namespace {
using namespace wgnn;

constexpr int kLWaves = 8;                    // ACCUMULATE: waves per workgroup - two workgroups of 64 KiB per CU are 16 waves
constexpr int kLBlock = 64 * kLWaves;
constexpr int kLMaxBlocks = 1024;             // 256 CUs x 4 workgroups (narrow slabs): grid-stride beyond that
constexpr int kLDefCells = 64;                // cells_per_unit = 0
constexpr int kLDefSlab = WGNN_POOL_MAX_SLAB_GENES;      // slab_genes = 0: 64 KiB of uint32

constexpr int kFWaves = 4;                    // FINISH
constexpr int kFBlock = 64 * kFWaves;
constexpr int kFMaxBlocks = 2048;
constexpr int kFAhead = 4;                    // 64-gene steps in flight per wave

struct LArgs {
    const void* rowptr; const int* col; const float* cnt; long n_rows; long nnz;
    const long long* group_ptr; const int* members; long n_groups; int n_genes;
    unsigned long long* acc; long ld_acc;
    int cells; int slab; int n_slabs;
    int* status;
};

struct FArgs {
    const unsigned long long* acc; long ld_acc; const long long* total; long n_groups; int n_genes;
    double scale; float thr;
    int* n_out;                                                                    // COUNT
    const long long* out_rowptr; int* out_col; float* out_val; long long* out_cnt; // FILL
    int* status;
};

template <typename TPtr>
__global__ void __launch_bounds__(kLBlock) pool_accumulate_kernel(const LArgs p) {
    extern __shared__ unsigned s_slab[];                       // [min(slab, n_genes)] uint32: the unit's counts
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TPtr* rp = reinterpret_cast<const TPtr*>(p.rowptr);
    unsigned bad = 0;
    // the whole group_ptr, once, spread over the grid (a window below looks only at the entries around it)
    for (long k = (long)blockIdx.x * kLBlock + threadIdx.x; k < p.n_groups; k += (long)gridDim.x * kLBlock) {
        const long a = p.group_ptr[k], b = p.group_ptr[k + 1];
        if (a < 0 || b < a || b > p.n_rows) bad |= WGNN_POOL_BAD_ROWPTR;
    }
    const long first = p.group_ptr[0], last = p.group_ptr[p.n_groups];
    if (first < 0 || last < first || last > p.n_rows) {
        bad |= WGNN_POOL_BAD_ROWPTR;                           // no window: nothing is added
    } else {
        const long n_items = (last - first + p.cells - 1) / p.cells * p.n_slabs;
        for (long item = blockIdx.x; item < n_items; item += gridDim.x) {                  // everything below is block-uniform
            const long w = item / p.n_slabs;
            const int g0 = (int)(item - w * p.n_slabs) * p.slab;
            const int g1 = g0 + p.slab < p.n_genes ? g0 + p.slab : p.n_genes;
            const long p0 = first + w * p.cells;
            const long p1 = p0 + p.cells < last ? p0 + p.cells : last;                     // first <= p0 < p1 <= last <= n_rows
            // the last group that starts at or before p0: the smallest k in [1, n_groups] with group_ptr[k] > p0, less one
            // (group_ptr[0] = first <= p0, so the search never answers 0; every probe is in [0, n_groups))
            long lo = 0, hi = p.n_groups;
            while (lo < hi) {
                const long mid = (lo + hi) >> 1;
                if (p.group_ptr[mid] <= p0) lo = mid + 1; else hi = mid;
            }
            for (long k = lo - 1; k < p.n_groups; ++k) {
                const long a = p.group_ptr[k], b = p.group_ptr[k + 1];
                if (a >= p1) break;
                if (a < first || b < a || b > last) { bad |= WGNN_POOL_BAD_ROWPTR; break; }
                const long q0 = a > p0 ? a : p0, q1 = b < p1 ? b : p1;
                if (q0 >= q1) continue;                                                    // an empty group, or one that ends before p0
                // the unit (k, members [q0, q1), genes [g0, g1)):  q1 - q0 <= cells <= 256
                for (int i = threadIdx.x; i < g1 - g0; i += kLBlock) s_slab[i] = 0u;
                __syncthreads();
                for (long q = q0 + wave; q < q1; q += kLWaves) {                           // wave-uniform
                    const int r = p.members[q];
                    if ((unsigned long)r >= (unsigned long)p.n_rows) { bad |= WGNN_POOL_BAD_INDEX; continue; }
                    const long e0 = rp[r], e1 = rp[r + 1];
                    if (e0 < 0 || e1 < e0 || e1 > p.nnz) { bad |= WGNN_POOL_BAD_ROWPTR; continue; }
                    for (long j = e0 + lane; j < e1; j += 64) {
                        const int g = p.col[j];
                        const float x = p.cnt[j];
                        if ((unsigned)g >= (unsigned)p.n_genes) { bad |= WGNN_POOL_BAD_COL; continue; }
                        if (g >= g0 && g < g1 && x >= 1.f && x <= kMaxCount) atomicAdd(&s_slab[g - g0], (unsigned)x);
                    }
                }
                __syncthreads();
                unsigned long long* row = p.acc + (size_t)k * p.ld_acc + g0;
                for (int i = threadIdx.x; i < g1 - g0; i += kLBlock) {
                    const unsigned v = s_slab[i];
                    if (v) atomicAdd(row + i, (unsigned long long)v);
                }
                __syncthreads();                                                           // the next unit zeroes the slab
            }
        }
    }
    if (bad) atomicOr(p.status, (int)bad);                     // malformed operands only
}

template <bool FILL>
__global__ void __launch_bounds__(kFBlock) pool_finish_kernel(const FArgs p) {
    const int lane = threadIdx.x & 63;
    const long stride = (long)gridDim.x * kFWaves;
    unsigned bad = 0;
    for (long k = (long)blockIdx.x * kFWaves + (threadIdx.x >> 6); k < p.n_groups; k += stride) {      // wave-uniform
        const long long t = p.total[k];
        const double total = (double)t;
        const unsigned long long* row = p.acc + (size_t)k * p.ld_acc;
        long base = FILL ? (long)p.out_rowptr[k] : 0;
        const long first = base;
        const long room = FILL ? (long)p.out_rowptr[k + 1] : 0;          // a slot at or past it is not written (see `bad`)
        const int n = t > 0 ? p.n_genes : 0;                             // total <= 0: the empty row
        for (int s0 = 0; s0 < n; s0 += 64 * kFAhead) {                   // wave-uniform
            unsigned long long c[kFAhead];
#pragma unroll
            for (int u = 0; u < kFAhead; ++u) {
                const int g = s0 + u * 64 + lane;
                c[u] = g < n ? row[g] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < kFAhead; ++u) {
                const int g = s0 + u * 64 + lane;
                float v = 0.f;
                bool keep = false;
                if (c[u]) {
                    v = lognorm((double)c[u], total, p.scale);
                    keep = v > p.thr;
                }
                const unsigned long long m = __ballot(keep);
                if constexpr (FILL) {
                    if (keep) {
                        const long s = base + below(m);
                        if (s < room) {
                            p.out_col[s] = g; p.out_val[s] = v;
                            if (p.out_cnt) p.out_cnt[s] = (long long)c[u];
                        } else bad |= WGNN_POOL_BAD_ROWPTR;
                    }
                }
                base += __popcll(m);
            }
        }
        if constexpr (!FILL) {
            if (lane == 0) p.n_out[k] = (int)(base - first);
        }
    }
    if (bad) atomicOr(p.status, (int)bad);
}

LdsMarks g_lds_i32, g_lds_i64;                // the accumulate kernel's raised LDS limit, per rowptr width

}  // namespace

extern "C" int wgnn_pool_rows_accumulate(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                                         const int64_t* group_ptr, const int32_t* members, int64_t n_groups, int32_t n_genes,
                                         uint64_t* acc, int64_t ld_acc, int32_t cells_per_unit, int32_t slab_genes,
                                         int32_t* status, uint32_t flags, void* stream) {
    const char* fn = "wgnn_pool_rows_accumulate";
    auto fail = [fn](int code, const char* what) { return wgnn::fail(code, fn, what); };
    wgnn::error_clear();
    if (int rc = wgnn::check_count_csr(fn, status, n_rows, nnz)) return rc;
    if (n_groups < 0 || n_groups > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_groups must be in [0, 2^31)");
    if (n_genes < 0) return fail(WGNN_ERR_BAD_ARG, "n_genes must not be negative");
    if (ld_acc < n_genes) return fail(WGNN_ERR_BAD_ARG, "ld_acc must be >= n_genes");
    if (cells_per_unit < 0 || cells_per_unit > WGNN_POOL_MAX_CELLS_PER_UNIT)
        return fail(WGNN_ERR_BAD_ARG, "cells_per_unit must be in [0, 256] (256 cells x 2^23 is what a uint32 slab entry holds)");
    if (slab_genes < 0 || slab_genes > WGNN_POOL_MAX_SLAB_GENES)
        return fail(WGNN_ERR_BAD_ARG, "slab_genes must be in [0, 16384] (a wider slab does not fit the LDS budget)");
    if (int rc = wgnn::check_rowptr_flag(fn, flags)) return rc;
    const bool work = n_groups > 0 && n_rows > 0;
    if (work && (!rowptr || !group_ptr || !members)) return fail(WGNN_ERR_BAD_ARG, "rowptr, group_ptr and members are required");
    if (int rc = wgnn::check_count_entries(fn, work, nnz, col, cnt)) return rc;
    if (work && n_genes > 0 && !acc) return fail(WGNN_ERR_BAD_ARG, "acc is required");
    if (!wgnn::aligned8(group_ptr) || !wgnn::aligned8(acc)) return fail(WGNN_ERR_ALIGNMENT, "group_ptr and acc must be 8-byte aligned");
    if (int rc = wgnn::check_rowptr_alignment(fn, rowptr, flags)) return rc;
    if (!aligned4(col) || !aligned4(cnt) || !aligned4(members) || !aligned4(status))
        return fail(WGNN_ERR_ALIGNMENT, "col, cnt, members and status must be 4-byte aligned");
    if (!work || n_genes == 0) return WGNN_OK;
    LArgs p{};
    p.rowptr = rowptr; p.col = col; p.cnt = cnt; p.n_rows = n_rows; p.nnz = nnz;
    p.group_ptr = reinterpret_cast<const long long*>(group_ptr); p.members = members; p.n_groups = n_groups; p.n_genes = n_genes;
    p.acc = reinterpret_cast<unsigned long long*>(acc); p.ld_acc = ld_acc;
    p.cells = cells_per_unit ? cells_per_unit : kLDefCells;
    p.slab = slab_genes ? slab_genes : kLDefSlab;
    if (p.slab > n_genes) p.slab = n_genes;
    p.n_slabs = (n_genes + p.slab - 1) / p.slab;
    p.status = status;
    const bool i64 = flags & WGNN_FLAG_ROWPTR_I64;
    const int lds = p.slab * (int)sizeof(unsigned);
    const void* kernel = i64 ? reinterpret_cast<const void*>(pool_accumulate_kernel<long long>)
                             : reinterpret_cast<const void*>(pool_accumulate_kernel<int>);
    if (raise_lds(i64 ? g_lds_i64 : g_lds_i32, kernel, lds) != WGNN_OK) return fail(WGNN_ERR_LAUNCH, "could not reserve the LDS slab");
    const long want = (n_rows + p.cells - 1) / p.cells * p.n_slabs;       // the items when every row is a member
    const unsigned nb = (unsigned)(want < kLMaxBlocks ? want : kLMaxBlocks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (i64) hipLaunchKernelGGL(pool_accumulate_kernel<long long>, dim3(nb), dim3(kLBlock), lds, st, p);
    else hipLaunchKernelGGL(pool_accumulate_kernel<int>, dim3(nb), dim3(kLBlock), lds, st, p);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

// the checks COUNT and FILL share, then the launch; fn names the entry point in the error detail
template <bool FILL>
static int pool_finish(const char* fn, const uint64_t* acc, int64_t ld_acc, const int64_t* total, int64_t n_groups, int32_t n_genes,
                       double scale, float threshold, int32_t* n_out, const int64_t* out_rowptr, int32_t* out_col, float* out_val,
                       int64_t* out_cnt, int32_t* status, void* stream) {
    auto fail = [fn](int code, const char* what) { return wgnn::fail(code, fn, what); };
    wgnn::error_clear();
    if (!status) return fail(WGNN_ERR_BAD_ARG, "status is required");
    if (n_groups < 0 || n_groups > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_groups must be in [0, 2^31)");
    if (n_genes < 0) return fail(WGNN_ERR_BAD_ARG, "n_genes must not be negative");
    if (ld_acc < n_genes) return fail(WGNN_ERR_BAD_ARG, "ld_acc must be >= n_genes");
    if (int rc = wgnn::check_lognorm(fn, scale, threshold)) return rc;
    if (n_groups > 0 && !total) return fail(WGNN_ERR_BAD_ARG, "total is required");
    if (n_groups > 0 && n_genes > 0 && !acc) return fail(WGNN_ERR_BAD_ARG, "acc is required");
    if (!FILL && n_groups > 0 && !n_out) return fail(WGNN_ERR_BAD_ARG, "n_out is required");
    if (FILL && n_groups > 0 && !out_rowptr) return fail(WGNN_ERR_BAD_ARG, "out_rowptr is required");
    if (!wgnn::aligned8(acc) || !wgnn::aligned8(total) || !wgnn::aligned8(out_rowptr) || !wgnn::aligned8(out_cnt))
        return fail(WGNN_ERR_ALIGNMENT, "acc, total, out_rowptr and out_cnt must be 8-byte aligned");
    if (!aligned4(n_out) || !aligned4(out_col) || !aligned4(out_val) || !aligned4(status))
        return fail(WGNN_ERR_ALIGNMENT, "n_out, out_col, out_val and status must be 4-byte aligned");
    if (n_groups == 0) return WGNN_OK;
    FArgs p{};
    p.acc = reinterpret_cast<const unsigned long long*>(acc); p.ld_acc = ld_acc;
    p.total = reinterpret_cast<const long long*>(total); p.n_groups = n_groups; p.n_genes = n_genes;
    p.scale = scale; p.thr = threshold; p.n_out = n_out;
    p.out_rowptr = reinterpret_cast<const long long*>(out_rowptr); p.out_col = out_col; p.out_val = out_val;
    p.out_cnt = reinterpret_cast<long long*>(out_cnt); p.status = status;
    const long want = (n_groups + kFWaves - 1) / kFWaves;
    const unsigned nb = (unsigned)(want < kFMaxBlocks ? want : kFMaxBlocks);
    hipLaunchKernelGGL(pool_finish_kernel<FILL>, dim3(nb), dim3(kFBlock), 0, static_cast<hipStream_t>(stream), p);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_pool_rows_count(const uint64_t* acc, int64_t ld_acc, const int64_t* total, int64_t n_groups, int32_t n_genes,
                                    double scale, float threshold, int32_t* n_out, int32_t* status, void* stream) {
    return pool_finish<false>("wgnn_pool_rows_count", acc, ld_acc, total, n_groups, n_genes, scale, threshold, n_out, nullptr,
                              nullptr, nullptr, nullptr, status, stream);
}

extern "C" int wgnn_pool_rows_fill(const uint64_t* acc, int64_t ld_acc, const int64_t* total, int64_t n_groups, int32_t n_genes,
                                   double scale, float threshold, const int64_t* out_rowptr, int32_t* out_col, float* out_val,
                                   int64_t* out_cnt, int32_t* status, void* stream) {
    return pool_finish<true>("wgnn_pool_rows_fill", acc, ld_acc, total, n_groups, n_genes, scale, threshold, nullptr, out_rowptr,
                             out_col, out_val, out_cnt, status, stream);
}
