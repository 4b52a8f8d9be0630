// wgnn_build_rows.h - what the units that BUILD a bundle-vocabulary CSR from raw counts (wgnn_pairs.hip, wgnn_pool.hip,
// wgnn_soup.hip, wgnn_hood.hip) share around their walks: the count cap, the per-device marks of a raised dynamic-LDS limit, and the entry
// checks of the count-CSR operand and of the log-normalisation.  below(), the lane's rank in a ballot, is one step further up,
// in wgnn_align_rows.h: the aligning and the thinning kernels use it too.
//
// Not shared, on purpose:
//   - the walks themselves (a merge path over two rows, a sweep of dense accumulators, a sweep of an LDS slab);
//   - the line that deposits an entry into the LDS slab (pool's accumulate, soup): behind a device helper - whether it adds,
//     or only answers the range test - the compiler allocates both kernels' registers differently, and these kernels' machine
//     code is what their measurements stand on.  The line stays in both walks, its cap is kMaxCount below;
//   - the lines in which a fill walk stores a kept entry ("rank in the ballot, store if the slot is below `room`, else
//     report").  They differ in what they store (pool and soup have an optional out_cnt, pairs has none), in the status bit and
//     in who advances the offset (soup's waves start from a folded prefix): one helper for the three takes a callback or ten
//     arguments, and neither reads better than the five lines it replaces.
#pragma once
#include <math.h>
#include <atomic>
#include "wgnn_common.h"
#include "wgnn_align_rows.h"

namespace wgnn {

constexpr float kMaxCount = 8388608.f;        // 2^23: the largest count an entry may hold (two of them add exactly in float32,
                                              // 256 of them fit a uint32 slab entry); a slab takes counts in [1, kMaxCount]

// hipFuncAttributeMaxDynamicSharedMemorySize is per device: one LdsMarks per kernel instantiation remembers, per device, the
// limit that was raised for it (the training path's wgnn_tiled.hip / wgnn_transpose.hip keep twins of their own)
constexpr int kMaxDevices = 64;
struct LdsMarks { std::atomic<int> v[kMaxDevices]; };

inline int raise_lds(LdsMarks& marks, const void* fn, int lds) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return WGNN_ERR_LAUNCH;
    std::atomic<int>& mark = marks.v[dev];
    if (mark.load(std::memory_order_acquire) >= lds) return WGNN_OK;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return WGNN_ERR_LAUNCH;
    int seen = mark.load(std::memory_order_relaxed);
    while (seen < lds && !mark.compare_exchange_weak(seen, lds, std::memory_order_release)) {}
    return WGNN_OK;
}

// The checks the entries make of the count-CSR operand and of the log-normalisation, one helper per run of checks that the
// entries make in one place: every entry calls them where it has always made these checks, between its own, so the first
// failing check - the one reported - stays what it was.  `fn` names the entry point in the error detail, `work` says that the
// call has rows to read; WGNN_OK = go on.

inline int check_count_csr(const char* fn, const int32_t* status, int64_t n_rows, int64_t nnz) {
    if (!status) return fail(WGNN_ERR_BAD_ARG, fn, "status is required");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, fn, "n_rows must be in [0, 2^31)");
    if (nnz < 0) return fail(WGNN_ERR_BAD_ARG, fn, "nnz must not be negative");
    return WGNN_OK;
}

inline int check_rowptr_flag(const char* fn, uint32_t flags) {
    return (flags & ~WGNN_FLAG_ROWPTR_I64) ? fail(WGNN_ERR_BAD_ARG, fn, "only WGNN_FLAG_ROWPTR_I64 is a valid flag") : WGNN_OK;
}

inline int check_lognorm(const char* fn, double scale, float threshold) {
    if (!(scale > 0.0 && scale < HUGE_VAL)) return fail(WGNN_ERR_BAD_ARG, fn, "scale must be positive and finite");
    if (!(threshold >= 0.f)) return fail(WGNN_ERR_BAD_ARG, fn, "threshold must be >= 0");
    return WGNN_OK;
}

inline int check_count_entries(const char* fn, bool work, int64_t nnz, const int32_t* col, const float* cnt) {
    return (work && nnz > 0 && (!col || !cnt)) ? fail(WGNN_ERR_BAD_ARG, fn, "col and cnt are required") : WGNN_OK;
}

inline int check_rowptr_alignment(const char* fn, const void* rowptr, uint32_t flags) {
    if ((flags & WGNN_FLAG_ROWPTR_I64) ? !aligned8(rowptr) : !aligned4(rowptr))
        return fail(WGNN_ERR_ALIGNMENT, fn, "rowptr must be aligned to its entries (8 bytes with WGNN_FLAG_ROWPTR_I64, else 4)");
    return WGNN_OK;
}

}  // namespace wgnn
