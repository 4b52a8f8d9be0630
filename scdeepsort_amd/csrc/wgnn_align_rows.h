// wgnn_align_rows.h - the row walk that fixes the order of a row's fp64 total, shared by wgnn_align.hip (wgnn_align_count_ln's
// total) and wgnn_coverage.hip (wgnn_coverage_rows' total / total_mapped): both sums come out of THIS code, so they agree bit
// for bit.  One wavefront per row; a lane visits its entries in ascending position, the 64 partial sums fold in a butterfly.
// Also here, for every kernel that compacts with a ballot or log-normalises a count: below() and lognorm().
#pragma once
#include <math.h>
#include "wgnn_common.h"

namespace wgnn {

constexpr int kAhead = 4;                     // 64-entry steps in flight per wave (scalar forms)
constexpr int kVecAhead = 2;                  // 256-entry steps in flight per wave (16-byte dense form)

enum { FORM_DENSE = 0, FORM_DENSE_V4 = 1, FORM_CSR = 2 };

// a count that can be kept - finite and > 0 (a -0.0, a NaN, a negative count and an infinity are none)
__device__ __forceinline__ bool countable(float x) { return x > 0.f && x < __builtin_inff(); }

// one count into a lane's partial sum; what cannot be counted and is not a zero is reported and left out
__device__ __forceinline__ void add_count(double& acc, float x, unsigned& bad) {
    if (countable(x)) acc += (double)x;
    else if (!(x == 0.f)) bad |= WGNN_ALIGN_BAD_VALUE;
}

// The log-normalised value of a count: fp64 throughout in Seurat's operation order (divide, scale, log1p), each step rounded on
// its own.  ONE definition for wgnn_align_count_ln / _fill_ln (and their merging forms) and for wgnn_predict_rows_thin, whose
// draws at keep == 1 must carry the bits of the aligned batch.  The count comes in fp64: wgnn_align_*_ln_merge's merged counts and
// wgnn_pool_rows_*'s pooled ones (integers up to 2^53, beyond what a float holds) enter here as they are; a float count is widened
// first, so (double)x is the first step of both forms.
__device__ __forceinline__ float lognorm(double x, double total, double scale) {
#pragma clang fp contract(off)
    const double q = x / total;
    const double y = q * scale;
    return (float)log1p(y);
}
__device__ __forceinline__ float lognorm(float x, double total, double scale) { return lognorm((double)x, total, scale); }

// Every entry of row r - ALL its columns (CSR: all its stored entries) - handed to visit(j, on, v) in the lane's order of
// addition: j = the column (dense) or the entry's position in col / val (CSR), on = the lane holds an entry there (else v = 0).
// A = any struct with the operand's fields (x, ld, rowptr, val, n_cols).  The loads of a step are issued before its visits.
template <int FORM, typename TPtr, typename A, typename Visit>
__device__ __forceinline__ void row_visit(const A& a, long r, int lane, Visit&& visit) {
    if constexpr (FORM == FORM_DENSE_V4) {
        const float* xr = a.x + (size_t)r * a.ld;
        for (long j0 = 0; j0 < a.n_cols; j0 += 256 * kVecAhead) {
            float4 v[kVecAhead];
#pragma unroll
            for (int u = 0; u < kVecAhead; ++u) {
                const long j = j0 + u * 256 + lane * 4;
                if (j + 3 < a.n_cols) v[u] = ld4(xr + j);
                else {
                    v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (j < a.n_cols) v[u].x = xr[j];
                    if (j + 1 < a.n_cols) v[u].y = xr[j + 1];
                    if (j + 2 < a.n_cols) v[u].z = xr[j + 2];
                }
            }
#pragma unroll
            for (int u = 0; u < kVecAhead; ++u) {
                const long j = j0 + u * 256 + lane * 4;
                visit(j, j < a.n_cols, v[u].x); visit(j + 1, j + 1 < a.n_cols, v[u].y);
                visit(j + 2, j + 2 < a.n_cols, v[u].z); visit(j + 3, j + 3 < a.n_cols, v[u].w);
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
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const long j = j0 + u * 64 + lane;
                v[u] = j < e ? vals[j] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const long j = j0 + u * 64 + lane;
                visit(j, j < e, v[u]);
            }
        }
    }
}

// number of set bits of `mask` below this lane: the lane's rank in a ballot
__device__ __forceinline__ int below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// the 64 partial sums of a wave folded in a fixed butterfly (both operands of every add are the same pair in both lanes): the
// same bits in every lane
__device__ __forceinline__ double wave_fold(double acc) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    return acc;
}

}  // namespace wgnn
