// wgnn_resident_rows.h - what the resident row ops (wgnn_predict_rows, wgnn_attrib_rows, wgnn_predict_rows_dropout,
// wgnn_predict_rows_thin) share AROUND their kernels: the head's LDS limit, three one-line device helpers, the ladder from a
// row width to the kernels' template arguments, and the argument handling of the two draw entries.  The kernel bodies restate
// one another on purpose (each file says why) and are not shared here.
#pragma once
#include <math.h>
#include <type_traits>
#include "wgnn_common.h"

namespace wgnn {

constexpr int kHeadLdsBytes = 64 * 1024;      // a fused head [C, H] is staged in LDS up to this size

// (value, index) maximum over the lane groups: larger value wins, the lower index among equal values
template <int LPR>
__device__ __forceinline__ void group_argmax_fold(float& m, int& am) {
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1) {
        const float mo = __shfl_xor(m, off, 64);
        const int ao = __shfl_xor(am, off, 64);
        if (mo > m || (mo == m && ao < am)) { m = mo; am = ao; }
    }
}

// lane `dst` receives this lane's value (dst is a permutation of 0..63 over the wave)
__device__ __forceinline__ int push_to_lane(int dst, int v) { return __builtin_amdgcn_ds_permute(dst << 2, v); }

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {        // splitmix64 finaliser
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ unsigned mix32(unsigned long long x) { return (unsigned)(mix64(x) >> 32); }      // its upper half

// The kernels' template arguments from the run-time shape: a table row of H <= 256 floats is covered by LPR lanes x float4.
// Calls f(integral_constant<int, LPR>, bool_constant<HEAD>, bool_constant<SELF_ROWS>) and returns what it returns.
template <typename F>
int dispatch_rows(int H, bool head, bool self_rows, F&& f) {
    auto with_lpr = [&](auto lpr) {
        if (head) return self_rows ? f(lpr, std::true_type{}, std::true_type{}) : f(lpr, std::true_type{}, std::false_type{});
        return self_rows ? f(lpr, std::false_type{}, std::true_type{}) : f(lpr, std::false_type{}, std::false_type{});
    };
    const int q = H / 4;
    if (q <= 4)  return with_lpr(std::integral_constant<int, 4>{});
    if (q <= 8)  return with_lpr(std::integral_constant<int, 8>{});
    if (q <= 16) return with_lpr(std::integral_constant<int, 16>{});
    if (q <= 32) return with_lpr(std::integral_constant<int, 32>{});
    return with_lpr(std::integral_constant<int, 64>{});
}

// The arguments wgnn_predict_rows_dropout and wgnn_predict_rows_thin have in common, in the order include/wgnn.h declares them
struct DrawCall {
    const void* rowptr; const int32_t* col; const float* raw; int64_t n_rows;
    const float* table; int64_t ld_table; int32_t n_genes; int32_t H;
    const float* alpha; const float* bias; const float* self_rows; int64_t ld_self;
    int32_t n_draws; int64_t row0; int32_t draw0; uint64_t seed; double keep;
    float* out; int64_t ld_out;
    const float* w_head; const float* b_head; int32_t n_classes; float unsure_threshold;
    int32_t* votes; int64_t ld_votes; int32_t* unsure; int32_t* empty; double* conf_sum;
    int32_t* draw_label; float* draw_prob; uint32_t flags;
};
// ... those wgnn_predict_rows_thin adds
struct ThinCall { const int64_t* rest; double scale; float threshold; int32_t* draw_reads; int32_t* draw_entries; };
// ... and what the two entries call differently (the accumulate bit has one value and two names)
struct DrawEntry { const char* fn; uint32_t accumulate; const char* valid_flags; const char* accumulate_needs_head; };

// Every check of a draw entry up to and including the head / no-head block, in the order the entries have always made them
// (the first failing check is the one reported); `thin`: wgnn_predict_rows_thin's operands, checked in their places.
inline int check_draw_call(const DrawEntry& entry, const DrawCall& c, const ThinCall* thin) {
    auto refuse = [&](int code, const char* what) { return fail(code, entry.fn, what); };
    if (!c.rowptr || !c.col || !c.raw || !c.table || !c.alpha || !c.bias)
        return refuse(WGNN_ERR_BAD_ARG, "rowptr, col, raw, table, alpha and bias are required");
    if (thin && !thin->rest)
        return refuse(WGNN_ERR_BAD_ARG, "rest is required (the cell's reads outside the bundle; zeros when there are none)");
    if (c.n_rows < 0 || c.n_rows > INT32_MAX) return refuse(WGNN_ERR_BAD_ARG, "n_rows must be in [0, 2^31)");
    if (c.n_draws < 1) return refuse(WGNN_ERR_BAD_ARG, "n_draws must be >= 1");
    if (c.n_rows * (int64_t)c.n_draws > INT32_MAX)
        return refuse(WGNN_ERR_BAD_ARG, "n_rows * n_draws must be < 2^31 (split the batch or the draws)");
    if (c.row0 < 0 || c.draw0 < 0) return refuse(WGNN_ERR_BAD_ARG, "row0 and draw0 must not be negative");
    if (!(c.keep >= 0.0 && c.keep <= 1.0)) return refuse(WGNN_ERR_BAD_ARG, "keep must be in [0, 1]");
    if (thin && !(thin->scale > 0.0 && thin->scale < HUGE_VAL)) return refuse(WGNN_ERR_BAD_ARG, "scale must be positive and finite");
    if (thin && !(thin->threshold >= 0.f)) return refuse(WGNN_ERR_BAD_ARG, "threshold must be >= 0");
    if (c.n_genes <= 0) return refuse(WGNN_ERR_BAD_ARG, "n_genes must be positive");
    if (c.flags & ~(uint32_t)(WGNN_FLAG_ROWPTR_I64 | entry.accumulate)) return refuse(WGNN_ERR_BAD_ARG, entry.valid_flags);
    if (c.H <= 0) return refuse(WGNN_ERR_BAD_ARG, "H must be positive");
    if (c.H % 4) return refuse(WGNN_ERR_ALIGNMENT, "H must be a multiple of 4 (zero-pad the table, bias and head)");
    if (c.H > 256) return refuse(WGNN_ERR_UNSUPPORTED, "H > 256 is not built");
    if (c.ld_table < c.H || c.ld_table % 4) return refuse(WGNN_ERR_ALIGNMENT, "ld_table must be >= H and a multiple of 4");
    if (!aligned16(c.table) || !aligned16(c.bias)) return refuse(WGNN_ERR_ALIGNMENT, "table and bias must be 16-byte aligned");
    if (c.self_rows && (c.ld_self < c.H || c.ld_self % 4 || !aligned16(c.self_rows)))
        return refuse(WGNN_ERR_ALIGNMENT, "self_rows: ld_self >= H, a multiple of 4, 16-byte aligned");
    if (thin && !aligned8(thin->rest)) return refuse(WGNN_ERR_ALIGNMENT, "rest must be 8-byte aligned");
    if (thin && (!aligned4(thin->draw_reads) || !aligned4(thin->draw_entries)))
        return refuse(WGNN_ERR_ALIGNMENT, "draw_reads and draw_entries must be 4-byte aligned");
    if (c.w_head) {
        if (!c.b_head || !c.votes || !c.unsure || !c.empty || !c.conf_sum)
            return refuse(WGNN_ERR_BAD_ARG, "a head needs b_head, votes, unsure, empty and conf_sum");
        if (c.n_classes <= 0) return refuse(WGNN_ERR_BAD_ARG, "n_classes must be positive");
        if ((int64_t)c.n_classes * c.H * 4 > kHeadLdsBytes) return refuse(WGNN_ERR_UNSUPPORTED, "the head needs C*H*4 <= 64 KiB");
        if (!aligned16(c.w_head)) return refuse(WGNN_ERR_ALIGNMENT, "w_head must be 16-byte aligned");
        if (c.ld_votes < c.n_classes) return refuse(WGNN_ERR_BAD_ARG, "ld_votes must be >= n_classes");
        if (!aligned8(c.conf_sum)) return refuse(WGNN_ERR_ALIGNMENT, "conf_sum must be 8-byte aligned");
        if (!aligned4(c.votes) || !aligned4(c.unsure) || !aligned4(c.empty) || !aligned4(c.draw_label) || !aligned4(c.draw_prob))
            return refuse(WGNN_ERR_ALIGNMENT, "votes, unsure, empty, draw_label and draw_prob must be 4-byte aligned");
    } else {
        if (c.flags & entry.accumulate) return refuse(WGNN_ERR_BAD_ARG, entry.accumulate_needs_head);
        if (!c.out) return refuse(WGNN_ERR_BAD_ARG, "without a head `out` is required");
        if (c.ld_out < c.H || c.ld_out % 4 || !aligned16(c.out))
            return refuse(WGNN_ERR_ALIGNMENT, "out: ld_out >= H, a multiple of 4, 16-byte aligned");
    }
    return WGNN_OK;
}

// The fields the two draw kernels' argument structs (SArgs, TArgs) share, from a checked call
template <typename Args>
void fill_draw_args(Args& a, const DrawCall& c, uint32_t accumulate_flag) {
    a.rowptr = c.rowptr; a.col = c.col; a.raw = c.raw; a.n_rows = c.n_rows;
    a.table = c.table; a.ld_table = c.ld_table; a.n_genes = c.n_genes; a.H = c.H;
    a.alpha = c.alpha; a.bias = c.bias; a.self_rows = c.self_rows; a.ld_self = c.ld_self;
    a.n_draws = c.n_draws; a.row0 = c.row0; a.draw0 = c.draw0; a.seed = c.seed;
    a.T = (unsigned long long)floor(c.keep * 4294967296.0);        // keep == 1: 2^32, above every 32-bit hash
    a.out = c.out; a.ld_out = c.ld_out;
    a.w_head = c.w_head; a.b_head = c.b_head; a.C = c.n_classes; a.thr = c.unsure_threshold;
    a.votes = c.votes; a.ld_votes = c.ld_votes; a.unsure = c.unsure; a.empty = c.empty; a.conf_sum = c.conf_sum;
    a.draw_label = c.draw_label; a.draw_prob = c.draw_prob; a.accumulate = (c.flags & accumulate_flag) ? 1 : 0;
}

}  // namespace wgnn
