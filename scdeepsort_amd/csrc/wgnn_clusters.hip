// wgnn_clusters.hip - wgnn_group_class_reduce: per-group, per-class sums of a batch's softmax (api.ResidentPredictor.annotate).
//
//   prob_sum[k, j] = sum over the cells i of group k of softmax(logits[i])[j]   (fp64 from the f32 logits)
//   conf_sum[k]    = sum of the cells' largest probability (1 / Z),   votes[k, j] = cells with label j,   tally[k] = {cells, unsure, bad}
//
// The operand is the batch GROUP-MAJOR (order / seg_ptr: the cell ids of group k, ascending, in order[seg_ptr[k] .. seg_ptr[k+1])).
// A group's run is cut into chunks of kCChunk cells - a constant of the kernel, not of the device - and a chunk has ONE owner, a
// wavefront.  Lanes are (cell slot, class): Cp = the power of two at or above min(C, 64), 64 / Cp cells side by side, class
// lane % Cp of cell slot lane / Cp.  Per step the Cp lanes of a cell find its max and its Z = sum exp(l - max) by an xor butterfly
// (a fixed tree, a + b commutes bit for bit: all Cp lanes hold the same Z) and every lane adds its p = e / Z into a private fp64
// sum; at the end of the chunk the cell slots fold by an xor butterfly and one [C] partial leaves for the workspace.  More than
// 64 classes: Cp = 64, one cell per step, a lane walks classes lane, lane + 64, ... for the max and Z, and the chunk is passed
// over once per 64 classes (the max and Z are recomputed per pass by the same instructions).  A second kernel, behind the
// launch boundary, adds a group's chunk partials in ascending chunk order and writes (or adds to) the outputs.
// No floating-point atomic, no integer atomic either: the counts take the same route.  The order of a bin's additions depends
// on the operand alone (order, seg_ptr, kCChunk): two launches are bit-identical whatever the grid.
//
// Chunk w of the workspace belongs to the group k with slot(k) <= w < slot(k + 1), slot(k) = seg_ptr[k] / kCChunk + k: group k
// needs ceil(n_k / kCChunk) <= slot(k + 1) - slot(k) chunks, so no scan over the groups is needed and slot(K) <=
// n_rows / kCChunk + K bounds the workspace from the host.  A wave finds its group by bisection over slot().

#include <math.h>
#include "wgnn_common.h"

namespace {
using namespace wgnn;

constexpr int kCChunk = 256;                  // cells per chunk: part of the result's addition order, never tuned per device
constexpr int kCPerLane = kCChunk / 64;       // cell ids a lane holds of its chunk
constexpr int kCWaves = 4;
constexpr int kCMaxBlocks = 4096;             // grid-stride beyond that

struct CArgs {
    const float* logits; long ld; const int* label; const int* order; const long long* seg;
    long n_rows; int n_groups; int n_classes; long n_slots;
    double* dpart; int* ipart;                // [n_slots][C + 1] {p[C], conf}, [n_slots][C + 3] {votes[C], cells, unsure, bad}
    double* prob_sum; double* conf_sum; int* votes; int* tally; int accumulate;
};

// how many entries of `order` count: seg_ptr[K] clamped into [0, n_rows]; nothing without the operands
__device__ __forceinline__ long entries(const CArgs& a) {
    if (!a.logits || !a.label || !a.order) return 0;
    const long n = a.seg[a.n_groups];
    return n < 0 ? 0 : (n > a.n_rows ? a.n_rows : n);
}
// seg_ptr[k] clamped into [0, n]: a malformed seg_ptr reads no position outside `order` and no slot outside the workspace
__device__ __forceinline__ long seg_at(const CArgs& a, long k, long n) {
    const long v = a.seg[k];
    return v < 0 ? 0 : (v > n ? n : v);
}
__device__ __forceinline__ long slot_at(const CArgs& a, long k, long n) { return seg_at(a, k, n) / kCChunk + k; }

template <int CP>
__global__ void __launch_bounds__(64 * kCWaves) class_chunk_kernel(const CArgs a) {
    constexpr int S = 64 / CP;                                      // cells side by side
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane / CP, j0 = lane % CP;
    const int C = a.n_classes;
    const int passes = CP == 64 ? (C + 63) / 64 : 1;
    const long n = entries(a);
    for (long w = (long)blockIdx.x * kCWaves + wave; w < a.n_slots; w += (long)gridDim.x * kCWaves) {      // wave-uniform
        if (slot_at(a, 0, n) > w) continue;
        long lo = 0, hi = a.n_groups;                               // the largest k in [0, K] with slot(k) <= w
        while (lo < hi) {
            const long mid = lo + (hi - lo + 1) / 2;
            if (slot_at(a, mid, n) <= w) lo = mid; else hi = mid - 1;
        }
        if (lo >= a.n_groups) continue;
        const long c0 = seg_at(a, lo, n) + (w - slot_at(a, lo, n)) * kCChunk, end = seg_at(a, lo + 1, n);
        if (c0 >= end) continue;                                    // a slot the group does not need
        const int cnt = (int)min((long)kCChunk, end - c0);
        // the chunk's cell ids and labels, lane i holding cells i, i + 64, ...; -1 = takes no part (id or label out of range)
        int cell[kCPerLane], lab[kCPerLane];
#pragma unroll
        for (int u = 0; u < kCPerLane; ++u) {
            const int ci = u * 64 + lane;
            int r = ci < cnt ? a.order[c0 + ci] : -1;
            if ((unsigned long)(long)r >= (unsigned long)a.n_rows) r = -1;
            const int l = r >= 0 ? a.label[r] : -1;
            if (l < -1 || l >= C) r = -1;
            cell[u] = r; lab[u] = l;
        }
        for (int t = 0; t < passes; ++t) {
            const int cls = t * 64 + j0;                            // this lane's class
            double acc = 0.0, conf = 0.0;
            int vote = 0, n_on = 0, n_unsure = 0, n_bad = 0;
#pragma unroll
            for (int u = 0; u < kCPerLane; ++u) {
                const int here = min(64, cnt - u * 64);             // cells of this 64-block (<= 0: none)
                for (int i0 = 0; i0 < here; i0 += S) {
                    const int r = __shfl(cell[u], i0 + s, 64), lb = __shfl(lab[u], i0 + s, 64);
                    const bool valid = r >= 0;
                    const float* row = a.logits + (size_t)(valid ? r : 0) * a.ld;
                    float mx = -INFINITY, mine = -INFINITY;
                    int flag = 0;                                   // 1: a NaN, 2: a +inf
                    if (valid) {
                        for (int j = j0; j < C; j += 64) {
                            const float v = row[j];
                            if (v != v) flag |= 1;
                            else { if (v == INFINITY) flag |= 2; mx = fmaxf(mx, v); }
                            if (j == cls) mine = v;
                        }
                    }
#pragma unroll
                    for (int off = CP / 2; off >= 1; off >>= 1) {
                        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
                        flag |= __shfl_xor(flag, off, 64);
                    }
                    const bool ok = valid && flag == 0 && mx != -INFINITY;      // else bad: NaN, +inf or all -inf
                    double e = 0.0, z = 0.0;
                    if (ok) {
                        if (CP < 64) {
                            z = e = exp((double)mine - (double)mx);             // a lane beyond C holds -inf: 0
                        } else {
                            for (int j = j0; j < C; j += 64) {
                                const double ej = exp((double)row[j] - (double)mx);
                                z += ej;
                                if (j == cls) e = ej;
                            }
                        }
                    }
#pragma unroll
                    for (int off = CP / 2; off >= 1; off >>= 1) z += __shfl_xor(z, off, 64);
                    if (ok) {
                        acc += e / z;
                        vote += lb == cls;
                    }
                    if (j0 == 0 && t == 0) {
                        if (ok) { conf += 1.0 / z; n_on += 1; n_unsure += lb == -1; }
                        n_bad += valid && !ok;
                    }
                }
            }
#pragma unroll
            for (int off = 32; off >= CP; off >>= 1) {              // fold the cell slots: lane j0 of slot 0 keeps class j0
                acc += __shfl_xor(acc, off, 64);
                vote += __shfl_xor(vote, off, 64);
                conf += __shfl_xor(conf, off, 64);
                n_on += __shfl_xor(n_on, off, 64);
                n_unsure += __shfl_xor(n_unsure, off, 64);
                n_bad += __shfl_xor(n_bad, off, 64);
            }
            double* dp = a.dpart + (size_t)w * (C + 1);
            int* ip = a.ipart + (size_t)w * (C + 3);
            if (lane < CP && cls < C) { dp[cls] = acc; ip[cls] = vote; }
            if (lane == 0 && t == 0) { dp[C] = conf; ip[C] = n_on; ip[C + 1] = n_unsure; ip[C + 2] = n_bad; }
        }
    }
}

// one thread per output element: a group's chunk partials in ascending chunk order, then written or added to the output
__global__ void __launch_bounds__(256) class_finish_kernel(const CArgs a) {
    const int C = a.n_classes;
    const long per = (long)C + 4, total = (long)a.n_groups * per;
    const long n = entries(a);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long k = i / per;
        const int j = (int)(i % per);
        const long b = seg_at(a, k, n), e = seg_at(a, k + 1, n), first = slot_at(a, k, n);
        long chunks = e > b ? (e - b + kCChunk - 1) / kCChunk : 0;
        if (first + chunks > a.n_slots) chunks = first < a.n_slots ? a.n_slots - first : 0;      // malformed seg_ptr only
        if (j <= C) {                                               // prob_sum[k, j], or conf_sum[k] at j == C
            double sum = 0.0;
            for (long c = 0; c < chunks; ++c) sum += a.dpart[(size_t)(first + c) * (C + 1) + j];
            double* out = j < C ? a.prob_sum + (size_t)k * C + j : a.conf_sum + k;
            *out = a.accumulate ? *out + sum : sum;
        }
        if (j != C) {                                               // votes[k, j], or tally[k, j - C - 1] beyond
            const int q = j < C ? j : j - 1;                        // the column of ipart
            int sum = 0;
            for (long c = 0; c < chunks; ++c) sum += a.ipart[(size_t)(first + c) * (C + 3) + q];
            int* out = j < C ? a.votes + (size_t)k * C + j : a.tally + (size_t)k * 3 + (j - C - 1);
            *out = a.accumulate ? *out + sum : sum;
        }
    }
}

int64_t slots_of(int64_t n_rows, int32_t n_groups) { return n_rows / kCChunk + n_groups; }
// bytes of n_slots partials, or -1 when that is beyond int64 (sizes no device holds)
int64_t bytes_of(int64_t n_slots, int32_t C) {
    int64_t bytes;
    return __builtin_mul_overflow(n_slots, ((int64_t)C + 1) * 8 + ((int64_t)C + 3) * 4, &bytes) ? -1 : bytes;
}

template <int CP>
void launch_chunks(unsigned nb, hipStream_t st, const CArgs& a) {
    hipLaunchKernelGGL(class_chunk_kernel<CP>, dim3(nb), dim3(64 * kCWaves), 0, st, a);
}

}  // namespace

extern "C" int wgnn_group_class_reduce_workspace(int64_t n_rows, int32_t n_groups, int32_t n_classes, int64_t* bytes) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_group_class_reduce_workspace", what); };
    wgnn::error_clear();
    if (!bytes) return fail(WGNN_ERR_BAD_ARG, "bytes is required");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [0, 2^31)");
    if (n_groups <= 0) return fail(WGNN_ERR_BAD_ARG, "n_groups must be positive");
    if (n_classes <= 0) return fail(WGNN_ERR_BAD_ARG, "n_classes must be positive");
    const int64_t need = bytes_of(slots_of(n_rows, n_groups), n_classes);
    if (need < 0) return fail(WGNN_ERR_UNSUPPORTED, "the workspace of these sizes is beyond 2^63 bytes");
    *bytes = need;
    return WGNN_OK;
}

extern "C" int wgnn_group_class_reduce(const float* logits, int64_t ld_logits, const int32_t* label, const int32_t* order,
                                       const void* seg_ptr, int64_t n_rows, int32_t n_groups, int32_t n_classes,
                                       double* prob_sum, double* conf_sum, int32_t* votes, int32_t* tally,
                                       void* workspace, int64_t workspace_bytes, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_group_class_reduce", what); };
    wgnn::error_clear();
    if (!prob_sum || !conf_sum || !votes || !tally) return fail(WGNN_ERR_BAD_ARG, "prob_sum, conf_sum, votes and tally are required");
    if (!seg_ptr) return fail(WGNN_ERR_BAD_ARG, "seg_ptr is required");
    if (n_groups <= 0) return fail(WGNN_ERR_BAD_ARG, "n_groups must be positive");
    if (n_classes <= 0) return fail(WGNN_ERR_BAD_ARG, "n_classes must be positive");
    if (ld_logits < n_classes) return fail(WGNN_ERR_BAD_ARG, "ld_logits < n_classes");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [0, 2^31)");
    if (flags & ~(uint32_t)WGNN_CLUSTERS_ACCUMULATE) return fail(WGNN_ERR_BAD_ARG, "only WGNN_CLUSTERS_ACCUMULATE is a valid flag");
    if (!wgnn::aligned8(prob_sum) || !wgnn::aligned8(conf_sum)) return fail(WGNN_ERR_ALIGNMENT, "prob_sum and conf_sum must be 8-byte aligned");
    if (!wgnn::aligned8(seg_ptr)) return fail(WGNN_ERR_ALIGNMENT, "seg_ptr must be 8-byte aligned");
    if (!aligned4(logits) || !aligned4(label) || !aligned4(order) || !aligned4(votes) || !aligned4(tally))
        return fail(WGNN_ERR_ALIGNMENT, "logits, label, order, votes and tally must be 4-byte aligned");
    const int64_t n_slots = slots_of(n_rows, n_groups);
    if (workspace_bytes < 0) return fail(WGNN_ERR_WORKSPACE, "workspace_bytes is negative");
    const int64_t need = bytes_of(n_slots, n_classes);
    if (!workspace || need < 0 || workspace_bytes < need)
        return fail(WGNN_ERR_WORKSPACE, "workspace is missing or smaller than wgnn_group_class_reduce_workspace asks for");
    if (!wgnn::aligned8(workspace)) return fail(WGNN_ERR_ALIGNMENT, "workspace must be 8-byte aligned");
    CArgs a{};
    a.logits = logits; a.ld = ld_logits; a.label = label; a.order = order; a.seg = static_cast<const long long*>(seg_ptr);
    a.n_rows = n_rows; a.n_groups = n_groups; a.n_classes = n_classes; a.n_slots = n_slots;
    a.dpart = static_cast<double*>(workspace);
    a.ipart = reinterpret_cast<int*>(a.dpart + n_slots * ((int64_t)n_classes + 1));
    a.prob_sum = prob_sum; a.conf_sum = conf_sum; a.votes = votes; a.tally = tally;
    a.accumulate = (flags & WGNN_CLUSTERS_ACCUMULATE) ? 1 : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_rows > 0 && logits && label && order) {                   // else no cell takes part: the finish alone writes the outputs
        const int64_t want = (n_slots + kCWaves - 1) / kCWaves;
        const unsigned nb = (unsigned)(want < kCMaxBlocks ? want : kCMaxBlocks);
        int cp = 1;
        while (cp < 64 && cp < n_classes) cp <<= 1;
        switch (cp) {
            case 1: launch_chunks<1>(nb, st, a); break;
            case 2: launch_chunks<2>(nb, st, a); break;
            case 4: launch_chunks<4>(nb, st, a); break;
            case 8: launch_chunks<8>(nb, st, a); break;
            case 16: launch_chunks<16>(nb, st, a); break;
            case 32: launch_chunks<32>(nb, st, a); break;
            default: launch_chunks<64>(nb, st, a); break;
        }
        if (hipGetLastError() != hipSuccess) return fail(WGNN_ERR_LAUNCH, "HIP launch failed");
    }
    const int64_t items = (int64_t)n_groups * ((int64_t)n_classes + 4);
    const int64_t want = (items + 255) / 256;
    hipLaunchKernelGGL(class_finish_kernel, dim3((unsigned)(want < kCMaxBlocks ? want : kCMaxBlocks)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}
