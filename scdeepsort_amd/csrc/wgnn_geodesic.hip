// wgnn_geodesic.hip - one round of a synchronous Bellman-Ford on a symmetric CSR with float32 edge lengths, behind
// ops.geodesic_rows / api.ResidentPredictor.pseudotime (include/wgnn.h has the contract).  A round reads the state before it
// (dist_in / pred_in) and writes a new one (dist_out / pred_out): no atomics on either, so the only floating-point operation -
// one rounded add per stored entry - and every comparison see the same operands whatever the grid.
//
// WGNN_GEODESIC_LANES = 16 lanes serve a row, four rows a wavefront (wgnn_layout_epoch's grouping: a union row of a k = 15 graph
// holds about 26 entries).  Lane l takes the row's entries l, l + 16, ... and keeps the least (cand, u) it met; the sixteen partial
// minima fold by halves.  (cand, u) is a total order and its minimum associative and commutative, so neither the lane count nor
// the fold changes a bit.  A hub row is a longer loop for its sixteen lanes.  Plain C++: no LDS, no scratch, no inline assembly.
// The integer types, the rowptr clamp, the grid and the n / nnz check are wgnn_graph.h's, shared with the other graph files; that
// header holds integer code only, so the contraction switched off below covers every floating-point operation of this file.
#include <float.h>
#include <limits.h>
#include <math.h>
#include "wgnn_graph.h"

#pragma clang fp contract(off)

namespace {
using namespace wgnn;
using namespace wgnn::graph;

constexpr int kLanes = WGNN_GEODESIC_LANES;        // lanes per row
constexpr int kRowsPerBlock = 256 / kLanes;
static_assert(kLanes == 16, "the fold below and include/wgnn.h state sixteen lanes");
static_assert(kMaxBlocks == WGNN_GEODESIC_MAX_BLOCKS, "grid_for's cap is the largest grid include/wgnn.h states");

struct GArgs {
    const i64* rowptr; const int* col; const float* length; long n; long nnz;
    const float* dist_in; const int* pred_in; float* dist_out; int* pred_out;
    u64* changed; u64* status;
};

__global__ void __launch_bounds__(256) geodesic_round_kernel(const GArgs a) {
    const int sub = threadIdx.x & (kLanes - 1), slot = threadIdx.x / kLanes;
    unsigned bits = 0;
    int changed = 0;
    for (long v = (long)blockIdx.x * kRowsPerBlock + slot; v < a.n; v += (long)gridDim.x * kRowsPerBlock) {
        i64 e0 = a.rowptr[v], e1 = a.rowptr[v + 1];
        if (e0 < 0 || e1 < e0 || e1 > a.nnz || (v == 0 && e0 != 0) || (v == a.n - 1 && e1 != a.nnz)) {
            bits |= WGNN_GEODESIC_BAD_ROWPTR;                      // nothing outside [0, nnz) is read
            e0 = clampl(e0, a.nnz);
            e1 = e1 < e0 ? e0 : (e1 > a.nnz ? a.nnz : e1);     // not clampl: a row that runs backwards is empty
        }
        float best = HUGE_VALF;
        int from = INT_MAX;
        for (i64 e = e0 + sub; e < e1; e += kLanes) {
            const int u = a.col[e];
            const float len = a.length[e];
            if (e > e0 && a.col[e - 1] >= u) bits |= WGNN_GEODESIC_UNSORTED;
            if (u < 0 || u >= a.n) { bits |= WGNN_GEODESIC_BAD_COL; continue; }
            if (!(len >= 0.f && len <= FLT_MAX)) { bits |= WGNN_GEODESIC_BAD_LENGTH; continue; }     // negative, infinite or NaN
            const float du = a.dist_in[u];
            if (!(du <= FLT_MAX)) continue;                        // u is not reached yet
            const float cand = du + len;
            if (cand < best || (cand == best && u < from)) { best = cand; from = u; }
        }
#pragma unroll
        for (int off = kLanes / 2; off >= 1; off >>= 1) {
            const float ob = __shfl_xor(best, off, kLanes);
            const int of = __shfl_xor(from, off, kLanes);
            if (ob < best || (ob == best && of < from)) { best = ob; from = of; }
        }
        if (sub == 0) {
            const float dv = a.dist_in[v];
            if (best < dv) {
                a.dist_out[v] = best;
                a.pred_out[v] = from;
                ++changed;
            } else {
                a.dist_out[v] = dv;
                a.pred_out[v] = a.pred_in[v];
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {                      // the loop is over: the whole wavefront is here
        changed += __shfl_xor(changed, off, 64);
        bits |= (unsigned)__shfl_xor((int)bits, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (changed) atomicAdd(a.changed, (u64)changed);
        if (bits) atomicOr(a.status, (u64)bits);
    }
}

}  // namespace

extern "C" int wgnn_geodesic_round(const int64_t* rowptr, const int32_t* col, const float* length, int64_t n, int64_t nnz,
                                   const float* dist_in, const int32_t* pred_in, float* dist_out, int32_t* pred_out,
                                   int64_t* changed, int64_t* status, int32_t grid_blocks, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_geodesic_round", what); };
    wgnn::error_clear();
    if (const char* what = check_graph_sizes(n, nnz)) return fail(WGNN_ERR_BAD_ARG, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (grid_blocks < 0 || grid_blocks > kMaxBlocks) return fail(WGNN_ERR_BAD_ARG, "grid_blocks must be in [0, 8192] (0 = from n)");
    if (!rowptr || !col || !length || !dist_in || !pred_in || !dist_out || !pred_out || !changed || !status)
        return fail(WGNN_ERR_BAD_ARG, "rowptr, col, length, dist_in, pred_in, dist_out, pred_out, changed and status are required");
    if (dist_in == dist_out || pred_in == pred_out)
        return fail(WGNN_ERR_BAD_ARG, "dist_out / pred_out must be other buffers than dist_in / pred_in (a round reads the state before it)");
    if (!aligned8(rowptr) || !aligned8(changed) || !aligned8(status))
        return fail(WGNN_ERR_ALIGNMENT, "rowptr, changed and status must be 8-byte aligned");
    if (!aligned4(col) || !aligned4(length) || !aligned4(dist_in) || !aligned4(pred_in) || !aligned4(dist_out) || !aligned4(pred_out))
        return fail(WGNN_ERR_ALIGNMENT, "col, length, dist_in, pred_in, dist_out and pred_out must be 4-byte aligned");
    if (n == 0) return WGNN_OK;
    GArgs a{};
    a.rowptr = reinterpret_cast<const i64*>(rowptr); a.col = col; a.length = length; a.n = n; a.nnz = nnz;
    a.dist_in = dist_in; a.pred_in = pred_in; a.dist_out = dist_out; a.pred_out = pred_out;
    a.changed = reinterpret_cast<u64*>(changed); a.status = reinterpret_cast<u64*>(status);
    unsigned blocks = grid_for(n, kRowsPerBlock);
    if (grid_blocks && (unsigned)grid_blocks < blocks) blocks = (unsigned)grid_blocks;
    hipLaunchKernelGGL(geodesic_round_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}
