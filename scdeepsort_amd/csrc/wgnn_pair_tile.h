// wgnn_pair_tile.h - the brute-force pair tile that wgnn_knn.hip, wgnn_knn_segments.hip and wgnn_silhouette.hip share: a
// workgroup of 256 threads holds 64 query rows and takes one tile of 64 candidate rows past them, 16 columns of D at a time,
// through two LDS buffers (k-major, so a lane reads four queries or four candidates with one 16-byte read).  Each lane owns a
// 4 x 4 micro-tile of (query, candidate) pairs and carries its 16 squared distances in registers across the slabs of D:
//     t = q[j] - x[j];  d = fmaf(t, t, d);   j = 0 .. D-1 ascending, d = 0 to start
// - the difference form, one chain per pair, never re-associated.  A pair's distance carries the same bits whichever entry
// computed it because every entry computes it HERE: the chain below is the only one of the three files.
//
// What a caller keeps: which rows its loader thread fetches (a plain row, a gathered one, a position within a group) and what
// becomes of the 16 distances (a top-k selection: wgnn_topk_select.h; a sum per group).
#pragma once
#include "wgnn_common.h"

namespace wgnn {

constexpr int kTQ = 64;                 // queries of a workgroup
constexpr int kTC = 64;                 // candidates of a tile: part of the addition order of wgnn_silhouette.hip's sums, so
                                        // a constraint on all three users - never tuned per device
constexpr int kKS = 16;                 // columns of D per slab
constexpr int kPitch = kTQ + 4;         // floats between two k-rows of a slab: 16-byte aligned, transposing writes 2-way at worst
constexpr int kSlabFloats = 2 * kKS * kPitch;             // one buffer: the query slab, then the candidate slab
constexpr int kPairBlock = 256;         // threads of a workgroup: 16 x 16 micro-tiles, 64 rows x 4 loaders
constexpr int kMaxD = 1024;

// The checks every entry makes of its row width, where it has always made them (after the flags, before its own ld_* check):
// `fn` names the entry point in the error detail; WGNN_OK = go on.
inline int check_row_width(const char* fn, int32_t D) {
    if (D < 4 || D > kMaxD) return fail(WGNN_ERR_UNSUPPORTED, fn, "D must be in [4, 1024]");
    if (D % 4) return fail(WGNN_ERR_ALIGNMENT, fn, "D must be a multiple of 4 (zero-pad the rows)");
    return WGNN_OK;
}

// the loader's store: a thread holds float4 number lk4 of row lrow of a slab and writes it transposed, to the columns
// lk4 * 4 + i of the slab, row lrow.  The address is spelled as the kernels' own loaders spelled it (measured:
// profiles/pair_tile_refactor.md section 3)
__device__ __forceinline__ void put(float* dst, const float4& v, int lrow, int lk4) {
    float* p = dst + (lk4 * 4) * kPitch + lrow;
    p[0] = v.x; p[kPitch] = v.y; p[2 * kPitch] = v.z; p[3 * kPitch] = v.w;
}

// acc[i][j] = the squared distance of query ty * 4 + i and candidate tx * 4 + j of the tile (ty = tid >> 4, tx = tid & 15), for
// all 256 threads of the workgroup together.  q_src / x_src: the loader's row (row tid >> 2 of the query tile / of the candidate
// tile) at its column (tid & 3) * 4; q_ok / x_ok: that row exists.  A missing row and the columns from D on are loaded as
// zeros: fmaf(0, 0, d) == d, so padding changes no bit.  s_slab: [2][2][kKS][kPitch] floats, 16-byte aligned.
//
// Barriers: the one after the first store also orders whatever the workgroup did before the call - the caller's set-up, the
// last tile's selection or sums - before this tile's; the last slab's barrier ends the function, so that the next call may
// write the first buffer at once.  A caller needs no barrier of its own between two calls.
__device__ __forceinline__ void pair_tile_d2(float (&acc)[4][4], float* s_slab, const float* q_src, bool q_ok,
                                             const float* x_src, bool x_ok, int D, int n_slabs, int tid) {
    const int ty = tid >> 4, tx = tid & 15, lrow = tid >> 2, lk4 = tid & 3;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    float4 gq = (q_ok && lk4 * 4 < D) ? ld4(q_src) : zero4;
    float4 gx = (x_ok && lk4 * 4 < D) ? ld4(x_src) : zero4;
    put(s_slab, gq, lrow, lk4); put(s_slab + kKS * kPitch, gx, lrow, lk4);
    __syncthreads();
    for (int s = 0; s < n_slabs; ++s) {
        const bool more = s + 1 < n_slabs;
        if (more) {
            const int col = (s + 1) * kKS + lk4 * 4;
            gq = (q_ok && col < D) ? ld4(q_src + (s + 1) * kKS) : zero4;
            gx = (x_ok && col < D) ? ld4(x_src + (s + 1) * kKS) : zero4;
        }
        const float* qs = s_slab + (s & 1) * kSlabFloats + ty * 4;
        const float* xs = s_slab + (s & 1) * kSlabFloats + kKS * kPitch + tx * 4;
#pragma unroll 8
        for (int kk = 0; kk < kKS; ++kk) {
            const float4 qa = ld4(qs + kk * kPitch), xb = ld4(xs + kk * kPitch);
            const float qv[4] = {qa.x, qa.y, qa.z, qa.w}, xv[4] = {xb.x, xb.y, xb.z, xb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d = qv[i] - xv[j];
                    acc[i][j] = fmaf(d, d, acc[i][j]);
                }
        }
        if (more) {
            float* nb = s_slab + ((s + 1) & 1) * kSlabFloats;
            put(nb, gq, lrow, lk4); put(nb + kKS * kPitch, gx, lrow, lk4);
        }
        __syncthreads();
    }
}

}  // namespace wgnn
