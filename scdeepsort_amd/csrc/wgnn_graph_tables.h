// wgnn_graph_tables.h - what the integer graph-cluster kernels share (wgnn_louvain.hip, wgnn_leiden.hip): the limits of the three
// routes by row length, the open-addressing LDS table keyed by a community id (a compare-and-swap on the key and an integer add on
// the value; at most half full), the total order of the candidates (higher score, lower id) and the integer reductions.
#pragma once
#include <limits.h>
#include "wgnn_common.h"

namespace wgnn {
namespace graph {

constexpr int kWaveSlots = 256, kWaveRows = 128;
constexpr int kBlockSlots = 4096, kBlockRows = 2048;
constexpr int kMaxBlocks = 8192;
constexpr int kMaxScratchBlocks = 256;

typedef long long i64;
typedef unsigned long long u64;

__device__ __forceinline__ i64 clampl(i64 v, i64 hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

struct Best { i64 score; int c; };
__device__ __forceinline__ void merge(Best& b, i64 score, int c) {
    if (c >= 0 && (b.c < 0 || score > b.score || (score == b.score && c < b.c))) { b.score = score; b.c = c; }
}
__device__ __forceinline__ void wave_best(Best& b) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const i64 so = __shfl_xor(b.score, off, 64);
        const int co = __shfl_xor(b.c, off, 64);
        merge(b, so, co);
    }
}

template <int SLOTS>
__device__ __forceinline__ int slot_of(int C) { return (int)(((unsigned)C * 2654435761u) >> 16) & (SLOTS - 1); }

template <int SLOTS>
__device__ __forceinline__ void table_add(int* keys, int* vals, int C, int w) {
    int s = slot_of<SLOTS>(C);
    for (;;) {
        const int seen = atomicCAS(&keys[s], -1, C);
        if (seen == -1 || seen == C) { atomicAdd(&vals[s], w); return; }
        s = (s + 1) & (SLOTS - 1);
    }
}
template <int SLOTS>
__device__ __forceinline__ int table_get(const int* keys, const int* vals, int C) {
    int s = slot_of<SLOTS>(C);
    for (;;) {
        const int seen = keys[s];
        if (seen == C) return vals[s];
        if (seen == -1) return 0;
        s = (s + 1) & (SLOTS - 1);
    }
}

// the sum of v over the workgroup's 256 threads, in thread 0 (integers: the order is free)
__device__ __forceinline__ i64 block_sum(i64 v, i64* s_red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

inline unsigned grid_for(int64_t items, int per_block) {
    const int64_t want = (items + per_block - 1) / per_block;
    return (unsigned)(want < 1 ? 1 : (want < kMaxBlocks ? want : kMaxBlocks));
}

inline const char* check_graph_sizes(int64_t n, int64_t nnz) {
    if (n < 0 || n > INT32_MAX) return "n must be in [0, 2^31)";
    if (nnz < 0) return "nnz must not be negative";
    return nullptr;
}

inline int64_t scratch_bytes(int64_t n, int32_t scratch_blocks) { return n * 4 * (int64_t)scratch_blocks; }

}  // namespace graph
}  // namespace wgnn
