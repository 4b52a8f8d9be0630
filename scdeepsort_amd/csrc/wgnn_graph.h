// wgnn_graph.h - what the kernels over a CSR graph share (wgnn_louvain.hip, wgnn_leiden.hip, wgnn_umap.hip, wgnn_geodesic.hip).
// Integer code only, so a file that pins its floating point (#pragma clang fp contract(off)) includes it without a change.
//   - for all four: the 64-bit integer types, the clamp of a rowptr entry, the grid of a launch and the n / nnz check;
//   - for the two cluster files: the kin sweep.  kin[K], the weight from a vertex v into key K (a community, a refined community),
//     is collected in a table keyed by K, and the candidate keys are scored against each other.  Three routes by row length:
//       rows of at most wave_rows (<= 128) entries: one wavefront (a workgroup of 64 threads), an LDS table of 256 slots;
//       rows of at most block_rows (<= 2048) entries: a workgroup of 256 threads, an LDS table of 4096 slots;
//       longer rows (a hub cell): a workgroup with a dense int32 scratch per key in global memory, zero before and after.
//     Tables are open addressing, a compare-and-swap on the key and an integer add on the value; at most half full.  The
//     candidates are under a total order (higher score, lower id), and every sum and comparison is an integer's: neither the route
//     nor the order of the atomics changes a bit.  A kernel supplies a policy (below) with what is its own - which key a
//     neighbour has, how a candidate scores, what is written - and the host side checks the route operands in one place.
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
// is x a vertex / community id of a graph of n vertices?
__device__ __forceinline__ bool is_id(int x, long n) { return (unsigned long)(unsigned)x < (unsigned long)n; }

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

// ---------------------------------------------------------------------------------------------------------------------------
// The kin sweep.  What its two kernels read of the graph and of the routes; a kernel's arguments embed it as `g`.
struct KinGraph {
    const i64* rowptr; const int* col; const int* w; long n; long nnz;
    const int* heavy; int n_heavy; int wave_rows; int block_rows;    // heavy[]: the rows above wave_rows
    int* scratch; int scratch_blocks;                                // the dense scratch [scratch_blocks, n], or null
    u64* stats;                                                      // stats[3]: the status word, only ever OR-ed into
};

// A policy P names the kernel's arguments and says what differs between the sweeps:
//   typedef ... Args;                 the kernel's arguments, with a KinGraph `g`
//   struct Vertex;                    what P keeps of the vertex at hand
//   static bool enter(a, v, x)        fills x; false = v stays and its row is not read.  Reads global memory alone and depends on
//                                     nothing but (a, v): the SAME ANSWER IN EVERY THREAD of the workgroup, because the barriers
//                                     of a route lie behind it.  It may OR a bit into the status word.
//   static int key(a, x, v, u)        the key of neighbour u of v, or -1 when u adds nothing to kin
//   static constexpr bool kOwnKin     with it: static int own(x), and static void own_kin(a, x, kin) receives kin[own(x)] in
//                                     every thread once the sums stand, before a candidate is scored
//   static void consider(b, a, x, K, kin)   key K with kin[K] = kin against the best so far; seeing a key twice changes nothing
//   static void write(a, v, x, b)     one thread: what v leaves.  b.c < 0: it stays, and x may not be filled
//
// One vertex by the THREADS threads of a workgroup through an LDS table of SLOTS slots (the row has at most SLOTS / 2 entries).
template <class P, int THREADS, int SLOTS>
__device__ __forceinline__ Best kin_in_lds(const typename P::Args& a, long v, i64 e0, i64 e1, typename P::Vertex& x, int* keys, int* vals) {
    const KinGraph& g = a.g;
    const int tid = threadIdx.x;
    for (int s = tid; s < SLOTS; s += THREADS) { keys[s] = -1; vals[s] = 0; }
    __syncthreads();
    for (i64 e = e0 + tid; e < e1; e += THREADS) {
        const int K = P::key(a, x, v, g.col[e]);
        if (K >= 0) table_add<SLOTS>(keys, vals, K, g.w[e]);
    }
    __syncthreads();
    if constexpr (P::kOwnKin) P::own_kin(a, x, (i64)table_get<SLOTS>(keys, vals, P::own(x)));
    Best b{0, -1};
    for (int s = tid; s < SLOTS; s += THREADS)
        if (keys[s] >= 0) P::consider(b, a, x, keys[s], (i64)vals[s]);
    __syncthreads();                                           // the table is free for the next vertex
    return b;
}

// The same through the workgroup's dense scratch kin[n]: zero on entry, zero again on return.  The sums are made by atomics, so
// they are read and zeroed where those ran (relaxed, agent scope).
template <class P, int THREADS>
__device__ __forceinline__ Best kin_in_scratch(const typename P::Args& a, long v, i64 e0, i64 e1, typename P::Vertex& x, int* kin) {
    const KinGraph& g = a.g;
    const int tid = threadIdx.x;
    for (i64 e = e0 + tid; e < e1; e += THREADS) {
        const int K = P::key(a, x, v, g.col[e]);
        if (K >= 0) atomicAdd(&kin[K], g.w[e]);
    }
    __syncthreads();
    if constexpr (P::kOwnKin) P::own_kin(a, x, (i64)__hip_atomic_load(&kin[P::own(x)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    Best b{0, -1};
    for (i64 e = e0 + tid; e < e1; e += THREADS) {
        const int K = P::key(a, x, v, g.col[e]);
        if (K >= 0) P::consider(b, a, x, K, (i64)__hip_atomic_load(&kin[K], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    __syncthreads();
    for (i64 e = e0 + tid; e < e1; e += THREADS) {             // zero again, for the next long row and the next sweep
        const int K = P::key(a, x, v, g.col[e]);
        if (K >= 0) __hip_atomic_store(&kin[K], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return b;
}

// rows of at most wave_rows entries, under __launch_bounds__(64): a workgroup IS a wavefront, so its barriers cost nothing.  A row
// without an entry stays and P::enter is not asked.
template <class P>
__device__ __forceinline__ void kin_sweep_wave(const typename P::Args& a) {
    __shared__ int keys[kWaveSlots];
    __shared__ int vals[kWaveSlots];
    const KinGraph& g = a.g;
    for (long v = blockIdx.x; v < g.n; v += gridDim.x) {
        const i64 e0 = clampl(g.rowptr[v], g.nnz), e1 = clampl(g.rowptr[v + 1], g.nnz);
        if (e1 - e0 > g.wave_rows) continue;                  // the heavy kernel's
        typename P::Vertex x;
        Best b{0, -1};
        if (e1 > e0 && P::enter(a, v, x)) {
            b = kin_in_lds<P, 64, kWaveSlots>(a, v, e0, e1, x, keys, vals);
            wave_best(b);
        }
        if (threadIdx.x == 0) P::write(a, v, x, b);
    }
}

// the rows above wave_rows (heavy[]), under __launch_bounds__(256): an LDS table up to block_rows entries, the workgroup's dense
// scratch beyond.  Every barrier is reached by the whole workgroup: v, the row's length and P::enter's answer are uniform.
template <class P>
__device__ __forceinline__ void kin_sweep_heavy(const typename P::Args& a) {
    __shared__ int keys[kBlockSlots];
    __shared__ int vals[kBlockSlots];
    __shared__ i64 s_score[4];
    __shared__ int s_c[4];
    const KinGraph& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int h = blockIdx.x; h < g.n_heavy; h += gridDim.x) {
        const long v = g.heavy[h];
        if (v < 0 || v >= g.n) continue;
        const i64 e0 = clampl(g.rowptr[v], g.nnz), e1 = clampl(g.rowptr[v + 1], g.nnz);
        typename P::Vertex x;
        Best b{0, -1};
        if (!P::enter(a, v, x)) {
            // stays
        } else if (e1 - e0 <= g.block_rows) {
            b = kin_in_lds<P, 256, kBlockSlots>(a, v, e0, e1, x, keys, vals);
        } else if (g.scratch && (int)blockIdx.x < g.scratch_blocks) {
            b = kin_in_scratch<P, 256>(a, v, e0, e1, x, g.scratch + (size_t)blockIdx.x * g.n);
        } else {                                               // a long row and no scratch: the caller sized the workspace wrong
            if (tid == 0) atomicOr(&g.stats[3], (u64)WGNN_LOUVAIN_NO_SCRATCH);
        }
        wave_best(b);
        if (lane == 0) { s_score[wave] = b.score; s_c[wave] = b.c; }
        __syncthreads();
        if (tid == 0) {
            Best all{0, -1};
            for (int i = 0; i < 4; ++i) merge(all, s_score[i], s_c[i]);
            P::write(a, v, x, all);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
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

// A refused call: code == WGNN_OK means none.  The route operands of a sweep entry are checked in two steps, because the entry's
// own alignment checks stand between them.
struct Refusal { int code; const char* what; };

inline Refusal check_routes(const int32_t* heavy, int32_t n_heavy, int32_t wave_rows, int32_t block_rows, int32_t scratch_blocks) {
    if (n_heavy < 0 || (n_heavy > 0 && !heavy)) return {WGNN_ERR_BAD_ARG, "n_heavy is negative, or heavy is missing"};
    if (wave_rows < 0 || wave_rows > kWaveRows) return {WGNN_ERR_UNSUPPORTED, "wave_rows must be in [0, 128]"};
    if (block_rows < 0 || block_rows > kBlockRows) return {WGNN_ERR_UNSUPPORTED, "block_rows must be in [0, 2048]"};
    if (scratch_blocks < 0 || scratch_blocks > kMaxScratchBlocks) return {WGNN_ERR_BAD_ARG, "scratch_blocks must be in [0, 256]"};
    return {WGNN_OK, nullptr};
}

inline Refusal check_scratch(int64_t n, const void* workspace, int64_t workspace_bytes, int32_t scratch_blocks) {
    if (workspace_bytes < 0) return {WGNN_ERR_WORKSPACE, "workspace_bytes is negative"};
    if (scratch_blocks > 0 && (!workspace || workspace_bytes < scratch_bytes(n, scratch_blocks)))
        return {WGNN_ERR_WORKSPACE, "workspace is missing or smaller than wgnn_louvain_sweep_workspace_bytes asks for"};
    if (!aligned4(workspace)) return {WGNN_ERR_ALIGNMENT, "workspace must be 4-byte aligned"};
    return {WGNN_OK, nullptr};
}

// the graph and route fields of a sweep's arguments, once both checks have passed
inline KinGraph kin_graph(const int64_t* rowptr, const int32_t* col, const int32_t* w, int64_t n, int64_t nnz, const int32_t* heavy,
                          int32_t n_heavy, int32_t wave_rows, int32_t block_rows, void* workspace, int32_t scratch_blocks,
                          int64_t* stats) {
    return KinGraph{reinterpret_cast<const i64*>(rowptr), col, w, (long)n, (long)nnz, heavy, n_heavy, wave_rows, block_rows,
                    scratch_blocks > 0 ? static_cast<int*>(workspace) : nullptr, scratch_blocks, reinterpret_cast<u64*>(stats)};
}

// the heavy kernel's grid (n_heavy > 0): with a scratch, a workgroup per slice of it
inline unsigned heavy_grid(int32_t n_heavy, int32_t scratch_blocks) {
    return scratch_blocks > 0 ? (unsigned)(n_heavy < scratch_blocks ? n_heavy : scratch_blocks) : grid_for(n_heavy, 1);
}

}  // namespace graph
}  // namespace wgnn
