// wgnn_knn.hip - wgnn_knn_rows: the exact k nearest candidates of every query row under squared Euclidean distance
// (include/wgnn.h has the contract).  Brute force, O(n_q * n_c * D); the [n_q, n_c] distance matrix is never stored.
//
// A workgroup of 256 threads holds a tile of 64 queries and streams tiles of 64 candidates past it, 16 columns of D at a time,
// through two LDS buffers (k-major, so a lane reads four queries or four candidates with one 16-byte read).  Each lane owns a
// 4 x 4 micro-tile of (query, candidate) pairs and carries its 16 distances in registers across the slabs of D:
//     t = q[j] - x[j];  d = fma(t, t, d) in f32;   j = 0 .. D-1 ascending, d = 0 to start
// - the difference form, one chain per pair, never re-associated.  Columns past D and rows past the end are loaded as zeros:
// fma(0, 0, d) == d, so padding changes no bit.
//
// Selection runs on the 64-bit key (bits(d) << 32 | candidate): d >= +0, so the f32 bits order as unsigned integers, every NaN
// sorts above +inf, and keys of one query are distinct - a total order.  Per query the k smallest keys live in LDS, sorted; a
// finished distance is compared with the k-th of them and a survivor is appended to the query's staging list (an LDS atomic
// claims the slot, nothing else is atomic).  A list that has taken more than 16 of its 32 slots is merged into the sorted list
// by one wavefront, every key placed at its rank in the union, and emptied; a lane whose key found no slot keeps it and
// appends again after the merge.  The order of a staging list depends on the hardware; the sorted set does not.
//
// With n_splits > 1 the candidate tiles are dealt to grid.y in contiguous ranges, every split writes its k keys per query
// into the workspace, and knn_merge - a wavefront per query, a lane per split - merges them under the same order.
// Symmetry (d(i, j) == d(j, i)) is not exploited: every ordered pair is computed.
//
// The tile - its geometry, the loader, the chain - is wgnn_pair_tile.h's, which wgnn_knn_segments.hip and wgnn_silhouette.hip
// run as well; the selection - the keys, the staging lists, the rank merge, the append rounds - is wgnn_topk_select.h's, shared
// with wgnn_knn_segments.hip.  This file keeps which rows a tile holds, the test that makes a pair a survivor, and the splits.
#include <limits.h>
#include "wgnn_build_rows.h"
#include "wgnn_pair_tile.h"
#include "wgnn_topk_select.h"

namespace wgnn {
namespace {

constexpr int kStage = 32;              // staging slots per query
constexpr int kStagePitch = kStage + 1; // 64-bit words between two queries' staging lists (odd: the merging lanes spread over banks)
constexpr int kMergeMark = 16;          // a staging list that has taken more keys than this is merged after the round
constexpr int kMaxK = 64;
constexpr int kMaxSplits = 64;          // knn_merge gives every split a lane

struct NArgs {
    const float* Q; long ld_q; const float* X; long ld_x;
    int n_q; int n_c; int D; int k;
    long self_offset; int n_splits;
    int* idx; float* d2; long ld_out;
    u64* ws;
};

inline int knn_lds_bytes(int k) {
    return kTQ * sorted_pitch(k) * 8 + kTQ * kStagePitch * 8 + 2 * kSlabFloats * 4 + kTQ * 4 + 16;
}

__global__ void __launch_bounds__(kPairBlock) knn_kernel(const NArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int k = a.k, sp = sorted_pitch(k);
    u64* s_sorted = reinterpret_cast<u64*>(smem);                               // [kTQ][sp]
    u64* s_stage = s_sorted + kTQ * sp;                                         // [kTQ][kStagePitch]
    float* s_slab = reinterpret_cast<float*>(s_stage + kTQ * kStagePitch);      // [2][2][kKS][kPitch]; 16-byte aligned: all above is 8 x even
    int* s_cnt = reinterpret_cast<int*>(s_slab + 2 * kSlabFloats);              // [kTQ]
    int* s_flag = s_cnt + kTQ;

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int ty = tid >> 4, tx = tid & 15;               // the micro-tile: queries ty*4 .. +3, candidates tx*4 .. +3
    const int lrow = tid >> 2, lk4 = tid & 3;             // the loader: row lrow of the tile, its float4 number lk4 of the slab
    const long q0 = (long)blockIdx.x * kTQ;
    const long n_tiles = ((long)a.n_c + kTC - 1) / kTC;
    const long t0 = n_tiles * blockIdx.y / a.n_splits, t1 = n_tiles * (blockIdx.y + 1) / a.n_splits;
    const int n_slabs = (a.D + kKS - 1) / kKS;

    for (int i = tid; i < kTQ * sp; i += kPairBlock) s_sorted[i] = kNone;
    if (tid < kTQ) s_cnt[tid] = 0;
    if (tid < 3) s_flag[tid] = 0;                         // "a lane has a survivor", and the two `over` words of the rounds

    const bool q_ok = q0 + lrow < a.n_q;
    const float* q_src = a.Q + (size_t)(q_ok ? q0 + lrow : 0) * a.ld_q + lk4 * 4;

    for (long t = t0; t < t1; ++t) {
        const long c0 = t * kTC;
        const bool x_ok = c0 + lrow < a.n_c;
        const float* x_src = a.X + (size_t)(x_ok ? c0 + lrow : 0) * a.ld_x + lk4 * 4;
        float acc[4][4];
        pair_tile_d2(acc, s_slab, q_src, q_ok, x_src, x_ok, a.D, n_slabs, tid);

        // selection: which of the 16 pairs beat their query's k-th key (read once; it only tightens)
        int cid[4];                                       // the lane's four candidates: one that counts is below n_c < 2^31
#pragma unroll
        for (int j = 0; j < 4; ++j) cid[j] = (int)(c0 + tx * 4 + j);
        unsigned mask = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long q = q0 + ty * 4 + i;
            const u64 kth = s_sorted[(ty * 4 + i) * sp + k - 1];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long c = c0 + tx * 4 + j;
                const u64 key = pair_key(acc[i][j], cid[j]);
                const bool self = a.self_offset >= 0 && c == a.self_offset + q;
                if (q < a.n_q && c < a.n_c && !self && key < kth) mask |= 1u << (i * 4 + j);
            }
        }
        stage_survivors(acc, cid, mask, s_sorted, s_stage, s_cnt, s_flag, kMergeMark, kStage, kStagePitch, sp, k, tid);
    }

    __syncthreads();
    merge_marked(s_sorted, s_stage, s_cnt, 0, kStage, kStagePitch, sp, k, wave, lane);
    __syncthreads();
    for (int e = tid; e < kTQ * k; e += kPairBlock) {
        const int ql = e / k, j = e - ql * k;
        const long q = q0 + ql;
        if (q >= a.n_q) continue;
        const u64 key = s_sorted[ql * sp + j];
        if (a.ws) {
            a.ws[((size_t)blockIdx.y * a.n_q + q) * k + j] = key;
        } else {
            a.idx[(size_t)q * a.ld_out + j] = key == kNone ? -1 : (int)(unsigned)key;
            a.d2[(size_t)q * a.ld_out + j] = __uint_as_float((unsigned)(key >> 32));
        }
    }
}

// a wavefront per query: lane s walks split s's sorted list, the wave takes the smallest head k times
__global__ void __launch_bounds__(256) knn_merge(const NArgs a) {
    const int lane = threadIdx.x & 63;
    const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.n_q) return;                               // wave-uniform
    const int k = a.k;
    const u64* mine = a.ws + ((size_t)(lane < a.n_splits ? lane : 0) * a.n_q + q) * k;
    int p = lane < a.n_splits ? 0 : k;
    u64 head = p < k ? mine[0] : kNone;
    for (int j = 0; j < k; ++j) {
        u64 best = head;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const u64 o = __shfl_xor(best, off, 64);
            best = o < best ? o : best;
        }
        if (lane == 0) {
            a.idx[(size_t)q * a.ld_out + j] = best == kNone ? -1 : (int)(unsigned)best;
            a.d2[(size_t)q * a.ld_out + j] = __uint_as_float((unsigned)(best >> 32));
        }
        if (head == best && p < k) {                      // real keys are distinct; among kNone heads any may advance
            ++p;
            head = p < k ? mine[p] : kNone;
        }
    }
}

LdsMarks g_knn_lds;

// 0 = chosen here: about 4096 workgroups - many rounds over the chip, so that the last one costs little - while every split
// keeps at least two candidate tiles (measured: profiles/resident_knn.md)
int resolve_splits(int64_t n_q, int64_t n_c, int32_t n_splits) {
    if (n_splits > 0) return n_splits;
    const int64_t q_tiles = (n_q + kTQ - 1) / kTQ, c_tiles = (n_c + kTC - 1) / kTC;
    int64_t want = q_tiles > 0 ? (4096 + q_tiles - 1) / q_tiles : 1;
    if (want > c_tiles / 2) want = c_tiles / 2;
    if (want > kMaxSplits) want = kMaxSplits;
    return want < 1 ? 1 : (int)want;
}

const char* check_sizes(int64_t n_q, int64_t n_c, int32_t k, int32_t n_splits, int* code) {
    *code = WGNN_ERR_BAD_ARG;
    if (n_q < 0 || n_q > INT32_MAX) return "n_q must be in [0, 2^31)";
    if (n_c < 0 || n_c > INT32_MAX) return "n_c must be in [0, 2^31)";
    if (n_splits < 0 || n_splits > kMaxSplits) return "n_splits must be in [0, 64] (0 = chosen from n_q and n_c)";
    *code = WGNN_ERR_UNSUPPORTED;
    if (k < 1 || k > kMaxK) return "k must be in [1, 64]";
    return nullptr;
}

int64_t workspace_bytes_for(int64_t n_q, int32_t k, int splits) { return splits > 1 ? (int64_t)splits * n_q * k * 8 : 0; }

}  // namespace
}  // namespace wgnn

using namespace wgnn;

extern "C" int wgnn_knn_workspace_bytes(int64_t n_q, int64_t n_c, int32_t k, int32_t n_splits, int64_t* bytes) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_knn_workspace_bytes", what); };
    wgnn::error_clear();
    if (!bytes) return fail(WGNN_ERR_BAD_ARG, "bytes is required");
    int code = 0;
    if (const char* what = check_sizes(n_q, n_c, k, n_splits, &code)) return fail(code, what);
    *bytes = workspace_bytes_for(n_q, k, resolve_splits(n_q, n_c, n_splits));
    return WGNN_OK;
}

extern "C" int wgnn_knn_rows(const float* Q, int64_t ld_q, int64_t n_q, const float* X, int64_t ld_x, int64_t n_c,
                             int32_t D, int32_t k, int64_t self_offset, int32_t n_splits,
                             int32_t* idx, float* d2, int64_t ld_out, void* workspace, int64_t workspace_bytes,
                             uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_knn_rows", what); };
    wgnn::error_clear();
    int code = 0;
    if (const char* what = check_sizes(n_q, n_c, k, n_splits, &code)) return fail(code, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (int rc = check_row_width("wgnn_knn_rows", D)) return rc;
    if (ld_q < D || ld_q % 4 || ld_x < D || ld_x % 4) return fail(WGNN_ERR_ALIGNMENT, "ld_q and ld_x must be >= D and multiples of 4");
    if (ld_out < k) return fail(WGNN_ERR_BAD_ARG, "ld_out must be >= k");
    if (self_offset < -1 || (self_offset >= 0 && self_offset + n_q > n_c))
        return fail(WGNN_ERR_BAD_ARG, "self_offset must be -1, or satisfy self_offset + n_q <= n_c");
    if (workspace_bytes < 0) return fail(WGNN_ERR_WORKSPACE, "workspace_bytes is negative");
    if (n_q == 0) return WGNN_OK;
    if (!Q || !idx || !d2 || (n_c > 0 && !X)) return fail(WGNN_ERR_BAD_ARG, "Q, X, idx and d2 are required");
    if (!aligned16(Q) || !aligned16(X)) return fail(WGNN_ERR_ALIGNMENT, "Q and X must be 16-byte aligned");
    if (!aligned4(idx) || !aligned4(d2)) return fail(WGNN_ERR_ALIGNMENT, "idx and d2 must be 4-byte aligned");
    const int splits = resolve_splits(n_q, n_c, n_splits);
    const int64_t need = workspace_bytes_for(n_q, k, splits);
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(WGNN_ERR_WORKSPACE, "workspace is smaller than wgnn_knn_workspace_bytes asks for");
    if (need > 0 && !aligned8(workspace)) return fail(WGNN_ERR_ALIGNMENT, "workspace must be 8-byte aligned");

    NArgs a{};
    a.Q = Q; a.ld_q = ld_q; a.X = X; a.ld_x = ld_x;
    a.n_q = (int)n_q; a.n_c = (int)n_c; a.D = D; a.k = k;
    a.self_offset = self_offset; a.n_splits = splits;
    a.idx = idx; a.d2 = d2; a.ld_out = ld_out;
    a.ws = need > 0 ? reinterpret_cast<u64*>(workspace) : nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto failed = [&fail]() { return fail(WGNN_ERR_LAUNCH, "HIP launch failed (or the LDS could not be reserved)"); };
    const int lds = knn_lds_bytes(k);
    if (raise_lds(g_knn_lds, reinterpret_cast<const void*>(knn_kernel), lds) != WGNN_OK) return failed();
    const unsigned q_tiles = (unsigned)((n_q + kTQ - 1) / kTQ);
    hipLaunchKernelGGL(knn_kernel, dim3(q_tiles, (unsigned)splits), dim3(kPairBlock), lds, st, a);
    if (hipGetLastError() != hipSuccess) return failed();
    if (need == 0) return WGNN_OK;
    hipLaunchKernelGGL(knn_merge, dim3((unsigned)((n_q + 3) / 4)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : failed();
}
