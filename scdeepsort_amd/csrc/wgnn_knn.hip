// wgnn_knn.hip - wgnn_knn_rows: the exact k nearest candidates of every query row under squared Euclidean distance
// (include/wgnn.h has the contract).  Brute force, O(n_q * n_c * D); the [n_q, n_c] distance matrix is never stored.
//
// A workgroup of 256 threads holds a tile of 64 queries and streams tiles of 64 candidates past it, 16 columns of D at a time,
// through two LDS buffers (k-major, so a lane reads four queries or four candidates with one 16-byte read).  Each lane owns a
// 4 x 4 micro-tile of (query, candidate) pairs and carries its 16 distances in registers across the slabs of D:
//     t = q[j] - x[j];  d = fmaf(t, t, d);   j = 0 .. D-1 ascending, d = 0 to start
// - the difference form, one chain per pair, never re-associated.  Columns past D and rows past the end are loaded as zeros:
// fmaf(0, 0, d) == d, so padding changes no bit.
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
#include <limits.h>
#include "wgnn_build_rows.h"

namespace wgnn {
namespace {

constexpr int kTQ = 64;                 // queries of a workgroup
constexpr int kTC = 64;                 // candidates of a tile
constexpr int kKS = 16;                 // columns of D per slab
constexpr int kPitch = kTQ + 4;         // floats between two k-rows of a slab: 16-byte aligned, transposing writes 2-way at worst
constexpr int kStage = 32;              // staging slots per query
constexpr int kStagePitch = kStage + 1; // 64-bit words between two queries' staging lists (odd: the merging lanes spread over banks)
constexpr int kMergeMark = 16;          // a staging list that has taken more keys than this is merged after the round
constexpr int kKnnBlock = 256;
constexpr int kMaxK = 64;
constexpr int kMaxD = 1024;
constexpr int kMaxSplits = 64;          // knn_merge gives every split a lane
constexpr int kSlabFloats = 2 * kKS * kPitch;             // one buffer: the query slab, then the candidate slab
typedef unsigned long long u64;
constexpr u64 kNone = ((u64)0x7f800000u << 32) | 0x7fffffffu;        // (+inf, no candidate): above every selectable key

struct NArgs {
    const float* Q; long ld_q; const float* X; long ld_x;
    int n_q; int n_c; int D; int k;
    long self_offset; int n_splits;
    int* idx; float* d2; long ld_out;
    u64* ws;
};

__host__ __device__ inline int sorted_pitch(int k) { return k | 1; }          // odd, as kStagePitch

inline int knn_lds_bytes(int k) {
    return kTQ * sorted_pitch(k) * 8 + kTQ * kStagePitch * 8 + 2 * kSlabFloats * 4 + kTQ * 4 + 16;
}

// Merge the n <= kStage staged keys of one query into its sorted list of k, one WAVEFRONT's work, by rank: a lane takes up to
// two keys of the union (k + n <= 96), counts the keys below each - every lane reads the whole union, one broadcast read per
// key - and stores a real key whose rank is below k at that rank.  Real keys are distinct, so the ranks below k are taken once
// each; kNone is above every real key, keeps its place at the tail (the real keys only grow in number) and is never stored.
// All of a lane's reads are issued before its first store, and a wavefront's LDS operations complete in order.
__device__ __forceinline__ void merge_staged(u64* list, const u64* stage, int n, int k, int lane) {
    const int total = k + n;
    const u64 mine0 = lane < k ? list[lane] : (lane < total ? stage[lane - k] : kNone);
    const u64 mine1 = lane + 64 < total ? stage[lane + 64 - k] : kNone;          // k <= 64: the second key is a staged one
    int r0 = 0, r1 = 0;
    for (int e = 0; e < k; ++e) { const u64 v = list[e]; r0 += v < mine0; r1 += v < mine1; }
    for (int e = 0; e < n; ++e) { const u64 v = stage[e]; r0 += v < mine0; r1 += v < mine1; }
    __builtin_amdgcn_wave_barrier();                      // the compiler keeps the stores below the reads
    if (mine0 != kNone && r0 < k) list[r0] = mine0;
    if (mine1 != kNone && r1 < k) list[r1] = mine1;
}

// Every query of the workgroup whose staging count is above `mark` is merged and its count cleared: wavefront w looks after
// the queries w, w + 4, ...; its first 16 lanes read their counts, a ballot names the lists to merge.  A count above kStage
// says that appends found no slot (their lanes still hold the keys): the list holds kStage keys.
__device__ __forceinline__ void merge_marked(u64* s_sorted, const u64* s_stage, int* s_cnt, int mark, int sp, int k, int wave, int lane) {
    const int mine = wave + (kKnnBlock / 64) * (lane & 15);
    const int n = s_cnt[mine];
    unsigned long long todo = __ballot(lane < 16 && n > mark);
    while (todo) {                                        // wave-uniform
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int ql = wave + (kKnnBlock / 64) * b;
        merge_staged(s_sorted + ql * sp, s_stage + ql * kStagePitch, min(__shfl(n, b, 64), kStage), k, lane);
        if (lane == 0) s_cnt[ql] = 0;
    }
}

__global__ void __launch_bounds__(kKnnBlock) knn_kernel(const NArgs a) {
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

    for (int i = tid; i < kTQ * sp; i += kKnnBlock) s_sorted[i] = kNone;
    if (tid < kTQ) s_cnt[tid] = 0;
    if (tid < 3) s_flag[tid] = 0;                         // "a lane has a survivor", and the two `over` words of the rounds

    const bool q_ok = q0 + lrow < a.n_q;
    const float* q_src = a.Q + (size_t)(q_ok ? q0 + lrow : 0) * a.ld_q + lk4 * 4;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto put = [&](float* dst, const float4& v) {         // transposed: column lk4*4 + i of the slab, row lrow
        float* p = dst + (lk4 * 4) * kPitch + lrow;
        p[0] = v.x; p[kPitch] = v.y; p[2 * kPitch] = v.z; p[3 * kPitch] = v.w;
    };

    for (long t = t0; t < t1; ++t) {
        const long c0 = t * kTC;
        const bool x_ok = c0 + lrow < a.n_c;
        const float* x_src = a.X + (size_t)(x_ok ? c0 + lrow : 0) * a.ld_x + lk4 * 4;
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

        float4 gq = (q_ok && lk4 * 4 < a.D) ? ld4(q_src) : zero4;
        float4 gx = (x_ok && lk4 * 4 < a.D) ? ld4(x_src) : zero4;
        put(s_slab, gq); put(s_slab + kKS * kPitch, gx);
        __syncthreads();              // also orders the last tile's selection (and the set-up above) before this tile's
        for (int s = 0; s < n_slabs; ++s) {
            const bool more = s + 1 < n_slabs;
            if (more) {
                const int col = (s + 1) * kKS + lk4 * 4;
                gq = (q_ok && col < a.D) ? ld4(q_src + (s + 1) * kKS) : zero4;
                gx = (x_ok && col < a.D) ? ld4(x_src + (s + 1) * kKS) : zero4;
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
                put(nb, gq); put(nb + kKS * kPitch, gx);
            }
            __syncthreads();
        }

        // selection: which of the 16 pairs beat their query's k-th key (read once; it only tightens)
        unsigned mask = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long q = q0 + ty * 4 + i;
            const u64 kth = s_sorted[(ty * 4 + i) * sp + k - 1];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long c = c0 + tx * 4 + j;
                const u64 key = ((u64)__float_as_uint(acc[i][j]) << 32) | (unsigned)c;
                const bool self = a.self_offset >= 0 && c == a.self_offset + q;
                if (q < a.n_q && c < a.n_c && !self && key < kth) mask |= 1u << (i * 4 + j);
            }
        }
        if (mask) *s_flag = 1;
        __syncthreads();
        if (*s_flag) {                                    // uniform over the workgroup
            // Rounds of: every lane appends what it still holds; then, if a list passed the merge mark or overflowed, the lists
            // above the mark are merged and emptied and the lanes whose keys found no slot try again.  A round without such a
            // list - the usual one - costs one barrier.  `over` alternates between two words: the one a round clears is set
            // again two rounds (at least one barrier) later.
            unsigned pending = mask;
            for (int round = 0;; ++round) {
                int* over = s_flag + 1 + (round & 1);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (pending & (1u << (i * 4 + j))) {
                            const int ql = ty * 4 + i;
                            const int slot = atomicAdd(&s_cnt[ql], 1);
                            if (slot < kStage) {
                                s_stage[ql * kStagePitch + slot] = ((u64)__float_as_uint(acc[i][j]) << 32) | (unsigned)(c0 + tx * 4 + j);
                                pending &= ~(1u << (i * 4 + j));
                            }
                            if (slot >= kMergeMark) *over = 1;
                        }
                __syncthreads();
                if (!*over) break;                        // uniform; no list overflowed, so no lane holds a key any more
                merge_marked(s_sorted, s_stage, s_cnt, kMergeMark, sp, k, wave, lane);
                __syncthreads();
                if (tid == 0) *over = 0;
            }
            if (tid == 0) *s_flag = 0;                    // read again only after the next tile's barriers
        }
    }

    __syncthreads();
    merge_marked(s_sorted, s_stage, s_cnt, 0, sp, k, wave, lane);
    __syncthreads();
    for (int e = tid; e < kTQ * k; e += kKnnBlock) {
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
    if (D < 4 || D > kMaxD) return fail(WGNN_ERR_UNSUPPORTED, "D must be in [4, 1024]");
    if (D % 4) return fail(WGNN_ERR_ALIGNMENT, "D must be a multiple of 4 (zero-pad the rows)");
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
    hipLaunchKernelGGL(knn_kernel, dim3(q_tiles, (unsigned)splits), dim3(kKnnBlock), lds, st, a);
    if (hipGetLastError() != hipSuccess) return failed();
    if (need == 0) return WGNN_OK;
    hipLaunchKernelGGL(knn_merge, dim3((unsigned)((n_q + 3) / 4)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : failed();
}
