// wgnn_kmeans.hip - the two ops of ops.kmeans_rows that are no distance kernel (include/wgnn.h has the contracts; the assignment of
// a Lloyd step is wgnn_knn_rows with k = 1 and the centres as candidates).
//
// wgnn_kmeans_seed: k-means++ seeding, every round on the device.  Round r is two launches.  seed_pass_kernel - the hot path, one
// read of X per round - has a workgroup of 256 threads own a chunk of 256 consecutive rows, a LANE per row: a wavefront streams
// its 64 rows through LDS 32 columns (one 128-byte line per row, read by 8 lanes) at a time, every lane walks its own row
//     t = x[j] - c[j];  d = fmaf(t, t, d);   j = 0 .. D-1 ascending, d = 0 to start
// - wgnn_knn_rows' chain, so no lane group ever splits a row - against the newest seed's row (found through seed_row[r - 1] in
// device memory: no read-back), lowers min_d2 and leaves the chunk's fp64 weight sum, 256 additions in row order by one thread.
// Pass 0 has no seed yet: it marks the rows that hold a non-finite value with NaN, the others with +inf.  seed_pick_kernel, one
// workgroup, adds the chunk sums in chunk order, draws the target, finds the chunk and walks its 256 weights.  The addition
// order is fixed by the 256-row chunk alone: a constant of the kernel, not of the grid.  No atomics; vector stores only.
//
// wgnn_group_rows_reduce: per group the fp64 sum of dense f32 rows, the batch group-major as wgnn_group_class_reduce takes it.  A
// group's run is cut into chunks of 64 members with one owner each per 64 columns, a wavefront, a lane per column: the rows are
// added in run order from 0.0.  A second kernel adds a group's chunk partials in chunk order, counts and divides.
#include <limits.h>
#include "wgnn_resident_rows.h"

namespace {
using namespace wgnn;

constexpr int kSeedChunk = 256;               // rows per chunk: part of the prefix's addition order, never tuned per device
constexpr int kSeedCols = 32;                 // columns of a slab
constexpr int kSeedPitch = kSeedCols + 1;     // floats between two rows of a slab (odd: the 64 lanes of a column read spread over banks)
constexpr int kSeedLoads = 64 * kSeedCols / 4 / 64;      // float4 loads per lane and slab
constexpr int kSeedMaxK = 4096;
constexpr int kSeedMaxD = 1024;
constexpr int kWalk = 2048;                   // chunk sums staged in LDS per step of the pick's walk

struct SArgs {
    const float* X; long ld; int n_rows; int D; int K; unsigned long long seed;
    int* seed_row; float* min_d2;
    double* sums; int* taken; long n_chunks;  // the workspace: a chunk's weight sum, and 1 for a row that is a seed
};

__device__ __forceinline__ bool is_nan(float v) { return v != v; }
__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7fc00000u); }
// a row's weight in `round` from its min_d2: 0 for an invalid row, 1 in round 0, else the distance to the nearest seed
__device__ __forceinline__ double weight_of(float m, int round) { return is_nan(m) ? 0.0 : (round == 0 ? 1.0 : (double)m); }

// pass `round` (0 .. K): round 0 tells valid rows from invalid ones, a later one lowers min_d2 against seed_row[round - 1];
// all but the last leave the chunk sums of the weights that round `round` draws from
__global__ void __launch_bounds__(kSeedChunk) seed_pass_kernel(const SArgs a, const int round) {
    __shared__ float s_x[kSeedChunk / 64][64 * kSeedPitch];
    __shared__ float s_c[kSeedMaxD];
    __shared__ double s_w[kSeedChunk];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long row0 = (long)blockIdx.x * kSeedChunk + wave * 64;
    const long row = row0 + lane;
    const int D = a.D;
    const int c = round > 0 ? a.seed_row[round - 1] : -1;
    const bool has_c = c >= 0 && c < a.n_rows;             // no seed (fewer valid rows than rounds): min_d2 stays
    float d = 0.f;
    bool bad = false;
    if (round == 0 || has_c) {                             // uniform over the grid
        if (has_c)
            for (int j = tid; j < D; j += kSeedChunk) s_c[j] = a.X[(size_t)c * a.ld + j];
        float* xs = s_x[wave];
        const int n_slabs = (D + kSeedCols - 1) / kSeedCols;
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 v[kSeedLoads];
        // 8 consecutive lanes read the 128 bytes of one row's slab
#define WGNN_SEED_FETCH(S)                                                                                           \
        _Pragma("unroll") for (int u = 0; u < kSeedLoads; ++u) {                                                     \
            const int e = u * 64 + lane, r = e >> 3, col = (S) * kSeedCols + (e & 7) * 4;                            \
            v[u] = (row0 + r < a.n_rows && col < D) ? ld4(a.X + (size_t)(row0 + r) * a.ld + col) : zero4;            \
        }
        WGNN_SEED_FETCH(0)
        for (int s = 0; s < n_slabs; ++s) {
            __syncthreads();                               // the slab before this one has been read (and s_c is written)
#pragma unroll
            for (int u = 0; u < kSeedLoads; ++u) {
                const int e = u * 64 + lane;
                float* p = xs + (e >> 3) * kSeedPitch + (e & 7) * 4;
                p[0] = v[u].x; p[1] = v[u].y; p[2] = v[u].z; p[3] = v[u].w;
            }
            if (s + 1 < n_slabs) { WGNN_SEED_FETCH(s + 1) }
            __syncthreads();
            const int jn = min(kSeedCols, D - s * kSeedCols);
            const float* mine = xs + lane * kSeedPitch;
            if (round == 0) {
                for (int j = 0; j < jn; ++j) bad |= (__float_as_uint(mine[j]) & 0x7f800000u) == 0x7f800000u;
            } else {
                const float* cs = s_c + s * kSeedCols;
#pragma unroll 8
                for (int j = 0; j < jn; ++j) {
                    const float t = mine[j] - cs[j];
                    d = fmaf(t, t, d);
                }
            }
        }
    }
#undef WGNN_SEED_FETCH
    float m = quiet_nan();
    if (row < a.n_rows) {
        if (round == 0) {
            m = bad ? quiet_nan() : INFINITY;
            a.taken[row] = 0;
        } else {
            const float old = a.min_d2[row];
            m = (is_nan(old) || !has_c) ? old : fminf(old, d);
        }
        a.min_d2[row] = m;
    }
    if (round >= a.K) return;                              // the last pass: nothing draws from it
    s_w[tid] = weight_of(m, round);
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
#pragma unroll 16
        for (int i = 0; i < kSeedChunk; ++i) acc += s_w[i];
        a.sums[blockIdx.x] = acc;
    }
}

// the lowest value over the workgroup's 256 threads (s_red: 256 entries of scratch LDS)
__device__ __forceinline__ long block_min(long v, long* s_red, int tid) {
    __syncthreads();                                       // s_red may still be read from the call before
    s_red[tid] = v;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (tid < off) s_red[tid] = min(s_red[tid], s_red[tid + off]);
        __syncthreads();
    }
    return s_red[0];
}

// s_v[0 .. n) becomes its own inclusive prefix, added sequentially from `carry` by ONE thread (the contract's order; the
// loop has no exit, so its LDS reads run ahead of the chain of additions); returns the last prefix.  Callers put barriers around.
__device__ __forceinline__ double prefix_in_place(double* s_v, int n, double carry) {
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        double v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = s_v[i + e];
#pragma unroll
        for (int e = 0; e < 8; ++e) { carry += v[e]; v[e] = carry; }
#pragma unroll
        for (int e = 0; e < 8; ++e) s_v[i + e] = v[e];
    }
    for (; i < n; ++i) { carry += s_v[i]; s_v[i] = carry; }
    return carry;
}

// round `round`'s seed: ONE workgroup.  T = the chunk sums added in chunk order from 0.0; t = u * T; the first chunk whose
// prefix passes t, then the first row of it whose prefix (the chunk's base + the rows' weights added in row order) does.
// One thread makes the additions - their order is the contract - and all 256 search the prefixes it leaves in LDS.
__global__ void __launch_bounds__(256) seed_pick_kernel(const SArgs a, const int round) {
    __shared__ double s_v[kWalk];
    __shared__ double s_in, s_out;                         // the prefix in front of the tile in s_v, and the tile's last prefix
    __shared__ long s_red[256];
    const int tid = threadIdx.x;
    const long n_tiles = (a.n_chunks + kWalk - 1) / kWalk;
    // tile `tile` of the chunk sums, as prefixes, into s_v; tiles are staged in ascending order, tile 0 starts from 0.0
    auto stage = [&](long tile) {
        const long first = tile * kWalk;
        const int n = (int)min((long)kWalk, a.n_chunks - first);
        __syncthreads();                                   // whoever read s_v or s_in before is done
        for (int i = tid; i < n; i += 256) s_v[i] = a.sums[first + i];
        __syncthreads();
        if (tid == 0) {
            const double in = tile == 0 ? 0.0 : s_out;
            s_in = in;
            s_out = prefix_in_place(s_v, n, in);
        }
        __syncthreads();
        return n;
    };
    for (long tile = 0; tile < n_tiles; ++tile) stage(tile);
    const double total = s_out;
    long pick = -1;
    if (total > 0.0) {                                     // uniform, as every branch below
        const double u = (double)(mix64(mix64(a.seed) + (unsigned long long)round) >> 11) * 0x1.0p-53;
        const double t = u * total;
        long chunk = LONG_MAX;                             // the first chunk whose prefix passes t
        double base = 0.0;                                 // ... and the prefix in front of it
        for (long tile = 0; tile < n_tiles; ++tile) {
            const int n = n_tiles > 1 ? stage(tile) : (int)a.n_chunks;      // one tile: its prefixes are still in s_v
            long mine = LONG_MAX;
            for (int i = tid; i < n; i += 256)
                if (s_v[i] > t) { mine = i; break; }       // prefixes do not decrease: a thread's first hit is its lowest
            const long hit = block_min(mine, s_red, tid);
            if (hit != LONG_MAX) {
                chunk = tile * kWalk + hit;
                base = hit > 0 ? s_v[hit - 1] : s_in;
                break;
            }
        }
        const bool clamp = chunk == LONG_MAX;              // rounding gave t >= T (or T is no finite number): the last weighted row
        if (clamp) {
            long mine = LONG_MAX;                          // the last chunk that holds a positive weight, as the lowest -c
            for (long c = a.n_chunks - 1 - tid; c >= 0; c -= 256)
                if (a.sums[c] > 0.0) { mine = -c; break; }
            chunk = -block_min(mine, s_red, tid);
        }
        const long i0 = chunk * kSeedChunk + tid;
        const double w = (i0 >= 0 && i0 < a.n_rows) ? weight_of(a.min_d2[i0], round) : 0.0;
        __syncthreads();                                   // `base` has been read from s_v
        s_v[tid] = w;
        __syncthreads();
        if (tid == 0) prefix_in_place(s_v, kSeedChunk, 0.0);
        __syncthreads();
        long hit = clamp ? LONG_MAX : block_min(base + s_v[tid] > t ? (long)tid : LONG_MAX, s_red, tid);
        if (hit == LONG_MAX) hit = -block_min(w > 0.0 ? -(long)tid : LONG_MAX, s_red, tid);      // the last row with w > 0
        pick = hit == -LONG_MAX ? -1 : chunk * kSeedChunk + hit;
    } else {
        // no weight is left: fewer distinct valid rows than rounds.  The lowest valid row that is no seed yet (-1: none)
        long mine = LONG_MAX;
        for (long i = tid; i < a.n_rows; i += 256)
            if (!is_nan(a.min_d2[i]) && !a.taken[i]) { mine = i; break; }
        const long hit = block_min(mine, s_red, tid);
        pick = hit == LONG_MAX ? -1 : hit;
    }
    if (tid == 0) {
        a.seed_row[round] = (int)pick;
        if (pick >= 0) a.taken[pick] = 1;
    }
}

int64_t seed_chunks(int64_t n_rows) { return (n_rows + kSeedChunk - 1) / kSeedChunk; }
int64_t seed_bytes(int64_t n_rows) { return seed_chunks(n_rows) * 8 + n_rows * 4; }

const char* check_seed_sizes(int64_t n_rows, int32_t K, int* code) {
    *code = WGNN_ERR_BAD_ARG;
    if (n_rows < 1 || n_rows > INT32_MAX) return "n_rows must be in [1, 2^31)";
    *code = WGNN_ERR_UNSUPPORTED;
    if (K < 1 || K > kSeedMaxK) return "K must be in [1, 4096] (the seeding costs O(K n_rows D))";
    return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kRChunk = 64;                   // members per chunk: part of the sum's addition order, never tuned per device
constexpr int kRWaves = 4;
constexpr int kRMaxBlocks = 4096;             // grid-stride beyond that
constexpr int kRMaxD = 65536;

struct RArgs {
    const float* X; long ld; const int* order; const long long* seg;
    long n_rows; int n_groups; int D; long n_slots; int n_cb;
    double* dpart; int* ipart;                // [n_slots][D] a chunk's column sums, [n_slots] its members in range
    double* sum; long ld_sum; long long* count; float* mean; long ld_mean;
};

// how many entries of `order` count: seg_ptr[K] clamped into [0, n_rows]; nothing without the operands
__device__ __forceinline__ long entries(const RArgs& a) {
    if (!a.X || !a.order) return 0;
    const long n = a.seg[a.n_groups];
    return n < 0 ? 0 : (n > a.n_rows ? a.n_rows : n);
}
// seg_ptr[k] clamped into [0, n]: a malformed seg_ptr reads no position outside `order` and no slot outside the workspace
__device__ __forceinline__ long seg_at(const RArgs& a, long k, long n) {
    const long v = a.seg[k];
    return v < 0 ? 0 : (v > n ? n : v);
}
// chunk w of the workspace belongs to the group k with slot(k) <= w < slot(k + 1) (wgnn_clusters.hip has the argument)
__device__ __forceinline__ long slot_at(const RArgs& a, long k, long n) { return seg_at(a, k, n) / kRChunk + k; }

// a wavefront per (chunk, block of 64 columns), a lane per column: the chunk's rows in run order, from 0.0
__global__ void __launch_bounds__(64 * kRWaves) rows_chunk_kernel(const RArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long n = entries(a);
    const long total = a.n_slots * a.n_cb;
    for (long item = (long)blockIdx.x * kRWaves + wave; item < total; item += (long)gridDim.x * kRWaves) {      // wave-uniform
        const long w = item / a.n_cb;
        const int col = (int)(item % a.n_cb) * 64 + lane;
        if (slot_at(a, 0, n) > w) continue;
        long lo = 0, hi = a.n_groups;                               // the largest k in [0, K] with slot(k) <= w
        while (lo < hi) {
            const long mid = lo + (hi - lo + 1) / 2;
            if (slot_at(a, mid, n) <= w) lo = mid; else hi = mid - 1;
        }
        if (lo >= a.n_groups) continue;
        const long c0 = seg_at(a, lo, n) + (w - slot_at(a, lo, n)) * kRChunk, end = seg_at(a, lo + 1, n);
        if (c0 >= end) continue;                                    // a slot the group does not need
        const int cnt = (int)min((long)kRChunk, end - c0);
        int r = lane < cnt ? a.order[c0 + lane] : -1;
        if ((unsigned long)(long)r >= (unsigned long)a.n_rows) r = -1;      // takes no part
        const int n_on = __popcll(__ballot(r >= 0));
        const float* src = a.X + (col < a.D ? col : 0);
        double acc = 0.0;
#pragma unroll 4
        for (int i = 0; i < cnt; ++i) {
            const int ri = __shfl(r, i, 64);
            if (ri >= 0) acc += (double)src[(size_t)ri * a.ld];
        }
        if (col < a.D) a.dpart[(size_t)w * a.D + col] = acc;
        if (col == 0) a.ipart[w] = n_on;
    }
}

// one thread per output element: a group's chunk partials in ascending chunk order, then the count and the mean
__global__ void __launch_bounds__(256) rows_finish_kernel(const RArgs a) {
    const long per = (long)a.D + 1, total = (long)a.n_groups * per;
    const long n = entries(a);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long k = i / per;
        const int j = (int)(i % per);
        const long b = seg_at(a, k, n), e = seg_at(a, k + 1, n), first = slot_at(a, k, n);
        long chunks = e > b ? (e - b + kRChunk - 1) / kRChunk : 0;
        if (first + chunks > a.n_slots) chunks = first < a.n_slots ? a.n_slots - first : 0;      // malformed seg_ptr only
        long long members = 0;
        for (long c = 0; c < chunks; ++c) members += a.ipart[first + c];
        if (j == a.D) { a.count[k] = members; continue; }
        double sum = 0.0;
        for (long c = 0; c < chunks; ++c) sum += a.dpart[(size_t)(first + c) * a.D + j];
        a.sum[(size_t)k * a.ld_sum + j] = sum;
        if (a.mean && members > 0) a.mean[(size_t)k * a.ld_mean + j] = (float)(sum / (double)members);
    }
}

int64_t rows_slots(int64_t n_rows, int32_t n_groups) { return n_rows / kRChunk + n_groups; }
// bytes of n_slots partials (the sums, then the counts, to a multiple of 8), or -1 when that is beyond int64
int64_t rows_bytes(int64_t n_slots, int32_t D) {
    int64_t bytes;
    if (__builtin_mul_overflow(n_slots, (int64_t)D * 8 + 4, &bytes) || bytes > INT64_MAX - 8) return -1;
    return (bytes + 7) / 8 * 8;
}

const char* check_rows_sizes(int64_t n_rows, int32_t n_groups, int32_t D, int* code) {
    *code = WGNN_ERR_BAD_ARG;
    if (n_rows < 0 || n_rows > INT32_MAX) return "n_rows must be in [0, 2^31)";
    if (n_groups <= 0) return "n_groups must be positive";
    if (D <= 0) return "D must be positive";
    *code = WGNN_ERR_UNSUPPORTED;
    if (D > kRMaxD) return "D > 65536 is not built";
    if (rows_bytes(rows_slots(n_rows, n_groups), D) < 0) return "the workspace of these sizes is beyond 2^63 bytes";
    return nullptr;
}

}  // namespace

extern "C" int wgnn_kmeans_seed_workspace_bytes(int64_t n_rows, int32_t K, int64_t* bytes) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_kmeans_seed_workspace_bytes", what); };
    wgnn::error_clear();
    if (!bytes) return fail(WGNN_ERR_BAD_ARG, "bytes is required");
    int code = 0;
    if (const char* what = check_seed_sizes(n_rows, K, &code)) return fail(code, what);
    *bytes = seed_bytes(n_rows);
    return WGNN_OK;
}

extern "C" int wgnn_kmeans_seed(const float* X, int64_t ld_x, int64_t n_rows, int32_t D, int32_t K, uint64_t seed,
                                int32_t* seed_row, float* min_d2, void* workspace, int64_t workspace_bytes,
                                uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_kmeans_seed", what); };
    wgnn::error_clear();
    int code = 0;
    if (const char* what = check_seed_sizes(n_rows, K, &code)) return fail(code, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (D < 4 || D > kSeedMaxD) return fail(WGNN_ERR_UNSUPPORTED, "D must be in [4, 1024]");
    if (D % 4) return fail(WGNN_ERR_ALIGNMENT, "D must be a multiple of 4 (zero-pad the rows)");
    if (ld_x < D || ld_x % 4) return fail(WGNN_ERR_ALIGNMENT, "ld_x must be >= D and a multiple of 4");
    if (!X || !seed_row || !min_d2) return fail(WGNN_ERR_BAD_ARG, "X, seed_row and min_d2 are required");
    if (!aligned16(X)) return fail(WGNN_ERR_ALIGNMENT, "X must be 16-byte aligned");
    if (!aligned4(seed_row) || !aligned4(min_d2)) return fail(WGNN_ERR_ALIGNMENT, "seed_row and min_d2 must be 4-byte aligned");
    if (workspace_bytes < 0) return fail(WGNN_ERR_WORKSPACE, "workspace_bytes is negative");
    if (!workspace || workspace_bytes < seed_bytes(n_rows))
        return fail(WGNN_ERR_WORKSPACE, "workspace is missing or smaller than wgnn_kmeans_seed_workspace_bytes asks for");
    if (!aligned8(workspace)) return fail(WGNN_ERR_ALIGNMENT, "workspace must be 8-byte aligned");

    SArgs a{};
    a.X = X; a.ld = ld_x; a.n_rows = (int)n_rows; a.D = D; a.K = K; a.seed = seed;
    a.seed_row = seed_row; a.min_d2 = min_d2;
    a.n_chunks = seed_chunks(n_rows);
    a.sums = static_cast<double*>(workspace);
    a.taken = reinterpret_cast<int*>(a.sums + a.n_chunks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int round = 0; round <= K; ++round) {             // pass r, then round r's seed; pass K closes min_d2 over all K seeds
        hipLaunchKernelGGL(seed_pass_kernel, dim3((unsigned)a.n_chunks), dim3(kSeedChunk), 0, st, a, round);
        if (round < K) hipLaunchKernelGGL(seed_pick_kernel, dim3(1), dim3(256), 0, st, a, round);
        if (hipGetLastError() != hipSuccess) return fail(WGNN_ERR_LAUNCH, "HIP launch failed");
    }
    return WGNN_OK;
}

extern "C" int wgnn_group_rows_reduce_workspace(int64_t n_rows, int32_t n_groups, int32_t D, int64_t* bytes) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_group_rows_reduce_workspace", what); };
    wgnn::error_clear();
    if (!bytes) return fail(WGNN_ERR_BAD_ARG, "bytes is required");
    int code = 0;
    if (const char* what = check_rows_sizes(n_rows, n_groups, D, &code)) return fail(code, what);
    *bytes = rows_bytes(rows_slots(n_rows, n_groups), D);
    return WGNN_OK;
}

extern "C" int wgnn_group_rows_reduce(const float* X, int64_t ld_x, const int32_t* order, const void* seg_ptr, int64_t n_rows,
                                      int32_t n_groups, int32_t D, double* sum, int64_t ld_sum, int64_t* count,
                                      float* mean, int64_t ld_mean, void* workspace, int64_t workspace_bytes,
                                      uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_group_rows_reduce", what); };
    wgnn::error_clear();
    if (!sum || !count) return fail(WGNN_ERR_BAD_ARG, "sum and count are required");
    if (!seg_ptr) return fail(WGNN_ERR_BAD_ARG, "seg_ptr is required");
    int code = 0;
    if (const char* what = check_rows_sizes(n_rows, n_groups, D, &code)) return fail(code, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (ld_x < D) return fail(WGNN_ERR_BAD_ARG, "ld_x < D");
    if (ld_sum < D || (mean && ld_mean < D)) return fail(WGNN_ERR_BAD_ARG, "ld_sum and ld_mean must be >= D");
    if (!aligned8(sum) || !aligned8(count) || !aligned8(seg_ptr)) return fail(WGNN_ERR_ALIGNMENT, "sum, count and seg_ptr must be 8-byte aligned");
    if (!aligned4(X) || !aligned4(order) || !aligned4(mean)) return fail(WGNN_ERR_ALIGNMENT, "X, order and mean must be 4-byte aligned");
    if (workspace_bytes < 0) return fail(WGNN_ERR_WORKSPACE, "workspace_bytes is negative");
    const int64_t n_slots = rows_slots(n_rows, n_groups);
    if (!workspace || workspace_bytes < rows_bytes(n_slots, D))
        return fail(WGNN_ERR_WORKSPACE, "workspace is missing or smaller than wgnn_group_rows_reduce_workspace asks for");
    if (!aligned8(workspace)) return fail(WGNN_ERR_ALIGNMENT, "workspace must be 8-byte aligned");

    RArgs a{};
    a.X = X; a.ld = ld_x; a.order = order; a.seg = static_cast<const long long*>(seg_ptr);
    a.n_rows = n_rows; a.n_groups = n_groups; a.D = D; a.n_slots = n_slots; a.n_cb = (D + 63) / 64;
    a.dpart = static_cast<double*>(workspace);
    a.ipart = reinterpret_cast<int*>(a.dpart + n_slots * (int64_t)D);
    a.sum = sum; a.ld_sum = ld_sum; a.count = reinterpret_cast<long long*>(count); a.mean = mean; a.ld_mean = ld_mean;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_rows > 0 && X && order) {                                 // else no row takes part: the finish alone writes the outputs
        const int64_t want = (n_slots * a.n_cb + kRWaves - 1) / kRWaves;
        hipLaunchKernelGGL(rows_chunk_kernel, dim3((unsigned)(want < kRMaxBlocks ? want : kRMaxBlocks)), dim3(64 * kRWaves), 0, st, a);
        if (hipGetLastError() != hipSuccess) return fail(WGNN_ERR_LAUNCH, "HIP launch failed");
    }
    const int64_t items = (int64_t)n_groups * ((int64_t)D + 1);
    const int64_t want = (items + 255) / 256;
    hipLaunchKernelGGL(rows_finish_kernel, dim3((unsigned)(want < kRMaxBlocks ? want : kRMaxBlocks)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}
