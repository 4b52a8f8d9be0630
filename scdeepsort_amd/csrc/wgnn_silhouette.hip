// wgnn_silhouette.hip - wgnn_silhouette_rows: the exact silhouette (Rousseeuw 1987) of every row of a group-major batch under
// Euclidean distance (include/wgnn.h has the contract).  Brute force over every ordered pair, O(n^2 D); the [n, n] distance matrix
// is never stored.
//
// The tile is the one wgnn_knn_rows runs (wgnn_pair_tile.h): a workgroup of 256 threads holds a tile of 64 queries and streams
// tiles of 64 candidates past it, 16 columns of D at a time, through two LDS buffers (k-major); each lane owns a 4 x 4 micro-tile
// of (query, candidate) pairs and carries the 16 squared distances in registers across the slabs of D
//     t = q[j] - x[j];  d2 = fma(t, t, d2) in f32;   j = 0 .. D-1 ascending, d2 = 0 to start
// - that kernel's chain bit for bit, being the same code.  In place of its selection stands a reduction per group.  A candidate tile never straddles
// two groups: a group's members are cut into tiles of 64 from the group's own start, and a position past the group's end adds a
// SELECTED +0.0 (its distance is computed against a row of zeros and thrown away).  The order of additions is fixed:
//     a lane adds sqrtf(d2) of its own four candidates, ascending, into one fp64 partial per owned query, carried over the
//     group's tiles - member position p of the group goes to partial (p % 64) / 4, each partial is summed sequentially in p;
//     at the group's end the 16 lanes that share a query add their partials in an xor butterfly over the offsets 1, 2, 4, 8:
//     a balanced tree, and since fp addition is commutative all 16 lanes end with the same bits.
// Then mean = S / n_c in fp64 enters the query's running (b, nearest) under the total order (mean, group id) - the groups come
// in ascending id, so a strictly smaller mean wins - or, for the query's own group, S is kept for a.  The query itself is a
// member of its own group and adds sqrtf(0) = +0.0: no self-exclusion branch.  No atomics.
//
// With n_splits > 1 sil_plan deals WHOLE groups to grid.y in contiguous ranges balanced by the number of candidate tiles, every
// split leaves (S_own or -1, its best mean, that group) per query in the workspace and sil_merge finishes.  Every S(i, c) is
// computed inside one workgroup, so neither n_splits nor the grid changes a bit.  A group is never cut, so one dominant group
// bounds the balance.
#include <limits.h>
#include "wgnn_pair_tile.h"

namespace wgnn {
namespace {

constexpr int kMaxGroups = 4096;
constexpr int kMaxSplits = 64;

struct SilArgs {
    const float* X; long ld; const long long* seg;
    int n; int D; int K; int n_splits;
    double* a; double* b; double* s; int* nearest;
    long long* split_ptr;                                 // [n_splits + 1] groups of a split (the workspace's head; null: one split)
    double* ws_own; double* ws_b; int* ws_g;              // [n_splits][n] each
};

// seg_ptr[k] clamped into [0, n]: a malformed seg_ptr reads no row outside X and writes no position outside the outputs
__device__ __forceinline__ long seg_at(const SilArgs& a, int k) {
    const long v = a.seg[k];
    return v < 0 ? 0 : (v > a.n ? a.n : v);
}

// the group of position p < seg_ptr[K]: the k with seg_ptr[k] <= p < seg_ptr[k + 1]
__device__ __forceinline__ int group_of(const SilArgs& a, long p) {
    int lo = 0, hi = a.K;                                 // the smallest k in [0, K] with seg_ptr[k] > p
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg_at(a, mid) > p) hi = mid; else lo = mid + 1;
    }
    return lo < 1 ? 0 : (lo > a.K ? a.K - 1 : lo - 1);
}

__device__ __forceinline__ double quiet_nan64() { return __longlong_as_double(0x7ff8000000000000ll); }

// a query's four outputs from S(i, own group), its group's size and the best other mean
__device__ __forceinline__ void finish(const SilArgs& a, long q, double s_own, long n_g, double b, int nearest) {
    const double av = n_g > 1 ? s_own / (double)(n_g - 1) : 0.0;
    double sv;
    if (nearest < 0) sv = quiet_nan64();                  // no other non-empty group: b = +inf
    else if (n_g <= 1) sv = 0.0;
    else {
        const double m = av > b ? av : b;
        sv = m == 0.0 ? 0.0 : (b - av) / m;
    }
    a.a[q] = av; a.b[q] = b; a.s[q] = sv; a.nearest[q] = nearest;
}

__global__ void __launch_bounds__(kPairBlock) sil_kernel(const SilArgs a) {
    __shared__ __align__(16) float s_slab[2 * kSlabFloats];                     // [2][2][kKS][kPitch]
    __shared__ int s_g[kTQ];

    const int tid = threadIdx.x;
    const int ty = tid >> 4, tx = tid & 15;               // the micro-tile: queries ty*4 .. +3, candidates tx*4 .. +3
    const int lrow = tid >> 2, lk4 = tid & 3;             // the loader: row lrow of the tile, its float4 number lk4 of the slab
    const long q0 = (long)blockIdx.x * kTQ;
    const long n_on = seg_at(a, a.K);                     // the rows that take part
    if (q0 >= n_on) {                                     // uniform: no query of this tile takes part (split: sil_merge writes them)
        if (!a.split_ptr && tid < kTQ && q0 + tid < a.n) {
            a.a[q0 + tid] = a.b[q0 + tid] = a.s[q0 + tid] = quiet_nan64(); a.nearest[q0 + tid] = -1;
        }
        return;
    }
    const int n_slabs = (a.D + kKS - 1) / kKS;
    int c_lo = 0, c_hi = a.K;
    if (a.split_ptr) {
        const long lo = a.split_ptr[blockIdx.y], hi = a.split_ptr[blockIdx.y + 1];
        c_lo = (int)(lo < 0 ? 0 : (lo > a.K ? a.K : lo));
        c_hi = (int)(hi < c_lo ? c_lo : (hi > a.K ? a.K : hi));
    }

    if (tid < kTQ) s_g[tid] = q0 + tid < n_on ? group_of(a, q0 + tid) : -1;
    __syncthreads();
    int g[4], nearest[4];
    double part[4], own[4], best[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { g[i] = s_g[ty * 4 + i]; nearest[i] = -1; own[i] = -1.0; best[i] = (double)INFINITY; }

    const bool q_ok = q0 + lrow < n_on;
    const float* q_src = a.X + (size_t)(q_ok ? q0 + lrow : 0) * a.ld + lk4 * 4;

    for (int c = c_lo; c < c_hi; ++c) {                   // uniform over the workgroup, as everything below but the selects
        const long begin = seg_at(a, c), end = seg_at(a, c + 1);
        if (end <= begin) continue;                       // an empty group
#pragma unroll
        for (int i = 0; i < 4; ++i) part[i] = 0.0;
        for (long c0 = begin; c0 < end; c0 += kTC) {
            const bool x_ok = c0 + lrow < end;
            const float* x_src = a.X + (size_t)(x_ok ? c0 + lrow : 0) * a.ld + lk4 * 4;
            float acc[4][4];
            pair_tile_d2(acc, s_slab, q_src, q_ok, x_src, x_ok, a.D, n_slabs, tid);
            // the lane's four candidates in ascending position; one past the group's end adds a selected +0.0
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = c0 + tx * 4 + j < end;
#pragma unroll
                for (int i = 0; i < 4; ++i) part[i] += (double)(in ? sqrtf(acc[i][j]) : 0.f);
            }
        }
        const double n_c = (double)(end - begin);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double S = part[i];
#pragma unroll
            for (int off = 1; off <= 8; off <<= 1) S += __shfl_xor(S, off, 64);
            const double mean = S / n_c;
            if (c == g[i]) own[i] = S;
            else if (nearest[i] < 0 || mean < best[i]) { best[i] = mean; nearest[i] = c; }
        }
    }

    if (tx != 0) return;                                  // the 16 lanes of a query hold the same bits: one of them writes
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long q = q0 + ty * 4 + i;
        if (q >= a.n) continue;
        if (a.split_ptr) {
            const size_t at = (size_t)blockIdx.y * a.n + q;
            a.ws_own[at] = own[i]; a.ws_b[at] = best[i]; a.ws_g[at] = nearest[i];
        } else if (q < n_on) {
            finish(a, q, own[i] < 0.0 ? 0.0 : own[i], seg_at(a, g[i] + 1) - seg_at(a, g[i]), best[i], nearest[i]);
        } else {
            a.a[q] = a.b[q] = a.s[q] = quiet_nan64(); a.nearest[q] = -1;
        }
    }
}

// split_ptr: group c goes to the split floor(T(c) * n_splits / T), T(c) = the candidate tiles of the groups before it
__global__ void __launch_bounds__(256) sil_plan(const SilArgs a) {
    __shared__ long s_start[kMaxGroups + 1];
    __shared__ long s_sum[256];
    const int tid = threadIdx.x;
    const int per = (a.K + 255) / 256;
    const int k0 = min(tid * per, a.K), k1 = min(k0 + per, a.K);
    auto tiles = [&](int k) { const long n_c = seg_at(a, k + 1) - seg_at(a, k); return n_c > 0 ? (n_c + kTC - 1) / kTC : 0l; };
    long mine = 0;
    for (int k = k0; k < k1; ++k) mine += tiles(k);
    s_sum[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        long run = 0;
        for (int t = 0; t < 256; ++t) { const long v = s_sum[t]; s_sum[t] = run; run += v; }
        s_start[a.K] = run;
    }
    __syncthreads();
    long run = s_sum[tid];
    for (int k = k0; k < k1; ++k) { s_start[k] = run; run += tiles(k); }
    __syncthreads();
    const long total = s_start[a.K];
    if (tid > a.n_splits) return;
    int lo = 0, hi = a.K;                                 // the smallest c in [0, K] with T(c) * n_splits >= tid * T
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_start[mid] * a.n_splits >= (long)tid * total) hi = mid; else lo = mid + 1;
    }
    a.split_ptr[tid] = tid == a.n_splits ? a.K : lo;
}

// a thread per query: the splits in ascending order (their groups ascend with them) under the kernel's own rule
__global__ void __launch_bounds__(256) sil_merge(const SilArgs a) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.n) return;
    if (q >= seg_at(a, a.K)) {
        a.a[q] = a.b[q] = a.s[q] = quiet_nan64(); a.nearest[q] = -1;
        return;
    }
    double own = 0.0, best = (double)INFINITY;
    int nearest = -1;
    for (int y = 0; y < a.n_splits; ++y) {
        const size_t at = (size_t)y * a.n + q;
        const double o = a.ws_own[at], m = a.ws_b[at];
        const int c = a.ws_g[at];
        if (!(o == -1.0)) own = o;
        if (c >= 0 && (nearest < 0 || m < best)) { best = m; nearest = c; }
    }
    const int g = group_of(a, q);
    finish(a, q, own, seg_at(a, g + 1) - seg_at(a, g), best, nearest);
}

// 0 = chosen here, as wgnn_knn_rows does: about 4096 workgroups, while every split keeps at least two candidate tiles (there
// are at least n / 64 of them) and at least one group
int resolve_splits(int64_t n, int32_t K, int32_t n_splits) {
    if (n_splits > 0) return n_splits;
    const int64_t q_tiles = (n + kTQ - 1) / kTQ;
    int64_t want = q_tiles > 0 ? (4096 + q_tiles - 1) / q_tiles : 1;
    if (want > q_tiles / 2) want = q_tiles / 2;
    if (want > K) want = K;
    if (want > kMaxSplits) want = kMaxSplits;
    return want < 1 ? 1 : (int)want;
}

const char* check_sizes(int64_t n, int32_t K, int32_t n_splits, int* code) {
    *code = WGNN_ERR_BAD_ARG;
    if (n < 0 || n > INT32_MAX) return "n must be in [0, 2^31)";
    if (n_splits < 0 || n_splits > kMaxSplits) return "n_splits must be in [0, 64] (0 = chosen from n and K)";
    *code = WGNN_ERR_UNSUPPORTED;
    if (K < 1 || K > kMaxGroups) return "K must be in [1, 4096]";
    return nullptr;
}

// the split bounds, then per split and row S_own, the best mean (fp64) and its group (int32), to a multiple of 8
int64_t workspace_bytes_for(int64_t n, int splits) {
    return splits > 1 ? ((int64_t)(splits + 1) * 8 + (int64_t)splits * n * 20 + 7) / 8 * 8 : 0;
}

}  // namespace
}  // namespace wgnn

using namespace wgnn;

extern "C" int wgnn_silhouette_workspace_bytes(int64_t n, int32_t K, int32_t n_splits, int64_t* bytes) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_silhouette_workspace_bytes", what); };
    wgnn::error_clear();
    if (!bytes) return fail(WGNN_ERR_BAD_ARG, "bytes is required");
    int code = 0;
    if (const char* what = check_sizes(n, K, n_splits, &code)) return fail(code, what);
    *bytes = workspace_bytes_for(n, resolve_splits(n, K, n_splits));
    return WGNN_OK;
}

extern "C" int wgnn_silhouette_rows(const float* X, int64_t ld_x, int64_t n, int32_t D, const void* seg_ptr, int32_t K,
                                    int32_t n_splits, double* a, double* b, double* s, int32_t* nearest,
                                    void* workspace, int64_t workspace_bytes, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_silhouette_rows", what); };
    wgnn::error_clear();
    int code = 0;
    if (const char* what = check_sizes(n, K, n_splits, &code)) return fail(code, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (int rc = check_row_width("wgnn_silhouette_rows", D)) return rc;
    if (ld_x < D || ld_x % 4) return fail(WGNN_ERR_ALIGNMENT, "ld_x must be >= D and a multiple of 4");
    if (workspace_bytes < 0) return fail(WGNN_ERR_WORKSPACE, "workspace_bytes is negative");
    if (n == 0) return WGNN_OK;
    if (!X || !seg_ptr || !a || !b || !s || !nearest) return fail(WGNN_ERR_BAD_ARG, "X, seg_ptr, a, b, s and nearest are required");
    if (!aligned16(X)) return fail(WGNN_ERR_ALIGNMENT, "X must be 16-byte aligned");
    if (!aligned8(seg_ptr) || !aligned8(a) || !aligned8(b) || !aligned8(s))
        return fail(WGNN_ERR_ALIGNMENT, "seg_ptr, a, b and s must be 8-byte aligned");
    if (!aligned4(nearest)) return fail(WGNN_ERR_ALIGNMENT, "nearest must be 4-byte aligned");
    const int splits = resolve_splits(n, K, n_splits);
    const int64_t need = workspace_bytes_for(n, splits);
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(WGNN_ERR_WORKSPACE, "workspace is smaller than wgnn_silhouette_workspace_bytes asks for");
    if (need > 0 && !aligned8(workspace)) return fail(WGNN_ERR_ALIGNMENT, "workspace must be 8-byte aligned");

    SilArgs g{};
    g.X = X; g.ld = ld_x; g.seg = static_cast<const long long*>(seg_ptr);
    g.n = (int)n; g.D = D; g.K = K; g.n_splits = splits;
    g.a = a; g.b = b; g.s = s; g.nearest = nearest;
    if (need > 0) {
        g.split_ptr = static_cast<long long*>(workspace);
        g.ws_own = reinterpret_cast<double*>(g.split_ptr + splits + 1);
        g.ws_b = g.ws_own + (int64_t)splits * n;
        g.ws_g = reinterpret_cast<int*>(g.ws_b + (int64_t)splits * n);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto failed = [&fail]() { return fail(WGNN_ERR_LAUNCH, "HIP launch failed"); };
    const unsigned q_tiles = (unsigned)((n + kTQ - 1) / kTQ);
    if (need > 0) {
        hipLaunchKernelGGL(sil_plan, dim3(1), dim3(256), 0, st, g);
        if (hipGetLastError() != hipSuccess) return failed();
    }
    hipLaunchKernelGGL(sil_kernel, dim3(q_tiles, (unsigned)splits), dim3(kPairBlock), 0, st, g);
    if (hipGetLastError() != hipSuccess) return failed();
    if (need == 0) return WGNN_OK;
    hipLaunchKernelGGL(sil_merge, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g);
    return hipGetLastError() == hipSuccess ? WGNN_OK : failed();
}
