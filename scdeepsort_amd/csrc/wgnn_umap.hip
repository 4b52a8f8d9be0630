// wgnn_umap.hip - the fuzzy kNN graph and the synchronous 2-D layout behind ops.fuzzy_graph / ops.layout_graph /
// api.ResidentPredictor.umap (include/wgnn.h has the contracts).  Every floating-point operation named there is rounded on its
// own: contraction into fused multiply-adds is switched off for the whole file, the sums run in a stated order, and nothing
// depends on the grid - so numpy restates each kernel (tests/umap_reference.py) and two calls give the same bits.
//
// wgnn_fuzzy_rows: a wavefront per row, a lane per entry of its list (k <= 64).  The 64 bisection steps of sigma are wave-uniform;
//   p, the sum of the memberships, is added up in list order from the lanes' terms (an entry that is not listed adds +0.0).
// wgnn_fuzzy_union: sixteen lanes per row of the union CSR, a lane per stored edge; both memberships by a linear scan of a list.
// wgnn_layout_init: the "hash" start positions, a thread per coordinate.
// wgnn_layout_epoch: WGNN_LAYOUT_LANES = 16 lanes per vertex.  Lane l takes the row's edges l, l + 16, ... in order and adds each
//   edge's terms (the attraction, then the negatives) to its own partial; the partials fold 8, 4, 2, 1.  Reads y_in only, writes
//   y_out only: no atomics, no scratch, and a hub row is a longer loop for its sixteen lanes.
// The integer types, the rowptr clamp, the grid and the n / nnz check are wgnn_graph.h's, shared with the other graph files; that
// header holds integer code only.
#include <float.h>
#include <limits.h>
#include <math.h>
#include "wgnn_resident_rows.h"
#include "wgnn_graph.h"

#pragma clang fp contract(off)

namespace {
using namespace wgnn;
using namespace wgnn::graph;

constexpr int kMaxK = 64;
constexpr int kLanes = WGNN_LAYOUT_LANES;          // lanes per vertex (and per row of the union)
constexpr int kRowsPerBlock = 256 / kLanes;
static_assert(kLanes == 16, "the fold below and include/wgnn.h state sixteen lanes");

// ---------------------------------------------------------------------------------------------------------------------------
struct FArgs {
    const void* idx; int idx64; long ld_idx; const float* d2; long ld_d2; long n; int k; double target;
    double* rho; double* sigma; float* member;
};

__device__ __forceinline__ i64 id_at(const void* idx, int idx64, long at) {
    return idx64 ? reinterpret_cast<const i64*>(idx)[at] : (i64)reinterpret_cast<const int*>(idx)[at];
}

// the sum of the lanes' values in lane order 0 .. k - 1 (wave-uniform result)
__device__ __forceinline__ double ordered_sum(double v, int k) {
    double sum = 0.0;
    for (int s = 0; s < k; ++s) sum = sum + __shfl(v, s, 64);
    return sum;
}

__global__ void __launch_bounds__(256) fuzzy_rows_kernel(const FArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long i = (long)blockIdx.x * 4 + wave; i < a.n; i += (long)gridDim.x * 4) {          // wave-uniform
        bool listed = false;
        double d = 0.0;
        if (lane < a.k) {
            const float v = a.d2[i * a.ld_d2 + lane];
            listed = id_at(a.idx, a.idx64, i * a.ld_idx + lane) >= 0 && fabsf(v) <= FLT_MAX;
            if (listed) d = (double)sqrtf(v);
        }
        const int count = __popcll(__ballot(listed));
        if (count == 0) {
            if (lane == 0) { a.rho[i] = 0.0; a.sigma[i] = 0.0; }
            if (lane < a.k) a.member[i * a.k + lane] = 0.f;
            continue;
        }
        double rho = (listed && d > 0.0) ? d : HUGE_VAL;                                       // the smallest positive distance
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) rho = fmin(rho, __shfl_xor(rho, off, 64));
        if (rho == HUGE_VAL) rho = 0.0;
        const double x = d - rho;
        const double mean = ordered_sum(listed ? d : 0.0, a.k) / (double)count;
        double lo = 0.0, hi = HUGE_VAL, s = 1.0;
        for (int it = 0; it < 64; ++it) {
            const double term = listed ? (x > 0.0 ? exp(-x / s) : 1.0) : 0.0;
            const double p = ordered_sum(term, a.k);
            if (p > a.target) { hi = s; s = (lo + hi) / 2.0; }
            else { lo = s; s = hi == HUGE_VAL ? 2.0 * s : (lo + hi) / 2.0; }
        }
        s = fmax(s, 1e-3 * mean);
        if (lane == 0) { a.rho[i] = rho; a.sigma[i] = s; }
        if (lane < a.k) a.member[i * a.k + lane] = listed ? (float)(x > 0.0 ? exp(-x / s) : 1.0) : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
struct UArgs {
    const void* idx; int idx64; long ld; const float* member; long n; int k;
    const i64* rowptr; const int* col; long nnz; float* w;
};

// the membership of c in row r's list: the first entry that names c, 0 without one
__device__ __forceinline__ float member_of(const UArgs& a, long r, long c) {
    for (int t = 0; t < a.k; ++t)
        if (id_at(a.idx, a.idx64, r * a.ld + t) == c) return a.member[r * a.k + t];
    return 0.f;
}

__global__ void __launch_bounds__(256) fuzzy_union_kernel(const UArgs a) {
    const int sub = threadIdx.x & (kLanes - 1), slot = threadIdx.x / kLanes;
    for (long i = (long)blockIdx.x * kRowsPerBlock + slot; i < a.n; i += (long)gridDim.x * kRowsPerBlock) {
        const i64 e0 = clampl(a.rowptr[i], a.nnz), e1 = clampl(a.rowptr[i + 1], a.nnz);
        for (i64 e = e0 + sub; e < e1; e += kLanes) {
            const long c = a.col[e];
            float w = 0.f;
            if (c >= 0 && c < a.n) {
                const float p = member_of(a, i, c), q = member_of(a, c, i);
                w = (p + q) - p * q;
            }
            a.w[e] = w;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 epoch_key(unsigned seed, unsigned epoch) { return mix64(((u64)seed << 32) | (u64)epoch); }

__global__ void __launch_bounds__(256) layout_init_kernel(float* y, long n, unsigned seed) {
    const u64 key = epoch_key(seed, 0xFFFFFFFFu);                  // no epoch has this number
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < 2 * n; t += (long)gridDim.x * 256) {
        const u64 h = mix64(key + (u64)t);
        y[t] = ((float)(unsigned)(h >> 40) * 0x1p-24f) * 20.f - 10.f;
    }
}

struct LArgs {
    const i64* rowptr; const int* col; const float* w; long n; long nnz; float wmax;
    const float2* y_in; float2* y_out; int epoch; float a; float b; float gamma; float alpha; int n_neg; unsigned seed;
    i64* fired;
};

__device__ __forceinline__ float clamp4(float v) { return v < -4.f ? -4.f : (v > 4.f ? 4.f : v); }      // a NaN stays a NaN

__device__ __forceinline__ float power_b(float q, float b) { return b == 1.0f ? q : (float)pow((double)q, (double)b); }

__global__ void __launch_bounds__(256) layout_epoch_kernel(const LArgs a) {
    const int sub = threadIdx.x & (kLanes - 1), slot = threadIdx.x / kLanes;
    const u64 key = epoch_key(a.seed, (unsigned)a.epoch);
    const float n0 = (float)a.epoch, n1 = (float)(a.epoch + 1);
    const float pull = (-2.f * a.a) * a.b, push = (2.f * a.gamma) * a.b;
    for (long i = (long)blockIdx.x * kRowsPerBlock + slot; i < a.n; i += (long)gridDim.x * kRowsPerBlock) {
        const i64 e0 = clampl(a.rowptr[i], a.nnz), e1 = clampl(a.rowptr[i + 1], a.nnz);
        const float2 yi = a.y_in[i];
        if (e1 <= e0) {                                            // no edge: the position is copied
            if (sub == 0) a.y_out[i] = yi;
            continue;
        }
        float g0 = 0.f, g1 = 0.f;
        int fired = 0;
        for (i64 e = e0 + sub; e < e1; e += kLanes) {
            const long j = a.col[e];
            const float r = a.w[e] / a.wmax;
            if (floorf(n1 * r) == floorf(n0 * r) || j < 0 || j >= a.n) continue;
            ++fired;
            {
                const float2 yj = a.y_in[j];
                const float dx0 = yi.x - yj.x, dx1 = yi.y - yj.y;
                const float q = dx0 * dx0 + dx1 * dx1;
                if (q > 0.f) {
                    const float qb = power_b(q, a.b);
                    const float c = ((pull * qb) / q) / (1.f + a.a * qb);
                    g0 = g0 + clamp4(c * dx0);
                    g1 = g1 + clamp4(c * dx1);
                }
            }
            for (int s = 0; s < a.n_neg; ++s) {
                const u64 h = mix64(key + (u64)e * (u64)a.n_neg + (u64)s);
                const long t = (long)(((h >> 32) * (u64)a.n) >> 32);
                if (t == i) continue;
                const float2 yt = a.y_in[t];
                const float dx0 = yi.x - yt.x, dx1 = yi.y - yt.y;
                const float q = dx0 * dx0 + dx1 * dx1;
                if (q > 0.f) {
                    const float qb = power_b(q, a.b);
                    const float c = push / ((0.001f + q) * (1.f + a.a * qb));
                    g0 = g0 + clamp4(c * dx0);
                    g1 = g1 + clamp4(c * dx1);
                }
            }
        }
#pragma unroll
        for (int off = kLanes / 2; off >= 1; off >>= 1) {         // lane l += lane l + off, for l < off
            g0 = g0 + __shfl_down(g0, off, kLanes);
            g1 = g1 + __shfl_down(g1, off, kLanes);
            fired += __shfl_down(fired, off, kLanes);
        }
        if (sub == 0) {
            a.y_out[i] = make_float2(yi.x + a.alpha * g0, yi.y + a.alpha * g1);
            if (a.fired) a.fired[i] += fired;
        }
    }
}

}  // namespace

extern "C" int wgnn_fuzzy_rows(const void* idx, int64_t ld_idx, const float* d2, int64_t ld_d2, int64_t n, int32_t k, double target,
                               double* rho, double* sigma, float* member, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_fuzzy_rows", what); };
    wgnn::error_clear();
    if (n < 0 || n > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n must be in [0, 2^31)");
    if (flags & ~(uint32_t)WGNN_FUZZY_IDX_I64) return fail(WGNN_ERR_BAD_ARG, "unknown flag (valid: WGNN_FUZZY_IDX_I64)");
    if (k < 1 || k > kMaxK) return fail(WGNN_ERR_UNSUPPORTED, "k must be in [1, 64]");
    if (ld_idx < k || ld_d2 < k) return fail(WGNN_ERR_BAD_ARG, "ld_idx and ld_d2 must be >= k");
    if (!(target > 0.0 && target < HUGE_VAL)) return fail(WGNN_ERR_BAD_ARG, "target must be positive and finite");
    if (!idx || !d2 || !rho || !sigma || !member) return fail(WGNN_ERR_BAD_ARG, "idx, d2, rho, sigma and member are required");
    if (!aligned8(rho) || !aligned8(sigma) || ((flags & WGNN_FUZZY_IDX_I64) && !aligned8(idx)))
        return fail(WGNN_ERR_ALIGNMENT, "rho, sigma and an int64 idx must be 8-byte aligned");
    if (!aligned4(idx) || !aligned4(d2) || !aligned4(member)) return fail(WGNN_ERR_ALIGNMENT, "idx, d2 and member must be 4-byte aligned");
    if (n == 0) return WGNN_OK;
    FArgs a{};
    a.idx = idx; a.idx64 = (flags & WGNN_FUZZY_IDX_I64) ? 1 : 0; a.ld_idx = ld_idx; a.d2 = d2; a.ld_d2 = ld_d2; a.n = n; a.k = k;
    a.target = target; a.rho = rho; a.sigma = sigma; a.member = member;
    hipLaunchKernelGGL(fuzzy_rows_kernel, dim3(grid_for(n, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_fuzzy_union(const void* idx, int64_t ld_idx, const float* member, int64_t n, int32_t k, const int64_t* rowptr,
                                const int32_t* col, int64_t nnz, float* w, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_fuzzy_union", what); };
    wgnn::error_clear();
    if (const char* what = check_graph_sizes(n, nnz)) return fail(WGNN_ERR_BAD_ARG, what);
    if (flags & ~(uint32_t)WGNN_FUZZY_IDX_I64) return fail(WGNN_ERR_BAD_ARG, "unknown flag (valid: WGNN_FUZZY_IDX_I64)");
    if (k < 1 || k > kMaxK) return fail(WGNN_ERR_UNSUPPORTED, "k must be in [1, 64]");
    if (ld_idx < k) return fail(WGNN_ERR_BAD_ARG, "ld_idx < k");
    if (!idx || !member || !rowptr || !col || !w) return fail(WGNN_ERR_BAD_ARG, "idx, member, rowptr, col and w are required");
    if (!aligned8(rowptr) || ((flags & WGNN_FUZZY_IDX_I64) && !aligned8(idx)))
        return fail(WGNN_ERR_ALIGNMENT, "rowptr and an int64 idx must be 8-byte aligned");
    if (!aligned4(idx) || !aligned4(member) || !aligned4(col) || !aligned4(w))
        return fail(WGNN_ERR_ALIGNMENT, "idx, member, col and w must be 4-byte aligned");
    if (n == 0 || nnz == 0) return WGNN_OK;
    UArgs a{};
    a.idx = idx; a.idx64 = (flags & WGNN_FUZZY_IDX_I64) ? 1 : 0; a.ld = ld_idx; a.member = member; a.n = n; a.k = k;
    a.rowptr = reinterpret_cast<const i64*>(rowptr); a.col = col; a.nnz = nnz; a.w = w;
    hipLaunchKernelGGL(fuzzy_union_kernel, dim3(grid_for(n, kRowsPerBlock)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_layout_init(float* y, int64_t n, uint32_t seed, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_layout_init", what); };
    wgnn::error_clear();
    if (n < 0 || n > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n must be in [0, 2^31)");
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (!y) return fail(WGNN_ERR_BAD_ARG, "y is required");
    if (!aligned4(y)) return fail(WGNN_ERR_ALIGNMENT, "y must be 4-byte aligned");
    if (n == 0) return WGNN_OK;
    hipLaunchKernelGGL(layout_init_kernel, dim3(grid_for(2 * n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), y, (long)n,
                       (unsigned)seed);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_layout_epoch(const int64_t* rowptr, const int32_t* col, const float* w, int64_t n, int64_t nnz, float wmax,
                                 const float* y_in, float* y_out, int32_t epoch, int32_t n_epochs, float a, float b, float gamma,
                                 float alpha, int32_t n_neg, uint32_t seed, int64_t* fired, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_layout_epoch", what); };
    wgnn::error_clear();
    if (const char* what = check_graph_sizes(n, nnz)) return fail(WGNN_ERR_BAD_ARG, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (!rowptr || !col || !w || !y_in || !y_out) return fail(WGNN_ERR_BAD_ARG, "rowptr, col, w, y_in and y_out are required");
    if (y_in == y_out) return fail(WGNN_ERR_BAD_ARG, "y_out must be another buffer than y_in (an epoch reads the positions before it)");
    if (n_epochs < 1 || n_epochs > WGNN_LAYOUT_MAX_EPOCHS) return fail(WGNN_ERR_BAD_ARG, "n_epochs must be in [1, 10000]");
    if (epoch < 0 || epoch >= n_epochs) return fail(WGNN_ERR_BAD_ARG, "epoch must be in [0, n_epochs)");
    if (n_neg < 0 || n_neg > WGNN_LAYOUT_MAX_NEG) return fail(WGNN_ERR_BAD_ARG, "n_neg must be in [0, 64]");
    if (!(wmax > 0.f && wmax <= FLT_MAX)) return fail(WGNN_ERR_BAD_ARG, "wmax must be positive and finite");
    if (!(fabsf(a) <= FLT_MAX && fabsf(b) <= FLT_MAX && fabsf(gamma) <= FLT_MAX && fabsf(alpha) <= FLT_MAX))
        return fail(WGNN_ERR_BAD_ARG, "a, b, gamma and alpha must be finite");
    if (!aligned8(rowptr) || !aligned8(y_in) || !aligned8(y_out) || !aligned8(fired))
        return fail(WGNN_ERR_ALIGNMENT, "rowptr, y_in, y_out and fired must be 8-byte aligned");
    if (!aligned4(col) || !aligned4(w)) return fail(WGNN_ERR_ALIGNMENT, "col and w must be 4-byte aligned");
    if (n == 0) return WGNN_OK;
    LArgs k{};
    k.rowptr = reinterpret_cast<const i64*>(rowptr); k.col = col; k.w = w; k.n = n; k.nnz = nnz; k.wmax = wmax;
    k.y_in = reinterpret_cast<const float2*>(y_in); k.y_out = reinterpret_cast<float2*>(y_out); k.epoch = epoch;
    k.a = a; k.b = b; k.gamma = gamma; k.alpha = alpha; k.n_neg = n_neg; k.seed = seed; k.fired = reinterpret_cast<i64*>(fired);
    hipLaunchKernelGGL(layout_epoch_kernel, dim3(grid_for(n, kRowsPerBlock)), dim3(256), 0, static_cast<hipStream_t>(stream), k);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}
