// wgnn_diffusion.hip - the diffusion operator of a symmetric CSR graph and a Lanczos iteration on it, behind
// ops.diffusion_operator / ops.lanczos_graph / ops.basis_combine / ops.diffusion_distance and api.ResidentPredictor.diffmap / dpt
// (include/wgnn.h has the contracts).  All float64.  Every product, sum, difference and quotient named there is rounded on its
// own - contraction into fused multiply-adds is switched off for the whole file - and every sum runs in a stated order that the
// grid does not enter, so numpy restates each kernel (tests/diffusion_reference.py) and two calls give the same bits.
//
// Two sum orders:
//   a ROW sum (wgnn_diffusion_degree, wgnn_lanczos_apply): wgnn_layout_epoch's.  Sixteen lanes serve a row, lane l adds the row's
//     entries l, l + 16, ... in order from +0.0, and the sixteen partials fold 8, 4, 2, 1.
//   a DOT (wgnn_lanczos_dots): chunks of WGNN_LANCZOS_CHUNK = 256 consecutive elements.  A workgroup takes a chunk for ALL basis
//     rows, so w is read once per pass and every read of V runs along a row; thread s holds the rounded product of element s
//     (+0.0 past n), sixteen rows' products are staged in LDS at a time, and a wavefront folds a row's 256 products by halves:
//     (p[s] + p[s + 128]) + (p[s + 64] + p[s + 192]) for s < 64 - the folds by 128 and by 64 - then 32 ... 1 by shuffles.  One
//     partial per (chunk, row); a second kernel adds a row's partials in ascending chunk order from +0.0.
// No atomics but the OR into the status word; the halt word is written by the one thread that takes a norm.  A kernel that finds
// the halt word set returns at once (a step after a breakdown is inert).  The integer types, the rowptr clamp, the grid and the
// n / nnz check are wgnn_graph.h's; mix64 is wgnn_resident_rows.h's.  Both headers hold no floating-point arithmetic.
#include <float.h>
#include <limits.h>
#include <math.h>
#include "wgnn_resident_rows.h"
#include "wgnn_graph.h"

#pragma clang fp contract(off)

namespace {
using namespace wgnn;
using namespace wgnn::graph;

constexpr int kLanes = WGNN_DIFFUSION_LANES;       // lanes per row
constexpr int kRowsPerBlock = 256 / kLanes;
constexpr int kChunk = WGNN_LANCZOS_CHUNK;         // elements per dot chunk = threads per workgroup
constexpr int kTile = 16;                          // basis rows staged in LDS at a time (32 KiB)
static_assert(kLanes == 16 && kChunk == 256, "the folds below and include/wgnn.h state sixteen lanes and chunks of 256");
static_assert(kMaxBlocks == WGNN_DIFFUSION_MAX_BLOCKS, "grid_for's cap is the largest grid include/wgnn.h states");

__device__ __forceinline__ bool halted(const i64* halt) { return halt && *halt != 0; }

struct Csr { const i64* rowptr; const int* col; long n; long nnz; };

// The row sum of term(e, u) over row v's entries: valid in the row's lane 0.  A column outside [0, n) is skipped, a row whose
// rowptr is out of order is clamped into [0, nnz]; both and an unsorted row leave their bit.
template <class Term>
__device__ __forceinline__ double row_sum(const Csr& g, long v, int sub, unsigned& bits, Term term) {
    i64 e0 = g.rowptr[v], e1 = g.rowptr[v + 1];
    if (e0 < 0 || e1 < e0 || e1 > g.nnz || (v == 0 && e0 != 0) || (v == g.n - 1 && e1 != g.nnz)) {
        bits |= WGNN_DIFFUSION_BAD_ROWPTR;                         // nothing outside [0, nnz) is read
        e0 = clampl(e0, g.nnz);
        e1 = e1 < e0 ? e0 : (e1 > g.nnz ? g.nnz : e1);             // a row that runs backwards is empty
    }
    double acc = 0.0;
    for (i64 e = e0 + sub; e < e1; e += kLanes) {
        const int u = g.col[e];
        if (e > e0 && g.col[e - 1] >= u) bits |= WGNN_DIFFUSION_UNSORTED;
        if (u < 0 || u >= g.n) { bits |= WGNN_DIFFUSION_BAD_COL; continue; }
        acc = acc + term(e, u, bits);
    }
#pragma unroll
    for (int off = kLanes / 2; off >= 1; off >>= 1) acc = acc + __shfl_down(acc, off, kLanes);     // lane l += lane l + off
    return acc;
}

__device__ __forceinline__ void leave_bits(unsigned bits, u64* status) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) bits |= (unsigned)__shfl_xor((int)bits, off, 64);
    if ((threadIdx.x & 63) == 0 && bits) atomicOr(status, (u64)bits);
}

__device__ __forceinline__ bool weight_ok(float w) { return w >= 0.f && w <= FLT_MAX; }           // not negative, infinite or NaN

// ---------------------------------------------------------------------------------------------------------------------------
// q_i = sum_j (double)w_ij (q_in == null), or z_i = sqrt(sum_j w_ij / (q_i q_j))
struct GArgs { Csr g; const float* w; const double* q; double* out; u64* status; };

__global__ void __launch_bounds__(256) degree_kernel(const GArgs a) {
    const int sub = threadIdx.x & (kLanes - 1), slot = threadIdx.x / kLanes;
    unsigned bits = 0;
    for (long v = (long)blockIdx.x * kRowsPerBlock + slot; v < a.g.n; v += (long)gridDim.x * kRowsPerBlock) {
        const double qv = a.q ? a.q[v] : 0.0;
        const double sum = row_sum(a.g, v, sub, bits, [&](i64 e, int u, unsigned& b) -> double {
            const float w = a.w[e];
            if (!weight_ok(w)) { b |= WGNN_DIFFUSION_BAD_WEIGHT; return 0.0; }
            if (!a.q) return (double)w;
            return w == 0.f ? 0.0 : (double)w / (qv * a.q[u]);
        });
        if (sub == 0) a.out[v] = a.q ? sqrt(sum) : sum;
    }
    leave_bits(bits, a.status);
}

// t_ij = (w_ij / (q_i q_j)) / (z_i z_j): both products are commutative, so t_ij and t_ji are the same bits
struct WArgs { Csr g; const float* w; const double* q; const double* z; double* t; u64* status; };

__global__ void __launch_bounds__(256) weights_kernel(const WArgs a) {
    const int sub = threadIdx.x & (kLanes - 1), slot = threadIdx.x / kLanes;
    unsigned bits = 0;
    for (long v = (long)blockIdx.x * kRowsPerBlock + slot; v < a.g.n; v += (long)gridDim.x * kRowsPerBlock) {
        const i64 e0 = clampl(a.g.rowptr[v], a.g.nnz), e1 = clampl(a.g.rowptr[v + 1], a.g.nnz);
        const double qv = a.q[v], zv = a.z[v];
        for (i64 e = e0 + sub; e < e1; e += kLanes) {
            const int u = a.g.col[e];
            const float w = a.w[e];
            double t = 0.0;
            if (u < 0 || u >= a.g.n) bits |= WGNN_DIFFUSION_BAD_COL;
            else if (!weight_ok(w)) bits |= WGNN_DIFFUSION_BAD_WEIGHT;
            else if (w != 0.f) t = ((double)w / (qv * a.q[u])) / (zv * a.z[u]);
            a.t[e] = t;
        }
    }
    leave_bits(bits, a.status);
}

// ---------------------------------------------------------------------------------------------------------------------------
struct IArgs { const double* z; const unsigned char* mask; long n; unsigned seed; double* w0; double* w1; };

__global__ void __launch_bounds__(256) init_kernel(const IArgs a) {
    const u64 key = mix64(((u64)a.seed << 32) | 0xFFFFFFFEull);     // wgnn_layout_init's family; its own key word is 0xFFFFFFFF
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256) {
        const bool on = a.mask[i] != 0;
        const u64 h = mix64(key + (u64)i);
        a.w0[i] = on ? a.z[i] : 0.0;
        a.w1[i] = on ? ((double)(h >> 11) * 0x1p-53) * 2.0 - 1.0 : 0.0;
    }
}

// y_i = sum_j t_ij x_j
struct AArgs { Csr g; const double* t; const double* x; double* y; const i64* halt; u64* status; };

__global__ void __launch_bounds__(256) apply_kernel(const AArgs a) {
    if (halted(a.halt)) return;
    const int sub = threadIdx.x & (kLanes - 1), slot = threadIdx.x / kLanes;
    unsigned bits = 0;
    for (long v = (long)blockIdx.x * kRowsPerBlock + slot; v < a.g.n; v += (long)gridDim.x * kRowsPerBlock) {
        const double sum = row_sum(a.g, v, sub, bits, [&](i64 e, int u, unsigned& b) -> double {
            const double t = a.t[e];
            if (!(t >= 0.0 && t <= DBL_MAX)) { b |= WGNN_DIFFUSION_BAD_WEIGHT; return 0.0; }
            return t * a.x[u];
        });
        if (sub == 0) a.y[v] = sum;
    }
    leave_bits(bits, a.status);
}

// partial[chunk, r] = the fold by halves of V[r, chunk] * w[chunk]
struct DArgs { const double* V; long ld; int n_rows; const double* w; long n; double* partial; long ldp; const i64* halt; };

__global__ void __launch_bounds__(256) dots_kernel(const DArgs a) {
    __shared__ double s_prod[kTile][kChunk];
    if (halted(a.halt)) return;                                    // uniform: before any barrier
    const int s = threadIdx.x, lane = s & 63, wave = s >> 6;
    const long n_chunks = (a.n + kChunk - 1) / kChunk;
    for (long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const long i = ch * kChunk + s;
        const bool in = i < a.n;
        const double wv = in ? a.w[i] : 0.0;
        for (int r0 = 0; r0 < a.n_rows; r0 += kTile) {
#pragma unroll
            for (int t = 0; t < kTile; ++t) {
                const int r = r0 + t;
                s_prod[t][s] = (in && r < a.n_rows) ? a.V[(long)r * a.ld + i] * wv : 0.0;
            }
            __syncthreads();
            for (int t = wave; t < kTile && r0 + t < a.n_rows; t += 4) {                   // wave-uniform
                double c = (s_prod[t][lane] + s_prod[t][lane + 128]) + (s_prod[t][lane + 64] + s_prod[t][lane + 192]);
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) c = c + __shfl_down(c, off, 64);
                if (lane == 0) a.partial[ch * a.ldp + (r0 + t)] = c;
            }
            __syncthreads();
        }
    }
}

// c[r] = the partials of row r in ascending chunk order; a norm takes the root and may halt the run
struct FArgs { const double* partial; long ldp; long n_chunks; int n_rows; double* c; double* keep; int norm; i64* halt; i64 tag; };

__global__ void __launch_bounds__(256) fold_kernel(const FArgs a) {
    if (halted(a.halt)) return;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n_rows) return;
    double sum = 0.0;
    for (long ch = 0; ch < a.n_chunks; ++ch) sum = sum + a.partial[ch * a.ldp + r];
    if (a.norm) sum = sqrt(sum);
    a.c[r] = sum;
    if (a.keep && r == a.n_rows - 1) *a.keep = sum;
    if (a.norm && a.halt && !(sum > WGNN_LANCZOS_BREAKDOWN)) *a.halt = a.tag;              // n_rows == 1: one thread; a NaN halts too
}

// w_i = w_i - V[r, i] * c[r], r ascending
struct UArgs { const double* V; long ld; int n_rows; const double* c; double* w; long n; const i64* halt; };

__global__ void __launch_bounds__(256) update_kernel(const UArgs a) {
    if (halted(a.halt)) return;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256) {
        double wv = a.w[i];
        const double* v = a.V + i;
#pragma unroll 8
        for (int r = 0; r < a.n_rows; ++r) wv = wv - v[(long)r * a.ld] * a.c[r];
        a.w[i] = wv;
    }
}

// v_i = w_i / beta
struct SArgs { const double* w; const double* beta; double* v; long n; const i64* halt; };

__global__ void __launch_bounds__(256) scale_kernel(const SArgs a) {
    if (halted(a.halt)) return;
    const double beta = *a.beta;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256) a.v[i] = a.w[i] / beta;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Y[i, 0] = V[0, i];  Y[i, c] = sum_{j = 1 .. m} V[j, i] * S[j - 1, c - 1], j ascending.  blockIdx.y is the column.
struct CArgs { const double* V; long ld; int m; const double* S; long lds; double* Y; long ldy; long n; };

__global__ void __launch_bounds__(256) combine_kernel(const CArgs a) {
    const int c = blockIdx.y;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256) {
        double sum = 0.0;
        if (c == 0) sum = a.V[i];
        else {
#pragma unroll 8
            for (int j = 1; j <= a.m; ++j) sum = sum + a.V[(long)j * a.ld + i] * a.S[(long)(j - 1) * a.lds + (c - 1)];
        }
        a.Y[i * a.ldy + c] = sum;
    }
}

// d_i = min over the roots r of sqrt(sum_{l = 1 .. n_dcs - 1} (g_l (Y[r, l] - Y[i, l]))^2), l ascending
struct XArgs { const double* Y; long ldy; long n; const double* g; int n_dcs; const i64* roots; int n_roots; double* d; };

__global__ void __launch_bounds__(256) distance_kernel(const XArgs a) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256) {
        double best = HUGE_VAL;
        for (int k = 0; k < a.n_roots; ++k) {
            const i64 r = a.roots[k];
            if (r < 0 || r >= a.n) continue;                       // no root: nothing is read
            double sum = 0.0;
            for (int l = 1; l < a.n_dcs; ++l) {
                const double p = a.g[l] * (a.Y[r * a.ldy + l] - a.Y[i * a.ldy + l]);
                sum = sum + p * p;
            }
            const double d = sqrt(sum);
            if (d < best || d != d) best = d;                      // a NaN coordinate shows
        }
        a.d[i] = best;
    }
}

// host side
unsigned capped(unsigned blocks, int32_t grid_blocks) { return grid_blocks && (unsigned)grid_blocks < blocks ? (unsigned)grid_blocks : blocks; }
bool bad_grid(int32_t grid_blocks) { return grid_blocks < 0 || grid_blocks > kMaxBlocks; }
bool overlap(const void* p, const void* base, int64_t bytes) {
    const char* q = static_cast<const char*>(p);
    const char* b = static_cast<const char*>(base);
    return q >= b && q < b + bytes;
}
bool launched() { return hipGetLastError() == hipSuccess; }

}  // namespace

#define WGNN_DIFF_ENTRY(name) \
    auto fail = [](int code, const char* what) { return wgnn::fail(code, name, what); }; \
    wgnn::error_clear()

extern "C" int wgnn_diffusion_degree(const int64_t* rowptr, const int32_t* col, const float* w, int64_t n, int64_t nnz, const double* q,
                                     double* out, int64_t* status, int32_t grid_blocks, uint32_t flags, void* stream) {
    WGNN_DIFF_ENTRY("wgnn_diffusion_degree");
    if (const char* what = check_graph_sizes(n, nnz)) return fail(WGNN_ERR_BAD_ARG, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (bad_grid(grid_blocks)) return fail(WGNN_ERR_BAD_ARG, "grid_blocks must be in [0, 8192] (0 = from n)");
    if (!rowptr || !col || !w || !out || !status) return fail(WGNN_ERR_BAD_ARG, "rowptr, col, w, out and status are required");
    if (q == out) return fail(WGNN_ERR_BAD_ARG, "out must be another buffer than q (every row reads its neighbours' q)");
    if (!aligned8(rowptr) || !aligned8(q) || !aligned8(out) || !aligned8(status))
        return fail(WGNN_ERR_ALIGNMENT, "rowptr, q, out and status must be 8-byte aligned");
    if (!aligned4(col) || !aligned4(w)) return fail(WGNN_ERR_ALIGNMENT, "col and w must be 4-byte aligned");
    if (n == 0) return WGNN_OK;
    GArgs a{{reinterpret_cast<const i64*>(rowptr), col, (long)n, (long)nnz}, w, q, out, reinterpret_cast<u64*>(status)};
    hipLaunchKernelGGL(degree_kernel, dim3(capped(grid_for(n, kRowsPerBlock), grid_blocks)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return launched() ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_diffusion_weights(const int64_t* rowptr, const int32_t* col, const float* w, int64_t n, int64_t nnz, const double* q,
                                      const double* z, double* t, int64_t* status, int32_t grid_blocks, uint32_t flags, void* stream) {
    WGNN_DIFF_ENTRY("wgnn_diffusion_weights");
    if (const char* what = check_graph_sizes(n, nnz)) return fail(WGNN_ERR_BAD_ARG, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (bad_grid(grid_blocks)) return fail(WGNN_ERR_BAD_ARG, "grid_blocks must be in [0, 8192] (0 = from n)");
    if (!rowptr || !col || !w || !q || !z || !t || !status) return fail(WGNN_ERR_BAD_ARG, "rowptr, col, w, q, z, t and status are required");
    if (t == q || t == z) return fail(WGNN_ERR_BAD_ARG, "t must be another buffer than q and z");
    if (!aligned8(rowptr) || !aligned8(q) || !aligned8(z) || !aligned8(t) || !aligned8(status))
        return fail(WGNN_ERR_ALIGNMENT, "rowptr, q, z, t and status must be 8-byte aligned");
    if (!aligned4(col) || !aligned4(w)) return fail(WGNN_ERR_ALIGNMENT, "col and w must be 4-byte aligned");
    if (n == 0 || nnz == 0) return WGNN_OK;
    WArgs a{{reinterpret_cast<const i64*>(rowptr), col, (long)n, (long)nnz}, w, q, z, t, reinterpret_cast<u64*>(status)};
    hipLaunchKernelGGL(weights_kernel, dim3(capped(grid_for(n, kRowsPerBlock), grid_blocks)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return launched() ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_lanczos_init(const double* z, const uint8_t* mask, int64_t n, uint32_t seed, double* w0, double* w1, uint32_t flags,
                                 void* stream) {
    WGNN_DIFF_ENTRY("wgnn_lanczos_init");
    if (n < 0 || n > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n must be in [0, 2^31)");
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (!z || !mask || !w0 || !w1) return fail(WGNN_ERR_BAD_ARG, "z, mask, w0 and w1 are required");
    if (w0 == w1 || w0 == z || w1 == z) return fail(WGNN_ERR_BAD_ARG, "z, w0 and w1 must be three buffers");
    if (!aligned8(z) || !aligned8(w0) || !aligned8(w1)) return fail(WGNN_ERR_ALIGNMENT, "z, w0 and w1 must be 8-byte aligned");
    if (n == 0) return WGNN_OK;
    IArgs a{z, mask, (long)n, (unsigned)seed, w0, w1};
    hipLaunchKernelGGL(init_kernel, dim3(grid_for(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return launched() ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_lanczos_apply(const int64_t* rowptr, const int32_t* col, const double* t, int64_t n, int64_t nnz, const double* x,
                                  double* y, const int64_t* halt, int64_t* status, int32_t grid_blocks, uint32_t flags, void* stream) {
    WGNN_DIFF_ENTRY("wgnn_lanczos_apply");
    if (const char* what = check_graph_sizes(n, nnz)) return fail(WGNN_ERR_BAD_ARG, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (bad_grid(grid_blocks)) return fail(WGNN_ERR_BAD_ARG, "grid_blocks must be in [0, 8192] (0 = from n)");
    if (!rowptr || !col || !t || !x || !y || !status) return fail(WGNN_ERR_BAD_ARG, "rowptr, col, t, x, y and status are required");
    if (x == y) return fail(WGNN_ERR_BAD_ARG, "y must be another buffer than x (every row reads its neighbours' x)");
    if (!aligned8(rowptr) || !aligned8(t) || !aligned8(x) || !aligned8(y) || !aligned8(halt) || !aligned8(status))
        return fail(WGNN_ERR_ALIGNMENT, "rowptr, t, x, y, halt and status must be 8-byte aligned");
    if (!aligned4(col)) return fail(WGNN_ERR_ALIGNMENT, "col must be 4-byte aligned");
    if (n == 0) return WGNN_OK;
    AArgs a{{reinterpret_cast<const i64*>(rowptr), col, (long)n, (long)nnz}, t, x, y, reinterpret_cast<const i64*>(halt),
            reinterpret_cast<u64*>(status)};
    hipLaunchKernelGGL(apply_kernel, dim3(capped(grid_for(n, kRowsPerBlock), grid_blocks)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return launched() ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int64_t wgnn_lanczos_dots_workspace_bytes(int64_t n, int32_t n_rows) {
    if (n < 0 || n_rows < 1) return 0;
    return ((n + kChunk - 1) / kChunk) * (int64_t)n_rows * 8;
}

extern "C" int wgnn_lanczos_dots(const double* V, int64_t ld, int32_t n_rows, const double* w, int64_t n, double* c, double* keep,
                                 int64_t* halt, int64_t tag, void* workspace, int64_t workspace_bytes, int32_t grid_blocks,
                                 uint32_t flags, void* stream) {
    WGNN_DIFF_ENTRY("wgnn_lanczos_dots");
    const bool norm = (flags & WGNN_LANCZOS_NORM) != 0;
    if (n < 0 || n > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n must be in [0, 2^31)");
    if (flags & ~(uint32_t)WGNN_LANCZOS_NORM) return fail(WGNN_ERR_BAD_ARG, "unknown flag (valid: WGNN_LANCZOS_NORM)");
    if (bad_grid(grid_blocks)) return fail(WGNN_ERR_BAD_ARG, "grid_blocks must be in [0, 8192] (0 = from n)");
    if (n_rows < 1 || n_rows > WGNN_LANCZOS_MAX_STEPS + 1) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [1, 1025]");
    if (!w || !c || !workspace) return fail(WGNN_ERR_BAD_ARG, "w, c and workspace are required");
    if (norm && (V || n_rows != 1)) return fail(WGNN_ERR_BAD_ARG, "a norm takes no V and n_rows = 1 (it is the dot of w with itself)");
    if (!norm && !V) return fail(WGNN_ERR_BAD_ARG, "V is required without WGNN_LANCZOS_NORM");
    if (!norm && ld < n) return fail(WGNN_ERR_BAD_ARG, "ld < n");
    if (tag == 0) return fail(WGNN_ERR_BAD_ARG, "tag must not be 0 (0 in the halt word means running)");
    if (workspace_bytes < wgnn_lanczos_dots_workspace_bytes(n, n_rows))
        return fail(WGNN_ERR_WORKSPACE, "workspace is smaller than wgnn_lanczos_dots_workspace_bytes asks for");
    if (c == w || overlap(c, workspace, workspace_bytes) || overlap(w, workspace, workspace_bytes) ||
        (V && (overlap(c, V, ((int64_t)(n_rows - 1) * ld + n) * 8) || overlap(workspace, V, ((int64_t)(n_rows - 1) * ld + n) * 8))))
        return fail(WGNN_ERR_BAD_ARG, "c, w, V and workspace must not overlap");
    if (!aligned8(V) || !aligned8(w) || !aligned8(c) || !aligned8(keep) || !aligned8(halt) || !aligned8(workspace))
        return fail(WGNN_ERR_ALIGNMENT, "V, w, c, keep, halt and workspace must be 8-byte aligned");
    if (n == 0) return WGNN_OK;
    const long n_chunks = (n + kChunk - 1) / kChunk;
    DArgs d{norm ? w : V, norm ? 0 : (long)ld, n_rows, w, (long)n, static_cast<double*>(workspace), (long)n_rows,
            reinterpret_cast<const i64*>(halt)};
    hipLaunchKernelGGL(dots_kernel, dim3(capped(grid_for(n_chunks, 1), grid_blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), d);
    FArgs f{static_cast<const double*>(workspace), (long)n_rows, n_chunks, n_rows, c, keep, norm ? 1 : 0, reinterpret_cast<i64*>(halt),
            (i64)tag};
    hipLaunchKernelGGL(fold_kernel, dim3(grid_for(n_rows, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), f);
    return launched() ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_lanczos_update(const double* V, int64_t ld, int32_t n_rows, const double* c, double* w, int64_t n,
                                   const int64_t* halt, int32_t grid_blocks, uint32_t flags, void* stream) {
    WGNN_DIFF_ENTRY("wgnn_lanczos_update");
    if (n < 0 || n > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n must be in [0, 2^31)");
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (bad_grid(grid_blocks)) return fail(WGNN_ERR_BAD_ARG, "grid_blocks must be in [0, 8192] (0 = from n)");
    if (n_rows < 1 || n_rows > WGNN_LANCZOS_MAX_STEPS + 1) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [1, 1025]");
    if (!V || !c || !w) return fail(WGNN_ERR_BAD_ARG, "V, c and w are required");
    if (ld < n) return fail(WGNN_ERR_BAD_ARG, "ld < n");
    if (c == w || overlap(w, V, ((int64_t)(n_rows - 1) * ld + n) * 8) || overlap(c, V, ((int64_t)(n_rows - 1) * ld + n) * 8))
        return fail(WGNN_ERR_BAD_ARG, "c, w and V must not overlap (w is updated in place against rows that stay)");
    if (!aligned8(V) || !aligned8(c) || !aligned8(w) || !aligned8(halt)) return fail(WGNN_ERR_ALIGNMENT, "V, c, w and halt must be 8-byte aligned");
    if (n == 0) return WGNN_OK;
    UArgs a{V, (long)ld, n_rows, c, w, (long)n, reinterpret_cast<const i64*>(halt)};
    hipLaunchKernelGGL(update_kernel, dim3(capped(grid_for(n, 256), grid_blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return launched() ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_lanczos_scale(const double* w, const double* beta, double* v, int64_t n, const int64_t* halt, int32_t grid_blocks,
                                  uint32_t flags, void* stream) {
    WGNN_DIFF_ENTRY("wgnn_lanczos_scale");
    if (n < 0 || n > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n must be in [0, 2^31)");
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (bad_grid(grid_blocks)) return fail(WGNN_ERR_BAD_ARG, "grid_blocks must be in [0, 8192] (0 = from n)");
    if (!w || !beta || !v) return fail(WGNN_ERR_BAD_ARG, "w, beta and v are required");
    if (v == w || beta == v || beta == w) return fail(WGNN_ERR_BAD_ARG, "w, beta and v must be three buffers");
    if (!aligned8(w) || !aligned8(beta) || !aligned8(v) || !aligned8(halt)) return fail(WGNN_ERR_ALIGNMENT, "w, beta, v and halt must be 8-byte aligned");
    if (n == 0) return WGNN_OK;
    SArgs a{w, beta, v, (long)n, reinterpret_cast<const i64*>(halt)};
    hipLaunchKernelGGL(scale_kernel, dim3(capped(grid_for(n, 256), grid_blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return launched() ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_basis_combine(const double* V, int64_t ld, int32_t m, const double* S, int64_t lds, int32_t n_cols, double* Y,
                                  int64_t ldy, int64_t n, uint32_t flags, void* stream) {
    WGNN_DIFF_ENTRY("wgnn_basis_combine");
    if (n < 0 || n > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n must be in [0, 2^31)");
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (m < 0 || m > WGNN_LANCZOS_MAX_STEPS) return fail(WGNN_ERR_BAD_ARG, "m must be in [0, 1024]");
    if (n_cols < 0 || n_cols >= WGNN_DIFFUSION_MAX_COMPS) return fail(WGNN_ERR_BAD_ARG, "n_cols must be in [0, 63]");
    if (!V || !Y || (n_cols > 0 && !S)) return fail(WGNN_ERR_BAD_ARG, "V, Y and (with a column) S are required");
    if (ld < n || lds < n_cols || ldy < n_cols + 1) return fail(WGNN_ERR_BAD_ARG, "ld < n, lds < n_cols or ldy < n_cols + 1");
    if (Y == V || Y == S || overlap(Y, V, ((int64_t)m * ld + n) * 8)) return fail(WGNN_ERR_BAD_ARG, "Y must not overlap V or S");
    if (!aligned8(V) || !aligned8(S) || !aligned8(Y)) return fail(WGNN_ERR_ALIGNMENT, "V, S and Y must be 8-byte aligned");
    if (n == 0) return WGNN_OK;
    CArgs a{V, (long)ld, m, S, (long)lds, Y, (long)ldy, (long)n};
    hipLaunchKernelGGL(combine_kernel, dim3(grid_for(n, 256), n_cols + 1), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return launched() ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_diffusion_distance(const double* Y, int64_t ldy, int64_t n, const double* g, int32_t n_dcs, const int64_t* roots,
                                       int32_t n_roots, double* d, uint32_t flags, void* stream) {
    WGNN_DIFF_ENTRY("wgnn_diffusion_distance");
    if (n < 0 || n > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n must be in [0, 2^31)");
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (n_dcs < 2 || n_dcs > WGNN_DIFFUSION_MAX_COMPS) return fail(WGNN_ERR_BAD_ARG, "n_dcs must be in [2, 64]");
    if (n_roots < 1) return fail(WGNN_ERR_BAD_ARG, "n_roots must be >= 1");
    if (ldy < n_dcs) return fail(WGNN_ERR_BAD_ARG, "ldy < n_dcs");
    if (!Y || !g || !roots || !d) return fail(WGNN_ERR_BAD_ARG, "Y, g, roots and d are required");
    if (d == Y || d == g) return fail(WGNN_ERR_BAD_ARG, "d must be another buffer than Y and g");
    if (!aligned8(Y) || !aligned8(g) || !aligned8(roots) || !aligned8(d)) return fail(WGNN_ERR_ALIGNMENT, "Y, g, roots and d must be 8-byte aligned");
    if (n == 0) return WGNN_OK;
    XArgs a{Y, (long)ldy, (long)n, g, n_dcs, reinterpret_cast<const i64*>(roots), n_roots, d};
    hipLaunchKernelGGL(distance_kernel, dim3(grid_for(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return launched() ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}
