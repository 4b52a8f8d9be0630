// wgnn_leiden.hip - the refinement of a deterministic, synchronous, integer Leiden (include/wgnn.h has the contract).  P is the
// partition the moving phase left, ref the refined one inside it: a refined community carries the id of the vertex that founded it, only a vertex
// that is alone moves, and a move is accepted only when the founder of its target stays, so that every refined community stays
// connected.
//
// wgnn_leiden_boundary: a wavefront per row; kinP[v] by a wavefront sum, ext[ref[v]] by one 64-bit atomic per row.
// wgnn_leiden_refine_sweep: the kin sweep of wgnn_graph.h - wgnn_louvain_sweep's tables and its three routes by row length - with
//   a policy of its own: keyed by the refined id of the neighbours in v's own P-community.  A vertex that may not move leaves
//   before its row is read.
// wgnn_leiden_accept: a thread per vertex.
#include "wgnn_graph.h"

namespace {
using namespace wgnn;
using namespace wgnn::graph;

struct RArgs {
    KinGraph g;
    const int* P; const int* ref; const i64* deg; const i64* totP; const i64* tot; const int* size;
    const i64* ext; const i64* kinP;
    i64 mden; i64 num; int odd;
    int* prop; i64* gain;
};

// ref[v] and P[v] are ids and the founder of ref[v] lies in P[v]
__device__ __forceinline__ bool part_ok(const int* P, const int* ref, long n, long v) {
    const int own = ref[v], Pv = P[v];
    return is_id(own, n) && is_id(Pv, n) && P[own] == Pv;
}

// the refinement's policy for the kin sweep (wgnn_graph.h): the key of a neighbour in v's own P-community is its refined id
struct Refine {
    typedef RArgs Args;
    struct Vertex { int own; int Pv; i64 degv; i64 totPv; };

    // may v move?  Alone in its refined community and well connected to its P-community; a malformed partition stays and is
    // reported.  The same in every thread of the workgroup.
    static __device__ __forceinline__ bool enter(const RArgs& a, long v, Vertex& x) {
        if (!part_ok(a.P, a.ref, a.g.n, v)) {
            if ((threadIdx.x & 63) == 0) atomicOr(&a.g.stats[3], (u64)WGNN_LEIDEN_BAD_PARTITION);
            return false;
        }
        x.own = a.ref[v]; x.Pv = a.P[v]; x.degv = a.deg[v]; x.totPv = a.totP[x.Pv];
        return a.size[x.own] == 1 && a.kinP[v] * a.mden >= a.num * x.degv * (x.totPv - x.degv);
    }
    // the refined community of neighbour u of v for kin: -1 for the diagonal, another P-community, or an id outside [0, n)
    static __device__ __forceinline__ int key(const RArgs& a, const Vertex& x, long v, int u) {
        if (u == v || !is_id(u, a.g.n) || a.P[u] != x.Pv) return -1;
        const int S = a.ref[u];
        return is_id(S, a.g.n) ? S : -1;
    }
    static constexpr bool kOwnKin = false;                     // a vertex that may move is alone: staying scores 0
    // refined community S with kin[S] = kin against the best so far: the gate, S's own well-connectedness, a score above 0; then
    // the total order (higher score, lower id)
    static __device__ __forceinline__ void consider(Best& b, const RArgs& a, const Vertex& x, int S, i64 kin) {
        if (S == x.own || (a.odd ? S < x.own : S > x.own) || !is_id(S, a.g.n)) return;
        const i64 ts = a.tot[S];
        if (a.ext[S] * a.mden < a.num * ts * (x.totPv - ts)) return;
        const i64 s = kin * a.mden - a.num * x.degv * ts;
        if (s <= 0) return;
        if (b.c < 0 || s > b.score || (s == b.score && S < b.c)) { b.score = s; b.c = S; }
    }
    static __device__ __forceinline__ void write(const RArgs& a, long v, const Vertex&, const Best& b) {
        a.prop[v] = b.c >= 0 ? b.c : a.ref[v];
        a.gain[v] = b.c >= 0 ? b.score : 0;
    }
};

__global__ void __launch_bounds__(64) refine_wave_kernel(const RArgs a) { kin_sweep_wave<Refine>(a); }
__global__ void __launch_bounds__(256) refine_heavy_kernel(const RArgs a) { kin_sweep_heavy<Refine>(a); }

struct BArgs { const i64* rowptr; const int* col; const int* w; long n; long nnz; const int* P; const int* ref; u64* ext; i64* kinP; u64* stats; };

__global__ void __launch_bounds__(256) boundary_kernel(const BArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long v = (long)blockIdx.x * 4 + wave; v < a.n; v += (long)gridDim.x * 4) {          // wave-uniform
        const i64 e0 = clampl(a.rowptr[v], a.nnz), e1 = clampl(a.rowptr[v + 1], a.nnz);
        const bool ok = part_ok(a.P, a.ref, a.n, v);
        if (!ok && lane == 0) atomicOr(&a.stats[3], (u64)WGNN_LEIDEN_BAD_PARTITION);
        const int own = a.ref[v], Pv = a.P[v];
        i64 inside = 0, out = 0;
        for (i64 e = e0 + lane; e < e1; e += 64) {
            const int u = a.col[e];
            if (u == v || !is_id(u, a.n) || a.P[u] != Pv) continue;
            inside += a.w[e];
            if (a.ref[u] != own) out += a.w[e];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            inside += __shfl_xor(inside, off, 64);
            out += __shfl_xor(out, off, 64);
        }
        if (lane == 0) {
            if (a.kinP) a.kinP[v] = inside;
            if (ok && out) atomicAdd(&a.ext[own], (u64)out);
        }
    }
}

struct CArgs { const int* ref; const int* prop; long n; int* next; i64* gain; u64* stats; };

__global__ void __launch_bounds__(256) accept_kernel(const CArgs a) {
    __shared__ i64 s_red[4];
    i64 moved = 0;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < a.n; v += (long)gridDim.x * 256) {
        const int r = a.ref[v], p = a.prop[v];
        const bool ok = p != r && is_id(p, a.n) && a.prop[p] == p;          // the founder of the target stays at home
        a.next[v] = ok ? p : r;
        if (!ok) a.gain[v] = 0;
        moved += ok;
    }
    moved = block_sum(moved, s_red);
    if (threadIdx.x == 0 && moved) atomicAdd(&a.stats[0], (u64)moved);
}

}  // namespace

extern "C" int wgnn_leiden_boundary(const int64_t* rowptr, const int32_t* col, const int32_t* w, int64_t n, int64_t nnz,
                                    const int32_t* P, const int32_t* ref, int64_t* ext, int64_t* kinP, int64_t* stats,
                                    uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_leiden_boundary", what); };
    wgnn::error_clear();
    if (const char* what = check_graph_sizes(n, nnz)) return fail(WGNN_ERR_BAD_ARG, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (!rowptr || !col || !w || !P || !ref || !ext || !stats) return fail(WGNN_ERR_BAD_ARG, "rowptr, col, w, P, ref, ext and stats are required");
    if (!aligned8(rowptr) || !aligned8(ext) || !aligned8(kinP) || !aligned8(stats))
        return fail(WGNN_ERR_ALIGNMENT, "rowptr, ext, kinP and stats must be 8-byte aligned");
    if (!aligned4(col) || !aligned4(w) || !aligned4(P) || !aligned4(ref)) return fail(WGNN_ERR_ALIGNMENT, "col, w, P and ref must be 4-byte aligned");
    if (n == 0) return WGNN_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(ext, 0, (size_t)n * 8, st) != hipSuccess) return fail(WGNN_ERR_LAUNCH, "hipMemsetAsync failed");
    BArgs a{reinterpret_cast<const i64*>(rowptr), col, w, (long)n, (long)nnz, P, ref, reinterpret_cast<u64*>(ext),
            reinterpret_cast<i64*>(kinP), reinterpret_cast<u64*>(stats)};
    hipLaunchKernelGGL(boundary_kernel, dim3(grid_for(n, 4)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_leiden_refine_sweep(const int64_t* rowptr, const int32_t* col, const int32_t* w, int64_t n, int64_t nnz,
                                        const int32_t* P, const int32_t* ref, const int64_t* deg, const int64_t* totP,
                                        const int64_t* tot, const int32_t* size, const int64_t* ext, const int64_t* kinP,
                                        int64_t m_den, int64_t num, int32_t sweep, const int32_t* heavy, int32_t n_heavy,
                                        int32_t wave_rows, int32_t block_rows, int32_t* prop, int64_t* gain, int64_t* stats,
                                        void* workspace, int64_t workspace_bytes, int32_t scratch_blocks, uint32_t flags,
                                        void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_leiden_refine_sweep", what); };
    wgnn::error_clear();
    if (const char* what = check_graph_sizes(n, nnz)) return fail(WGNN_ERR_BAD_ARG, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (!rowptr || !col || !w || !P || !ref || !deg || !totP || !tot || !size || !ext || !kinP || !prop || !gain || !stats)
        return fail(WGNN_ERR_BAD_ARG, "rowptr, col, w, P, ref, deg, totP, tot, size, ext, kinP, prop, gain and stats are required");
    if (m_den < 1 || num < 1) return fail(WGNN_ERR_BAD_ARG, "m_den and num must be positive");
    if (sweep < 0) return fail(WGNN_ERR_BAD_ARG, "sweep must not be negative");
    if (const Refusal r = check_routes(heavy, n_heavy, wave_rows, block_rows, scratch_blocks); r.code) return fail(r.code, r.what);
    if (!aligned8(rowptr) || !aligned8(deg) || !aligned8(totP) || !aligned8(tot) || !aligned8(ext) || !aligned8(kinP) || !aligned8(gain) ||
        !aligned8(stats))
        return fail(WGNN_ERR_ALIGNMENT, "rowptr, deg, totP, tot, ext, kinP, gain and stats must be 8-byte aligned");
    if (!aligned4(col) || !aligned4(w) || !aligned4(P) || !aligned4(ref) || !aligned4(size) || !aligned4(prop) || !aligned4(heavy))
        return fail(WGNN_ERR_ALIGNMENT, "col, w, P, ref, size, prop and heavy must be 4-byte aligned");
    if (const Refusal r = check_scratch(n, workspace, workspace_bytes, scratch_blocks); r.code) return fail(r.code, r.what);
    if (n == 0) return WGNN_OK;

    RArgs a{};
    a.g = kin_graph(rowptr, col, w, n, nnz, heavy, n_heavy, wave_rows, block_rows, workspace, scratch_blocks, stats);
    a.P = P; a.ref = ref; a.deg = reinterpret_cast<const i64*>(deg); a.totP = reinterpret_cast<const i64*>(totP);
    a.tot = reinterpret_cast<const i64*>(tot); a.size = size;
    a.ext = reinterpret_cast<const i64*>(ext); a.kinP = reinterpret_cast<const i64*>(kinP);
    a.mden = m_den; a.num = num; a.odd = sweep & 1;
    a.prop = prop; a.gain = reinterpret_cast<i64*>(gain);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(refine_wave_kernel, dim3(grid_for(n, 1)), dim3(64), 0, st, a);
    if (n_heavy > 0) hipLaunchKernelGGL(refine_heavy_kernel, dim3(heavy_grid(n_heavy, scratch_blocks)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_leiden_accept(const int32_t* ref, const int32_t* prop, int64_t n, int32_t* next, int64_t* gain, int64_t* stats,
                                  uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_leiden_accept", what); };
    wgnn::error_clear();
    if (n < 0 || n > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n must be in [0, 2^31)");
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (!ref || !prop || !next || !gain || !stats) return fail(WGNN_ERR_BAD_ARG, "ref, prop, next, gain and stats are required");
    if (!aligned8(gain) || !aligned8(stats)) return fail(WGNN_ERR_ALIGNMENT, "gain and stats must be 8-byte aligned");
    if (!aligned4(ref) || !aligned4(prop) || !aligned4(next)) return fail(WGNN_ERR_ALIGNMENT, "ref, prop and next must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(stats, 0, sizeof(int64_t), st) != hipSuccess) return fail(WGNN_ERR_LAUNCH, "hipMemsetAsync failed");
    if (n == 0) return WGNN_OK;
    CArgs a{ref, prop, (long)n, next, reinterpret_cast<i64*>(gain), reinterpret_cast<u64*>(stats)};
    hipLaunchKernelGGL(accept_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}
