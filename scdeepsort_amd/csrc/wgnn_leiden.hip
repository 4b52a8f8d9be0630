// wgnn_leiden.hip - the refinement of a deterministic, synchronous, integer Leiden (include/wgnn.h has the contract).  P is the
// partition the moving phase left, ref the refined one inside it: a refined community carries the id of the vertex that founded it, only a vertex
// that is alone moves, and a move is accepted only when the founder of its target stays, so that every refined community stays
// connected.
//
// wgnn_leiden_boundary: a wavefront per row; kinP[v] by a wavefront sum, ext[ref[v]] by one 64-bit atomic per row.
// wgnn_leiden_refine_sweep: wgnn_louvain_sweep's tables and its three routes by row length, keyed by the refined id of the
//   neighbours in v's own P-community.  A vertex that may not move leaves before its row is read.
// wgnn_leiden_accept: a thread per vertex.
#include "wgnn_graph_tables.h"

namespace {
using namespace wgnn;
using namespace wgnn::graph;

struct RArgs {
    const i64* rowptr; const int* col; const int* w; long n; long nnz;
    const int* P; const int* ref; const i64* deg; const i64* totP; const i64* tot; const int* size;
    const i64* ext; const i64* kinP;
    i64 mden; i64 num; int odd;
    const int* heavy; int n_heavy; int wave_rows; int block_rows;
    int* prop; i64* gain; u64* stats;
    int* scratch; int scratch_blocks;
};

__device__ __forceinline__ bool is_id(int x, long n) { return (unsigned long)(unsigned)x < (unsigned long)n; }

// ref[v] and P[v] are ids and the founder of ref[v] lies in P[v]
__device__ __forceinline__ bool part_ok(const int* P, const int* ref, long n, long v) {
    const int own = ref[v], Pv = P[v];
    return is_id(own, n) && is_id(Pv, n) && P[own] == Pv;
}

struct Mover { int own; int Pv; i64 degv; i64 totPv; };

// may v move?  Alone in its refined community and well connected to its P-community.  The same for every thread of a workgroup.
__device__ __forceinline__ bool mover(const RArgs& a, long v, Mover& m) {
    if (!part_ok(a.P, a.ref, a.n, v)) {
        if ((threadIdx.x & 63) == 0) atomicOr(&a.stats[3], (u64)WGNN_LEIDEN_BAD_PARTITION);
        return false;
    }
    m.own = a.ref[v]; m.Pv = a.P[v]; m.degv = a.deg[v]; m.totPv = a.totP[m.Pv];
    return a.size[m.own] == 1 && a.kinP[v] * a.mden >= a.num * m.degv * (m.totPv - m.degv);
}

// the refined community of neighbour u of v for kin: -1 for the diagonal, another P-community, or an id outside [0, n)
__device__ __forceinline__ int kin_ref(const RArgs& a, long v, int Pv, int u) {
    if (u == v || !is_id(u, a.n) || a.P[u] != Pv) return -1;
    const int S = a.ref[u];
    return is_id(S, a.n) ? S : -1;
}

// refined community S with kin[S] = kin against the best so far: the gate, S's own well-connectedness, a score above 0; then the
// total order (higher score, lower id)
__device__ __forceinline__ void consider_ref(Best& b, const RArgs& a, int S, i64 kin, const Mover& m) {
    if (S == m.own || (a.odd ? S < m.own : S > m.own) || !is_id(S, a.n)) return;
    const i64 ts = a.tot[S];
    if (a.ext[S] * a.mden < a.num * ts * (m.totPv - ts)) return;
    const i64 s = kin * a.mden - a.num * m.degv * ts;
    if (s <= 0) return;
    if (b.c < 0 || s > b.score || (s == b.score && S < b.c)) { b.score = s; b.c = S; }
}

template <int THREADS, int SLOTS>
__device__ __forceinline__ Best refine_in_lds(const RArgs& a, long v, i64 e0, i64 e1, const Mover& m, int* keys, int* vals) {
    const int tid = threadIdx.x;
    for (int s = tid; s < SLOTS; s += THREADS) { keys[s] = -1; vals[s] = 0; }
    __syncthreads();
    for (i64 e = e0 + tid; e < e1; e += THREADS) {
        const int S = kin_ref(a, v, m.Pv, a.col[e]);
        if (S >= 0) table_add<SLOTS>(keys, vals, S, a.w[e]);
    }
    __syncthreads();
    Best b{0, -1};
    for (int s = tid; s < SLOTS; s += THREADS)
        if (keys[s] >= 0) consider_ref(b, a, keys[s], (i64)vals[s], m);
    __syncthreads();                                           // the table is free for the next vertex
    return b;
}

__device__ __forceinline__ void propose(const RArgs& a, long v, const Best& b) {
    a.prop[v] = b.c >= 0 ? b.c : a.ref[v];
    a.gain[v] = b.c >= 0 ? b.score : 0;
}

__global__ void __launch_bounds__(64) refine_wave_kernel(const RArgs a) {
    __shared__ int keys[kWaveSlots];
    __shared__ int vals[kWaveSlots];
    for (long v = blockIdx.x; v < a.n; v += gridDim.x) {
        const i64 e0 = clampl(a.rowptr[v], a.nnz), e1 = clampl(a.rowptr[v + 1], a.nnz);
        if (e1 - e0 > a.wave_rows) continue;                  // the heavy kernel's
        Mover m;
        Best b{0, -1};
        if (e1 > e0 && mover(a, v, m)) {
            b = refine_in_lds<64, kWaveSlots>(a, v, e0, e1, m, keys, vals);
            wave_best(b);
        }
        if (threadIdx.x == 0) propose(a, v, b);
    }
}

__global__ void __launch_bounds__(256) refine_heavy_kernel(const RArgs a) {
    __shared__ int keys[kBlockSlots];
    __shared__ int vals[kBlockSlots];
    __shared__ i64 s_score[4];
    __shared__ int s_c[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int h = blockIdx.x; h < a.n_heavy; h += gridDim.x) {
        const long v = a.heavy[h];
        if (v < 0 || v >= a.n) continue;
        const i64 e0 = clampl(a.rowptr[v], a.nnz), e1 = clampl(a.rowptr[v + 1], a.nnz);
        Mover m;
        Best b{0, -1};
        if (!mover(a, v, m)) {
            // stays
        } else if (e1 - e0 <= a.block_rows) {
            b = refine_in_lds<256, kBlockSlots>(a, v, e0, e1, m, keys, vals);
        } else if (a.scratch && (int)blockIdx.x < a.scratch_blocks) {
            int* kin = a.scratch + (size_t)blockIdx.x * a.n;
            for (i64 e = e0 + tid; e < e1; e += 256) {
                const int S = kin_ref(a, v, m.Pv, a.col[e]);
                if (S >= 0) atomicAdd(&kin[S], a.w[e]);
            }
            __syncthreads();
            for (i64 e = e0 + tid; e < e1; e += 256) {         // the sums were made by atomics: read them where those ran
                const int S = kin_ref(a, v, m.Pv, a.col[e]);
                if (S >= 0) consider_ref(b, a, S, (i64)__hip_atomic_load(&kin[S], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), m);
            }
            __syncthreads();
            for (i64 e = e0 + tid; e < e1; e += 256) {         // zero again, for the next long row and the next sweep
                const int S = kin_ref(a, v, m.Pv, a.col[e]);
                if (S >= 0) __hip_atomic_store(&kin[S], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
        } else {                                               // a long row and no scratch: the caller sized the workspace wrong
            if (tid == 0) atomicOr(&a.stats[3], (u64)WGNN_LOUVAIN_NO_SCRATCH);
        }
        wave_best(b);
        if (lane == 0) { s_score[wave] = b.score; s_c[wave] = b.c; }
        __syncthreads();
        if (tid == 0) {
            Best all{0, -1};
            for (int i = 0; i < 4; ++i) merge(all, s_score[i], s_c[i]);
            propose(a, v, all);
        }
        __syncthreads();
    }
}

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
    if (n_heavy < 0 || (n_heavy > 0 && !heavy)) return fail(WGNN_ERR_BAD_ARG, "n_heavy is negative, or heavy is missing");
    if (wave_rows < 0 || wave_rows > kWaveRows) return fail(WGNN_ERR_UNSUPPORTED, "wave_rows must be in [0, 128]");
    if (block_rows < 0 || block_rows > kBlockRows) return fail(WGNN_ERR_UNSUPPORTED, "block_rows must be in [0, 2048]");
    if (scratch_blocks < 0 || scratch_blocks > kMaxScratchBlocks) return fail(WGNN_ERR_BAD_ARG, "scratch_blocks must be in [0, 256]");
    if (!aligned8(rowptr) || !aligned8(deg) || !aligned8(totP) || !aligned8(tot) || !aligned8(ext) || !aligned8(kinP) || !aligned8(gain) ||
        !aligned8(stats))
        return fail(WGNN_ERR_ALIGNMENT, "rowptr, deg, totP, tot, ext, kinP, gain and stats must be 8-byte aligned");
    if (!aligned4(col) || !aligned4(w) || !aligned4(P) || !aligned4(ref) || !aligned4(size) || !aligned4(prop) || !aligned4(heavy))
        return fail(WGNN_ERR_ALIGNMENT, "col, w, P, ref, size, prop and heavy must be 4-byte aligned");
    if (workspace_bytes < 0) return fail(WGNN_ERR_WORKSPACE, "workspace_bytes is negative");
    if (scratch_blocks > 0 && (!workspace || workspace_bytes < scratch_bytes(n, scratch_blocks)))
        return fail(WGNN_ERR_WORKSPACE, "workspace is missing or smaller than wgnn_louvain_sweep_workspace_bytes asks for");
    if (!aligned4(workspace)) return fail(WGNN_ERR_ALIGNMENT, "workspace must be 4-byte aligned");
    if (n == 0) return WGNN_OK;

    RArgs a{};
    a.rowptr = reinterpret_cast<const i64*>(rowptr); a.col = col; a.w = w; a.n = n; a.nnz = nnz;
    a.P = P; a.ref = ref; a.deg = reinterpret_cast<const i64*>(deg); a.totP = reinterpret_cast<const i64*>(totP);
    a.tot = reinterpret_cast<const i64*>(tot); a.size = size;
    a.ext = reinterpret_cast<const i64*>(ext); a.kinP = reinterpret_cast<const i64*>(kinP);
    a.mden = m_den; a.num = num; a.odd = sweep & 1;
    a.heavy = heavy; a.n_heavy = n_heavy; a.wave_rows = wave_rows; a.block_rows = block_rows;
    a.prop = prop; a.gain = reinterpret_cast<i64*>(gain); a.stats = reinterpret_cast<u64*>(stats);
    a.scratch = scratch_blocks > 0 ? static_cast<int*>(workspace) : nullptr; a.scratch_blocks = scratch_blocks;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(refine_wave_kernel, dim3(grid_for(n, 1)), dim3(64), 0, st, a);
    if (n_heavy > 0) {
        const unsigned blocks = scratch_blocks > 0 ? (unsigned)(n_heavy < scratch_blocks ? n_heavy : scratch_blocks) : grid_for(n_heavy, 1);
        hipLaunchKernelGGL(refine_heavy_kernel, dim3(blocks), dim3(256), 0, st, a);
    }
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
