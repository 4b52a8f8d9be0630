// wgnn_louvain.hip - graph clusters in integers (include/wgnn.h has the contracts): the shared-neighbour weights of a kNN union
// graph and the three kernels of a synchronous Louvain sweep.  Every value is an int32 / int64, every decision a comparison of
// 64-bit integers: the order of the atomic additions below changes no bit, and neither does the grid.
//
// wgnn_snn_weights: a wavefront per row i, a lane per entry of i's neighbour list (k <= 64).  For every stored neighbour j of the
// union graph the lanes load j's list and count the distinct entries of N+(i) = {i} + list(i) that are in N+(j).
//
// wgnn_louvain_sweep: every vertex reads the state before the sweep (comm, tot, size) and leaves the community it moves to and
// its gain.  kin[C], the weight from v into community C, is collected in a table keyed by the community id by the kin sweep of
// wgnn_graph.h - its three routes by row length, its tables and its scratch are there, shared with wgnn_leiden.hip; here is only
// the policy: the key, the score and what is written.
//
// wgnn_louvain_apply: tot / size of an assignment by 64-bit integer atomics, and how many vertices moved.
// wgnn_louvain_modularity: IN (the stored weight inside communities, the diagonal included) and sum tot^2, and the checks of the
// CSR that need the entries (status bits).
#include "wgnn_graph.h"

namespace {
using namespace wgnn;
using namespace wgnn::graph;

constexpr int kSnnMaxK = 64;

// ---------------------------------------------------------------------------------------------------------------------------
struct GArgs {
    const void* idx; int idx64; long ld; long n; int k;
    const i64* rowptr; const int* col; long nnz; int* w;
};

// entry t of row i's list: -1 for none, an id outside [0, n), or the row itself
__device__ __forceinline__ int list_at(const GArgs& a, long i, int t) {
    const i64 v = a.idx64 ? reinterpret_cast<const i64*>(a.idx)[i * a.ld + t] : (i64)reinterpret_cast<const int*>(a.idx)[i * a.ld + t];
    return (v < 0 || v >= a.n || v == i) ? -1 : (int)v;
}

__global__ void __launch_bounds__(256) snn_weights_kernel(const GArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long i = (long)blockIdx.x * 4 + wave; i < a.n; i += (long)gridDim.x * 4) {          // wave-uniform
        int mine = lane < a.k ? list_at(a, i, lane) : -1;
        bool again = false;                                                                   // an entry listed before: counted once
        for (int s = 0; s < a.k; ++s) {
            const int v = __shfl(mine, s, 64);
            again |= s < lane && v == mine;
        }
        if (again) mine = -1;
        const i64 e0 = clampl(a.rowptr[i], a.nnz), e1 = clampl(a.rowptr[i + 1], a.nnz);
        for (i64 e = e0; e < e1; ++e) {
            const int j = a.col[e];
            int count = 0;
            if ((unsigned)j < (unsigned long)a.n) {
                const int theirs = lane < a.k ? list_at(a, j, lane) : -1;
                bool hit = mine == j;                                                         // j is in N+(j)
                for (int s = 0; s < a.k; ++s) hit |= __shfl(theirs, s, 64) == mine;
                hit &= mine >= 0;
                count = __popcll(__ballot(hit)) + (__ballot(theirs == (int)i) ? 1 : 0);      // ... and i itself when j lists it
            }
            if (lane == 0) a.w[e] = count;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
struct LArgs {
    KinGraph g;
    const int* comm; const i64* deg; const i64* tot; const int* size;
    i64 mden; i64 num; int odd;
    int* next; i64* gain;
};

// the sweep's policy for the kin sweep (wgnn_graph.h): the key of a neighbour is its community
struct Move {
    typedef LArgs Args;
    struct Vertex { int own; int size_own; i64 degv; i64 score_own; };

    // v's own community; a comm[v] that is no id stays and is reported.  The same in every thread of the workgroup.
    static __device__ __forceinline__ bool enter(const LArgs& a, long v, Vertex& x) {
        x.own = a.comm[v];
        if (!is_id(x.own, a.g.n)) {
            if ((threadIdx.x & 63) == 0) atomicOr(&a.g.stats[3], (u64)WGNN_LOUVAIN_BAD_LABEL);
            return false;
        }
        x.size_own = a.size[x.own]; x.degv = a.deg[v];
        return true;
    }
    // the community of neighbour u of v for kin: -1 for the diagonal, for a column or a community id outside [0, n)
    static __device__ __forceinline__ int key(const LArgs& a, const Vertex&, long v, int u) {
        if (u == v || !is_id(u, a.g.n)) return -1;
        const int C = a.comm[u];
        return is_id(C, a.g.n) ? C : -1;
    }
    static constexpr bool kOwnKin = true;                      // staying has a score of its own
    static __device__ __forceinline__ int own(const Vertex& x) { return x.own; }
    static __device__ __forceinline__ void own_kin(const LArgs& a, Vertex& x, i64 kin) {
        x.score_own = kin * a.mden - a.num * x.degv * (a.tot[x.own] - x.degv);
    }
    // community C with kin[C] = kin against the best so far: the gate, the singleton rule, a score above the own one; then the
    // total order (higher score, lower id).  Seeing a community twice changes nothing.
    static __device__ __forceinline__ void consider(Best& b, const LArgs& a, const Vertex& x, int C, i64 kin) {
        if (C == x.own || (a.odd ? C < x.own : C > x.own) || !is_id(C, a.g.n)) return;
        if (x.size_own == 1 && C > x.own && a.size[C] == 1) return;
        const i64 s = kin * a.mden - a.num * x.degv * a.tot[C];
        if (s <= x.score_own) return;
        if (b.c < 0 || s > b.score || (s == b.score && C < b.c)) { b.score = s; b.c = C; }
    }
    static __device__ __forceinline__ void write(const LArgs& a, long v, const Vertex& x, const Best& b) {
        a.next[v] = b.c >= 0 ? b.c : a.comm[v];               // stays where it is
        a.gain[v] = b.c >= 0 ? b.score - x.score_own : 0;
    }
};

__global__ void __launch_bounds__(64) sweep_wave_kernel(const LArgs a) { kin_sweep_wave<Move>(a); }
__global__ void __launch_bounds__(256) sweep_heavy_kernel(const LArgs a) { kin_sweep_heavy<Move>(a); }

// ---------------------------------------------------------------------------------------------------------------------------
struct AArgs { const int* old_label; const int* label; const i64* deg; long n; u64* tot; int* size; u64* stats; };

__global__ void __launch_bounds__(256) apply_kernel(const AArgs a) {
    __shared__ i64 s_red[4];
    i64 moved = 0;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < a.n; v += (long)gridDim.x * 256) {
        const int c = a.label[v];
        if ((unsigned long)(unsigned)c >= (unsigned long)a.n) { atomicOr(&a.stats[3], (u64)WGNN_LOUVAIN_BAD_LABEL); continue; }
        atomicAdd(&a.tot[c], (u64)a.deg[v]);
        atomicAdd(&a.size[c], 1);
        if (a.old_label) moved += a.old_label[v] != c;
    }
    moved = block_sum(moved, s_red);
    if (threadIdx.x == 0 && moved) atomicAdd(&a.stats[0], (u64)moved);
}

struct MArgs { const i64* rowptr; const int* col; const int* w; long n; long nnz; const int* label; const i64* tot; u64* stats; };

// a wavefront per row: the weight of the entries whose two ends share a label, and the row's checks
__global__ void __launch_bounds__(256) inside_kernel(const MArgs a) {
    __shared__ i64 s_red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    i64 inside = 0;
    unsigned bad = 0;
    for (long v = (long)blockIdx.x * 4 + wave; v < a.n; v += (long)gridDim.x * 4) {
        const i64 r0 = a.rowptr[v], r1 = a.rowptr[v + 1];
        if (r0 < 0 || r1 < r0 || r1 > a.nnz || (v == 0 && r0 != 0) || (v == a.n - 1 && r1 != a.nnz)) bad |= WGNN_LOUVAIN_BAD_ROWPTR;
        const i64 e0 = clampl(r0, a.nnz), e1 = clampl(r1, a.nnz);
        const int mine = a.label[v];
        for (i64 e = e0 + lane; e < e1; e += 64) {
            const int u = a.col[e];
            if ((unsigned long)(unsigned)u >= (unsigned long)a.n) { bad |= WGNN_LOUVAIN_BAD_COL; continue; }
            if (e > e0 && a.col[e - 1] >= u) bad |= WGNN_LOUVAIN_UNSORTED;
            if (a.w[e] < 0) bad |= WGNN_LOUVAIN_BAD_WEIGHT;
            if (a.label[u] == mine) inside += a.w[e];
        }
    }
    if (bad) atomicOr(&a.stats[3], (u64)bad);
    inside = block_sum(inside, s_red);
    if (threadIdx.x == 0 && inside) atomicAdd(&a.stats[1], (u64)inside);
}

__global__ void __launch_bounds__(256) tot2_kernel(const MArgs a) {
    __shared__ i64 s_red[4];
    i64 sum = 0;
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < a.n; c += (long)gridDim.x * 256) sum += a.tot[c] * a.tot[c];
    sum = block_sum(sum, s_red);
    if (threadIdx.x == 0 && sum) atomicAdd(&a.stats[2], (u64)sum);
}

}  // namespace

extern "C" int wgnn_snn_weights(const void* idx, int64_t ld_idx, int64_t n, int32_t k, const int64_t* rowptr, const int32_t* col,
                                int64_t nnz, int32_t* w, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_snn_weights", what); };
    wgnn::error_clear();
    if (const char* what = check_graph_sizes(n, nnz)) return fail(WGNN_ERR_BAD_ARG, what);
    if (flags & ~(uint32_t)WGNN_SNN_IDX_I64) return fail(WGNN_ERR_BAD_ARG, "unknown flag (valid: WGNN_SNN_IDX_I64)");
    if (k < 1 || k > kSnnMaxK) return fail(WGNN_ERR_UNSUPPORTED, "k must be in [1, 64]");
    if (ld_idx < k) return fail(WGNN_ERR_BAD_ARG, "ld_idx < k");
    if (!idx || !rowptr || !col || !w) return fail(WGNN_ERR_BAD_ARG, "idx, rowptr, col and w are required");
    if (!aligned8(rowptr) || ((flags & WGNN_SNN_IDX_I64) && !aligned8(idx)))
        return fail(WGNN_ERR_ALIGNMENT, "rowptr and an int64 idx must be 8-byte aligned");
    if (!aligned4(idx) || !aligned4(col) || !aligned4(w)) return fail(WGNN_ERR_ALIGNMENT, "idx, col and w must be 4-byte aligned");
    if (n == 0 || nnz == 0) return WGNN_OK;
    GArgs a{};
    a.idx = idx; a.idx64 = (flags & WGNN_SNN_IDX_I64) ? 1 : 0; a.ld = ld_idx; a.n = n; a.k = k;
    a.rowptr = reinterpret_cast<const i64*>(rowptr); a.col = col; a.nnz = nnz; a.w = w;
    hipLaunchKernelGGL(snn_weights_kernel, dim3(grid_for(n, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_louvain_sweep_workspace_bytes(int64_t n, int32_t scratch_blocks, int64_t* bytes) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_louvain_sweep_workspace_bytes", what); };
    wgnn::error_clear();
    if (!bytes) return fail(WGNN_ERR_BAD_ARG, "bytes is required");
    if (n < 0 || n > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n must be in [0, 2^31)");
    if (scratch_blocks < 0 || scratch_blocks > kMaxScratchBlocks) return fail(WGNN_ERR_BAD_ARG, "scratch_blocks must be in [0, 256]");
    *bytes = scratch_bytes(n, scratch_blocks);
    return WGNN_OK;
}

extern "C" int wgnn_louvain_sweep(const int64_t* rowptr, const int32_t* col, const int32_t* w, int64_t n, int64_t nnz,
                                  const int32_t* comm, const int64_t* deg, const int64_t* tot, const int32_t* size,
                                  int64_t m_den, int64_t num, int32_t sweep, const int32_t* heavy, int32_t n_heavy,
                                  int32_t wave_rows, int32_t block_rows, int32_t* next, int64_t* gain, int64_t* stats,
                                  void* workspace, int64_t workspace_bytes, int32_t scratch_blocks, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_louvain_sweep", what); };
    wgnn::error_clear();
    if (const char* what = check_graph_sizes(n, nnz)) return fail(WGNN_ERR_BAD_ARG, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (!rowptr || !col || !w || !comm || !deg || !tot || !size || !next || !gain || !stats)
        return fail(WGNN_ERR_BAD_ARG, "rowptr, col, w, comm, deg, tot, size, next, gain and stats are required");
    if (m_den < 1 || num < 1) return fail(WGNN_ERR_BAD_ARG, "m_den and num must be positive");
    if (sweep < 0) return fail(WGNN_ERR_BAD_ARG, "sweep must not be negative");
    if (const Refusal r = check_routes(heavy, n_heavy, wave_rows, block_rows, scratch_blocks); r.code) return fail(r.code, r.what);
    if (!aligned8(rowptr) || !aligned8(deg) || !aligned8(tot) || !aligned8(gain) || !aligned8(stats))
        return fail(WGNN_ERR_ALIGNMENT, "rowptr, deg, tot, gain and stats must be 8-byte aligned");
    if (!aligned4(col) || !aligned4(w) || !aligned4(comm) || !aligned4(size) || !aligned4(next) || !aligned4(heavy))
        return fail(WGNN_ERR_ALIGNMENT, "col, w, comm, size, next and heavy must be 4-byte aligned");
    if (const Refusal r = check_scratch(n, workspace, workspace_bytes, scratch_blocks); r.code) return fail(r.code, r.what);
    if (n == 0) return WGNN_OK;

    LArgs a{};
    a.g = kin_graph(rowptr, col, w, n, nnz, heavy, n_heavy, wave_rows, block_rows, workspace, scratch_blocks, stats);
    a.comm = comm; a.deg = reinterpret_cast<const i64*>(deg); a.tot = reinterpret_cast<const i64*>(tot); a.size = size;
    a.mden = m_den; a.num = num; a.odd = sweep & 1;
    a.next = next; a.gain = reinterpret_cast<i64*>(gain);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sweep_wave_kernel, dim3(grid_for(n, 1)), dim3(64), 0, st, a);
    if (n_heavy > 0) hipLaunchKernelGGL(sweep_heavy_kernel, dim3(heavy_grid(n_heavy, scratch_blocks)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_louvain_apply(const int32_t* old_label, const int32_t* label, const int64_t* deg, int64_t n, int64_t* tot,
                                  int32_t* size, int64_t* stats, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_louvain_apply", what); };
    wgnn::error_clear();
    if (n < 0 || n > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n must be in [0, 2^31)");
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (!label || !deg || !tot || !size || !stats) return fail(WGNN_ERR_BAD_ARG, "label, deg, tot, size and stats are required");
    if (!aligned8(deg) || !aligned8(tot) || !aligned8(stats)) return fail(WGNN_ERR_ALIGNMENT, "deg, tot and stats must be 8-byte aligned");
    if (!aligned4(old_label) || !aligned4(label) || !aligned4(size))
        return fail(WGNN_ERR_ALIGNMENT, "old_label, label and size must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(stats, 0, 3 * sizeof(int64_t), st) != hipSuccess) return fail(WGNN_ERR_LAUNCH, "hipMemsetAsync failed");
    if (n == 0) return WGNN_OK;
    if (hipMemsetAsync(tot, 0, (size_t)n * 8, st) != hipSuccess || hipMemsetAsync(size, 0, (size_t)n * 4, st) != hipSuccess)
        return fail(WGNN_ERR_LAUNCH, "hipMemsetAsync failed");
    AArgs a{old_label, label, reinterpret_cast<const i64*>(deg), (long)n, reinterpret_cast<u64*>(tot), size,
            reinterpret_cast<u64*>(stats)};
    hipLaunchKernelGGL(apply_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}

extern "C" int wgnn_louvain_modularity(const int64_t* rowptr, const int32_t* col, const int32_t* w, int64_t n, int64_t nnz,
                                       const int32_t* label, const int64_t* tot, int64_t* stats, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_louvain_modularity", what); };
    wgnn::error_clear();
    if (const char* what = check_graph_sizes(n, nnz)) return fail(WGNN_ERR_BAD_ARG, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (!rowptr || !col || !w || !label || !tot || !stats) return fail(WGNN_ERR_BAD_ARG, "rowptr, col, w, label, tot and stats are required");
    if (!aligned8(rowptr) || !aligned8(tot) || !aligned8(stats)) return fail(WGNN_ERR_ALIGNMENT, "rowptr, tot and stats must be 8-byte aligned");
    if (!aligned4(col) || !aligned4(w) || !aligned4(label)) return fail(WGNN_ERR_ALIGNMENT, "col, w and label must be 4-byte aligned");
    if (n == 0) return WGNN_OK;
    MArgs a{reinterpret_cast<const i64*>(rowptr), col, w, (long)n, (long)nnz, label, reinterpret_cast<const i64*>(tot),
            reinterpret_cast<u64*>(stats)};
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(inside_kernel, dim3(grid_for(n, 4)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(tot2_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}
