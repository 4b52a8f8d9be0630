// wgnn_markers.hip - wgnn_group_gene_reduce: per-group, per-gene sums of attribution scores (api.ResidentPredictor.markers).
//
//   sum[k, g] = sum over the cells i of group k that list gene g of score[i, g]   (fp64)        count[k, g] = how many
//
// The operand is the batch's GENE-MAJOR copy (t_rowptr [G + 1], cell ids ascending inside a gene, the f32 scores in that order -
// what wgnn_csr_transpose_count / _fill make of explain's scores), so a gene's terms are one contiguous run and an output
// column [., g] has ONE owner: a wavefront.  Lane i takes entries i, i + 64, ... of the run (ascending), looks up group[cell] and
// adds into a bin of its own: LDS holds, per wave, P groups x 64 lanes of fp64 sums and int32 counts, group-major and
// lane-minor - a lane only ever touches column `lane` (no barrier, no atomic, race-free by construction), and the 64 lanes of
// one ds access touch 64 different 8-byte words (ds_read_b64 / ds_write_b64 bank = (addr / 4) mod 64 per 32-lane half: 2 * lane,
// conflict-free whatever the groups are).  At the end of the run every group's 64 lane bins are folded by an xor butterfly -
// a fixed tree, a + b is commutative bit for bit, so every lane ends with the same sum - and lane k % 64 keeps group k for one
// store per 64 groups.  The order of a bin's additions depends on the run (CSR structure and `group`) alone: two launches are
// bit-identical.  More groups than fit (64 KiB of LDS per workgroup, 12 bytes per lane and group: 85 per wave) are cut into
// passes over the run, which L2 holds by then.  Up to 4 waves per workgroup while their bins fit.

#include "wgnn_common.h"

namespace {
using namespace wgnn;

constexpr int kMLdsBytes = 64 * 1024;         // bins of one workgroup
constexpr int kMBinBytes = 64 * 12;           // one group's 64 lane bins: fp64 sum + int32 count
constexpr int kMMaxWaves = 4;
constexpr int kMMaxBlocks = 4096;             // grid-stride beyond that
constexpr int kMMaxGroups = 1 << 20;
constexpr int kMAhead = 4;                    // 64-entry chunks in flight per wave

struct MArgs {
    const int* t_rowptr; const int* t_cell; const float* t_score; const int* group;
    long n_rows; int n_groups; int n_genes; int per_pass;
    double* sum; int* count; int accumulate;
};

__global__ void __launch_bounds__(64 * kMMaxWaves) group_gene_reduce_kernel(const MArgs a) {
    extern __shared__ double s_bins[];            // [waves][per_pass][64] fp64, then [waves][per_pass][64] int32
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int P = a.per_pass;
    double* bs = s_bins + (size_t)wave * P * 64 + lane;
    int* bc = reinterpret_cast<int*>(s_bins + (size_t)waves * P * 64) + (size_t)wave * P * 64 + lane;
    const long stride = (long)gridDim.x * waves;
    for (long g = (long)blockIdx.x * waves + wave; g < a.n_genes; g += stride) {      // wave-uniform
        const int b = a.t_rowptr[g], e = a.t_rowptr[g + 1];
        for (int k0 = 0; k0 < a.n_groups; k0 += P) {
            const int np = min(P, a.n_groups - k0);
            for (int i = 0; i < np; ++i) { bs[i * 64] = 0.0; bc[i * 64] = 0; }
            for (int j0 = b; j0 < e; j0 += 64 * kMAhead) {
                int cell[kMAhead], grp[kMAhead];
                float sc[kMAhead];
#pragma unroll
                for (int u = 0; u < kMAhead; ++u) {
                    const long j = (long)j0 + u * 64 + lane;
                    const bool on = j < e;
                    cell[u] = on ? a.t_cell[j] : -1;
                    sc[u] = on ? a.t_score[j] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < kMAhead; ++u)     // a cell id outside the batch takes no part (the wrapper checks; no fault)
                    grp[u] = (unsigned)cell[u] < (unsigned long)a.n_rows ? a.group[cell[u]] : -1;
#pragma unroll
                for (int u = 0; u < kMAhead; ++u) {   // group -1 (or one beyond n_groups) takes no part
                    const unsigned r = (unsigned)(grp[u] - k0);
                    if (grp[u] >= 0 && r < (unsigned)np) {
                        bs[r * 64] += (double)sc[u];
                        bc[r * 64] += 1;
                    }
                }
            }
            // fold the 64 lane bins of every group; lane k % 64 keeps group k, one store per 64 groups
            for (int i0 = 0; i0 < np; i0 += 64) {
                double my_s = 0.0; int my_c = 0;
                const int n = min(64, np - i0);
                for (int i = 0; i < n; ++i) {
                    double s = bs[(i0 + i) * 64];
                    int c = bc[(i0 + i) * 64];
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
                        s += __shfl_xor(s, off, 64);
                        c += __shfl_xor(c, off, 64);
                    }
                    if (lane == i) { my_s = s; my_c = c; }
                }
                if (lane < n) {
                    const size_t o = (size_t)(k0 + i0 + lane) * a.n_genes + g;
                    if (a.accumulate) { my_s += a.sum[o]; my_c += a.count[o]; }
                    a.sum[o] = my_s;
                    a.count[o] = my_c;
                }
            }
        }
    }
}

// groups per pass and waves per workgroup for n_groups: even passes, as many waves (<= 4) as their bins leave room for
void geometry(int n_groups, int* per_pass, int* waves) {
    const int fit = kMLdsBytes / kMBinBytes;                  // 85 groups per wave and pass at most
    const int passes = (n_groups + fit - 1) / fit;
    *per_pass = (n_groups + passes - 1) / passes;
    const int w = fit / *per_pass;
    *waves = w < 1 ? 1 : (w > kMMaxWaves ? kMMaxWaves : w);
}

}  // namespace

extern "C" int wgnn_group_gene_reduce_workspace(int64_t n_rows, int64_t nnz, int32_t n_groups, int32_t n_genes, int64_t* bytes) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_group_gene_reduce_workspace", what); };
    wgnn::error_clear();
    if (!bytes) return fail(WGNN_ERR_BAD_ARG, "bytes is required");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [0, 2^31)");
    if (nnz < 0 || nnz > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "nnz must be in [0, 2^31)");
    if (n_groups <= 0) return fail(WGNN_ERR_BAD_ARG, "n_groups must be positive");
    if (n_genes <= 0) return fail(WGNN_ERR_BAD_ARG, "n_genes must be positive");
    if (n_groups > kMMaxGroups) return fail(WGNN_ERR_UNSUPPORTED, "n_groups > 2^20 is not built");
    *bytes = 0;                                   // every partial sum lives in LDS
    return WGNN_OK;
}

extern "C" int wgnn_group_gene_reduce(const int32_t* t_rowptr, const int32_t* t_cell, const float* t_score, const int32_t* group,
                                      int64_t n_rows, int32_t n_groups, int32_t n_genes, double* sum, int32_t* count,
                                      void* workspace, int64_t workspace_bytes, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_group_gene_reduce", what); };
    wgnn::error_clear();
    (void)workspace;
    if (!sum || !count) return fail(WGNN_ERR_BAD_ARG, "sum and count are required");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [0, 2^31)");
    if (n_groups <= 0) return fail(WGNN_ERR_BAD_ARG, "n_groups must be positive");
    if (n_genes <= 0) return fail(WGNN_ERR_BAD_ARG, "n_genes must be positive");
    if (n_groups > kMMaxGroups) return fail(WGNN_ERR_UNSUPPORTED, "n_groups > 2^20 is not built");
    if (workspace_bytes < 0) return fail(WGNN_ERR_WORKSPACE, "workspace_bytes is negative");
    if (flags & ~(uint32_t)WGNN_MARKERS_ACCUMULATE) return fail(WGNN_ERR_BAD_ARG, "only WGNN_MARKERS_ACCUMULATE is a valid flag");
    if (!t_rowptr) return fail(WGNN_ERR_BAD_ARG, "t_rowptr is required");
    if (n_rows > 0 && (!t_cell || !t_score || !group))
        return fail(WGNN_ERR_BAD_ARG, "t_cell, t_score and group are required for a batch with cells");
    if (!aligned8(sum)) return fail(WGNN_ERR_ALIGNMENT, "sum must be 8-byte aligned");
    MArgs a{};
    a.t_rowptr = t_rowptr; a.t_cell = t_cell; a.t_score = t_score; a.group = group;
    a.n_rows = n_rows; a.n_groups = n_groups; a.n_genes = n_genes;
    a.sum = sum; a.count = count; a.accumulate = (flags & WGNN_MARKERS_ACCUMULATE) ? 1 : 0;
    int waves;
    geometry(n_groups, &a.per_pass, &waves);
    const long want = ((long)n_genes + waves - 1) / waves;
    const unsigned nb = (unsigned)(want < kMMaxBlocks ? want : kMMaxBlocks);
    const size_t lds = (size_t)waves * a.per_pass * kMBinBytes;
    hipLaunchKernelGGL(group_gene_reduce_kernel, dim3(nb), dim3(64 * waves), lds, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}
