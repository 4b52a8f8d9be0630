// wgnn_rank_genes.hip - wgnn_rank_genes_groups: the integer part of a Wilcoxon rank-sum (Mann-Whitney) test of every gene, each
// group of cells against the rest (api.ResidentPredictor.rank_genes).  The contract is the rank-genes block of include/wgnn.h; for
// one gene g with its n_g participating stored entries and z = N - n_g implicit zeros (N = the participating cells):
//
//   key_i  = rank_key(val_i), the order-preserving integer of wgnn_signatures.hip; key0 = rank_key(+0.0f)
//   R2_j   = 2 * #{less} + #{equal, j included} + 1 over ALL N values      twice the tie-averaged rank, rank 1 = the lowest value
//   R2_0   = 2 * #{stored below key0} + t0 + 1,  t0 = z + #{stored equal to key0}              the doubled rank of an implicit zero
//   rank2_sum[k, g] = sum of R2 over the cells of group k, (N_k - count[k, g]) implicit zeros included;  count[k, g] = the stored
//   tie_sum[g] = sum over tie groups of t^3 - t = sum over the N values of eq^2 - 1
//
// Why counting.  A rank is needed of every stored entry, along the CELL axis, and a gene's run is as long as the batch has cells.
// Counting "less" and "equal" against every key of the gene gives the doubled mid-rank exactly, as an integer, without moving a
// key: no sort network, no scatter, nothing whose result could depend on an order.  It costs sum_g n_g^2 compares.
//
// Layout.  A work unit is (gene, block of 512 stored entries of that gene); the units are numbered gene by gene by a scan of
// ceil(stored / 512) (rank_genes_scan, one workgroup) and walked grid-stride, a unit finds its gene by bisection of that scan.
//   1   LANE j OWNS entry j of the block: its key, and group[t_cell[j]].
//   2   the gene's keys are streamed through an LDS slab, min(n_rows rounded up to 4, 16 384) keys at a time (64 KiB at most;
//       with the 12 KiB of bins below two workgroups share a CU's 160 KiB).
//   3   every lane walks the staged chunk - the same 16-byte address in all lanes, one broadcast ds_read_b128 per four keys -
//       counting lt and eq in its own registers.  There is no cross-lane reduction per entry.
//   4   the implicit zeros join by arithmetic (z more "less" above key0, z more "equal" at key0), then R2_j and eq_j^2 - 1 are
//       known per lane.  The block's R2 and entry counts meet in LDS bins, one per group (integer LDS atomics, 1 024 groups per
//       pass, more groups = more passes), and a non-empty bin leaves with one 64-bit global atomic add; eq^2 - 1 is folded per
//       wave and leaves with one add per wave.  Integer addition commutes: the bits do not depend on the order, two launches are
//       bit-identical, and neither grid nor chunking shows in the result.
// Why the owner split.  One owner per gene would leave the few genes almost every cell expresses - n_g^2 = 10^10 compares at
// 100 000 cells - to one workgroup each, while the rest of the device idles.  Blocks of 512 owners make those genes many units
// (each streams the whole gene once; the keys come from L2 by then), so the compares spread over every CU.
//
// rank_genes_prep clears the outputs (the caller does not) and, one wave per gene, counts n_g and the stored entries below and at
// key0; rank_genes_finish adds the implicit zeros' (N_k - count) * R2_0 to rank2_sum and their z * (t0^2 - 1) to tie_sum, so the
// export returns complete tables.
//
// Stray entries.  An entry whose cell id is outside [0, n_rows) or whose group is outside [0, n_groups) takes no part.  The API
// never makes one (its transpose drops the cells without a group), so a gene WITHOUT strays - prep knows, n_g == stored - is
// staged by a plain copy.  A gene with one is staged by ballot compaction: a wave reserves its slots in the slab with one LDS
// atomic add and every kept key takes its rank in the ballot; the order of the keys in the slab is then arbitrary, which
// counting does not see.  A stray owner lane counts along and adds nothing.  No id is used as an index before its range check.
//
// Not done: an in-LDS sort.  A gene of at most 16 384 entries fits the slab whole; a bitonic sort there is O(n log^2 n), a
// radix sort O(n), ranks then follow from run boundaries, the same integers.  By operation count (n^2 compares against
// n log^2 n compare-exchanges, each several LDS accesses and a barrier stage) counting stays ahead up to a thousand entries or
// so - most genes of most batches - and loses beyond: the sort would pay for the popular genes, whose n^2 this kernel runs at
// the VALU bound (profiles/resident_rank_genes.md).  An estimate, not a measurement.  Genes beyond the slab would still need
// this kernel, or a merge of sorted chunks.  Not done either: a per-entry group cache in the workspace that
// would spare step 1's and the compaction's gather of group[].
//
// No floating-point arithmetic beyond the key function, vector stores only, plain C++.

#include "wgnn_align_rows.h"             // below
#include "wgnn_build_rows.h"             // raise_lds

namespace {
using namespace wgnn;

constexpr int kGBlock = 512;                  // owners per unit, 8 waves
constexpr int kGMaxBlocks = 4096;             // grid-stride beyond that
constexpr int kGMaxSlab = 16384;              // keys staged per chunk at most: 64 KiB
constexpr int kGBins = 1024;                  // groups per pass of the block reduction: 12 KiB
constexpr int kGMaxGroups = 4096;
constexpr long kGMaxRows = 1L << 20;          // N^3 fits int64
constexpr int kGFixedBytes = kGBins * 8 + kGBins * 4 + 16;
constexpr int kGScanThreads = 1024;
constexpr unsigned kKey0 = 0x80000000u;       // rank_key(+0.0f)

struct GArgs {
    const int* t_rowptr; const int* t_cell; const float* t_val; const int* group; const long long* group_size;
    long n_rows; int n_groups; int n_genes;
    long long* rank2_sum; long ld_sum; int* count; long ld_count; long long* tie_sum;
    long long* n_total;                       // workspace: [1]          N = the sum of group_size
    long long* unit_ptr;                      //            [n_genes + 1] the exclusive scan of the genes' units
    int* info;                                //            [n_genes][4]  n_g, stored below key0, stored equal to key0, unused
    int slab;
};

// wgnn_signatures.hip's key: one total order over every f32 bit pattern, the numeric order on finite values (-0.0 below +0.0)
__device__ __forceinline__ unsigned rank_key(float x) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the group of stored entry j, or -1 when the entry takes no part; no id indexes anything before its range check
__device__ __forceinline__ int entry_group(const GArgs& a, long j) {
    const unsigned cell = (unsigned)a.t_cell[j];
    if (cell >= (unsigned long)a.n_rows) return -1;
    const int k = a.group[cell];
    return (unsigned)k < (unsigned)a.n_groups ? k : -1;
}

__global__ void __launch_bounds__(256) rank_genes_prep(const GArgs a) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    const long cells = (long)a.n_groups * a.n_genes;
    for (long i = tid; i < cells; i += nth) {
        const long k = i / a.n_genes, g = i - k * a.n_genes;
        a.rank2_sum[k * a.ld_sum + g] = 0;
        a.count[k * a.ld_count + g] = 0;
    }
    for (long g = tid; g < a.n_genes; g += nth) a.tie_sum[g] = 0;
    if (a.n_rows == 0) return;                                                 // an empty batch: the tables are complete
    const int lane = threadIdx.x & 63;
    for (long g = tid >> 6; g < a.n_genes; g += nth >> 6) {                    // wave-uniform
        const int b = a.t_rowptr[g], e = a.t_rowptr[g + 1];
        int nv = 0, lt0 = 0, eq0 = 0;
        for (long j0 = b; j0 < e; j0 += 64) {
            const long j = j0 + lane;
            const bool ok = j < e && entry_group(a, j) >= 0;
            const unsigned key = ok ? rank_key(a.t_val[j]) : kKey0 + 1u;
            nv += __popcll(__ballot(ok));
            lt0 += __popcll(__ballot(key < kKey0));
            eq0 += __popcll(__ballot(key == kKey0));
        }
        if (lane == 0) {
            int* o = a.info + g * 4;
            o[0] = nv; o[1] = lt0; o[2] = eq0; o[3] = 0;
        }
    }
}

// one workgroup: N, and the exclusive scan of the genes' unit counts (thread t takes a contiguous run of genes)
__global__ void __launch_bounds__(kGScanThreads) rank_genes_scan(const GArgs a) {
    __shared__ long long s_part[kGScanThreads];
    const int t = threadIdx.x;
    long long n = 0;
    for (int k = t; k < a.n_groups; k += kGScanThreads) n += a.group_size[k];
    s_part[t] = n;
    __syncthreads();
    if (t == 0) {
        long long s = 0;
        for (int i = 0; i < kGScanThreads; ++i) s += s_part[i];
        a.n_total[0] = s;
    }
    __syncthreads();
    const long per = ((long)a.n_genes + kGScanThreads - 1) / kGScanThreads;
    const long g0 = min(per * t, (long)a.n_genes), g1 = min(g0 + per, (long)a.n_genes);
    long long mine = 0;
    for (long g = g0; g < g1; ++g) {
        const long len = (long)a.t_rowptr[g + 1] - a.t_rowptr[g];
        mine += len > 0 ? (len + kGBlock - 1) / kGBlock : 0;
    }
    s_part[t] = mine;
    __syncthreads();
    if (t == 0) {
        long long s = 0;
        for (int i = 0; i < kGScanThreads; ++i) { const long long c = s_part[i]; s_part[i] = s; s += c; }
        a.unit_ptr[a.n_genes] = s;
    }
    __syncthreads();
    long long at = s_part[t];
    for (long g = g0; g < g1; ++g) {
        a.unit_ptr[g] = at;
        const long len = (long)a.t_rowptr[g + 1] - a.t_rowptr[g];
        at += len > 0 ? (len + kGBlock - 1) / kGBlock : 0;
    }
}

__global__ void __launch_bounds__(kGBlock) rank_genes_kernel(const GArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
    unsigned* s_key = reinterpret_cast<unsigned*>(s_mem);                                          // [slab]
    unsigned long long* s_bsum = reinterpret_cast<unsigned long long*>(s_mem + (size_t)a.slab * 4); // [kGBins]; slab % 4 == 0
    int* s_bcnt = reinterpret_cast<int*>(s_bsum + kGBins);                                         // [kGBins]
    int* s_fill = s_bcnt + kGBins;
    const int tid = threadIdx.x, lane = tid & 63;
    const long long N = a.n_total[0];
    const long long total = a.unit_ptr[a.n_genes];

    for (long long u = blockIdx.x; u < total; u += gridDim.x) {                // everything below is block-uniform but tid
        int lo = 0, hi = a.n_genes;                                            // unit_ptr[lo] <= u < unit_ptr[hi]
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (a.unit_ptr[mid] <= u) lo = mid; else hi = mid;
        }
        const int g = lo;
        const long b = a.t_rowptr[g], e = a.t_rowptr[g + 1];                   // e > b: the gene has units
        const int nv = a.info[(long)g * 4];
        const bool clean = nv == e - b;                                        // no stray entry: a plain copy stages the keys

        const long j = b + (u - a.unit_ptr[g]) * kGBlock + tid;                // this lane's entry
        const int grp = j < e ? entry_group(a, j) : -1;
        const bool valid = grp >= 0;
        const unsigned kj = valid ? rank_key(a.t_val[j]) : 0u;
        const bool wave_on = __ballot(valid) != 0ull;
        unsigned lt = 0, eq = 0;

        for (long c0 = b; c0 < e; c0 += a.slab) {
            const long c1 = c0 + a.slab < e ? c0 + a.slab : e;
            __syncthreads();                                                   // the last chunk's (and the last unit's) readers
            int m;
            if (clean) {
                for (long i = c0 + tid; i < c1; i += kGBlock) s_key[i - c0] = rank_key(a.t_val[i]);
                m = (int)(c1 - c0);
                __syncthreads();
            } else {
                if (tid == 0) *s_fill = 0;
                __syncthreads();
                for (long i0 = c0; i0 < c1; i0 += kGBlock) {                   // block-uniform trip count
                    const long i = i0 + tid;
                    const bool ok = i < c1 && entry_group(a, i) >= 0;
                    const unsigned long long km = __ballot(ok);
                    int base = 0;
                    if (lane == 0 && km) base = atomicAdd(s_fill, __popcll(km));
                    base = __shfl(base, 0, 64);
                    if (ok) s_key[base + below(km)] = rank_key(a.t_val[i]);    // < c1 - c0 <= slab kept keys
                }
                __syncthreads();
                m = *s_fill;
            }
            if (wave_on) {                                                     // wave-uniform
                const uint4* k4 = reinterpret_cast<const uint4*>(s_key);
                const int n4 = m >> 2;
#pragma unroll 4
                for (int t = 0; t < n4; ++t) {                                 // one address for the wave: a broadcast 16-byte read
                    const uint4 q = k4[t];
                    lt += (q.x < kj) + (q.y < kj) + (q.z < kj) + (q.w < kj);
                    eq += (q.x == kj) + (q.y == kj) + (q.z == kj) + (q.w == kj);
                }
                for (int t = n4 << 2; t < m; ++t) {
                    const unsigned k = s_key[t];
                    lt += k < kj; eq += k == kj;
                }
            }
        }
        const unsigned long long z = (unsigned long long)(N - nv);            // the implicit zeros
        unsigned long long lt_all = lt, eq_all = eq;
        if (kj > kKey0) lt_all += z; else if (kj == kKey0) eq_all += z;
        const unsigned long long r2 = 2ull * lt_all + eq_all + 1ull;

        unsigned long long tie = valid ? eq_all * eq_all - 1ull : 0ull;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) tie += __shfl_xor(tie, off, 64);
        if (lane == 0 && tie) atomicAdd(reinterpret_cast<unsigned long long*>(a.tie_sum) + g, tie);

        for (int k0 = 0; k0 < a.n_groups; k0 += kGBins) {
            const int np = a.n_groups - k0 < kGBins ? a.n_groups - k0 : kGBins;
            for (int i = tid; i < np; i += kGBlock) { s_bsum[i] = 0ull; s_bcnt[i] = 0; }
            __syncthreads();
            const unsigned r = (unsigned)(grp - k0);
            if (valid && r < (unsigned)np) {
                atomicAdd(&s_bsum[r], r2);
                atomicAdd(&s_bcnt[r], 1);
            }
            __syncthreads();
            for (int i = tid; i < np; i += kGBlock) {                          // the thread that cleared bin i, and clears it next
                const int c = s_bcnt[i];
                if (c) {
                    atomicAdd(reinterpret_cast<unsigned long long*>(a.rank2_sum) + (size_t)(k0 + i) * a.ld_sum + g, s_bsum[i]);
                    atomicAdd(a.count + (size_t)(k0 + i) * a.ld_count + g, c);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(256) rank_genes_finish(const GArgs a) {
    const long nth = (long)gridDim.x * blockDim.x;
    const long cells = (long)a.n_groups * a.n_genes;
    const long long N = a.n_total[0];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += nth) {
        const long k = i / a.n_genes, g = i - k * a.n_genes;
        const int* o = a.info + g * 4;
        const long long z = N - o[0], t0 = z + o[2];
        const long long r2_zero = 2ll * o[1] + t0 + 1ll;
        a.rank2_sum[k * a.ld_sum + g] += (a.group_size[k] - a.count[k * a.ld_count + g]) * r2_zero;
        if (k == 0) a.tie_sum[g] += z * (t0 * t0 - 1ll);
    }
}

LdsMarks g_lds;

int64_t workspace_bytes_for(int32_t n_genes) { return 8 * ((int64_t)n_genes + 2) + 16 * (int64_t)n_genes; }

const char* check_sizes(int64_t n_rows, int32_t n_groups, int32_t n_genes) {
    if (n_rows < 0 || n_rows > kGMaxRows) return "n_rows must be in [0, 2^20] (N^3 must fit int64)";
    if (n_groups < 1 || n_groups > kGMaxGroups) return "n_groups must be in [1, 4096]";
    if (n_genes <= 0) return "n_genes must be positive";
    return nullptr;
}

}  // namespace

extern "C" int wgnn_rank_genes_groups_workspace(int64_t n_rows, int64_t nnz, int32_t n_groups, int32_t n_genes, int64_t* bytes) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_rank_genes_groups_workspace", what); };
    wgnn::error_clear();
    if (!bytes) return fail(WGNN_ERR_BAD_ARG, "bytes is required");
    if (const char* what = check_sizes(n_rows, n_groups, n_genes)) return fail(WGNN_ERR_BAD_ARG, what);
    if (nnz < 0 || nnz > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "nnz must be in [0, 2^31)");
    *bytes = workspace_bytes_for(n_genes);        // N, the unit scan and four counters per gene; nothing per entry
    return WGNN_OK;
}

extern "C" int wgnn_rank_genes_groups(const int32_t* t_rowptr, const int32_t* t_cell, const float* t_val, const int32_t* group,
                                      const int64_t* group_size, int64_t n_rows, int32_t n_groups, int32_t n_genes,
                                      int64_t* rank2_sum, int64_t ld_sum, int32_t* count, int64_t ld_count, int64_t* tie_sum,
                                      void* workspace, int64_t workspace_bytes, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_rank_genes_groups", what); };
    wgnn::error_clear();
    if (!rank2_sum || !count || !tie_sum) return fail(WGNN_ERR_BAD_ARG, "rank2_sum, count and tie_sum are required");
    if (const char* what = check_sizes(n_rows, n_groups, n_genes)) return fail(WGNN_ERR_BAD_ARG, what);
    if (ld_sum < n_genes || ld_count < n_genes) return fail(WGNN_ERR_BAD_ARG, "ld_sum and ld_count must be >= n_genes");
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (!t_rowptr || !group_size) return fail(WGNN_ERR_BAD_ARG, "t_rowptr and group_size are required");
    if (n_rows > 0 && (!t_cell || !t_val || !group))
        return fail(WGNN_ERR_BAD_ARG, "t_cell, t_val and group are required for a batch with cells");
    if (workspace_bytes < 0) return fail(WGNN_ERR_WORKSPACE, "workspace_bytes is negative");
    if (n_rows > 0 && (!workspace || workspace_bytes < workspace_bytes_for(n_genes)))
        return fail(WGNN_ERR_WORKSPACE, "workspace is smaller than wgnn_rank_genes_groups_workspace asks for");
    if (!aligned8(rank2_sum) || !aligned8(tie_sum) || !aligned8(group_size) || !aligned8(workspace))
        return fail(WGNN_ERR_ALIGNMENT, "rank2_sum, tie_sum, group_size and workspace must be 8-byte aligned");
    if (!aligned4(t_rowptr) || !aligned4(t_cell) || !aligned4(t_val) || !aligned4(group) || !aligned4(count))
        return fail(WGNN_ERR_ALIGNMENT, "t_rowptr, t_cell, t_val, group and count must be 4-byte aligned");
    GArgs a{};
    a.t_rowptr = t_rowptr; a.t_cell = t_cell; a.t_val = t_val; a.group = group;
    a.group_size = reinterpret_cast<const long long*>(group_size);
    a.n_rows = n_rows; a.n_groups = n_groups; a.n_genes = n_genes;
    a.rank2_sum = reinterpret_cast<long long*>(rank2_sum); a.ld_sum = ld_sum; a.count = count; a.ld_count = ld_count;
    a.tie_sum = reinterpret_cast<long long*>(tie_sum);
    a.n_total = reinterpret_cast<long long*>(workspace);
    a.unit_ptr = a.n_total + 1;
    a.info = reinterpret_cast<int*>(a.unit_ptr + (size_t)n_genes + 1);
    const int64_t r4 = (n_rows + 3) & ~(int64_t)3;
    a.slab = (int)(r4 < 4 ? 4 : (r4 < kGMaxSlab ? r4 : kGMaxSlab));
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto failed = [&fail]() { return fail(WGNN_ERR_LAUNCH, "HIP launch failed (or the LDS slab could not be reserved)"); };

    const long cells = (long)n_groups * n_genes;
    const long waves = n_rows > 0 ? n_genes : 0;                               // prep: a thread per output cell, a wave per gene
    const long want = ((cells > waves * 64 ? cells : waves * 64) + 255) / 256;
    const unsigned nb = (unsigned)(want < kGMaxBlocks ? want : kGMaxBlocks);
    hipLaunchKernelGGL(rank_genes_prep, dim3(nb), dim3(256), 0, st, a);
    if (hipGetLastError() != hipSuccess) return failed();
    if (n_rows == 0) return WGNN_OK;
    hipLaunchKernelGGL(rank_genes_scan, dim3(1), dim3(kGScanThreads), 0, st, a);
    if (hipGetLastError() != hipSuccess) return failed();
    const int lds = a.slab * 4 + kGFixedBytes;
    if (raise_lds(g_lds, reinterpret_cast<const void*>(rank_genes_kernel), lds) != WGNN_OK) return failed();
    hipLaunchKernelGGL(rank_genes_kernel, dim3(kGMaxBlocks), dim3(kGBlock), lds, st, a);
    if (hipGetLastError() != hipSuccess) return failed();
    const long fwant = (cells + 255) / 256;
    hipLaunchKernelGGL(rank_genes_finish, dim3((unsigned)(fwant < kGMaxBlocks ? fwant : kGMaxBlocks)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : failed();
}
