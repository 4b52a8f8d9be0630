// wgnn_hood.hip - wgnn_hood_rows_count / wgnn_hood_rows_fill: every cell's count row POOLED with the count rows of its
// neighbours - the caller's kNN lists - and the pooled row log-normalised against the pooled library size: kNN-smoothing in one
// step (api.ResidentPredictor.smooth).  The contract is the hood-rows block of include/wgnn.h; for unit q with the members
// members[hood_ptr[q] : hood_ptr[q + 1]]:
//
//   c(g) = sum over the members r, over the entries j of row r with col[j] == g, of uint64(cnt[j]);  total = sum of lib[r];
//   v = lognorm(double(c), total, scale) - the ONE definition of wgnn_align_rows.h; (g, v) leaves iff c > 0 && v > threshold.
//
// Why not wgnn_pool_rows_accumulate: its dense uint64 [groups, genes] table is B x G x 8 bytes with one group per cell (DESIGN.md
// section 3).  Here a unit's sums never leave the LDS.
//
// Layout: one workgroup per unit, grid-stride.  The unit's members are checked once and their row ranges and library sizes staged
// in LDS (at most 256 of them); the genes are cut into slabs of slab_genes, per slab the workgroup zeroes a uint32 LDS slab, its
// waves take the member rows (one wave per row, 64 entries per step, entries outside the slab skipped by comparison: a row is
// read once per slab), LDS integer atomics take the counts (256 members x 2^23 = 2^31 fits the counter), then the slab is swept
// as wgnn_soup.hip sweeps its slab: every wave owns a contiguous run of 64-gene steps, a wave ballot of the keep test counts its
// entries, the eight counts are folded in wave order, and FILL walks its run a second time to store.  COUNT and FILL are the
// same walk up to the stores.  Integer sums only: exact in every order of the members and of a row's entries.  At threshold == 0
// (and scale >= 1) every non-zero counter is kept - see hood_run - so the counting walks skip lognorm().
//
// Never a fault: a member outside [0, n_rows) or with a row range outside [0, nnz] (skipped, counts and library size), a
// hood_ptr range that descends or leaves [0, n_members] or holds more than 256 members (the empty row), a gene id outside
// [0, n_genes) (skipped), a slot at or past out_rowptr[q + 1] (not written) are reported in the status word (an ordinary global
// atomic OR, off the data path).

#include <math.h>
#include "wgnn_align_rows.h"             // lognorm, below
#include "wgnn_build_rows.h"

namespace {
using namespace wgnn;

constexpr int kHWaves = 8;                    // waves per workgroup - two workgroups of 64 KiB + 6 KiB per CU are 16 waves
constexpr int kHBlock = 64 * kHWaves;
constexpr int kHMaxBlocks = 1024;             // 256 CUs x 2 resident workgroups, twice: grid-stride beyond that
constexpr int kHDefSlab = WGNN_HOOD_MAX_SLAB_GENES;      // slab_genes = 0: 64 KiB of uint32
constexpr int kHMax = WGNN_HOOD_MAX_MEMBERS;
constexpr int kHStage = 3 * kHMax * 8 + 64;   // bytes of LDS before the slab: e0, e1, lib of every member, the per-wave counts

struct HArgs {
    const void* rowptr; const int* col; const float* cnt; long n_rows; long nnz;
    const long long* lib; const long long* hood_ptr; const int* members; long n_units; long n_members; int n_genes;
    double scale; float thr;
    int slab; int n_slabs;
    int all_kept;                                // threshold == 0 && scale >= 1: every c > 0 is kept, the counting walk skips lognorm()
    int* n_out;                                                                                 // COUNT
    const long long* out_rowptr; int* out_col; float* out_val; long long* out_cnt; int writable; // FILL
    int* status;
};

template <bool FILL, typename TPtr>
__global__ void __launch_bounds__(kHBlock) hood_rows_kernel(const HArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
    long long* s_e0 = reinterpret_cast<long long*>(s_mem);                                     // [kHMax] a member's first entry
    long long* s_e1 = s_e0 + kHMax;                                                            // [kHMax] and the end of its row
    long long* s_lib = s_e1 + kHMax;                                                           // [kHMax] its library size
    int* s_keep = reinterpret_cast<int*>(s_lib + kHMax);                                       // [kHWaves] entries kept per wave
    unsigned* s_slab = reinterpret_cast<unsigned*>(s_mem + kHStage);                           // [slab] the unit's counts
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TPtr* rp = reinterpret_cast<const TPtr*>(p.rowptr);
    const int G = p.n_genes;
    unsigned bad = 0;
    for (long q = blockIdx.x; q < p.n_units; q += gridDim.x) {             // everything below is block-uniform but lane / wave
        const long a = p.hood_ptr[q], b = p.hood_ptr[q + 1];
        int n_mem = 0;
        if (a < 0 || b < a || b > p.n_members) bad |= WGNN_HOOD_BAD_ROWPTR;            // the empty row
        else if (b - a > kHMax) bad |= WGNN_HOOD_BAD_SIZE;                             // the empty row
        else n_mem = (int)(b - a);
        __syncthreads();                                                   // the unit before has read its staged members
        if ((int)threadIdx.x < n_mem) {
            const int r = p.members[a + threadIdx.x];
            long e0 = 0, e1 = 0;
            long long reads = 0;
            if ((unsigned long)r >= (unsigned long)p.n_rows) bad |= WGNN_HOOD_BAD_INDEX;       // the member is skipped
            else {
                e0 = rp[r]; e1 = rp[r + 1];
                if (e0 < 0 || e1 < e0 || e1 > p.nnz) { bad |= WGNN_HOOD_BAD_ROWPTR; e0 = e1 = 0; }       // skipped too
                else reads = p.lib[r];
            }
            s_e0[threadIdx.x] = e0; s_e1[threadIdx.x] = e1; s_lib[threadIdx.x] = reads;
        }
        __syncthreads();
        long long reads = 0;
        for (int i = 0; i < n_mem; ++i) reads += s_lib[i];                 // every lane the same LDS word: a broadcast
        const double total = (double)reads;
        long base = FILL ? (long)p.out_rowptr[q] : 0;
        const long first = base;
        long room = FILL ? (long)p.out_rowptr[q + 1] : 0;                  // a slot at or past it is not written (see `bad`)
        if (FILL && (!p.writable || base < 0)) room = base;
        const int n_slabs = reads > 0 ? p.n_slabs : 0;                     // total <= 0, or no member: the empty row
        for (int s = 0; s < n_slabs; ++s) {
            const int g0 = s * p.slab;
            const int g1 = g0 + p.slab < G ? g0 + p.slab : G;
            const int n = g1 - g0;
            for (int i = threadIdx.x; i < n; i += kHBlock) s_slab[i] = 0u;
            __syncthreads();
            for (int m = wave; m < n_mem; m += kHWaves) {                  // wave-uniform
                const long e0 = s_e0[m], e1 = s_e1[m];
                for (long j = e0 + lane; j < e1; j += 64) {
                    const int g = p.col[j];
                    const float x = p.cnt[j];
                    if ((unsigned)g >= (unsigned)G) { bad |= WGNN_HOOD_BAD_COL; continue; }
                    if (g >= g0 && g < g1 && x >= 1.f && x <= kMaxCount) atomicAdd(&s_slab[g - g0], (unsigned)x);
                }
            }
            __syncthreads();
            // the sweep: wave w owns the genes [c0, c1) of the slab, 64 per step
            const int run = (n + kHBlock - 1) / kHBlock * 64;
            const int c0 = wave * run < n ? wave * run : n;
            const int c1 = c0 + run < n ? c0 + run : n;
            int kept = 0;
            for (int i0 = c0; i0 < c1; i0 += 64) {                         // wave-uniform
                const int i = i0 + lane;
                const unsigned c = i < c1 ? s_slab[i] : 0u;
                bool keep = false;
                if (c) keep = p.all_kept || lognorm((double)c, total, p.scale) > p.thr;
                kept += __popcll(__ballot(keep));
            }
            if (lane == 0) s_keep[wave] = kept;
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < kHWaves; ++w) {
                const int k = s_keep[w];
                before += w < wave ? k : 0;
                all += k;
            }
            if constexpr (FILL) {
                long slot = base + before;
                for (int i0 = c0; i0 < c1; i0 += 64) {                     // the same walk, now with the wave's first slot
                    const int i = i0 + lane;
                    const unsigned c = i < c1 ? s_slab[i] : 0u;
                    float v = 0.f;
                    bool keep = false;
                    if (c) {
                        v = lognorm((double)c, total, p.scale);
                        keep = p.all_kept || v > p.thr;                    // the counting walk's decision
                    }
                    const unsigned long long m = __ballot(keep);
                    if (keep) {
                        const long at = slot + below(m);
                        if (at < room) {
                            p.out_col[at] = g0 + i; p.out_val[at] = v;
                            if (p.out_cnt) p.out_cnt[at] = (long long)c;
                        } else bad |= WGNN_HOOD_BAD_ROWPTR;
                    }
                    slot += __popcll(m);
                }
            }
            base += all;
            __syncthreads();                                               // the next slab zeroes s_slab, the next sweep s_keep
        }
        if constexpr (!FILL) {
            if (threadIdx.x == 0) p.n_out[q] = (int)(base - first);
        }
    }
    if (bad) atomicOr(p.status, (int)bad);                     // malformed operands only
}

LdsMarks g_lds[4];                            // the raised LDS limit of COUNT / FILL x rowptr width

template <bool FILL, typename TPtr>
int launch(const HArgs& p, int which, int lds, unsigned nb, hipStream_t st) {
    const void* fn = reinterpret_cast<const void*>(hood_rows_kernel<FILL, TPtr>);
    if (raise_lds(g_lds[which], fn, lds) != WGNN_OK) return WGNN_ERR_LAUNCH;
    hipLaunchKernelGGL((hood_rows_kernel<FILL, TPtr>), dim3(nb), dim3(kHBlock), lds, st, p);
    return hipGetLastError() == hipSuccess ? WGNN_OK : WGNN_ERR_LAUNCH;
}

}  // namespace

// the checks COUNT and FILL share, then the launch; fn names the entry point in the error detail
template <bool FILL>
static int hood_run(const char* fn, const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                    const int64_t* lib, const int64_t* hood_ptr, const int32_t* members, int64_t n_units, int64_t n_members,
                    int32_t n_genes, double scale, float threshold, int32_t slab_genes, int32_t* n_out, const int64_t* out_rowptr,
                    int32_t* out_col, float* out_val, int64_t* out_cnt, int32_t* status, uint32_t flags, void* stream) {
    auto fail = [fn](int code, const char* what) { return wgnn::fail(code, fn, what); };
    wgnn::error_clear();
    if (int rc = wgnn::check_count_csr(fn, status, n_rows, nnz)) return rc;
    if (n_units < 0 || n_units > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_units must be in [0, 2^31)");
    if (n_members < 0) return fail(WGNN_ERR_BAD_ARG, "n_members must not be negative");
    if (n_genes < 0) return fail(WGNN_ERR_BAD_ARG, "n_genes must not be negative");
    if (int rc = wgnn::check_lognorm(fn, scale, threshold)) return rc;
    if (slab_genes < 0 || slab_genes > WGNN_HOOD_MAX_SLAB_GENES)
        return fail(WGNN_ERR_BAD_ARG, "slab_genes must be in [0, 16384] (a wider slab does not fit the LDS budget)");
    if (int rc = wgnn::check_rowptr_flag(fn, flags)) return rc;
    const bool work = n_units > 0;
    if (work && !hood_ptr) return fail(WGNN_ERR_BAD_ARG, "hood_ptr is required");
    if (work && n_members > 0 && !members) return fail(WGNN_ERR_BAD_ARG, "members is required");
    if (work && n_rows > 0 && (!rowptr || !lib)) return fail(WGNN_ERR_BAD_ARG, "rowptr and lib are required");
    if (int rc = wgnn::check_count_entries(fn, work && n_rows > 0, nnz, col, cnt)) return rc;
    if (!FILL && work && !n_out) return fail(WGNN_ERR_BAD_ARG, "n_out is required");
    if (FILL && work && !out_rowptr) return fail(WGNN_ERR_BAD_ARG, "out_rowptr is required");
    if (!wgnn::aligned8(lib) || !wgnn::aligned8(hood_ptr) || !wgnn::aligned8(out_rowptr) || !wgnn::aligned8(out_cnt))
        return fail(WGNN_ERR_ALIGNMENT, "lib, hood_ptr, out_rowptr and out_cnt must be 8-byte aligned");
    if (int rc = wgnn::check_rowptr_alignment(fn, rowptr, flags)) return rc;
    if (!aligned4(col) || !aligned4(cnt) || !aligned4(members) || !aligned4(n_out) || !aligned4(out_col) || !aligned4(out_val) ||
        !aligned4(status))
        return fail(WGNN_ERR_ALIGNMENT, "col, cnt, members, n_out, out_col, out_val and status must be 4-byte aligned");
    if (!work) return WGNN_OK;
    HArgs p{};
    p.rowptr = rowptr; p.col = col; p.cnt = cnt; p.n_rows = n_rows; p.nnz = nnz;
    p.lib = reinterpret_cast<const long long*>(lib); p.hood_ptr = reinterpret_cast<const long long*>(hood_ptr);
    p.members = members; p.n_units = n_units; p.n_members = n_members; p.n_genes = n_genes;
    p.scale = scale; p.thr = threshold;
    p.slab = slab_genes ? slab_genes : kHDefSlab;
    if (p.slab > n_genes) p.slab = n_genes > 0 ? n_genes : 1;
    p.n_slabs = (n_genes + p.slab - 1) / p.slab;
    // c >= 1 and total < 2^63 give y = c / total * scale > 2^-63 for scale >= 1, log1p(y) > 2^-64 and a positive float32: with
    // threshold == 0 the keep test is c > 0, and only the storing walk of FILL evaluates the logarithm
    p.all_kept = threshold == 0.f && scale >= 1.0;
    p.n_out = n_out;
    p.out_rowptr = reinterpret_cast<const long long*>(out_rowptr); p.out_col = out_col; p.out_val = out_val;
    p.out_cnt = reinterpret_cast<long long*>(out_cnt); p.writable = out_col && out_val;
    p.status = status;
    const int lds = kHStage + p.slab * (int)sizeof(unsigned);
    const unsigned nb = (unsigned)(n_units < kHMaxBlocks ? n_units : kHMaxBlocks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = (flags & WGNN_FLAG_ROWPTR_I64) ? launch<FILL, long long>(p, FILL ? 3 : 1, lds, nb, st)
                                                  : launch<FILL, int>(p, FILL ? 2 : 0, lds, nb, st);
    return rc == WGNN_OK ? rc : fail(rc, "HIP launch failed (or the LDS slab could not be reserved)");
}

extern "C" int wgnn_hood_rows_count(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                                    const int64_t* lib, const int64_t* hood_ptr, const int32_t* members, int64_t n_units,
                                    int64_t n_members, int32_t n_genes, double scale, float threshold, int32_t slab_genes,
                                    int32_t* n_out, int32_t* status, uint32_t flags, void* stream) {
    return hood_run<false>("wgnn_hood_rows_count", rowptr, col, cnt, n_rows, nnz, lib, hood_ptr, members, n_units, n_members,
                           n_genes, scale, threshold, slab_genes, n_out, nullptr, nullptr, nullptr, nullptr, status, flags, stream);
}

extern "C" int wgnn_hood_rows_fill(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                                   const int64_t* lib, const int64_t* hood_ptr, const int32_t* members, int64_t n_units,
                                   int64_t n_members, int32_t n_genes, double scale, float threshold, int32_t slab_genes,
                                   const int64_t* out_rowptr, int32_t* out_col, float* out_val, int64_t* out_cnt, int32_t* status,
                                   uint32_t flags, void* stream) {
    return hood_run<true>("wgnn_hood_rows_fill", rowptr, col, cnt, n_rows, nnz, lib, hood_ptr, members, n_units, n_members,
                          n_genes, scale, threshold, slab_genes, nullptr, out_rowptr, out_col, out_val, out_cnt, status, flags,
                          stream);
}
