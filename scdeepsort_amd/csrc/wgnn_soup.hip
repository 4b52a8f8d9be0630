// wgnn_soup.hip - wgnn_soup_rows_count / wgnn_soup_rows_fill: a cell's count row with n_add reads of AMBIENT RNA (the "soup")
// drawn from a batch-wide profile and added to it, log-normalised against the contaminated library size
// (api.ResidentPredictor.ambient).  The contract is the soup-rows block of include/wgnn.h; for unit q = r * n_draws + d:
//
//   sk = mix64(key(seed, row0 + r, draw0 + d) + K_SOUP);  read t in [0, n_add[r]):  x_t = mulhi64(mix64(sk + t * K_READ), W)
//   falls into the bin k with cdf[k] <= x_t < cdf[k + 1];  c(g) = cnt_r(g) + #{t : bin_t == g};  total = lib[r] + n_add[r];
//   v = lognorm(double(c), total, scale) - the ONE definition of wgnn_align_rows.h; (g, v) leaves iff c > 0 && v > threshold.
//
// Layout: one workgroup per unit, grid-stride.  The genes are cut into slabs of slab_genes; per slab the workgroup zeroes a uint32
// LDS slab, adds the cell's own entries and the unit's reads with LDS integer atomics (entries and reads outside the slab are
// skipped by comparison: a second slab hashes the reads again), then sweeps the slab: every wave owns a contiguous run of 64-gene
// steps, a wave ballot of the keep test counts its entries, the eight counts are folded in wave order, and FILL walks its run a
// second time to store.  COUNT and FILL are the same walk up to the stores.  Integer sums only: exact in every order.  At
// threshold == 0 (and scale >= 1) every non-zero counter is kept - its value is a positive float32, see soup_run - so the counting
// walks skip lognorm() and the logarithm is evaluated once per kept entry, in FILL's storing walk.
//
// The bin of a read is found in two levels: a coarse table of every 2^sh-th boundary of cdf (sh >= 6, at most 512 entries, staged
// in LDS once per workgroup) narrows the search to 2^sh boundaries, which are searched in global memory (sh probes, served by L1 /
// L2: the whole cdf of a 20 000-gene bundle is 160 KB).  DESIGN.md section 3 has the arithmetic.
//
// Never a fault: a row range outside [0, nnz] (the unit leaves the empty row), a gene id outside [0, n_genes) (skipped), an
// n_add outside [0, 2^23] (0 reads), a slot at or past out_rowptr[q + 1] (not written) are reported in the status word (an
// ordinary global atomic OR, off the data path).  Every probe of cdf lies in [1, n_genes] and every probe of the coarse table
// inside it whatever cdf holds, so a cdf that is not ascending gives unspecified bins in [0, n_genes], nothing else.

#include <math.h>
#include "wgnn_align_rows.h"             // lognorm, below
#include "wgnn_build_rows.h"
#include "wgnn_resident_rows.h"          // mix64

namespace {
using namespace wgnn;

constexpr int kSWaves = 8;                    // waves per workgroup - two workgroups of 64 KiB + 4 KiB per CU are 16 waves
constexpr int kSBlock = 64 * kSWaves;
constexpr int kSMaxBlocks = 1024;             // 256 CUs x 2 resident workgroups, twice: grid-stride beyond that
constexpr int kSDefSlab = WGNN_SOUP_MAX_SLAB_GENES;      // slab_genes = 0: 64 KiB of uint32
constexpr int kSCoarse = 512;                 // coarse boundaries kept in LDS, at most
constexpr int kSFolds = 64;                   // bytes of LDS for the per-wave counts (2 x kSWaves int)
constexpr long long kSMaxAdd = 1ll << 23;
constexpr unsigned long long kCell = 0x9FB21C651E98DF25ull, kDraw = 0xD6E8FEB86659FD93ull;     // key() of the dropout block
constexpr unsigned long long kSoup = 0x94D049BB133111EBull, kRead = 0xA0761D6478BD642Full;

struct SArgs {
    const void* rowptr; const int* col; const float* cnt; long n_rows; long nnz;
    const long long* lib; const long long* n_add; const unsigned long long* cdf; int n_genes;
    int n_draws; long row0; int draw0; unsigned long long seed; double scale; float thr;
    int slab; int n_slabs; int sh; int n_coarse;
    int all_kept;                                // threshold == 0 && scale >= 1: every c > 0 is kept, the counting walk skips lognorm()
    int* n_out; int* soup_mapped;                                                               // COUNT
    const long long* out_rowptr; int* out_col; float* out_val; long long* out_cnt; int writable; // FILL
    int* status;
};

// The bin of x: the k in [0, n_genes] with cdf[k] <= x < cdf[k + 1], i.e. the smallest boundary j in [1, n_genes + 1] with
// cdf[j] > x, less one (cdf[n_genes + 1] = W > x is never probed).  coarse[c] = cdf[min(c << sh, n_genes + 1)], c in [0, nc].
__device__ __forceinline__ int locate(unsigned long long x, const unsigned long long* coarse, int nc, int sh,
                                      const unsigned long long* cdf, int n_genes) {
    int lo = 1, hi = nc;                                       // probes in [1, nc - 1]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (coarse[mid] <= x) lo = mid + 1; else hi = mid;
    }
    long jl = ((long)(lo - 1) << sh) + 1, jh = (long)lo << sh;
    if (jh > (long)n_genes + 1) jh = (long)n_genes + 1;
    while (jl < jh) {                                          // probes in [jl, jh - 1] within [1, n_genes]
        const long mid = (jl + jh) >> 1;
        if (cdf[mid] <= x) jl = mid + 1; else jh = mid;
    }
    return (int)(jl - 1);
}

template <bool FILL, typename TPtr>
__global__ void __launch_bounds__(kSBlock) soup_rows_kernel(const SArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
    unsigned long long* s_coarse = reinterpret_cast<unsigned long long*>(s_mem);               // [n_coarse + 1]
    const int coarse_bytes = ((p.n_coarse + 1) * 8 + 15) & ~15;
    int* s_keep = reinterpret_cast<int*>(s_mem + coarse_bytes);                                // [kSWaves] entries kept per wave
    int* s_rest = s_keep + kSWaves;                                                            // [kSWaves] reads of the rest bin
    unsigned* s_slab = reinterpret_cast<unsigned*>(s_mem + coarse_bytes + kSFolds);            // [slab] the unit's counts
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TPtr* rp = reinterpret_cast<const TPtr*>(p.rowptr);
    const int G = p.n_genes;
    const unsigned long long W = p.cdf[(long)G + 1];
    for (int c = threadIdx.x; c <= p.n_coarse; c += kSBlock) {
        long j = (long)c << p.sh;
        if (j > (long)G + 1) j = (long)G + 1;
        s_coarse[c] = p.cdf[j];
    }
    __syncthreads();
    unsigned bad = 0;
    const long n_units = p.n_rows * p.n_draws;
    for (long q = blockIdx.x; q < n_units; q += gridDim.x) {               // everything below is block-uniform but lane / wave
        const long r = q / p.n_draws;
        const int d = (int)(q - r * p.n_draws);
        long e0 = rp[r], e1 = rp[r + 1];
        long long na = p.n_add[r];
        bool row_ok = true;
        if (e0 < 0 || e1 < e0 || e1 > p.nnz) { bad |= WGNN_SOUP_BAD_ROWPTR; row_ok = false; e0 = e1 = 0; }
        if (na < 0 || na > kSMaxAdd) { bad |= WGNN_SOUP_BAD_ADD; na = 0; }
        if (!row_ok) na = 0;                                               // the empty row
        const long long reads = row_ok ? p.lib[r] + na : 0;
        const double total = (double)reads;
        const unsigned long long key = p.seed ^ ((unsigned long long)(p.row0 + r) * kCell) ^
                                       ((unsigned long long)(long long)(p.draw0 + d) * kDraw);
        const unsigned long long sk = mix64(key + kSoup);
        long base = FILL ? (long)p.out_rowptr[q] : 0;
        const long first = base;
        long room = FILL ? (long)p.out_rowptr[q + 1] : 0;                  // a slot at or past it is not written (see `bad`)
        if (FILL && (!p.writable || base < 0)) room = base;
        for (int s = 0; s < p.n_slabs; ++s) {
            const int g0 = s * p.slab;
            const int g1 = g0 + p.slab < G ? g0 + p.slab : G;
            const int n = g1 - g0;
            for (int i = threadIdx.x; i < n; i += kSBlock) s_slab[i] = 0u;
            __syncthreads();
            for (long j = e0 + threadIdx.x; j < e1; j += kSBlock) {
                const int g = p.col[j];
                const float x = p.cnt[j];
                if ((unsigned)g >= (unsigned)G) { bad |= WGNN_SOUP_BAD_COL; continue; }
                if (g >= g0 && g < g1 && x >= 1.f && x <= kMaxCount) atomicAdd(&s_slab[g - g0], (unsigned)x);
            }
            int rest = 0;                                                  // wave-uniform
            for (long t0 = (long)wave * 64; t0 < na; t0 += kSBlock) {      // wave-uniform
                const long t = t0 + lane;
                bool to_rest = false;
                if (t < na) {
                    const unsigned long long u = mix64(sk + (unsigned long long)t * kRead);
                    const int k = locate(__umul64hi(u, W), s_coarse, p.n_coarse, p.sh, p.cdf, G);
                    if (k >= g0 && k < g1) atomicAdd(&s_slab[k - g0], 1u);
                    to_rest = k == G;
                }
                if (!FILL && s == 0) rest += __popcll(__ballot(to_rest));
            }
            if (!FILL && s == 0 && lane == 0) s_rest[wave] = rest;
            __syncthreads();
            if (!FILL && s == 0 && threadIdx.x == 0) {
                int sum = 0;
#pragma unroll
                for (int w = 0; w < kSWaves; ++w) sum += s_rest[w];
                if (p.soup_mapped) p.soup_mapped[q] = (int)(na - sum);
            }
            if (!(reads > 0)) continue;                                    // the empty row (block-uniform)
            // the sweep: wave w owns the genes [c0, c1) of the slab, 64 per step
            const int run = (n + kSBlock - 1) / kSBlock * 64;
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
            for (int w = 0; w < kSWaves; ++w) {
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
                        } else bad |= WGNN_SOUP_BAD_ROWPTR;
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
int launch(const SArgs& p, int which, int lds, unsigned nb, hipStream_t st) {
    const void* fn = reinterpret_cast<const void*>(soup_rows_kernel<FILL, TPtr>);
    if (raise_lds(g_lds[which], fn, lds) != WGNN_OK) return WGNN_ERR_LAUNCH;
    hipLaunchKernelGGL((soup_rows_kernel<FILL, TPtr>), dim3(nb), dim3(kSBlock), lds, st, p);
    return hipGetLastError() == hipSuccess ? WGNN_OK : WGNN_ERR_LAUNCH;
}

}  // namespace

// the checks COUNT and FILL share, then the launch; fn names the entry point in the error detail
template <bool FILL>
static int soup_run(const char* fn, const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                    const int64_t* lib, const int64_t* n_add, const uint64_t* cdf, int32_t n_genes, int32_t n_draws, int64_t row0,
                    int32_t draw0, uint64_t seed, double scale, float threshold, int32_t slab_genes, int32_t* n_out,
                    int32_t* soup_mapped, const int64_t* out_rowptr, int32_t* out_col, float* out_val, int64_t* out_cnt,
                    int32_t* status, uint32_t flags, void* stream) {
    auto fail = [fn](int code, const char* what) { return wgnn::fail(code, fn, what); };
    wgnn::error_clear();
    if (int rc = wgnn::check_count_csr(fn, status, n_rows, nnz)) return rc;
    if (n_genes < 0 || n_genes == INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_genes must be in [0, 2^31 - 1)");
    if (n_draws < 1) return fail(WGNN_ERR_BAD_ARG, "n_draws must be >= 1");
    if (n_rows * (int64_t)n_draws > INT32_MAX)
        return fail(WGNN_ERR_BAD_ARG, "n_rows * n_draws must be < 2^31 (split the batch or the draws)");
    if (row0 < 0 || draw0 < 0) return fail(WGNN_ERR_BAD_ARG, "row0 and draw0 must not be negative");
    if (int rc = wgnn::check_lognorm(fn, scale, threshold)) return rc;
    if (slab_genes < 0 || slab_genes > WGNN_SOUP_MAX_SLAB_GENES)
        return fail(WGNN_ERR_BAD_ARG, "slab_genes must be in [0, 16384] (a wider slab does not fit the LDS budget)");
    if (int rc = wgnn::check_rowptr_flag(fn, flags)) return rc;
    if (n_rows > 0 && (!rowptr || !lib || !n_add || !cdf)) return fail(WGNN_ERR_BAD_ARG, "rowptr, lib, n_add and cdf are required");
    if (int rc = wgnn::check_count_entries(fn, n_rows > 0, nnz, col, cnt)) return rc;
    if (!FILL && n_rows > 0 && !n_out) return fail(WGNN_ERR_BAD_ARG, "n_out is required");
    if (FILL && n_rows > 0 && !out_rowptr) return fail(WGNN_ERR_BAD_ARG, "out_rowptr is required");
    if (!wgnn::aligned8(lib) || !wgnn::aligned8(n_add) || !wgnn::aligned8(cdf) || !wgnn::aligned8(out_rowptr) || !wgnn::aligned8(out_cnt))
        return fail(WGNN_ERR_ALIGNMENT, "lib, n_add, cdf, out_rowptr and out_cnt must be 8-byte aligned");
    if (int rc = wgnn::check_rowptr_alignment(fn, rowptr, flags)) return rc;
    if (!aligned4(col) || !aligned4(cnt) || !aligned4(n_out) || !aligned4(soup_mapped) || !aligned4(out_col) || !aligned4(out_val) ||
        !aligned4(status))
        return fail(WGNN_ERR_ALIGNMENT, "col, cnt, n_out, soup_mapped, out_col, out_val and status must be 4-byte aligned");
    if (n_rows == 0) return WGNN_OK;
    SArgs p{};
    p.rowptr = rowptr; p.col = col; p.cnt = cnt; p.n_rows = n_rows; p.nnz = nnz;
    p.lib = reinterpret_cast<const long long*>(lib); p.n_add = reinterpret_cast<const long long*>(n_add);
    p.cdf = reinterpret_cast<const unsigned long long*>(cdf); p.n_genes = n_genes;
    p.n_draws = n_draws; p.row0 = row0; p.draw0 = draw0; p.seed = seed; p.scale = scale; p.thr = threshold;
    p.slab = slab_genes ? slab_genes : kSDefSlab;
    if (p.slab > n_genes) p.slab = n_genes > 0 ? n_genes : 1;
    p.n_slabs = n_genes > 0 ? (n_genes + p.slab - 1) / p.slab : 1;          // n_genes == 0: one slab of no gene (the rest bin only)
    p.sh = 6;
    while ((((int64_t)n_genes + 1 + ((int64_t)1 << p.sh) - 1) >> p.sh) > kSCoarse) ++p.sh;
    p.n_coarse = (int)(((int64_t)n_genes + 1 + ((int64_t)1 << p.sh) - 1) >> p.sh);
    // c >= 1 and total <= 2^63 give y = c / total * scale >= 2^-63 for scale >= 1, log1p(y) > 2^-64 and a positive float32: with
    // threshold == 0 the keep test is c > 0, and only the storing walk of FILL evaluates the logarithm
    p.all_kept = threshold == 0.f && scale >= 1.0;
    p.n_out = n_out; p.soup_mapped = soup_mapped;
    p.out_rowptr = reinterpret_cast<const long long*>(out_rowptr); p.out_col = out_col; p.out_val = out_val;
    p.out_cnt = reinterpret_cast<long long*>(out_cnt); p.writable = out_col && out_val;
    p.status = status;
    const int lds = (((p.n_coarse + 1) * 8 + 15) & ~15) + kSFolds + p.slab * (int)sizeof(unsigned);
    const int64_t want = n_rows * n_draws;
    const unsigned nb = (unsigned)(want < kSMaxBlocks ? want : kSMaxBlocks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = (flags & WGNN_FLAG_ROWPTR_I64) ? launch<FILL, long long>(p, FILL ? 3 : 1, lds, nb, st)
                                                  : launch<FILL, int>(p, FILL ? 2 : 0, lds, nb, st);
    return rc == WGNN_OK ? rc : fail(rc, "HIP launch failed (or the LDS slab could not be reserved)");
}

extern "C" int wgnn_soup_rows_count(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                                    const int64_t* lib, const int64_t* n_add, const uint64_t* cdf, int32_t n_genes,
                                    int32_t n_draws, int64_t row0, int32_t draw0, uint64_t seed, double scale, float threshold,
                                    int32_t slab_genes, int32_t* n_out, int32_t* soup_mapped, int32_t* status, uint32_t flags,
                                    void* stream) {
    return soup_run<false>("wgnn_soup_rows_count", rowptr, col, cnt, n_rows, nnz, lib, n_add, cdf, n_genes, n_draws, row0, draw0,
                           seed, scale, threshold, slab_genes, n_out, soup_mapped, nullptr, nullptr, nullptr, nullptr, status,
                           flags, stream);
}

extern "C" int wgnn_soup_rows_fill(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                                   const int64_t* lib, const int64_t* n_add, const uint64_t* cdf, int32_t n_genes,
                                   int32_t n_draws, int64_t row0, int32_t draw0, uint64_t seed, double scale, float threshold,
                                   int32_t slab_genes, const int64_t* out_rowptr, int32_t* out_col, float* out_val,
                                   int64_t* out_cnt, int32_t* status, uint32_t flags, void* stream) {
    return soup_run<true>("wgnn_soup_rows_fill", rowptr, col, cnt, n_rows, nnz, lib, n_add, cdf, n_genes, n_draws, row0, draw0,
                          seed, scale, threshold, slab_genes, nullptr, nullptr, out_rowptr, out_col, out_val, out_cnt, status,
                          flags, stream);
}
