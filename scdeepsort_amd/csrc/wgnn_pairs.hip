// wgnn_pairs.hip - wgnn_pair_rows_count / wgnn_pair_rows_fill: two cells' count rows merged into the log-normalised row of their
// SUM - a synthetic doublet (api.ResidentPredictor.doublets).  The operand is a bundle-vocabulary CSR of raw counts whose rows
// are strictly ascending in col; for pair q = (a, b):
//
//   total = double(lib[a] + lib[b]);   c(g) = cnt_a(g) + cnt_b(g) over the union of the two rows (a missing entry counts 0);
//   v = lognorm(c, total, scale)       - the ONE definition of wgnn_align_rows.h, so a merged row carries the bits
//                                        wgnn_align_count_ln / _fill_ln leave on the summed count matrix;
//   an entry leaves iff c > 0 && v > threshold, in ascending gene id.
//
// The merged rows are written out and classified by wgnn_predict_rows unchanged (DESIGN.md section 3 has the arithmetic of
// materialising against fusing): the count / cumsum / fill scheme of wgnn_align_count_ln / _fill_ln.
//
// Layout: one wavefront per pair, grid-stride.  COUNT and FILL are the same walk, a merge path over the two sorted rows taken
// 64 merged positions at a time: lane l of a step owns position k = k0 + l of the merged sequence (ties: a's element first) and
// finds how many of a's elements precede it by a binary search on the diagonal i + j = k.  The wave carries i0 = the a-elements
// consumed by the earlier steps, so a lane's search is confined to [i0, i0 + l]: at most 6 probes, whatever the rows' lengths.
//   position held by a[i]:  its match, if any, is b[j] (j = the b-elements below a[i]); c = cnt_a[i] (+ cnt_b[j])
//   position held by b[j]:  a duplicate iff a[i - 1] == b[j] (already added to a's element) - it leaves nothing
// A wave ballot of the keep test gives the step's slots (popcount of the mask below the lane) and advances the wave-uniform
// output offset; another ballot advances i0.  No atomics on the data path, no LDS, vector stores only, a slot depends on the
// pair alone: two launches are bit-identical and splitting the pair list changes no bit.  The rows are read from L2 / L1 (a
// batch's rows are re-read by all their partners).
// Never a fault: a pair index outside [0, n_rows), a row range outside [0, nnz], a slot past out_rowptr[q + 1] are skipped and
// reported in the status word (an ordinary global atomic OR, off the data path); a row that is not strictly ascending is
// reported too (every probe stays inside the two rows whatever their order).

#include <math.h>
#include "wgnn_align_rows.h"             // lognorm, countable, below
#include "wgnn_build_rows.h"

namespace {
using namespace wgnn;

constexpr int kPWaves = 4;                    // waves per workgroup
constexpr int kPBlock = 64 * kPWaves;
constexpr int kPMaxBlocks = 2048;             // 256 CUs x 8 workgroups: grid-stride beyond that

struct PArgs {
    const void* rowptr; const int* col; const float* cnt; long n_rows; long nnz;
    const long long* lib;
    const int* a; const int* b; long n_pairs;
    double scale; float thr;
    int* n_out;                                                // COUNT
    const long long* out_rowptr; int* out_col; float* out_val; // FILL
    int* status;
};

template <bool FILL, typename TPtr>
__global__ void __launch_bounds__(kPBlock) pair_rows_kernel(const PArgs p) {
    const int lane = threadIdx.x & 63;
    const long stride = (long)gridDim.x * kPWaves;
    const TPtr* rp = reinterpret_cast<const TPtr*>(p.rowptr);
    unsigned bad = 0;
    for (long q = (long)blockIdx.x * kPWaves + (threadIdx.x >> 6); q < p.n_pairs; q += stride) {      // wave-uniform
        const int ra = p.a[q], rb = p.b[q];
        long a0 = 0, na = 0, b0 = 0, nb = 0;
        double total = 0.0;
        if ((unsigned long)ra >= (unsigned long)p.n_rows || (unsigned long)rb >= (unsigned long)p.n_rows) {
            bad |= WGNN_PAIR_BAD_INDEX;                                  // the empty row
        } else {
            const long a1 = rp[ra + 1], b1 = rp[rb + 1];
            a0 = rp[ra]; b0 = rp[rb];
            if (a0 < 0 || a1 < a0 || a1 > p.nnz || b0 < 0 || b1 < b0 || b1 > p.nnz) {
                bad |= WGNN_PAIR_BAD_ROWPTR;                             // the empty row
            } else {
                total = (double)(p.lib[ra] + p.lib[rb]);
                if (total > 0.0) { na = a1 - a0; nb = b1 - b0; }         // total == 0: the empty row
            }
        }
        const int* ca = p.col + a0;
        const int* cb = p.col + b0;
        const long n = na + nb;
        long base = FILL ? (long)p.out_rowptr[q] : 0;
        const long first = base;
        const long room = FILL ? (long)p.out_rowptr[q + 1] : 0;         // a slot at or past it is not written (see `bad`)
        long i0 = 0;                                                     // a's elements consumed by the earlier steps
        for (long k0 = 0; k0 < n; k0 += 64) {                            // wave-uniform
            const long k = k0 + lane;
            const bool on = k < n;
            bool from_a = false, keep = false;
            int g = 0;
            float v = 0.f;
            if (on) {
                // the order check, off the merge: position k of "a's row, then b's row" against its predecessor in that row, so
                // every neighbouring pair of both rows is looked at once whatever the merge makes of rows out of order
                const int* row = k < na ? ca : cb;
                const long t = k < na ? k : k - na;
                if (t > 0 && row[t - 1] >= row[t]) bad |= WGNN_PAIR_UNSORTED;
                // i = a's elements among the first k merged positions, ties to a first: the smallest i in [lo, hi] with
                // !(a[i] <= b[k - 1 - i]); every probe has lo <= i < hi <= na and 0 <= k - 1 - i < nb
                long lo = i0 > k - nb ? i0 : k - nb;
                long hi = i0 + lane < na ? i0 + lane : na;
                while (lo < hi) {
                    const long mid = (lo + hi) >> 1;
                    if (ca[mid] <= cb[k - 1 - mid]) lo = mid + 1; else hi = mid;
                }
                const long i = lo, j = k - lo;                           // 0 <= i <= na, j >= 0 (i0 <= min(k0, na))
                const bool has_a = i < na, has_b = j < nb;
                const int ga = has_a ? ca[i] : 0, gb = has_b ? cb[j] : 0;
                from_a = has_a && (!has_b || ga <= gb);
                float c = 0.f;
                if (from_a) {
                    g = ga;
                    c = p.cnt[a0 + i];
                    if (has_b && gb == ga) c += p.cnt[b0 + j];           // counts <= 2^23 each: the f32 sum is exact
                } else if (has_b) {
                    g = gb;
                    if (!(i > 0 && ca[i - 1] == gb)) c = p.cnt[b0 + j];  // else the duplicate: added to a's element, leaves nothing
                } else bad |= WGNN_PAIR_UNSORTED;                        // neither row holds this position: only rows out of order
                if (countable(c)) {
                    v = lognorm(c, total, p.scale);
                    keep = v > p.thr;
                }
            }
            const unsigned long long m = __ballot(keep);
            if constexpr (FILL) {
                if (keep) {
                    const long s = base + below(m);
                    if (s < room) { p.out_col[s] = g; p.out_val[s] = v; }
                    else bad |= WGNN_PAIR_BAD_ROWPTR;
                }
            }
            base += __popcll(m);
            i0 += __popcll(__ballot(from_a));
            if (i0 > na) i0 = na;                                        // never for ascending rows; keeps every probe inside a's row
        }
        if constexpr (!FILL) {
            if (lane == 0) p.n_out[q] = (int)(base - first);
        }
    }
    if (bad) atomicOr(p.status, (int)bad);                     // malformed operands only
}

template <bool FILL>
int launch(const PArgs& p, bool i64, hipStream_t st) {
    const long want = (p.n_pairs + kPWaves - 1) / kPWaves;
    const unsigned nb = (unsigned)(want < kPMaxBlocks ? want : kPMaxBlocks);
    if (i64) hipLaunchKernelGGL((pair_rows_kernel<FILL, long long>), dim3(nb), dim3(kPBlock), 0, st, p);
    else hipLaunchKernelGGL((pair_rows_kernel<FILL, int>), dim3(nb), dim3(kPBlock), 0, st, p);
    return hipGetLastError() == hipSuccess ? WGNN_OK : WGNN_ERR_LAUNCH;
}

}  // namespace

// the checks COUNT and FILL share, then the launch; fn names the entry point in the error detail
template <bool FILL>
static int pair_run(const char* fn, const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                    const int64_t* lib, const int32_t* a, const int32_t* b, int64_t n_pairs, double scale, float threshold,
                    int32_t* n_out, const int64_t* out_rowptr, int32_t* out_col, float* out_val, int32_t* status,
                    uint32_t flags, void* stream) {
    auto fail = [fn](int code, const char* what) { return wgnn::fail(code, fn, what); };
    wgnn::error_clear();
    if (int rc = wgnn::check_count_csr(fn, status, n_rows, nnz)) return rc;
    if (n_pairs < 0 || n_pairs > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_pairs must be in [0, 2^31)");
    if (int rc = wgnn::check_rowptr_flag(fn, flags)) return rc;
    if (int rc = wgnn::check_lognorm(fn, scale, threshold)) return rc;
    if (n_pairs > 0 && (!rowptr || !lib || !a || !b)) return fail(WGNN_ERR_BAD_ARG, "rowptr, lib, a and b are required");
    if (int rc = wgnn::check_count_entries(fn, n_pairs > 0, nnz, col, cnt)) return rc;
    if (!FILL && n_pairs > 0 && !n_out) return fail(WGNN_ERR_BAD_ARG, "n_out is required");
    if (FILL && n_pairs > 0 && !out_rowptr) return fail(WGNN_ERR_BAD_ARG, "out_rowptr is required");
    if (!wgnn::aligned8(lib)) return fail(WGNN_ERR_ALIGNMENT, "lib must be 8-byte aligned");
    if (FILL && !wgnn::aligned8(out_rowptr)) return fail(WGNN_ERR_ALIGNMENT, "out_rowptr must be 8-byte aligned");
    if (int rc = wgnn::check_rowptr_alignment(fn, rowptr, flags)) return rc;
    if (!aligned4(col) || !aligned4(cnt) || !aligned4(a) || !aligned4(b) || !aligned4(n_out) || !aligned4(out_col) ||
        !aligned4(out_val) || !aligned4(status))
        return fail(WGNN_ERR_ALIGNMENT, "col, cnt, a, b, n_out, out_col, out_val and status must be 4-byte aligned");
    if (n_pairs == 0) return WGNN_OK;
    PArgs p{};
    p.rowptr = rowptr; p.col = col; p.cnt = cnt; p.n_rows = n_rows; p.nnz = nnz;
    p.lib = reinterpret_cast<const long long*>(lib); p.a = a; p.b = b; p.n_pairs = n_pairs;
    p.scale = scale; p.thr = threshold; p.n_out = n_out;
    p.out_rowptr = reinterpret_cast<const long long*>(out_rowptr); p.out_col = out_col; p.out_val = out_val; p.status = status;
    const int rc = launch<FILL>(p, flags & WGNN_FLAG_ROWPTR_I64, static_cast<hipStream_t>(stream));
    return rc == WGNN_OK ? rc : fail(rc, "HIP launch failed");
}

extern "C" int wgnn_pair_rows_count(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                                    const int64_t* lib, const int32_t* a, const int32_t* b, int64_t n_pairs, double scale,
                                    float threshold, int32_t* n_out, int32_t* status, uint32_t flags, void* stream) {
    return pair_run<false>("wgnn_pair_rows_count", rowptr, col, cnt, n_rows, nnz, lib, a, b, n_pairs, scale, threshold, n_out,
                           nullptr, nullptr, nullptr, status, flags, stream);
}

extern "C" int wgnn_pair_rows_fill(const void* rowptr, const int32_t* col, const float* cnt, int64_t n_rows, int64_t nnz,
                                   const int64_t* lib, const int32_t* a, const int32_t* b, int64_t n_pairs, double scale,
                                   float threshold, const int64_t* out_rowptr, int32_t* out_col, float* out_val, int32_t* status,
                                   uint32_t flags, void* stream) {
    return pair_run<true>("wgnn_pair_rows_fill", rowptr, col, cnt, n_rows, nnz, lib, a, b, n_pairs, scale, threshold, nullptr,
                          out_rowptr, out_col, out_val, status, flags, stream);
}
