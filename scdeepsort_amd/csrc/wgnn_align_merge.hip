// wgnn_align_merge.hip - wgnn_align_count_ln_merge / wgnn_align_fill_ln_merge: the log-normalising walk of wgnn_align.hip for a
// caller whose gene list names some bundle genes MORE THAN ONCE (several Ensembl ids of one symbol, a symbol and its synonym):
// the counts of the columns that name one gene are added per cell before the logarithm is taken.
//
//   a GROUP = the columns that name one bundle gene, two or more of them (its MEMBERS).  col_group[j] = the group of column j
//   or -1 when the column is alone; group_ptr / group_cols = the members of each group, ascending (a CSR over the groups).
//   For cell r and a group with members M:   c = sum over the members that count (finite, > 0), in the row's input order, of
//   double(x[r, j]);   v = float(log1p(c / total[r] * scale));   ONE entry (gene, v) is kept iff c > 0 && v > threshold, and it
//   sits where the FIRST counting member sits in the row's input order.  total[r] is what wgnn_align_count_ln stores: every
//   column, members like any other.  A column that is alone behaves exactly as in wgnn_align_count_ln / _fill_ln.
//
// The walk is wgnn_align.hip's (one wavefront per row, grid-stride; 64 consecutive entries a step, one per lane - or 4 per lane
// and 16-byte loads for aligned dense rows; slots from wave ballots; COUNT and FILL the same instructions).  What is new sits
// between the loads and the logarithm: a candidate lane whose column is a member decides whether it OWNS the group's entry in
// this row - no member that counts comes before it - and, if so, adds the later counting members to its own count in fp64:
//   dense: the other members are gathered from the row itself through group_cols (2-5 loads that hit the lines the wave has
//          just read); a counting member at a lower column makes the lane drop out.
//   CSR  : a row's input order is its stored order, which the column ids do not tell.  One pass before the walk packs the
//          row's counting member entries (group, count), in position order, into a per-wave LDS list of kList entries
//          (ballot + mbcnt); resolve_list gives each listed entry the count its group leaves there (0 = a later member), and
//          the walk, which numbers the member entries by the same ballots, reads its entry's result.  A row with more than
//          kList of them - no limit is put on a valid row - is resolved against its own global entries (slow, correct).
// A lane that does not own its group's entry is no candidate any more and leaves nothing.  Candidates' counts are packed as
// DOUBLES into the wave's slab (a sum of float counts need not be a float), evaluated 64 at a time and read back; for a
// count that is a float, double(x) is the operand wgnn_align.hip's walk divides, so a row in which no group has two counting
// members leaves bit for bit what that walk leaves.  No atomics on the data path, a slot depends on the row alone: two
// launches are bit-identical.
// Never a fault: col_group values outside [-1, n_groups), group_ptr ranges outside [0, n_members] and members outside
// [0, n_cols) are clamped or skipped and raise WGNN_ALIGN_BAD_MAP; everything else as wgnn_align.hip.

#include <limits.h>
#include <math.h>
#include "wgnn_common.h"
#include "wgnn_align_rows.h"

namespace {
using namespace wgnn;

constexpr int kMWaves = 8;                    // waves per workgroup, as wgnn_align.hip
constexpr int kMBlock = 64 * kMWaves;
constexpr int kMMaxBlocks = 1024;
constexpr int kList = 256;                    // CSR: counting member entries of a row the LDS list holds

struct MArgs {
    const float* x; long ld;                                   // dense
    const void* rowptr; const int* col; const float* val;      // CSR over the caller's columns
    long n_rows; int n_cols;
    const int* gene_map; int n_genes; float thr;
    const int* col_group; const int* group_ptr; const int* group_cols; int n_groups; int n_members;
    int* row_count;                                            // COUNT
    const long long* out_rowptr; int* out_col; float* out_raw; // FILL
    int* status;
    const double* total; double scale;                         // the row totals (FILL reads them), Seurat's scale.factor
    const double* lib; double* total_out;                      // COUNT: the caller's library sizes (or null), the totals it stores
};

struct MList { int group[kList]; float val[kList]; double sum[kList]; };   // one wave's counting member entries, position order

__device__ __forceinline__ void wave_sync() {                  // orders LDS writes and reads among the lanes of this one wave
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ bool keep_entry(const MArgs& a, bool on, int g, float v, unsigned& bad) {
    if (on && (g < -1 || g >= a.n_genes)) { bad |= WGNN_ALIGN_BAD_MAP; return false; }
    return on && g >= 0 && v > a.thr;
}

__device__ __forceinline__ void put(const MArgs& a, long s, long room, int g, float v, unsigned& bad) {
    if (s < room) { a.out_col[s] = g; a.out_raw[s] = v; }
    else bad |= WGNN_ALIGN_BAD_ROWPTR;
}

// the wave's candidates among the 4 entries per lane it holds (counts c[k]) become their values v[k], every other entry 0:
// lognorm_group of wgnn_align.hip over a slab of doubles (the value comes back as a double that holds a float exactly)
__device__ __forceinline__ void lognorm_group(double* slab, int lane, const double (&c)[4], const bool (&cand)[4], float (&v)[4],
                                              double total, double scale) {
    int pos[4], n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long m = __ballot(cand[k]);
        pos[k] = n + below(m);
        n += __popcll(m);
    }
    if (n == 0) {                                                // wave-uniform
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = 0.f;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (cand[k]) slab[pos[k]] = c[k];                        // pos < n <= 256
    wave_sync();
    for (int i = lane; i < n; i += 64) slab[i] = (double)lognorm(slab[i], total, scale);
    wave_sync();
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = cand[k] ? (float)slab[pos[k]] : 0.f;
    wave_sync();
}

// a column's group: -1 = alone; a value outside [-1, n_groups) is reported and the column is alone
__device__ __forceinline__ int group_of(const MArgs& a, int s, unsigned& bad) {
    if (s < -1 || s >= a.n_groups) { bad |= WGNN_ALIGN_BAD_MAP; return -1; }
    return s;
}

// Dense: does the counting entry of column j (group s, valid) own its group's entry in row xr?  Not if a member at a lower
// column counts.  The owner's c (its own count on entry) grows by the later counting members, in the list's (ascending) order.
// One flat loop without an early exit: what does not count adds a +0.0, which leaves c (>= 0) as it is.
__device__ __forceinline__ bool own_dense(const MArgs& a, const float* xr, long j, int s, double& c, unsigned& bad) {
    int lo = a.group_ptr[s], hi = a.group_ptr[s + 1];
    if (lo < 0 || hi > a.n_members) { bad |= WGNN_ALIGN_BAD_MAP; lo = lo < 0 ? 0 : lo; hi = hi > a.n_members ? a.n_members : hi; }
    bool owner = true;
    for (int i = lo; i < hi; ++i) {
        const int m = a.group_cols[i];
        const bool in = (unsigned)m < (unsigned)a.n_cols;
        if (!in) bad |= WGNN_ALIGN_BAD_MAP;
        const float xm = in ? xr[m] : 0.f;
        const bool counts = countable(xm);
        owner = owner && !(counts && m < j);
        c += counts && m > j ? (double)xm : 0.0;
    }
    return owner;
}

// CSR: every listed entry i - the row's i-th counting member entry, so the list's order is the row's input order - becomes the
// count its group leaves at that place: the fp64 sum of the group's entries from i on when none of them comes before i, else 0
// (an owner's sum is > 0).  Lanes take entries, the scan over the list is wave-uniform and has no branch.
__device__ __forceinline__ void resolve_list(MList& l, int listed, int lane) {
    for (int i = lane; i < listed; i += 64) {
        const int gi = l.group[i];
        double c = 0.0;
        bool owner = true;
        for (int k = 0; k < listed; ++k) {
            const bool same = l.group[k] == gi;
            owner = owner && !(same && k < i);
            c += same && k >= i ? (double)l.val[k] : 0.0;
        }
        l.sum[i] = owner ? c : 0.0;
    }
}

// CSR: the group of a stored entry (column jc, count v) that is a counting member - column in range, count finite and > 0,
// col_group in [0, n_groups) - else -1.  The list pass and the walk both ask THIS, so they number the same entries.
__device__ __forceinline__ int member_group(const MArgs& a, int jc, float v) {
    if (!((unsigned)jc < (unsigned)a.n_cols && countable(v))) return -1;
    const int grp = a.col_group[jc];
    return grp >= a.n_groups ? -1 : grp;
}

// CSR, a row with more counting member entries than the list holds: the four entries a lane holds in this step (positions
// p + 64 u, groups grp[u] or -1) are resolved against the row's own entries [b, e), which every lane reads in position order
// (wave-uniform addresses, no branch in the body) - resolve_list's rule, one global read per entry of the row and step.
__device__ __forceinline__ void scan_row(const MArgs& a, long b, long e, long p, const int (&grp)[4], double (&c)[4], bool (&cand)[4]) {
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    bool owner[4] = {true, true, true, true};
    for (long q = b; q < e; ++q) {
        const float xq = a.val[q];
        const int gq = member_group(a, a.col[q], xq);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool same = gq >= 0 && gq == grp[u];
            owner[u] = owner[u] && !(same && q < p + 64 * u);
            sum[u] += same && q >= p + 64 * u ? (double)xq : 0.0;
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (grp[u] >= 0) { c[u] = sum[u]; cand[u] = cand[u] && owner[u]; }
}

template <int FORM, typename TPtr>
__device__ __forceinline__ double row_total(const MArgs& a, long r, int lane, unsigned& bad) {      // wgnn_align.hip's, same bits
    double acc = 0.0;
    row_visit<FORM, TPtr>(a, r, lane, [&](long, bool, float v) { add_count(acc, v, bad); });
    acc = wave_fold(acc);
    if (a.lib && acc > 0.0) {
        const double size = a.lib[r];
        if (size > 0.0 && size < __builtin_inf()) acc = size;
        else { bad |= WGNN_ALIGN_BAD_VALUE; acc = 0.0; }
    }
    return acc;
}

template <int FORM, bool FILL, typename TPtr>
__global__ void __launch_bounds__(kMBlock) align_merge_kernel(const MArgs a) {
    __shared__ double s_slab[kMWaves][256];                          // the wave's candidates, packed (lognorm_group)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const long stride = (long)gridDim.x * kMWaves;
    double* slab = s_slab[wave];
    unsigned bad = 0;
    for (long r = (long)blockIdx.x * kMWaves + wave; r < a.n_rows; r += stride) {      // wave-uniform
        long base = FILL ? (long)a.out_rowptr[r] : 0;
        const long first = base;
        const long room = FILL ? (long)a.out_rowptr[r + 1] : 0;
        double total;
        if constexpr (!FILL) {
            total = row_total<FORM, TPtr>(a, r, lane, bad);
            if (lane == 0) a.total_out[r] = total;
        } else total = a.total[r];
        const bool live = total > 0.0;                               // wave-uniform; a row without a total has no candidate
        if constexpr (FORM == FORM_DENSE_V4) {
            const float* xr = a.x + (size_t)r * a.ld;
            for (long j0 = 0; j0 < a.n_cols; j0 += 256 * kVecAhead) {
                float4 v[kVecAhead];
                int4 g[kVecAhead], s[kVecAhead];
#pragma unroll
                for (int u = 0; u < kVecAhead; ++u) {
                    const long j = j0 + u * 256 + lane * 4;
                    if (j + 3 < a.n_cols) {
                        v[u] = ld4(xr + j);
                        g[u] = *reinterpret_cast<const int4*>(a.gene_map + j);
                        s[u] = *reinterpret_cast<const int4*>(a.col_group + j);
                    } else {
                        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                        g[u] = make_int4(-1, -1, -1, -1);
                        s[u] = make_int4(-1, -1, -1, -1);
                        if (j < a.n_cols)     { v[u].x = xr[j];     g[u].x = a.gene_map[j];     s[u].x = a.col_group[j]; }
                        if (j + 1 < a.n_cols) { v[u].y = xr[j + 1]; g[u].y = a.gene_map[j + 1]; s[u].y = a.col_group[j + 1]; }
                        if (j + 2 < a.n_cols) { v[u].z = xr[j + 2]; g[u].z = a.gene_map[j + 2]; s[u].z = a.col_group[j + 2]; }
                    }
                }
#pragma unroll
                for (int u = 0; u < kVecAhead; ++u) {                // counts -> merged counts -> values; no candidate -> 0
                    const long j = j0 + u * 256 + lane * 4;
                    float x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                    const int gg[4] = {g[u].x, g[u].y, g[u].z, g[u].w};
                    const int ss[4] = {s[u].x, s[u].y, s[u].z, s[u].w};
                    double c[4];
                    bool cand[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int grp = group_of(a, ss[k], bad);
                        cand[k] = live && gg[k] >= 0 && countable(x[k]);
                        c[k] = (double)x[k];
                        if (cand[k] && grp >= 0) cand[k] = own_dense(a, xr, j + k, grp, c[k], bad);
                    }
                    lognorm_group(slab, lane, c, cand, x, total, a.scale);
                    v[u] = make_float4(x[0], x[1], x[2], x[3]);
                }
#pragma unroll
                for (int u = 0; u < kVecAhead; ++u) {
                    const bool k0 = keep_entry(a, true, g[u].x, v[u].x, bad), k1 = keep_entry(a, true, g[u].y, v[u].y, bad);
                    const bool k2 = keep_entry(a, true, g[u].z, v[u].z, bad), k3 = keep_entry(a, true, g[u].w, v[u].w, bad);
                    const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1), m2 = __ballot(k2), m3 = __ballot(k3);
                    if constexpr (FILL) {
                        long slot = base + below(m0) + below(m1) + below(m2) + below(m3);
                        if (k0) { put(a, slot, room, g[u].x, v[u].x, bad); ++slot; }
                        if (k1) { put(a, slot, room, g[u].y, v[u].y, bad); ++slot; }
                        if (k2) { put(a, slot, room, g[u].z, v[u].z, bad); ++slot; }
                        if (k3) put(a, slot, room, g[u].w, v[u].w, bad);
                    }
                    base += __popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3);
                }
            }
        } else {
            long b = 0, e = a.n_cols;
            const float* vals = a.x + (FORM == FORM_DENSE ? (size_t)r * a.ld : 0);
            MList* list = nullptr;
            int listed = 0;                                          // CSR: the row's counting member entries
            if constexpr (FORM == FORM_CSR) {
                __shared__ MList s_list[kMWaves];
                const TPtr* rp = reinterpret_cast<const TPtr*>(a.rowptr);
                b = rp[r]; e = rp[r + 1];
                vals = a.val;
                list = &s_list[wave];
                for (long j0 = b; live && j0 < e; j0 += 64 * kAhead) {       // the list, in position order
                    float v[kAhead];
                    int jc[kAhead];
#pragma unroll
                    for (int u = 0; u < kAhead; ++u) {
                        const long j = j0 + u * 64 + lane;
                        v[u] = j < e ? vals[j] : 0.f;
                        jc[u] = j < e ? a.col[j] : -1;
                    }
#pragma unroll
                    for (int u = 0; u < kAhead; ++u) {
                        const int grp = member_group(a, jc[u], v[u]);
                        const unsigned long long m = __ballot(grp >= 0);
                        const int at = listed + below(m);
                        if (grp >= 0 && at < kList) { list->group[at] = grp; list->val[at] = v[u]; }
                        listed += __popcll(m);
                    }
                }
                wave_sync();
                if (listed <= kList) resolve_list(*list, listed, lane);      // wave-uniform; a longer row: scan_row below
                wave_sync();
            }
            int seen = 0;                                            // CSR: listed entries before this step
            for (long j0 = b; j0 < e; j0 += 64 * kAhead) {
                float v[kAhead];
                int g[kAhead], s[kAhead];
                bool on[kAhead];
#pragma unroll
                for (int u = 0; u < kAhead; ++u) {
                    const long j = j0 + u * 64 + lane;
                    on[u] = j < e;
                    v[u] = on[u] ? vals[j] : 0.f;
                    if constexpr (FORM == FORM_CSR) g[u] = on[u] ? a.col[j] : -1;
                    else { g[u] = on[u] ? a.gene_map[j] : -1; s[u] = on[u] ? a.col_group[j] : -1; }
                }
                static_assert(kAhead == 4, "lognorm_group takes 4 entries per lane");
                double c[4];
                bool cand[4];
                if constexpr (FORM == FORM_CSR) {
                    int at[4], grp[4];
                    bool any = false;
#pragma unroll
                    for (int u = 0; u < kAhead; ++u) {               // the list pass's own test and count: at = the entry's place
                        grp[u] = live ? member_group(a, g[u], v[u]) : -1;
                        const unsigned long long m = __ballot(grp[u] >= 0);
                        at[u] = seen + below(m);
                        seen += __popcll(m);
                        any = any || m != 0;
                    }
#pragma unroll
                    for (int u = 0; u < kAhead; ++u) {
                        const bool in = (unsigned)g[u] < (unsigned)a.n_cols;
                        if (on[u] && !in) bad |= WGNN_ALIGN_BAD_COL;
                        on[u] = on[u] && in;
                        if (on[u]) (void)group_of(a, a.col_group[g[u]], bad);
                        g[u] = on[u] ? a.gene_map[g[u]] : -1;
                        cand[u] = live && on[u] && g[u] >= 0 && countable(v[u]);
                        c[u] = (double)v[u];
                    }
                    if (listed <= kList) {                           // wave-uniform
#pragma unroll
                        for (int u = 0; u < kAhead; ++u)
                            if (grp[u] >= 0) { c[u] = list->sum[at[u]]; cand[u] = cand[u] && c[u] > 0.0; }
                    } else if (any) scan_row(a, b, e, j0 + lane, grp, c, cand);
                } else {
#pragma unroll
                    for (int u = 0; u < kAhead; ++u) {
                        const long j = j0 + u * 64 + lane;
                        const int grp = group_of(a, s[u], bad);
                        cand[u] = live && on[u] && g[u] >= 0 && countable(v[u]);
                        c[u] = (double)v[u];
                        if (cand[u] && grp >= 0) cand[u] = own_dense(a, vals, j, grp, c[u], bad);
                    }
                }
                lognorm_group(slab, lane, c, cand, v, total, a.scale);
#pragma unroll
                for (int u = 0; u < kAhead; ++u) {
                    const bool k = keep_entry(a, on[u], g[u], v[u], bad);
                    const unsigned long long m = __ballot(k);
                    if constexpr (FILL) {
                        if (k) put(a, base + below(m), room, g[u], v[u], bad);
                    }
                    base += __popcll(m);
                }
            }
            if constexpr (FORM == FORM_CSR) wave_sync();             // the list is rewritten for the wave's next row
        }
        if constexpr (!FILL) {
            if (lane == 0) a.row_count[r] = (int)(base - first);
        }
    }
    if (bad) atomicOr(a.status, (int)bad);                           // malformed operands only
}

template <int FORM, bool FILL>
int launch(const MArgs& a, bool i64, hipStream_t st) {
    const long want = (a.n_rows + kMWaves - 1) / kMWaves;
    const unsigned nb = (unsigned)(want < kMMaxBlocks ? want : kMMaxBlocks);
    if (i64) hipLaunchKernelGGL((align_merge_kernel<FORM, FILL, long long>), dim3(nb), dim3(kMBlock), 0, st, a);
    else hipLaunchKernelGGL((align_merge_kernel<FORM, FILL, int>), dim3(nb), dim3(kMBlock), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : WGNN_ERR_LAUNCH;
}

// the checks COUNT and FILL share (those of wgnn_align.hip's align_run and the group tables'), then the launch
template <bool FILL>
int merge_run(const char* fn, const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val, int64_t n_rows,
              int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold, const int32_t* col_group,
              const int32_t* group_ptr, const int32_t* group_cols, int32_t n_groups, int32_t n_members, int32_t* row_count,
              const int64_t* out_rowptr, int32_t* out_col, float* out_raw, int32_t* status, uint32_t flags, void* stream,
              const double* total, double scale, double* total_out, const double* library_size) {
    auto fail = [fn](int code, const char* what) { return wgnn::fail(code, fn, what); };
    wgnn::error_clear();
    if (!status) return fail(WGNN_ERR_BAD_ARG, "status is required");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [0, 2^31)");
    if (n_cols < 0) return fail(WGNN_ERR_BAD_ARG, "n_cols must not be negative");
    if (n_genes <= 0) return fail(WGNN_ERR_BAD_ARG, "n_genes must be positive");
    if (n_groups <= 0 || n_members < 0) return fail(WGNN_ERR_BAD_ARG, "n_groups must be positive, n_members not negative");
    if (!col_group || !group_ptr || (n_members > 0 && !group_cols))
        return fail(WGNN_ERR_BAD_ARG, "col_group, group_ptr and group_cols are required");
    if (flags & ~WGNN_FLAG_ROWPTR_I64) return fail(WGNN_ERR_BAD_ARG, "only WGNN_FLAG_ROWPTR_I64 is a valid flag");
    if ((x != nullptr) == (rowptr != nullptr) && n_rows > 0 && (x || n_cols > 0))
        return fail(WGNN_ERR_BAD_ARG, "pass either x (dense) or rowptr / col / val (CSR)");
    const bool dense = rowptr == nullptr;
    if (dense && (flags & WGNN_FLAG_ROWPTR_I64)) return fail(WGNN_ERR_BAD_ARG, "WGNN_FLAG_ROWPTR_I64 belongs to the CSR form");
    if (dense && x && ld < n_cols) return fail(WGNN_ERR_BAD_ARG, "ld must be >= n_cols");
    if (n_cols > 0 && !gene_map) return fail(WGNN_ERR_BAD_ARG, "gene_map is required");
    if (!FILL && n_rows > 0 && !row_count) return fail(WGNN_ERR_BAD_ARG, "row_count is required");
    if (FILL && n_rows > 0 && !out_rowptr) return fail(WGNN_ERR_BAD_ARG, "out_rowptr is required");
    if (FILL && !wgnn::aligned8(out_rowptr)) return fail(WGNN_ERR_ALIGNMENT, "out_rowptr must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(val) | reinterpret_cast<uintptr_t>(gene_map) |
         reinterpret_cast<uintptr_t>(col_group) | reinterpret_cast<uintptr_t>(group_ptr) | reinterpret_cast<uintptr_t>(group_cols)) & 3u)
        return fail(WGNN_ERR_ALIGNMENT, "x, val, gene_map and the group tables must be 4-byte aligned");
    if (!(threshold >= 0.f)) return fail(WGNN_ERR_BAD_ARG, "threshold must be >= 0 when normalising");
    if (!(scale > 0.0 && scale < HUGE_VAL)) return fail(WGNN_ERR_BAD_ARG, "scale must be positive and finite");
    if (n_rows > 0 && !(FILL ? total != nullptr : total_out != nullptr)) return fail(WGNN_ERR_BAD_ARG, "total is required");
    if (!wgnn::aligned8(total) || !wgnn::aligned8(total_out) || !wgnn::aligned8(library_size))
        return fail(WGNN_ERR_ALIGNMENT, "total and library_size must be 8-byte aligned");
    if (n_rows == 0) return WGNN_OK;
    MArgs a{};
    a.x = x; a.ld = ld; a.rowptr = rowptr; a.col = col; a.val = val; a.n_rows = n_rows; a.n_cols = n_cols;
    a.gene_map = gene_map; a.n_genes = n_genes; a.thr = threshold;
    a.col_group = col_group; a.group_ptr = group_ptr; a.group_cols = group_cols; a.n_groups = n_groups; a.n_members = n_members;
    a.row_count = row_count; a.out_rowptr = reinterpret_cast<const long long*>(out_rowptr); a.out_col = out_col; a.out_raw = out_raw;
    a.status = status; a.total = total; a.scale = scale; a.total_out = total_out; a.lib = library_size;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc;
    if (!dense) rc = launch<FORM_CSR, FILL>(a, flags & WGNN_FLAG_ROWPTR_I64, st);
    else if (wgnn::aligned16(x) && wgnn::aligned16(gene_map) && wgnn::aligned16(col_group) && ld % 4 == 0)
        rc = launch<FORM_DENSE_V4, FILL>(a, false, st);
    else rc = launch<FORM_DENSE, FILL>(a, false, st);
    return rc == WGNN_OK ? rc : fail(rc, "HIP launch failed");
}

}  // namespace

// a map without groups is the existing walk's: nobody without duplicates runs the kernels of this file
extern "C" int wgnn_align_count_ln_merge(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                                         int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold,
                                         const int32_t* col_group, const int32_t* group_ptr, const int32_t* group_cols,
                                         int32_t n_groups, int32_t n_members, const double* library_size, double* total,
                                         double scale, int32_t* row_count, int32_t* status, uint32_t flags, void* stream) {
    if (n_groups == 0)
        return wgnn_align_count_ln(x, ld, rowptr, col, val, n_rows, n_cols, gene_map, n_genes, threshold, library_size, total, scale,
                                   row_count, status, flags, stream);
    return merge_run<false>("wgnn_align_count_ln_merge", x, ld, rowptr, col, val, n_rows, n_cols, gene_map, n_genes, threshold,
                            col_group, group_ptr, group_cols, n_groups, n_members, row_count, nullptr, nullptr, nullptr, status,
                            flags, stream, nullptr, scale, total, library_size);
}

extern "C" int wgnn_align_fill_ln_merge(const float* x, int64_t ld, const void* rowptr, const int32_t* col, const float* val,
                                        int64_t n_rows, int32_t n_cols, const int32_t* gene_map, int32_t n_genes, float threshold,
                                        const int32_t* col_group, const int32_t* group_ptr, const int32_t* group_cols,
                                        int32_t n_groups, int32_t n_members, const double* total, double scale,
                                        const int64_t* out_rowptr, int32_t* out_col, float* out_raw, int32_t* status,
                                        uint32_t flags, void* stream) {
    if (n_groups == 0)
        return wgnn_align_fill_ln(x, ld, rowptr, col, val, n_rows, n_cols, gene_map, n_genes, threshold, total, scale, out_rowptr,
                                  out_col, out_raw, status, flags, stream);
    return merge_run<true>("wgnn_align_fill_ln_merge", x, ld, rowptr, col, val, n_rows, n_cols, gene_map, n_genes, threshold,
                           col_group, group_ptr, group_cols, n_groups, n_members, nullptr, out_rowptr, out_col, out_raw, status,
                           flags, stream, total, scale, nullptr, nullptr);
}
