// wgnn_panels.hip - wgnn_predict_rows_panels: one layer of wgnn_predict_rows for every (cell, panel) pair of a batch, a panel
// being a GIVEN subset of the genes (api.ResidentPredictor.panels): the third member of the family of wgnn_predict_rows_dropout
// (a mask drawn per gene) and wgnn_predict_rows_thin (reads drawn, values re-normalised).  Here nothing is drawn: bit p of
// member[g] says whether gene g belongs to panel p of the launch, one 8-byte load beside col[j] answers for all 64 panels.
//
// Values mode (lib == NULL): the kept entries of pair (r, p) are the row's entries whose gene is in the panel, values as given.
// Counts mode: raw holds counts, lib[r, p] is the cell's reads inside the panel (over ALL the caller's columns, computed by the
// host), v' = lognorm(count, lib[r, p], scale) - THE function of wgnn_align_rows.h - and an entry takes part iff its gene is in
// the panel, its count is countable and v' > threshold; lib[r, p] <= 0 is the empty row.  The participating entries, in row
// order, are a row of wgnn_predict_rows: deg' = their number, S' = their f32 sum, the same weights, gather, fold, head, softmax
// maximum and label rule.  No sub-matrix is stored.  (include/wgnn.h has the definition.)
//
// Layout: one WORKGROUP per cell (grid-stride), its 8 waves take the panels p, p + 8, ... (a cell's panels re-read the same
// (col, raw, member[col]) and table rows back to back out of L2, the head image is staged in LDS once per workgroup).  With
// fewer than 8 panels the waves beyond n_panels idle: such a launch is small anyway (P < 8 sub-rows per cell).
// A pair runs in three sweeps of one wave:
//   1   membership (and, in counts mode, v') of every entry, 64 entries per step; the participating ones are compacted (ballot
//       + mbcnt) into the wave's STASH in LDS as (gene, value).
//   2   S' and deg' over the participating entries.
//   3   the weighted gather over them, then the epilogue.
// The arithmetic order is wgnn_predict_rows' order on the COMPACTED row - a lane sums the values at compacted positions lane,
// lane + 64, ..., lane group `sub` accumulates the positions sub, sub + NG, ... ascending - so a pair carries THE BITS that
// wgnn_predict_rows leaves on the materialised sub-row (counts mode: on wgnn_align_count_ln / _fill_ln of the count matrix with
// the other columns zeroed).  The per-64-chunk compaction of wgnn_stability.hip does not give that (a kept entry's lane there
// is its lane in the stored row); the stash and the rotation below are wgnn_thin.hip's.
//
// Stash: kNStash = 1024 (gene, value) pairs per wave, 8 KiB, 64 KiB per workgroup; with a head image of at most 64 KiB that is
// at most 128 KiB of the CU's 160 KiB.  A chunk of 64 entries is stashed whole or not at all; from the first chunk that does not
// fit, the rest of the row is NOT stashed and sweeps 2 and 3 test its membership (and evaluate its v') again.  The tail's
// participating entries continue the compacted row where the stash ends: a cross-lane rotation puts the entry of compacted
// position q into lane q % 64, which keeps every lane's and every lane group's order of addition.
//
// Not done: keeping the cell's (col, raw, member[col]) in LDS once per cell instead of re-gathering member[col] per panel.  The
// stash already makes sweeps 2 and 3 free of member loads for rows up to 1024 kept entries, so the re-gather is one 8-byte L2
// hit per entry and panel in sweep 1, next to a 4 * H-byte table row per kept entry in sweep 3.  The timing (profiles/
// resident_panels.md) has the whole call slower than P classify calls on framework-masked sub-CSRs on plain values, without
// telling the kernel from the host side apart: the staging is the first thing to try, and nothing is claimed for it here.
//
// No atomics of any kind, vector stores only, one addition order whatever the grid: two launches are bit-identical.  The gather
// and head below restate wgnn_thin.hip's and wgnn_predict.hip's on purpose: those files' kernels stay as they are.

#include <math.h>
#include "wgnn_resident_rows.h"
#include "wgnn_align_rows.h"

namespace {
using namespace wgnn;

constexpr int kNWaves = 8;                    // waves per workgroup = panels of one cell in flight
constexpr int kNBlock = 64 * kNWaves;
constexpr int kNMaxBlocks = 1024;             // grid-stride beyond that
constexpr int kNStash = 1024;                 // (gene, value) pairs a wave keeps of one pair
constexpr int kNStashBytes = kNStash * 8;
constexpr int kNMaxPanels = 64;               // bits of a member word

struct NArgs {
    const void* rowptr; const int* col; const float* raw; long n_rows;
    const float* table; long ld_table; int n_genes; int H;
    const float* alpha; const float* bias;
    const float* self_rows; long ld_self;
    const unsigned long long* member; int n_panels;
    const long long* lib; long ld_lib; double scale; float vthr;
    float* out; long ld_out;
    const float* w_head; const float* b_head; int C; float thr;
    float* logits; long ld_logits; int* label; float* max_prob; int* entries;
};

// orders this wave's LDS writes before its later reads (and reads before later writes): the stash is private to the wave
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Entry j of the stored row as pair (., p) sees it: its gene g (a valid id also where the lane holds no entry), its value v
// (counts mode: v' against the pair's library size `total`), and whether it takes part.
__device__ __forceinline__ bool panel_entry(const NArgs& a, long j, bool on, int p, double total, int& g, float& v) {
    g = on ? a.col[j] : 0;
    const float x = on ? a.raw[j] : 0.f;
    bool k = on && ((a.member[g] >> p) & 1ull) != 0;
    if (a.lib) {                                                                   // wave-uniform
        v = lognorm(x, total, a.scale);
        k = k && countable(x) && v > a.vthr;
    } else v = x;
    return k;
}

// One pair's participating entries, handed to f(gene, value, on, p0) 64 lanes at a time in row order: `on` lanes hold an
// entry, their compacted positions are p0, p0 + 1, ... in lane order (p0 is a multiple of 64 for the stashed part, where the
// `on` lanes are the low ones).  First the stash's m entries, then - for a row that outgrew it - the entries from j_over on,
// tested again.  Lanes that are not `on` carry a valid gene id.  Returns the number of entries handed out.
template <typename F>
__device__ __forceinline__ int for_participating(const NArgs& a, const int* scol, const float* sval, int m, long j_over, long e,
                                                 int p, double total, int lane, F&& f) {
    for (int q = 0; q < m; q += 64) {
        const int n = min(64, m - q);
        const int i = q + min(lane, n - 1);
        f(scol[i], sval[i], lane < n, q);
    }
    int p0 = m;
    for (long base = j_over; base < e; base += 64) {
        const long j = base + lane;
        int g; float v;
        const bool k = panel_entry(a, j, j < e, p, total, g, v);
        f(g, v, k, p0);
        p0 += __popcll(__ballot(k));
    }
    return p0;
}

// the lane that takes this lane's value when the `on` lanes (mask km, nk of them) go to the positions p0, p0 + 1, ... mod 64
// and the others fill the remaining lanes: a permutation of 0..63, the identity when p0 % 64 == 0 and the `on` lanes are the low ones
__device__ __forceinline__ int rotated_lane(bool on, unsigned long long km, int nk, int p0, int lane) {
    const int rank = below(km);
    return (on ? p0 + rank : p0 + nk + (lane - rank)) & 63;
}

template <int LPR, bool HEAD, bool SELF_ROWS, typename TPtr>
__global__ void __launch_bounds__(kNBlock) predict_rows_panels_kernel(const NArgs a) {
    extern __shared__ float4 s_mem4[];            // HEAD: [C, H] head image; then the waves' stashes
    char* s_base = reinterpret_cast<char*>(s_mem4);
    const float* s_head = reinterpret_cast<const float*>(s_base);
    constexpr int NG = 64 / LPR;                  // entries of one row processed side by side
    constexpr int U = 8;                          // table rows in flight per lane
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / LPR, l = lane % LPR;
    int* scol = reinterpret_cast<int*>(s_base + (HEAD ? (size_t)a.C * a.H * sizeof(float) : 0) + (size_t)wave * kNStashBytes);
    float* sval = reinterpret_cast<float*>(scol + kNStash);
    const int c0 = l * 4;
    const bool col_on = c0 < a.H;
    if constexpr (HEAD) {
        const int n4 = a.C * a.H / 4;
        for (int i = threadIdx.x; i < n4; i += kNBlock) s_mem4[i] = ld4(a.w_head + 4 * i);
        __syncthreads();
    }
    const float a_self = a.alpha[a.n_genes + 1];
    const TPtr* rp = reinterpret_cast<const TPtr*>(a.rowptr);
    for (long r = blockIdx.x; r < a.n_rows; r += gridDim.x) {                  // block-uniform
        const long b = rp[r], e_row = rp[r + 1];
        for (int p = wave; p < a.n_panels; p += kNWaves) {                       // wave-uniform
            const size_t o = (size_t)r * a.n_panels + p;                         // the pair's row in out / self_rows / logits / ...
            double total = 1.0;
            long e = e_row;
            if (a.lib) {
                const long long lb = a.lib[(size_t)r * a.ld_lib + p];
                total = (double)lb;
                if (lb <= 0) e = b;                                              // no reads in the panel: the empty row
            }
            // sweep 1: the participating entries into the stash
            int m = 0;
            long j_over = e;                                                     // first entry that is not stashed
            for (long base = b; base < e; base += 64) {
                const long j = base + lane;
                int g; float v;
                const bool k = panel_entry(a, j, j < e, p, total, g, v);
                const unsigned long long km = __ballot(k);
                const int nk = __popcll(km);
                if (m + nk > kNStash) { j_over = base; break; }                  // wave-uniform
                if (k) { const int s = m + below(km); scol[s] = g; sval[s] = v; }
                m += nk;
            }
            wave_sync();
            // sweep 2: S' (a lane adds the values at compacted positions lane, lane + 64, ...; then a butterfly) and deg'
            float s = 0.f;
            const int cnt = for_participating(a, scol, sval, m, j_over, e, p, total, lane,
                [&](int, float x, bool on, int p0) {
                    const unsigned long long km = __ballot(on);
                    const int dst = rotated_lane(on, km, __popcll(km), p0, lane);
                    s += __builtin_bit_cast(float, push_to_lane(dst, __builtin_bit_cast(int, on ? x : 0.f)));
                });
            s = group_sum<64>(s);
            const float deg = (float)cnt;
            const bool s_ok = s != 0.f;
            const float self_coef = SELF_ROWS ? 0.f : a_self / (s + 1e-6f);
            // sweep 3: the weighted gather (predict_rows_kernel's, over the compacted row)
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for_participating(a, scol, sval, m, j_over, e, p, total, lane,
                [&](int cc, float x, bool on, int p0) {
                    float w = a.alpha[cc] * (deg * x / s);
                    if constexpr (!SELF_ROWS) w = fmaf(x, self_coef, w);
                    w = on && s_ok ? w : 0.f;
                    const unsigned long long km = __ballot(on);
                    const int nk = __popcll(km);
                    if (nk == 0) return;                                         // wave-uniform
                    const int dst = rotated_lane(on, km, nk, p0, lane);
                    cc = push_to_lane(dst, cc);
                    w = __builtin_bit_cast(float, push_to_lane(dst, __builtin_bit_cast(int, w)));
                    const int start = p0 & 63;                                   // the entries sit in lanes start .. start + nk - 1 (mod 64)
                    const int g0 = start / NG * NG;
                    const int steps = (start - g0 + nk + NG - 1) / NG;
                    for (int j0 = 0; j0 < steps; j0 += U) {
                        float4 xv[U];
                        float wu[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {           // steps past the end re-read the last row with weight 0
                            const int j = min(j0 + u, steps - 1);
                            const int q = g0 + j * NG + sub;                     // position of this group's entry, before the wrap
                            int c; float wj;
                            if constexpr (NG == 1) {
                                c = __builtin_amdgcn_readlane(cc, q & 63);
                                wj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, w), q & 63));
                            } else {
                                c = __shfl(cc, q & 63, 64);
                                wj = __shfl(w, q & 63, 64);
                            }
                            wu[u] = j0 + u < steps && q >= start && q < start + nk ? wj : 0.f;
                            xv[u] = col_on ? ld4(a.table + (size_t)c * a.ld_table + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
                        }
#pragma unroll
                        for (int u = 0; u < U; ++u) fma4(acc, wu[u], xv[u]);
                    }
                });
            wave_sync();                                                         // the stash is read before the next pair rewrites it
#pragma unroll
            for (int off = LPR; off < 64; off <<= 1) {
                acc.x += __shfl_xor(acc.x, off, 64); acc.y += __shfl_xor(acc.y, off, 64);
                acc.z += __shfl_xor(acc.z, off, 64); acc.w += __shfl_xor(acc.w, off, 64);
            }
            float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
            if (col_on) {
                const float invd = 1.0f / (deg + 1.0f);
                if constexpr (SELF_ROWS) fma4(acc, a_self, ld4(a.self_rows + o * a.ld_self + c0));
                const float4 bb = ld4(a.bias + c0);
                h.x = fmaxf(fmaf(acc.x, invd, bb.x), 0.f); h.y = fmaxf(fmaf(acc.y, invd, bb.y), 0.f);
                h.z = fmaxf(fmaf(acc.z, invd, bb.z), 0.f); h.w = fmaxf(fmaf(acc.w, invd, bb.w), 0.f);
            }
            if (lane == 0 && a.entries) a.entries[o] = cnt;
            if constexpr (!HEAD) {
                if (sub == 0 && col_on) st4(a.out + o * a.ld_out + c0, h);
            } else {
                // the head, softmax maximum and label of predict_rows_kernel, operation for operation
                float mx = -INFINITY; int am = 0;
                for (int j0 = 0; j0 < a.C; j0 += NG) {
                    const int j = j0 + sub;
                    float pj = (j < a.C && col_on) ? dot4(h, *reinterpret_cast<const float4*>(s_head + (size_t)j * a.H + c0)) : 0.f;
                    pj = group_sum<LPR>(pj);
                    if (j < a.C) {
                        const float lj = pj + a.b_head[j];
                        if (a.logits && l == 0) a.logits[o * a.ld_logits + j] = lj;
                        if (lj > mx) { mx = lj; am = j; }
                    }
                }
                group_argmax_fold<LPR>(mx, am);
                float se = 0.f;
                for (int j0 = 0; j0 < a.C; j0 += NG) {
                    const int j = j0 + sub;
                    float pj = (j < a.C && col_on) ? dot4(h, *reinterpret_cast<const float4*>(s_head + (size_t)j * a.H + c0)) : 0.f;
                    pj = group_sum<LPR>(pj);
                    if (j < a.C) se += expf(pj + a.b_head[j] - mx);
                }
#pragma unroll
                for (int off = LPR; off < 64; off <<= 1) se += __shfl_xor(se, off, 64);
                if (lane == 0) {
                    const float mp = 1.0f / se;
                    a.max_prob[o] = mp;
                    a.label[o] = mp < a.thr ? -1 : am;
                }
            }
        }
    }
}

template <int LPR, bool HEAD, bool SELF_ROWS, typename TPtr>
int launch_one(const NArgs& a, hipStream_t st) {
    const unsigned nb = (unsigned)(a.n_rows < kNMaxBlocks ? a.n_rows : kNMaxBlocks);
    const size_t lds = (HEAD ? (size_t)a.C * a.H * sizeof(float) : 0) + (size_t)kNWaves * kNStashBytes;
    auto fn = predict_rows_panels_kernel<LPR, HEAD, SELF_ROWS, TPtr>;
    if (lds > (size_t)kHeadLdsBytes &&                   // beyond the default window: ask for the larger one
        hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return WGNN_ERR_LAUNCH;
    hipLaunchKernelGGL(fn, dim3(nb), dim3(kNBlock), lds, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : WGNN_ERR_LAUNCH;
}

template <int LPR, bool HEAD, bool SELF_ROWS>
int launch_lpr(const NArgs& a, bool i64, hipStream_t st) {
    return i64 ? launch_one<LPR, HEAD, SELF_ROWS, long long>(a, st) : launch_one<LPR, HEAD, SELF_ROWS, int>(a, st);
}

}  // namespace

extern "C" int wgnn_predict_rows_panels(const void* rowptr, const int32_t* col, const float* raw, int64_t n_rows,
                                        const float* table, int64_t ld_table, int32_t n_genes, int32_t H,
                                        const float* alpha, const float* bias, const float* self_rows, int64_t ld_self,
                                        const uint64_t* member, int32_t n_panels,
                                        const int64_t* lib, int64_t ld_lib, double scale, float threshold,
                                        float* out, int64_t ld_out,
                                        const float* w_head, const float* b_head, int32_t n_classes, float unsure_threshold,
                                        float* logits, int64_t ld_logits, int32_t* label, float* max_prob, int32_t* entries,
                                        uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_predict_rows_panels", what); };
    wgnn::error_clear();
    if (!rowptr || !col || !raw || !table || !alpha || !bias)
        return fail(WGNN_ERR_BAD_ARG, "rowptr, col, raw, table, alpha and bias are required");
    if (!member) return fail(WGNN_ERR_BAD_ARG, "member is required (uint64 [n_genes], bit p = the gene belongs to panel p)");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [0, 2^31)");
    if (n_panels < 1 || n_panels > kNMaxPanels) return fail(WGNN_ERR_BAD_ARG, "n_panels must be in [1, 64] (split the panels)");
    if (n_rows * (int64_t)n_panels > INT32_MAX)
        return fail(WGNN_ERR_BAD_ARG, "n_rows * n_panels must be < 2^31 (split the batch or the panels)");
    if (lib) {
        if (ld_lib < n_panels) return fail(WGNN_ERR_BAD_ARG, "ld_lib must be >= n_panels");
        if (!(scale > 0.0 && scale < HUGE_VAL)) return fail(WGNN_ERR_BAD_ARG, "scale must be positive and finite");
        if (!(threshold >= 0.f)) return fail(WGNN_ERR_BAD_ARG, "threshold must be >= 0");
    }
    if (n_genes <= 0) return fail(WGNN_ERR_BAD_ARG, "n_genes must be positive");
    if (flags & ~(uint32_t)WGNN_FLAG_ROWPTR_I64) return fail(WGNN_ERR_BAD_ARG, "only WGNN_FLAG_ROWPTR_I64 is a valid flag");
    if (H <= 0) return fail(WGNN_ERR_BAD_ARG, "H must be positive");
    if (H % 4) return fail(WGNN_ERR_ALIGNMENT, "H must be a multiple of 4 (zero-pad the table, bias and head)");
    if (H > 256) return fail(WGNN_ERR_UNSUPPORTED, "H > 256 is not built");
    if (ld_table < H || ld_table % 4) return fail(WGNN_ERR_ALIGNMENT, "ld_table must be >= H and a multiple of 4");
    if (!aligned16(table) || !aligned16(bias)) return fail(WGNN_ERR_ALIGNMENT, "table and bias must be 16-byte aligned");
    if (self_rows && (ld_self < H || ld_self % 4 || !aligned16(self_rows)))
        return fail(WGNN_ERR_ALIGNMENT, "self_rows: ld_self >= H, a multiple of 4, 16-byte aligned");
    if (!aligned8(member) || !aligned8(lib)) return fail(WGNN_ERR_ALIGNMENT, "member and lib must be 8-byte aligned");
    if (!aligned4(entries)) return fail(WGNN_ERR_ALIGNMENT, "entries must be 4-byte aligned");
    const bool head = w_head != nullptr;
    if (head) {
        if (!b_head || !label || !max_prob) return fail(WGNN_ERR_BAD_ARG, "a head needs b_head, label and max_prob");
        if (n_classes <= 0) return fail(WGNN_ERR_BAD_ARG, "n_classes must be positive");
        if ((int64_t)n_classes * H * 4 > kHeadLdsBytes) return fail(WGNN_ERR_UNSUPPORTED, "the head needs C*H*4 <= 64 KiB");
        if (!aligned16(w_head)) return fail(WGNN_ERR_ALIGNMENT, "w_head must be 16-byte aligned");
        if (logits && ld_logits < n_classes) return fail(WGNN_ERR_BAD_ARG, "ld_logits must be >= n_classes");
        if (!aligned4(logits) || !aligned4(label) || !aligned4(max_prob))
            return fail(WGNN_ERR_ALIGNMENT, "logits, label and max_prob must be 4-byte aligned");
    } else {
        if (!out) return fail(WGNN_ERR_BAD_ARG, "without a head `out` is required");
        if (ld_out < H || ld_out % 4 || !aligned16(out))
            return fail(WGNN_ERR_ALIGNMENT, "out: ld_out >= H, a multiple of 4, 16-byte aligned");
    }
    if (n_rows == 0) return WGNN_OK;
    NArgs a{};
    a.rowptr = rowptr; a.col = col; a.raw = raw; a.n_rows = n_rows;
    a.table = table; a.ld_table = ld_table; a.n_genes = n_genes; a.H = H;
    a.alpha = alpha; a.bias = bias; a.self_rows = self_rows; a.ld_self = ld_self;
    a.member = reinterpret_cast<const unsigned long long*>(member); a.n_panels = n_panels;
    a.lib = reinterpret_cast<const long long*>(lib); a.ld_lib = ld_lib; a.scale = scale; a.vthr = threshold;
    a.out = out; a.ld_out = ld_out;
    a.w_head = w_head; a.b_head = b_head; a.C = n_classes; a.thr = unsure_threshold;
    a.logits = logits; a.ld_logits = ld_logits; a.label = label; a.max_prob = max_prob; a.entries = entries;
    const bool i64 = flags & WGNN_FLAG_ROWPTR_I64;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = wgnn::dispatch_rows(H, head, self_rows != nullptr, [&](auto lpr, auto hd, auto sf) {
        return launch_lpr<decltype(lpr)::value, decltype(hd)::value, decltype(sf)::value>(a, i64, st);
    });
    return rc == WGNN_OK ? rc : fail(rc, "HIP launch failed");
}
