// wgnn_stability.hip - wgnn_predict_rows_dropout: one layer of wgnn_predict_rows for every (cell, draw) pair of a batch, a draw
// being the cell with a random subset of its stored entries kept (api.ResidentPredictor.stability).
//
// The mask is a pure function of (seed, cell, draw, gene id) - no generator state, no mask array: an entry is kept iff
// mix32(key(seed, cell, draw) + gene * K) < T (include/wgnn.h).  A draw is wgnn_predict_rows' formula over the kept entries:
// deg' = their number, S' = their f32 sum, the same weights, the same gather, the same fold order - a masked entry has weight
// 0.  With keep == 1 every draw carries the bits of wgnn_predict_rows.
//
// Layout: one WORKGROUP per cell (grid-stride over the batch), its 8 waves take the draws d, d + 8, ... of that cell, so the
// draws of a cell re-read the same (col, raw) and the same table rows back to back (L1 / L2 hits), and the head image is
// staged in LDS once per workgroup.  Inside a wave a draw runs as predict_rows_kernel does: LPR lanes x float4 per table row,
// 64 / LPR lane groups side by side, (col, raw) of 64 entries per coalesced load.  The kept entries of such a 64-entry chunk
// are COMPACTED to the low lanes before the gather (one cross-lane permutation of (col, weight); the identity when nothing
// is masked, which is what keeps the keep == 1 bits), so a chunk costs ceil(kept / NG) table-row steps instead of
// ceil(64 / NG): masked entries load nothing.
// With a head the draws of a cell are tallied in LDS: every draw leaves (max_prob, label, empty) in a slot; after a chunk of
// up to 256 draws one lane adds the max_prob slots in ascending draw order in fp64 and thread j counts the slots of class j.
// No atomics of any kind; the addition order depends on the operands alone: two launches are bit-identical.
//
// A draw that keeps nothing, or whose kept values sum to exactly 0, is an empty row: z = bias (+ alpha[G+1] self_rows) - the
// weights are SELECTED to 0, never multiplied, so no NaN comes out of 0 / 0.

#include <math.h>
#include "wgnn_resident_rows.h"

namespace {
using namespace wgnn;

constexpr int kSWaves = 8;                    // waves per workgroup = draws of one cell in flight
constexpr int kSBlock = 64 * kSWaves;
constexpr int kSMaxBlocks = 1024;             // 256 CUs x 4 workgroups: grid-stride beyond that
constexpr int kSSlots = 256;                  // draws tallied per LDS round
constexpr int kSSlotBytes = kSSlots * 12;     // max_prob f32, label int32, empty int32

struct SArgs {
    const void* rowptr; const int* col; const float* raw; long n_rows;
    const float* table; long ld_table; int n_genes; int H;
    const float* alpha; const float* bias;
    const float* self_rows; long ld_self;
    int n_draws; long long row0; long long draw0; unsigned long long seed; unsigned long long T;
    float* out; long ld_out;
    const float* w_head; const float* b_head; int C; float thr;
    int* votes; long ld_votes; int* unsure; int* empty; double* conf_sum;
    int* draw_label; float* draw_prob; int accumulate;
};

__device__ __forceinline__ bool kept_entry(unsigned long long key, int gene, unsigned long long T) {
    return (unsigned long long)mix32(key + (unsigned long long)(long long)gene * 0xC2B2AE3D27D4EB4Full) < T;
}

template <int LPR, bool HEAD, bool SELF_ROWS, typename TPtr>
__global__ void __launch_bounds__(kSBlock) predict_rows_dropout_kernel(const SArgs a) {
    extern __shared__ float4 s_mem4[];            // HEAD: [C, H] head image, then the draw slots
    const float* s_head = reinterpret_cast<const float*>(s_mem4);
    float* s_prob = reinterpret_cast<float*>(s_mem4) + (HEAD ? (size_t)a.C * a.H : 0);
    int* s_lab = reinterpret_cast<int*>(s_prob + kSSlots);
    int* s_emp = s_lab + kSSlots;
    constexpr int NG = 64 / LPR;                  // entries of one row processed side by side
    constexpr int U = 8;                          // table rows in flight per lane
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / LPR, l = lane % LPR;
    const int c0 = l * 4;
    const bool col_on = c0 < a.H;
    if constexpr (HEAD) {
        const int n4 = a.C * a.H / 4;
        for (int i = threadIdx.x; i < n4; i += kSBlock) s_mem4[i] = ld4(a.w_head + 4 * i);
        __syncthreads();
    }
    const float a_self = a.alpha[a.n_genes + 1];
    const TPtr* rp = reinterpret_cast<const TPtr*>(a.rowptr);
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (long r = blockIdx.x; r < a.n_rows; r += gridDim.x) {                  // block-uniform
        const long b = rp[r], e = rp[r + 1];
        const unsigned long long ckey = a.seed ^ ((unsigned long long)(a.row0 + r) * 0x9FB21C651E98DF25ull);
        double csum = 0.0;                                                       // thread 0: the cell's running conf_sum
        if constexpr (HEAD) { if (threadIdx.x == 0 && a.accumulate) csum = a.conf_sum[r]; }
        for (int dc = 0; dc < a.n_draws; dc += kSSlots) {
            const int nd = min(kSSlots, a.n_draws - dc);
            for (int d = dc + wave; d < dc + nd; d += kSWaves) {                 // wave-uniform
                const unsigned long long key = ckey ^ ((unsigned long long)(a.draw0 + d) * 0xD6E8FEB86659FD93ull);
                const size_t o = (size_t)r * a.n_draws + d;                      // the pair's row in out / self_rows / draw_*
                // pass 1: S' and deg' over the kept entries (lane-strided, then a butterfly, as predict_rows_kernel)
                float s = 0.f; int cnt = 0;
                for (long j = b + lane; j < e; j += 64) {
                    const bool k = kept_entry(key, a.col[j], a.T);
                    s += k ? a.raw[j] : 0.f;
                    cnt += k ? 1 : 0;
                }
                s = group_sum<64>(s);
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
                const float deg = (float)cnt;
                const bool s_ok = s != 0.f;
                const float self_coef = SELF_ROWS ? 0.f : a_self / (s + 1e-6f);
                // pass 2: the weighted gather over the kept entries, compacted per 64-entry chunk
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                for (long base = b; base < e; base += 64) {
                    const int n = (int)min(64L, e - base);
                    const long idx = base + min(lane, n - 1);
                    int cc = a.col[idx];
                    const float x = a.raw[idx];
                    float w = a.alpha[cc] * (deg * x / s);
                    if constexpr (!SELF_ROWS) w = fmaf(x, self_coef, w);
                    const bool k = lane < n && s_ok && kept_entry(key, cc, a.T);
                    w = k ? w : 0.f;
                    const unsigned long long km = __ballot(k);
                    const int nk = __popcll(km);
                    if (nk == 0) continue;                                       // wave-uniform: nothing of this chunk is kept
                    const int dst = k ? __popcll(km & lt) : nk + __popcll(~km & lt);
                    cc = push_to_lane(dst, cc);
                    w = __builtin_bit_cast(float, push_to_lane(dst, __builtin_bit_cast(int, w)));
                    const int steps = (nk + NG - 1) / NG;
                    for (int j0 = 0; j0 < steps; j0 += U) {
                        float4 xv[U];
                        float wu[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {   // steps past the end re-read the last row with weight 0
                            const int j = min(j0 + u, steps - 1);
                            int c; float wj;
                            if constexpr (NG == 1) {
                                c = __builtin_amdgcn_readlane(cc, j);
                                wj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, w), j));
                            } else {
                                c = __shfl(cc, j * NG + sub, 64);
                                wj = __shfl(w, j * NG + sub, 64);
                            }
                            wu[u] = j0 + u < steps ? wj : 0.f;
                            xv[u] = col_on ? ld4(a.table + (size_t)c * a.ld_table + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
                        }
#pragma unroll
                        for (int u = 0; u < U; ++u) fma4(acc, wu[u], xv[u]);
                    }
                }
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
                if constexpr (!HEAD) {
                    if (sub == 0 && col_on) st4(a.out + o * a.ld_out + c0, h);
                } else {
                    // the head, softmax maximum and label of predict_rows_kernel, operation for operation
                    float m = -INFINITY; int am = 0;
                    for (int j0 = 0; j0 < a.C; j0 += NG) {
                        const int j = j0 + sub;
                        float p = (j < a.C && col_on) ? dot4(h, *reinterpret_cast<const float4*>(s_head + (size_t)j * a.H + c0)) : 0.f;
                        p = group_sum<LPR>(p);
                        if (j < a.C) {
                            const float lj = p + a.b_head[j];
                            if (lj > m) { m = lj; am = j; }
                        }
                    }
                    group_argmax_fold<LPR>(m, am);
                    float se = 0.f;
                    for (int j0 = 0; j0 < a.C; j0 += NG) {
                        const int j = j0 + sub;
                        float p = (j < a.C && col_on) ? dot4(h, *reinterpret_cast<const float4*>(s_head + (size_t)j * a.H + c0)) : 0.f;
                        p = group_sum<LPR>(p);
                        if (j < a.C) se += expf(p + a.b_head[j] - m);
                    }
#pragma unroll
                    for (int off = LPR; off < 64; off <<= 1) se += __shfl_xor(se, off, 64);
                    if (lane == 0) {
                        const float mp = 1.0f / se;
                        const int lab = mp < a.thr ? -1 : am;
                        s_prob[d - dc] = mp; s_lab[d - dc] = lab; s_emp[d - dc] = cnt == 0 ? 1 : 0;
                        if (a.draw_label) a.draw_label[o] = lab;
                        if (a.draw_prob) a.draw_prob[o] = mp;
                    }
                }
            }
            if constexpr (HEAD) {
                __syncthreads();                                                 // the slots of this round are written
                if (threadIdx.x == 0)
                    for (int i = 0; i < nd; ++i) csum += (double)s_prob[i];      // ascending draw order
                const bool add = a.accumulate || dc > 0;
                for (int j = threadIdx.x; j < a.C + 2; j += kSBlock) {           // class j | unsure | empty: one owner each
                    int n = 0;
                    if (j <= a.C) {
                        const int want = j < a.C ? j : -1;
                        for (int i = 0; i < nd; ++i) n += s_lab[i] == want ? 1 : 0;
                    } else {
                        for (int i = 0; i < nd; ++i) n += s_emp[i];
                    }
                    int* p = j < a.C ? a.votes + (size_t)r * a.ld_votes + j : (j == a.C ? a.unsure + r : a.empty + r);
                    *p = add ? *p + n : n;
                }
                __syncthreads();                                                 // before the next round overwrites the slots
            }
        }
        if constexpr (HEAD) { if (threadIdx.x == 0) a.conf_sum[r] = csum; }
    }
}

template <int LPR, bool HEAD, bool SELF_ROWS, typename TPtr>
int launch_one(const SArgs& a, hipStream_t st) {
    const unsigned nb = (unsigned)(a.n_rows < kSMaxBlocks ? a.n_rows : kSMaxBlocks);
    const size_t lds = HEAD ? (size_t)a.C * a.H * sizeof(float) + kSSlotBytes : 0;
    auto fn = predict_rows_dropout_kernel<LPR, HEAD, SELF_ROWS, TPtr>;
    if (lds > (size_t)kHeadLdsBytes &&                   // a head of (nearly) 64 KiB plus the slots: ask for the larger window
        hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return WGNN_ERR_LAUNCH;
    hipLaunchKernelGGL(fn, dim3(nb), dim3(kSBlock), lds, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : WGNN_ERR_LAUNCH;
}

template <int LPR, bool HEAD, bool SELF_ROWS>
int launch_lpr(const SArgs& a, bool i64, hipStream_t st) {
    return i64 ? launch_one<LPR, HEAD, SELF_ROWS, long long>(a, st) : launch_one<LPR, HEAD, SELF_ROWS, int>(a, st);
}

}  // namespace

extern "C" int wgnn_predict_rows_dropout(const void* rowptr, const int32_t* col, const float* raw, int64_t n_rows,
                                         const float* table, int64_t ld_table, int32_t n_genes, int32_t H,
                                         const float* alpha, const float* bias, const float* self_rows, int64_t ld_self,
                                         int32_t n_draws, int64_t row0, int32_t draw0, uint64_t seed, double keep,
                                         float* out, int64_t ld_out,
                                         const float* w_head, const float* b_head, int32_t n_classes, float unsure_threshold,
                                         int32_t* votes, int64_t ld_votes, int32_t* unsure, int32_t* empty, double* conf_sum,
                                         int32_t* draw_label, float* draw_prob, uint32_t flags, void* stream) {
    static const wgnn::DrawEntry entry{"wgnn_predict_rows_dropout", WGNN_STABILITY_ACCUMULATE,
                                       "only WGNN_FLAG_ROWPTR_I64 and WGNN_STABILITY_ACCUMULATE are valid flags",
                                       "WGNN_STABILITY_ACCUMULATE needs a head"};
    const wgnn::DrawCall c{rowptr, col, raw, n_rows, table, ld_table, n_genes, H, alpha, bias, self_rows, ld_self,
                           n_draws, row0, draw0, seed, keep, out, ld_out, w_head, b_head, n_classes, unsure_threshold,
                           votes, ld_votes, unsure, empty, conf_sum, draw_label, draw_prob, flags};
    wgnn::error_clear();
    if (const int bad = wgnn::check_draw_call(entry, c, nullptr)) return bad;
    if (n_rows == 0) return WGNN_OK;
    SArgs a{};
    wgnn::fill_draw_args(a, c, entry.accumulate);
    const bool i64 = flags & WGNN_FLAG_ROWPTR_I64;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = wgnn::dispatch_rows(H, w_head != nullptr, self_rows != nullptr, [&](auto lpr, auto hd, auto sf) {
        return launch_lpr<decltype(lpr)::value, decltype(hd)::value, decltype(sf)::value>(a, i64, st);
    });
    return rc == WGNN_OK ? rc : wgnn::fail(rc, entry.fn, "HIP launch failed");
}
