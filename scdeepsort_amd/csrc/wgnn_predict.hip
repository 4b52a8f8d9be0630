// wgnn_predict.hip - wgnn_predict_rows: one layer of a trained model over a batch of TEST cells, against gene-side tables
// that stay resident on the device (api.ResidentPredictor).
//
// Why a test cell needs nothing but its own expression row: test cells get gene->cell edges only (reference
// preprocess.py:184-187), PCA is fitted on the support cells (preprocess.py:194-196), so every gene's row at every layer
// is a constant of the bundle.  For one cell with raw values x_g over its deg expressed genes and S = sum_g x_g:
//
//   normalised message weight   w_g = deg * x_g / S                            (normalize_weight, preprocess_internal.py:23)
//   layer 1, self from the row: z = sum_g x_g (alpha[g] deg / S + alpha[G+1] / (S + 1e-6)) Q[g] / (deg + 1) + b
//                               with Q = gene_feat . W1^T; the second term is the self-loop on the cell feature
//                               rownorm(X) . gene_feat (preprocess.py:201-204) folded through W1
//   explicit self rows:         z = (sum_g alpha[g] w_g T[g] + alpha[G+1] self[c]) / (deg + 1) + b
//   then ReLU, and on the last layer the [C, H] head, softmax and the unsure rule (predict.py:78-88).
//
// Layout: one wavefront per cell (grid-stride over the batch, so that a workgroup stages the head in LDS once for many
// cells).  A table row of H <= 256 floats is covered by LPR lanes x float4; for narrow H the 64/LPR lane groups take
// different non-zeros of the row and are folded with xor-shuffles at the end, as agg_main does.  (col, raw) of 64
// non-zeros are fetched with one coalesced load each and broadcast from registers; U table rows are in flight per lane
// before the first FMA.  No plan, no atomics: every sum is folded in a fixed order, two launches are bit-identical.

#include <math.h>
#include "wgnn_resident_rows.h"

namespace {
using namespace wgnn;

constexpr int kPWaves = 8;                    // waves per workgroup (one head image in LDS serves all of them)
constexpr int kPBlock = 64 * kPWaves;
constexpr int kPMaxBlocks = 1024;             // 256 CUs x 4 workgroups: grid-stride beyond that

struct PArgs {
    const void* rowptr; const int* col; const float* raw; long n_rows;
    const float* table; long ld_table; int n_genes; int H;
    const float* alpha; const float* bias;
    const float* self_rows; long ld_self;
    float* out; long ld_out;
    const float* w_head; const float* b_head; int C; float thr;
    float* logits; long ld_logits; int* label; float* max_prob;
};

template <int LPR, bool HEAD, bool SELF_ROWS, typename TPtr>
__global__ void __launch_bounds__(kPBlock) predict_rows_kernel(const PArgs a) {
    extern __shared__ float4 s_head4[];           // [C, H] head image (HEAD only)
    const float* s_head = reinterpret_cast<const float*>(s_head4);
    constexpr int NG = 64 / LPR;                  // non-zeros of one row processed side by side
    constexpr int U = 8;                          // table rows in flight per lane
    const int lane = threadIdx.x & 63, sub = lane / LPR, l = lane % LPR;
    const int c0 = l * 4;
    const bool col_on = c0 < a.H;
    if constexpr (HEAD) {
        const int n4 = a.C * a.H / 4;
        for (int i = threadIdx.x; i < n4; i += kPBlock) s_head4[i] = ld4(a.w_head + 4 * i);
        __syncthreads();
    }
    const float a_self = a.alpha[a.n_genes + 1];
    const TPtr* rp = reinterpret_cast<const TPtr*>(a.rowptr);
    const long stride = (long)gridDim.x * kPWaves;
    for (long r = (long)blockIdx.x * kPWaves + (threadIdx.x >> 6); r < a.n_rows; r += stride) {   // wave-uniform
        const long b = rp[r], e = rp[r + 1];
        const float deg = (float)(e - b);
        // pass 1: S = sum of the raw values (lane-strided, then a butterfly: every lane holds the same bits)
        float s = 0.f;
        for (long j = b + lane; j < e; j += 64) s += a.raw[j];
        s = group_sum<64>(s);
        const float self_coef = SELF_ROWS ? 0.f : a_self / (s + 1e-6f);
        // pass 2: the weighted gather
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (long base = b; base < e; base += 64) {
            const int n = (int)min(64L, e - base);
            const long idx = base + min(lane, n - 1);
            const int cc = a.col[idx];
            const float x = a.raw[idx];
            float w = a.alpha[cc] * (deg * x / s);
            if constexpr (!SELF_ROWS) w = fmaf(x, self_coef, w);
            w = lane < n ? w : 0.f;
            const int steps = (n + NG - 1) / NG;
            for (int j0 = 0; j0 < steps; j0 += U) {
                float4 xv[U];
                float wu[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {       // steps past the end re-read the last row with weight 0
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
        // fold the lane groups in a fixed order: afterwards every group holds the whole row
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1) {
            acc.x += __shfl_xor(acc.x, off, 64); acc.y += __shfl_xor(acc.y, off, 64);
            acc.z += __shfl_xor(acc.z, off, 64); acc.w += __shfl_xor(acc.w, off, 64);
        }
        float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col_on) {
            const float invd = 1.0f / (deg + 1.0f);
            if constexpr (SELF_ROWS) fma4(acc, a_self, ld4(a.self_rows + (size_t)r * a.ld_self + c0));
            const float4 bb = ld4(a.bias + c0);
            h.x = fmaxf(fmaf(acc.x, invd, bb.x), 0.f); h.y = fmaxf(fmaf(acc.y, invd, bb.y), 0.f);
            h.z = fmaxf(fmaf(acc.z, invd, bb.z), 0.f); h.w = fmaxf(fmaf(acc.w, invd, bb.w), 0.f);
        }
        if constexpr (!HEAD) {
            if (sub == 0 && col_on) st4(a.out + (size_t)r * a.ld_out + c0, h);
        } else {
            // head: group `sub` takes classes sub, sub + NG, ...; a logit is the group sum of its lanes' float4 dots.
            // Pass A finds the maximum and its (lowest) index, pass B recomputes the same logits (same bits) for the
            // softmax denominator - no logit buffer, no rescaling.
            float m = -INFINITY; int am = 0;
            for (int j0 = 0; j0 < a.C; j0 += NG) {
                const int j = j0 + sub;
                float p = (j < a.C && col_on) ? dot4(h, *reinterpret_cast<const float4*>(s_head + (size_t)j * a.H + c0)) : 0.f;
                p = group_sum<LPR>(p);
                if (j < a.C) {
                    const float lj = p + a.b_head[j];
                    if (a.logits && l == 0) a.logits[(size_t)r * a.ld_logits + j] = lj;
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
                a.max_prob[r] = mp;
                a.label[r] = mp < a.thr ? -1 : am;
            }
        }
    }
}

template <int LPR, bool HEAD, bool SELF_ROWS>
int launch_lpr(const PArgs& a, bool rowptr_i64, hipStream_t st) {
    const long want = (a.n_rows + kPWaves - 1) / kPWaves;
    const unsigned nb = (unsigned)(want < kPMaxBlocks ? want : kPMaxBlocks);
    const size_t lds = HEAD ? (size_t)a.C * a.H * sizeof(float) : 0;
    if (rowptr_i64)
        hipLaunchKernelGGL((predict_rows_kernel<LPR, HEAD, SELF_ROWS, long long>), dim3(nb), dim3(kPBlock), lds, st, a);
    else
        hipLaunchKernelGGL((predict_rows_kernel<LPR, HEAD, SELF_ROWS, int>), dim3(nb), dim3(kPBlock), lds, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : WGNN_ERR_LAUNCH;
}

}  // namespace

extern "C" int wgnn_predict_rows(const void* rowptr, const int32_t* col, const float* raw, int64_t n_rows,
                                 const float* table, int64_t ld_table, int32_t n_genes, int32_t H,
                                 const float* alpha, const float* bias, const float* self_rows, int64_t ld_self,
                                 float* out, int64_t ld_out,
                                 const float* w_head, const float* b_head, int32_t n_classes, float unsure_threshold,
                                 float* logits, int64_t ld_logits, int32_t* label, float* max_prob,
                                 uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_predict_rows", what); };
    wgnn::error_clear();
    if (!rowptr || !col || !raw || !table || !alpha || !bias)
        return fail(WGNN_ERR_BAD_ARG, "rowptr, col, raw, table, alpha and bias are required");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [0, 2^31)");
    if (n_genes <= 0) return fail(WGNN_ERR_BAD_ARG, "n_genes must be positive");
    if (flags & ~WGNN_FLAG_ROWPTR_I64) return fail(WGNN_ERR_BAD_ARG, "only WGNN_FLAG_ROWPTR_I64 is a valid flag");
    if (H <= 0) return fail(WGNN_ERR_BAD_ARG, "H must be positive");
    if (H % 4) return fail(WGNN_ERR_ALIGNMENT, "H must be a multiple of 4 (zero-pad the table, bias and head)");
    if (H > 256) return fail(WGNN_ERR_UNSUPPORTED, "H > 256 is not built (use the graph route)");
    if (ld_table < H || ld_table % 4) return fail(WGNN_ERR_ALIGNMENT, "ld_table must be >= H and a multiple of 4");
    if (!aligned16(table) || !aligned16(bias)) return fail(WGNN_ERR_ALIGNMENT, "table and bias must be 16-byte aligned");
    if (self_rows && (ld_self < H || ld_self % 4 || !aligned16(self_rows)))
        return fail(WGNN_ERR_ALIGNMENT, "self_rows: ld_self >= H, a multiple of 4, 16-byte aligned");
    const bool head = w_head != nullptr;
    if (head) {
        if (!b_head || !label || !max_prob) return fail(WGNN_ERR_BAD_ARG, "a head needs b_head, label and max_prob");
        if (n_classes <= 0) return fail(WGNN_ERR_BAD_ARG, "n_classes must be positive");
        if ((int64_t)n_classes * H * 4 > kHeadLdsBytes)
            return fail(WGNN_ERR_UNSUPPORTED, "the head needs C*H*4 <= 64 KiB (run it as a GEMM)");
        if (!aligned16(w_head)) return fail(WGNN_ERR_ALIGNMENT, "w_head must be 16-byte aligned");
        if (logits && ld_logits < n_classes) return fail(WGNN_ERR_BAD_ARG, "ld_logits must be >= n_classes");
    } else {
        if (!out) return fail(WGNN_ERR_BAD_ARG, "without a head `out` is required");
        if (ld_out < H || ld_out % 4 || !aligned16(out))
            return fail(WGNN_ERR_ALIGNMENT, "out: ld_out >= H, a multiple of 4, 16-byte aligned");
    }
    if (n_rows == 0) return WGNN_OK;
    PArgs a{};
    a.rowptr = rowptr; a.col = col; a.raw = raw; a.n_rows = n_rows;
    a.table = table; a.ld_table = ld_table; a.n_genes = n_genes; a.H = H;
    a.alpha = alpha; a.bias = bias; a.self_rows = self_rows; a.ld_self = ld_self;
    a.out = out; a.ld_out = ld_out;
    a.w_head = w_head; a.b_head = b_head; a.C = n_classes; a.thr = unsure_threshold;
    a.logits = logits; a.ld_logits = ld_logits; a.label = label; a.max_prob = max_prob;
    const bool i64 = flags & WGNN_FLAG_ROWPTR_I64;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = wgnn::dispatch_rows(H, head, self_rows != nullptr, [&](auto lpr, auto hd, auto sf) {
        return launch_lpr<decltype(lpr)::value, decltype(hd)::value, decltype(sf)::value>(a, i64, st);
    });
    return rc == WGNN_OK ? rc : fail(rc, "HIP launch failed");
}
