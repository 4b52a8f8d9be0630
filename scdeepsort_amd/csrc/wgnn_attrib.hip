// wgnn_attrib.hip - wgnn_attrib_rows / wgnn_rows_topk: which genes made a test cell's logit (api.ResidentPredictor.explain).
//
// Notation as in wgnn_predict.hip.  Once the ReLU pattern m_l = (z_l > 0) of one cell is fixed, the target logit is LINEAR in
// the cell's per-gene message weights
//
//   u_{1,g} = x_g (alpha[g] deg / S + alpha[G+1] / (S + 1e-6)) / (deg + 1)          layer 1, self-loop from the row
//   u_{l,g} = alpha[g] (deg x_g / S) / (deg + 1)                                    explicit-self layers (l >= 2)
//
// so with the direction vectors v_L = m_L * Wh[t], v_{l-1} = m_{l-1} * (W_l^T v_l) * alpha[G+1] / (deg + 1) the logit splits,
// without approximation, into phi_g = sum_l u_{l,g} <T_l[g], v_l> per expressed gene plus base = bh[t] + sum_l <v_l, b_l>.
//
// Head mode (the model's last layer) repeats wgnn_predict_rows' weighted gather operation for operation - z, the logits and the
// arg max carry the bits of a classify call - forms v in registers and walks the row a second time (the table rows it has just
// pulled through L2): entry j gets u_j <T[col_j], v>.  Direction mode (layers below the last) is the second walk alone, with v
// given.  Layout as predict_rows_kernel: one wavefront per cell, grid-stride, LPR lanes x float4 per table row, 64 / LPR
// entries side by side.  The scores of a 64-entry chunk are collected into one register per lane and leave with one coalesced
// store.  A row is owned by one wave (the accumulate is race-free); no atomics, fixed fold order: two launches are bit-identical.

#include <math.h>
#include "wgnn_resident_rows.h"

namespace {
using namespace wgnn;

constexpr int kAWaves = 8;                    // waves per workgroup (one head image in LDS serves all of them)
constexpr int kABlock = 64 * kAWaves;
constexpr int kAMaxBlocks = 1024;             // 256 CUs x 4 workgroups: grid-stride beyond that
constexpr int kTWaves = 4;                    // wgnn_rows_topk
constexpr int kTBlock = 64 * kTWaves;
constexpr int kTMaxBlocks = 2048;

struct AArgs {
    const void* rowptr; const int* col; const float* raw; long n_rows;
    const float* table; long ld_table; int n_genes; int H;
    const float* alpha; const float* bias;
    const float* self_rows; long ld_self;
    const float* w_head; const float* b_head; int C; const int* target; float thr; int* label_out;
    const float* direction; long ld_dir;
    float* score; int accumulate;
    int* target_out; float* logit_out; float* base_out; float* dir_out; long ld_dir_out;
};

// HEAD: gather + head + scores of the last layer; else scores against a given direction.  SELF_ROWS: the layer's self-loop is
// explicit (no self term in the per-entry coefficient; in head mode a.self_rows enters z).
template <int LPR, bool HEAD, bool SELF_ROWS, typename TPtr>
__global__ void __launch_bounds__(kABlock) attrib_rows_kernel(const AArgs a) {
    extern __shared__ float4 s_head4[];           // [C, H] head image (HEAD only)
    const float* s_head = reinterpret_cast<const float*>(s_head4);
    constexpr int NG = 64 / LPR;                  // non-zeros of one row processed side by side
    constexpr int U = 8;                          // table rows in flight per lane
    const int lane = threadIdx.x & 63, sub = lane / LPR, l = lane % LPR;
    const int c0 = l * 4;
    const bool col_on = c0 < a.H;
    if constexpr (HEAD) {
        const int n4 = a.C * a.H / 4;
        for (int i = threadIdx.x; i < n4; i += kABlock) s_head4[i] = ld4(a.w_head + 4 * i);
        __syncthreads();
    }
    const float a_self = a.alpha[a.n_genes + 1];
    const TPtr* rp = reinterpret_cast<const TPtr*>(a.rowptr);
    const long stride = (long)gridDim.x * kAWaves;
    for (long r = (long)blockIdx.x * kAWaves + (threadIdx.x >> 6); r < a.n_rows; r += stride) {   // wave-uniform
        const long b = rp[r], e = rp[r + 1];
        const float deg = (float)(e - b);
        // S = sum of the raw values (lane-strided, then a butterfly: every lane holds the same bits)
        float s = 0.f;
        for (long j = b + lane; j < e; j += 64) s += a.raw[j];
        s = group_sum<64>(s);
        const float self_coef = SELF_ROWS ? 0.f : a_self / (s + 1e-6f);
        const float invd = 1.0f / (deg + 1.0f);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (HEAD) {
            // pass 1: the weighted gather, operation for operation that of predict_rows_kernel
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
#pragma unroll
            for (int off = LPR; off < 64; off <<= 1) {
                acc.x += __shfl_xor(acc.x, off, 64); acc.y += __shfl_xor(acc.y, off, 64);
                acc.z += __shfl_xor(acc.z, off, 64); acc.w += __shfl_xor(acc.w, off, 64);
            }
            float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
            if (col_on) {
                if constexpr (SELF_ROWS) fma4(acc, a_self, ld4(a.self_rows + (size_t)r * a.ld_self + c0));
                bb = ld4(a.bias + c0);
                h.x = fmaxf(fmaf(acc.x, invd, bb.x), 0.f); h.y = fmaxf(fmaf(acc.y, invd, bb.y), 0.f);
                h.z = fmaxf(fmaf(acc.z, invd, bb.z), 0.f); h.w = fmaxf(fmaf(acc.w, invd, bb.w), 0.f);
            }
            // the arg max as predict_rows_kernel finds it (lowest index among equal maxima), its softmax rule for the label,
            // and the target: the caller's, or that arg max
            float m = -INFINITY; int am = 0;
            if (!a.target || a.label_out) {                  // wave-uniform
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
            }
            if (a.label_out) {
                float se = 0.f;
                for (int j0 = 0; j0 < a.C; j0 += NG) {
                    const int j = j0 + sub;
                    float p = (j < a.C && col_on) ? dot4(h, *reinterpret_cast<const float4*>(s_head + (size_t)j * a.H + c0)) : 0.f;
                    p = group_sum<LPR>(p);
                    if (j < a.C) se += expf(p + a.b_head[j] - m);
                }
#pragma unroll
                for (int off = LPR; off < 64; off <<= 1) se += __shfl_xor(se, off, 64);
                if (lane == 0) a.label_out[r] = 1.0f / se < a.thr ? -1 : am;
            }
            const int t = a.target ? min(max(a.target[r], 0), a.C - 1) : am;   // the wrapper checks the range; the clamp keeps
                                                                               // LDS reads inside the head whatever it holds
            // the target logit, by every lane group (the bits of the loop above and of predict_rows' logits), then
            // v = m * Wh[t] and the bias share
            const float4 wt = col_on ? *reinterpret_cast<const float4*>(s_head + (size_t)t * a.H + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
            float p = col_on ? dot4(h, wt) : 0.f;
            p = group_sum<LPR>(p);
            const float bt = a.b_head[t];
            const float logit = p + bt;
            v.x = h.x > 0.f ? wt.x : 0.f; v.y = h.y > 0.f ? wt.y : 0.f;
            v.z = h.z > 0.f ? wt.z : 0.f; v.w = h.w > 0.f ? wt.w : 0.f;
            const float vb = group_sum<LPR>(dot4(v, bb));
            if (lane == 0) {
                a.target_out[r] = t;
                a.logit_out[r] = logit;
                a.base_out[r] = bt + vb;
            }
            if (a.dir_out && sub == 0 && col_on) st4(a.dir_out + (size_t)r * a.ld_dir_out + c0, v);
        } else {
            if (col_on) v = ld4(a.direction + (size_t)r * a.ld_dir + c0);
        }
        // pass 2: score of entry j = u_j <T[col_j], v>.  Lane group `sub` takes entries sub, sub + NG, ... of the chunk; the
        // dot of entry i is handed to lane i, which holds the entry's coefficient and stores the chunk's scores in one go.
        for (long base = b; base < e; base += 64) {
            const int n = (int)min(64L, e - base);
            const long idx = base + min(lane, n - 1);
            const int cc = a.col[idx];
            const float x = a.raw[idx];
            float w = a.alpha[cc] * (deg * x / s);
            if constexpr (!SELF_ROWS) w = fmaf(x, self_coef, w);
            float mine = 0.f;
            const int steps = (n + NG - 1) / NG;
            for (int j0 = 0; j0 < steps; j0 += U) {
                float4 xv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {           // steps past the end re-read the last row; no lane below n keeps them
                    const int j = min(j0 + u, steps - 1);
                    int c;
                    if constexpr (NG == 1) c = __builtin_amdgcn_readlane(cc, j);
                    else c = __shfl(cc, j * NG + sub, 64);
                    xv[u] = col_on ? ld4(a.table + (size_t)c * a.ld_table + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float d = group_sum<LPR>(dot4(xv[u], v));
                    if constexpr (NG > 1) d = __shfl(d, (lane % NG) * LPR, 64);     // entry `lane` was group lane % NG's
                    if (lane / NG == j0 + u) mine = d;
                }
            }
            if (lane < n) {
                const float sc = (w * invd) * mine;
                a.score[idx] = a.accumulate ? a.score[idx] + sc : sc;
            }
        }
    }
}

template <int LPR, bool HEAD, bool SELF_ROWS>
int launch_lpr(const AArgs& a, bool rowptr_i64, hipStream_t st) {
    const long want = (a.n_rows + kAWaves - 1) / kAWaves;
    const unsigned nb = (unsigned)(want < kAMaxBlocks ? want : kAMaxBlocks);
    const size_t lds = HEAD ? (size_t)a.C * a.H * sizeof(float) : 0;
    if (rowptr_i64)
        hipLaunchKernelGGL((attrib_rows_kernel<LPR, HEAD, SELF_ROWS, long long>), dim3(nb), dim3(kABlock), lds, st, a);
    else
        hipLaunchKernelGGL((attrib_rows_kernel<LPR, HEAD, SELF_ROWS, int>), dim3(nb), dim3(kABlock), lds, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : WGNN_ERR_LAUNCH;
}

// wgnn_rows_topk: k rounds of "the best entry after the one taken last" in the order (score descending, position ascending).
// Lane i scans positions i, i + 64, ... (ascending, so a strict > keeps its lowest position), a butterfly picks the wave's
// best.  Round i's result is kept by lane i and the k results leave with one store.  `score` is only read.
template <typename TPtr>
__global__ void __launch_bounds__(kTBlock) rows_topk_kernel(const TPtr* rp, const int* col, const float* score, long n_rows,
                                                            int k, int* gene_out, float* score_out) {
    const int lane = threadIdx.x & 63;
    const long stride = (long)gridDim.x * kTWaves;
    for (long r = (long)blockIdx.x * kTWaves + (threadIdx.x >> 6); r < n_rows; r += stride) {     // wave-uniform
        const long b = rp[r];
        const int n = (int)(rp[r + 1] - b);
        float prev_s = INFINITY; int prev_p = -1;
        int my_gene = -1; float my_score = 0.f;
        for (int i = 0; i < k; ++i) {
            float bs = 0.f; int bp = -1;
            for (int p = lane; p < n; p += 64) {
                const float sc = score[b + p];
                const bool after = sc < prev_s || (sc == prev_s && p > prev_p);
                if (after && (bp < 0 || sc > bs)) { bs = sc; bp = p; }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float os = __shfl_xor(bs, off, 64);
                const int op = __shfl_xor(bp, off, 64);
                if (op >= 0 && (bp < 0 || os > bs || (os == bs && op < bp))) { bs = os; bp = op; }
            }
            if (bp < 0) break;                      // wave-uniform: the row is exhausted
            if (lane == i) { my_gene = col[b + bp]; my_score = bs; }
            prev_s = bs; prev_p = bp;
        }
        if (lane < k) {
            gene_out[r * k + lane] = my_gene;
            score_out[r * k + lane] = my_score;
        }
    }
}

}  // namespace

extern "C" int wgnn_attrib_rows(const void* rowptr, const int32_t* col, const float* raw, int64_t n_rows,
                                const float* table, int64_t ld_table, int32_t n_genes, int32_t H,
                                const float* alpha, const float* bias, const float* self_rows, int64_t ld_self,
                                const float* w_head, const float* b_head, int32_t n_classes, const int32_t* target,
                                float unsure_threshold, int32_t* label_out, const float* direction, int64_t ld_dir,
                                float* score, int32_t* target_out, float* logit_out, float* base_out,
                                float* dir_out, int64_t ld_dir_out, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_attrib_rows", what); };
    wgnn::error_clear();
    if (!rowptr || !col || !raw || !table || !alpha || !score)
        return fail(WGNN_ERR_BAD_ARG, "rowptr, col, raw, table, alpha and score are required");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [0, 2^31)");
    if (n_genes <= 0) return fail(WGNN_ERR_BAD_ARG, "n_genes must be positive");
    if (flags & ~(uint32_t)(WGNN_FLAG_ROWPTR_I64 | WGNN_ATTRIB_ACCUMULATE | WGNN_ATTRIB_EXPLICIT_SELF))
        return fail(WGNN_ERR_BAD_ARG, "valid flags: WGNN_FLAG_ROWPTR_I64, WGNN_ATTRIB_ACCUMULATE, WGNN_ATTRIB_EXPLICIT_SELF");
    if (H <= 0) return fail(WGNN_ERR_BAD_ARG, "H must be positive");
    if (H % 4) return fail(WGNN_ERR_ALIGNMENT, "H must be a multiple of 4 (zero-pad the table, bias, head and direction)");
    if (H > 256) return fail(WGNN_ERR_UNSUPPORTED, "H > 256 is not built");
    if (ld_table < H || ld_table % 4) return fail(WGNN_ERR_ALIGNMENT, "ld_table must be >= H and a multiple of 4");
    if (!aligned16(table)) return fail(WGNN_ERR_ALIGNMENT, "table must be 16-byte aligned");
    const bool head = w_head != nullptr;
    if (head == (direction != nullptr)) return fail(WGNN_ERR_BAD_ARG, "give either a head (w_head) or a direction");
    bool explicit_self;
    if (head) {
        if (!bias || !b_head || !target_out || !logit_out || !base_out)
            return fail(WGNN_ERR_BAD_ARG, "a head needs bias, b_head, target_out, logit_out and base_out");
        if (flags & (WGNN_ATTRIB_ACCUMULATE | WGNN_ATTRIB_EXPLICIT_SELF))
            return fail(WGNN_ERR_BAD_ARG, "head mode overwrites score and takes its self rule from self_rows");
        if (!aligned16(bias)) return fail(WGNN_ERR_ALIGNMENT, "bias must be 16-byte aligned");
        if (self_rows && (ld_self < H || ld_self % 4 || !aligned16(self_rows)))
            return fail(WGNN_ERR_ALIGNMENT, "self_rows: ld_self >= H, a multiple of 4, 16-byte aligned");
        if (n_classes <= 0) return fail(WGNN_ERR_BAD_ARG, "n_classes must be positive");
        if ((int64_t)n_classes * H * 4 > kHeadLdsBytes)
            return fail(WGNN_ERR_UNSUPPORTED, "the head needs C*H*4 <= 64 KiB");
        if (!aligned16(w_head)) return fail(WGNN_ERR_ALIGNMENT, "w_head must be 16-byte aligned");
        if (dir_out && (ld_dir_out < H || ld_dir_out % 4 || !aligned16(dir_out)))
            return fail(WGNN_ERR_ALIGNMENT, "dir_out: ld_dir_out >= H, a multiple of 4, 16-byte aligned");
        explicit_self = self_rows != nullptr;
    } else {
        if (ld_dir < H || ld_dir % 4 || !aligned16(direction))
            return fail(WGNN_ERR_ALIGNMENT, "direction: ld_dir >= H, a multiple of 4, 16-byte aligned");
        explicit_self = (flags & WGNN_ATTRIB_EXPLICIT_SELF) != 0;
    }
    if (n_rows == 0) return WGNN_OK;
    AArgs a{};
    a.rowptr = rowptr; a.col = col; a.raw = raw; a.n_rows = n_rows;
    a.table = table; a.ld_table = ld_table; a.n_genes = n_genes; a.H = H;
    a.alpha = alpha; a.bias = bias; a.self_rows = self_rows; a.ld_self = ld_self;
    a.w_head = w_head; a.b_head = b_head; a.C = n_classes; a.target = target; a.thr = unsure_threshold; a.label_out = label_out;
    a.direction = direction; a.ld_dir = ld_dir;
    a.score = score; a.accumulate = (flags & WGNN_ATTRIB_ACCUMULATE) ? 1 : 0;
    a.target_out = target_out; a.logit_out = logit_out; a.base_out = base_out; a.dir_out = dir_out; a.ld_dir_out = ld_dir_out;
    const bool i64 = flags & WGNN_FLAG_ROWPTR_I64;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = wgnn::dispatch_rows(H, head, explicit_self, [&](auto lpr, auto hd, auto sf) {
        return launch_lpr<decltype(lpr)::value, decltype(hd)::value, decltype(sf)::value>(a, i64, st);
    });
    return rc == WGNN_OK ? rc : fail(rc, "HIP launch failed");
}

extern "C" int wgnn_rows_topk(const void* rowptr, const int32_t* col, const float* score, int64_t n_rows, int32_t k,
                              int32_t* gene_out, float* score_out, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_rows_topk", what); };
    wgnn::error_clear();
    if (!rowptr || !col || !score || !gene_out || !score_out)
        return fail(WGNN_ERR_BAD_ARG, "rowptr, col, score, gene_out and score_out are required");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [0, 2^31)");
    if (k < 1 || k > 64) return fail(WGNN_ERR_UNSUPPORTED, "k must be in [1, 64]");
    if (flags & ~(uint32_t)WGNN_FLAG_ROWPTR_I64) return fail(WGNN_ERR_BAD_ARG, "only WGNN_FLAG_ROWPTR_I64 is a valid flag");
    if (n_rows == 0) return WGNN_OK;
    const long want = (n_rows + kTWaves - 1) / kTWaves;
    const unsigned nb = (unsigned)(want < kTMaxBlocks ? want : kTMaxBlocks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (flags & WGNN_FLAG_ROWPTR_I64)
        hipLaunchKernelGGL(rows_topk_kernel<long long>, dim3(nb), dim3(kTBlock), 0, st,
                           reinterpret_cast<const long long*>(rowptr), col, score, (long)n_rows, k, gene_out, score_out);
    else
        hipLaunchKernelGGL(rows_topk_kernel<int>, dim3(nb), dim3(kTBlock), 0, st,
                           reinterpret_cast<const int*>(rowptr), col, score, (long)n_rows, k, gene_out, score_out);
    return hipGetLastError() == hipSuccess ? WGNN_OK : fail(WGNN_ERR_LAUNCH, "HIP launch failed");
}
