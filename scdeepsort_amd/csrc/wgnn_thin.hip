// wgnn_thin.hip - wgnn_predict_rows_thin: one layer of wgnn_predict_rows for every (cell, draw) pair of a batch of RAW COUNTS, a
// draw being the cell re-sequenced at a share `keep` of its depth (api.ResidentPredictor.stability(thin="reads")).
//
// Every READ of the cell survives on its own: read i of the entry (cell, gene g, count c) is kept iff
// mix32(mix64(key(seed, cell, draw) + g * K_GENE) + i * K_READ) < T, c' = the kept reads of the entry; the cell's reads outside
// the bundle (rest[r]) are thinned the same way under g = n_genes.  The draw's library size is total' = sum c' + rest', its
// values v' = lognorm(c', total', scale) - THE function of wgnn_align_rows.h that wgnn_align_count_ln evaluates - and an entry
// takes part iff c' > 0 && v' > threshold.  The participating entries, in row order, are a row of wgnn_predict_rows: deg' =
// their number, S' = their f32 sum, the same weights, the same gather, the same fold, then the head, label rule and tallies of
// wgnn_predict_rows_dropout.  No thinned matrix is stored.  (include/wgnn.h has the definition.)
//
// Layout: one WORKGROUP per cell (grid-stride), its 8 waves take the draws d, d + 8, ... (as wgnn_predict_rows_dropout: a
// cell's draws re-read the same (col, raw) and table rows back to back, the head image is staged in LDS once).
// A draw runs in four sweeps of one wave:
//   1a  c' of every entry, 64 entries per step, and rest'.  The entries with c' > 0 are compacted (ballot + mbcnt) into the
//       wave's STASH in LDS as (gene, c'), and total' is the wave's sum.
//   1b  with total' known the stash is rewritten in place as (gene, v') of the participating entries (the threshold may drop
//       some: the write position never passes the read position).
//   1c  S' and deg' over the participating entries.
//   2   the weighted gather over them, then the epilogue.
// The hash costs O(reads), so 1a is the hot sweep and its result is what the stash keeps: sweeps 1b, 1c and 2 hash nothing.
// The arithmetic order is wgnn_predict_rows' order on the COMPACTED row - a lane sums the values at compacted positions lane,
// lane + 64, ..., lane group `sub` accumulates the positions sub, sub + NG, ... ascending - so a draw carries the bits
// wgnn_predict_rows leaves on the materialised draw, and at keep == 1 those of the lognorm-aligned batch.
//
// Stash: kTStash = 1024 (gene, value) pairs per wave, 8 KiB, 64 KiB per workgroup.  With a head image of at most 64 KiB and the
// 3 KiB of draw slots that is at most 131 KiB of the CU's 160 KiB, i.e. one workgroup of 8 waves per CU, two waves per SIMD.
// That occupancy is chosen on purpose: sweep 1a is bound by the hash's 64-bit integer arithmetic (two 64-bit multiplies per
// read), not by memory latency, and a second resident workgroup would need the stash halved - a cell with more than 512
// surviving genes (common at 10x depth) would then pay the hash three times, see below.  Reasoned from the instruction mix,
// not measured.  A chunk of 64 entries is stashed whole or not at all; from the first chunk that does not fit, the rest of
// the row is NOT stashed and sweeps 1c and 2 recompute its c' and v' (three hashes instead of one for that tail).  The tail's
// participating entries continue the compacted row where the stash ends: a cross-lane rotation puts the entry of compacted
// position p into lane p % 64, which keeps every lane's and every lane group's order of addition.
//
// Cooperative bound: kTCoop = 16.  An entry with c < 16 is thinned by its own lane (a loop of c hashes; a 64-entry step costs
// the largest such c, at most 15 rounds).  An entry with c >= 16, and rest, is thinned by the whole wave: 64 reads per round,
// ballot and popcount, ceil(c / 64) rounds plus a broadcast.  Counts are geometric: at 10x depth an entry >= 16 is rare (about
// one per 64-entry step), so the lane loop is bounded at a cost comparable to the one or two cooperative entries of the step,
// and a 70 000-read entry costs 1 094 rounds instead of stalling 63 lanes for 70 000.
//
// No atomics of any kind, vector stores only, one addition order whatever the grid: two launches are bit-identical.  The head
// / tally code below restates wgnn_stability.hip's on purpose: that file's kernel stays as it is.

#include <math.h>
#include "wgnn_resident_rows.h"
#include "wgnn_align_rows.h"

namespace {
using namespace wgnn;

constexpr int kTWaves = 8;                    // waves per workgroup = draws of one cell in flight
constexpr int kTBlock = 64 * kTWaves;
constexpr int kTMaxBlocks = 1024;             // grid-stride beyond that
constexpr int kTSlots = 256;                  // draws tallied per LDS round
constexpr int kTSlotBytes = kTSlots * 12;     // max_prob f32, label int32, empty int32
constexpr int kTStash = 1024;                 // (gene, value) pairs a wave keeps of one draw
constexpr int kTStashBytes = kTStash * 8;
constexpr unsigned kTCoop = 16;               // counts from here on, and rest, are thinned by the whole wave
constexpr unsigned long long kGene = 0xC2B2AE3D27D4EB4Full, kRead = 0xA0761D6478BD642Full;

struct TArgs {
    const void* rowptr; const int* col; const float* raw; long n_rows;
    const float* table; long ld_table; int n_genes; int H;
    const float* alpha; const float* bias;
    const float* self_rows; long ld_self;
    const long long* rest; double scale; float vthr;
    int n_draws; long long row0; long long draw0; unsigned long long seed; unsigned long long T;
    float* out; long ld_out;
    const float* w_head; const float* b_head; int C; float thr;
    int* votes; long ld_votes; int* unsure; int* empty; double* conf_sum;
    int* draw_label; float* draw_prob; int* draw_reads; int* draw_entries; int accumulate;
};

// orders this wave's LDS writes before its later reads (and reads before later writes): the stash is private to the wave
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// an entry's count as an integer; the caller promises integers in [1, 2^24], anything else counts as no read
__device__ __forceinline__ unsigned count_of(float x) { return x >= 1.f && x <= 16777216.f ? (unsigned)x : 0u; }

// kept reads among the c reads of the entry with key ek, by the whole wave (ek, c wave-uniform): the same value in every lane
__device__ __forceinline__ unsigned long long thin_wave(unsigned long long ek, unsigned long long c, unsigned long long T, int lane) {
    if (T >= (1ull << 32)) return c;                                               // keep == 1: every 32-bit hash is below T
    if (T == 0) return 0;
    unsigned long long n = 0;
    for (unsigned long long i0 = 0; i0 < c; i0 += 64) {
        const unsigned long long i = i0 + (unsigned long long)lane;
        const bool k = i < c && (unsigned long long)mix32(ek + i * kRead) < T;
        n += (unsigned long long)__popcll(__ballot(k));
    }
    return n;
}

// c' of this lane's entry (gene g, count c; c == 0 where the lane holds none).  All 64 lanes call it together.
__device__ __forceinline__ unsigned thin_entry(unsigned long long key, int g, unsigned c, unsigned long long T, int lane) {
    if (T >= (1ull << 32)) return c;                                               // wave-uniform
    if (T == 0) return 0u;
    const unsigned long long ek = mix64(key + (unsigned long long)(long long)g * kGene);
    unsigned kept = 0;
    if (c < kTCoop)
        for (unsigned i = 0; i < c; ++i) kept += (unsigned long long)mix32(ek + (unsigned long long)i * kRead) < T ? 1u : 0u;
    unsigned long long big = __ballot(c >= kTCoop);
    while (big) {                                                                  // wave-uniform
        const int src = __builtin_ctzll(big);
        big &= big - 1;
        const unsigned long long ek_s = (unsigned long long)__shfl((long long)ek, src, 64);
        const unsigned c_s = (unsigned)__shfl((int)c, src, 64);
        const unsigned n = (unsigned)thin_wave(ek_s, c_s, T, lane);
        if (lane == src) kept = n;
    }
    return kept;
}

// One draw's participating entries, handed to f(gene, value, on, p0) 64 lanes at a time in row order: `on` lanes hold an
// entry, their compacted positions are p0, p0 + 1, ... in lane order (p0 is a multiple of 64 for the stashed part, where the
// `on` lanes are the low ones).  First the stash's m entries, then - for a row that outgrew it - the entries from j_over on,
// whose c' and v' are computed again.  Lanes that are not `on` carry a valid gene id.  Returns the number of entries handed out.
template <typename F>
__device__ __forceinline__ int for_participating(const TArgs& a, const int* scol, const float* sval, int m, long j_over, long e,
                                                 unsigned long long key, double total, int lane, F&& f) {
    for (int q = 0; q < m; q += 64) {
        const int n = min(64, m - q);
        const int i = q + min(lane, n - 1);
        f(scol[i], sval[i], lane < n, q);
    }
    int p0 = m;
    for (long base = j_over; base < e; base += 64) {
        const long j = base + lane;
        const bool on = j < e;
        const int g = on ? a.col[j] : 0;
        const unsigned ck = thin_entry(key, g, on ? count_of(a.raw[j]) : 0u, a.T, lane);
        const float v = lognorm((float)ck, total, a.scale);
        const bool k = ck > 0 && v > a.vthr;
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
__global__ void __launch_bounds__(kTBlock) predict_rows_thin_kernel(const TArgs a) {
    extern __shared__ float4 s_mem4[];            // HEAD: [C, H] head image, the draw slots; then the waves' stashes
    char* s_base = reinterpret_cast<char*>(s_mem4);
    const float* s_head = reinterpret_cast<const float*>(s_base);
    float* s_prob = reinterpret_cast<float*>(s_base + (HEAD ? (size_t)a.C * a.H * sizeof(float) : 0));
    int* s_lab = reinterpret_cast<int*>(s_prob + kTSlots);
    int* s_emp = s_lab + kTSlots;
    constexpr int NG = 64 / LPR;                  // entries of one row processed side by side
    constexpr int U = 8;                          // table rows in flight per lane
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / LPR, l = lane % LPR;
    int* scol = reinterpret_cast<int*>(s_base + (HEAD ? (size_t)a.C * a.H * sizeof(float) + kTSlotBytes : 0) + (size_t)wave * kTStashBytes);
    float* sval = reinterpret_cast<float*>(scol + kTStash);
    const int c0 = l * 4;
    const bool col_on = c0 < a.H;
    if constexpr (HEAD) {
        const int n4 = a.C * a.H / 4;
        for (int i = threadIdx.x; i < n4; i += kTBlock) s_mem4[i] = ld4(a.w_head + 4 * i);
        __syncthreads();
    }
    const float a_self = a.alpha[a.n_genes + 1];
    const TPtr* rp = reinterpret_cast<const TPtr*>(a.rowptr);
    for (long r = blockIdx.x; r < a.n_rows; r += gridDim.x) {                  // block-uniform
        const long b = rp[r], e = rp[r + 1];
        const long long rest_in = a.rest[r];
        const unsigned long long rest_r = rest_in > 0 ? (unsigned long long)rest_in : 0ull;
        const unsigned long long ckey = a.seed ^ ((unsigned long long)(a.row0 + r) * 0x9FB21C651E98DF25ull);
        double csum = 0.0;                                                       // thread 0: the cell's running conf_sum
        if constexpr (HEAD) { if (threadIdx.x == 0 && a.accumulate) csum = a.conf_sum[r]; }
        for (int dc = 0; dc < a.n_draws; dc += kTSlots) {
            const int nd = min(kTSlots, a.n_draws - dc);
            for (int d = dc + wave; d < dc + nd; d += kTWaves) {                 // wave-uniform
                const unsigned long long key = ckey ^ ((unsigned long long)(a.draw0 + d) * 0xD6E8FEB86659FD93ull);
                const size_t o = (size_t)r * a.n_draws + d;                      // the pair's row in out / self_rows / draw_*
                // sweep 1a: c' of every entry, the surviving ones into the stash, total'
                unsigned long long tot = 0;
                int m = 0;
                long j_over = e;                                                 // first entry that is not stashed
                for (long base = b; base < e; base += 64) {
                    const long j = base + lane;
                    const bool on = j < e;
                    const int g = on ? a.col[j] : 0;
                    const unsigned ck = thin_entry(key, g, on ? count_of(a.raw[j]) : 0u, a.T, lane);
                    tot += ck;
                    const unsigned long long km = __ballot(ck > 0);
                    const int nk = __popcll(km);
                    if (j_over == e) {                                           // wave-uniform: still stashing
                        if (m + nk <= kTStash) {
                            if (ck > 0) { const int s = m + below(km); scol[s] = g; sval[s] = __builtin_bit_cast(float, ck); }
                            m += nk;
                        } else j_over = base;
                    }
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) tot += (unsigned long long)__shfl_xor((long long)tot, off, 64);
                tot += thin_wave(mix64(key + (unsigned long long)(long long)a.n_genes * kGene), rest_r, a.T, lane);
                const double total = (double)tot;
                wave_sync();
                // sweep 1b: the stash in place as (gene, v') of the participating entries
                if (tot == 0) { m = 0; j_over = e; }                             // nothing left: the empty row
                int mm = 0;
                for (int q = 0; q < m; q += 64) {
                    const bool on = q + lane < m;
                    const int g = on ? scol[q + lane] : 0;
                    const unsigned ck = on ? __builtin_bit_cast(unsigned, sval[q + lane]) : 0u;
                    const float v = lognorm((float)ck, total, a.scale);
                    const bool k = ck > 0 && v > a.vthr;
                    const unsigned long long km = __ballot(k);
                    wave_sync();                                                 // the chunk is read before its slots are reused
                    if (k) { const int s = mm + below(km); scol[s] = g; sval[s] = v; }
                    mm += __popcll(km);
                }
                m = mm;
                wave_sync();
                // sweep 1c: S' (a lane adds the values at compacted positions lane, lane + 64, ...; then a butterfly) and deg'
                float s = 0.f;
                const int cnt = for_participating(a, scol, sval, m, j_over, e, key, total, lane,
                    [&](int, float x, bool on, int p0) {
                        const unsigned long long km = __ballot(on);
                        const int dst = rotated_lane(on, km, __popcll(km), p0, lane);
                        s += __builtin_bit_cast(float, push_to_lane(dst, __builtin_bit_cast(int, on ? x : 0.f)));
                    });
                s = group_sum<64>(s);
                const float deg = (float)cnt;
                const bool s_ok = s != 0.f;
                const float self_coef = SELF_ROWS ? 0.f : a_self / (s + 1e-6f);
                // sweep 2: the weighted gather (predict_rows_kernel's, over the compacted row)
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                for_participating(a, scol, sval, m, j_over, e, key, total, lane,
                    [&](int cc, float x, bool on, int p0) {
                        float w = a.alpha[cc] * (deg * x / s);
                        if constexpr (!SELF_ROWS) w = fmaf(x, self_coef, w);
                        w = on && s_ok ? w : 0.f;
                        const unsigned long long km = __ballot(on);
                        const int nk = __popcll(km);
                        if (nk == 0) return;                                     // wave-uniform
                        const int dst = rotated_lane(on, km, nk, p0, lane);
                        cc = push_to_lane(dst, cc);
                        w = __builtin_bit_cast(float, push_to_lane(dst, __builtin_bit_cast(int, w)));
                        const int start = p0 & 63;                               // the entries sit in lanes start .. start + nk - 1 (mod 64)
                        const int g0 = start / NG * NG;
                        const int steps = (start - g0 + nk + NG - 1) / NG;
                        for (int j0 = 0; j0 < steps; j0 += U) {
                            float4 xv[U];
                            float wu[U];
#pragma unroll
                            for (int u = 0; u < U; ++u) {       // steps past the end re-read the last row with weight 0
                                const int j = min(j0 + u, steps - 1);
                                const int q = g0 + j * NG + sub;                 // position of this group's entry, before the wrap
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
                wave_sync();                                                     // the stash is read before the next draw rewrites it
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
                if (lane == 0) {
                    if (a.draw_reads) a.draw_reads[o] = (int)(tot < 0x7FFFFFFFull ? tot : 0x7FFFFFFFull);
                    if (a.draw_entries) a.draw_entries[o] = cnt;
                }
                if constexpr (!HEAD) {
                    if (sub == 0 && col_on) st4(a.out + o * a.ld_out + c0, h);
                } else {
                    // the head, softmax maximum and label of predict_rows_kernel, operation for operation
                    float mx = -INFINITY; int am = 0;
                    for (int j0 = 0; j0 < a.C; j0 += NG) {
                        const int j = j0 + sub;
                        float p = (j < a.C && col_on) ? dot4(h, *reinterpret_cast<const float4*>(s_head + (size_t)j * a.H + c0)) : 0.f;
                        p = group_sum<LPR>(p);
                        if (j < a.C) {
                            const float lj = p + a.b_head[j];
                            if (lj > mx) { mx = lj; am = j; }
                        }
                    }
                    group_argmax_fold<LPR>(mx, am);
                    float se = 0.f;
                    for (int j0 = 0; j0 < a.C; j0 += NG) {
                        const int j = j0 + sub;
                        float p = (j < a.C && col_on) ? dot4(h, *reinterpret_cast<const float4*>(s_head + (size_t)j * a.H + c0)) : 0.f;
                        p = group_sum<LPR>(p);
                        if (j < a.C) se += expf(p + a.b_head[j] - mx);
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
                for (int j = threadIdx.x; j < a.C + 2; j += kTBlock) {           // class j | unsure | empty: one owner each
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
int launch_one(const TArgs& a, hipStream_t st) {
    const unsigned nb = (unsigned)(a.n_rows < kTMaxBlocks ? a.n_rows : kTMaxBlocks);
    const size_t lds = (HEAD ? (size_t)a.C * a.H * sizeof(float) + kTSlotBytes : 0) + (size_t)kTWaves * kTStashBytes;
    auto fn = predict_rows_thin_kernel<LPR, HEAD, SELF_ROWS, TPtr>;
    if (lds > (size_t)kHeadLdsBytes &&                   // beyond the default window: ask for the larger one
        hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return WGNN_ERR_LAUNCH;
    hipLaunchKernelGGL(fn, dim3(nb), dim3(kTBlock), lds, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : WGNN_ERR_LAUNCH;
}

template <int LPR, bool HEAD, bool SELF_ROWS>
int launch_lpr(const TArgs& a, bool i64, hipStream_t st) {
    return i64 ? launch_one<LPR, HEAD, SELF_ROWS, long long>(a, st) : launch_one<LPR, HEAD, SELF_ROWS, int>(a, st);
}

}  // namespace

extern "C" int wgnn_predict_rows_thin(const void* rowptr, const int32_t* col, const float* raw, int64_t n_rows,
                                      const float* table, int64_t ld_table, int32_t n_genes, int32_t H,
                                      const float* alpha, const float* bias, const float* self_rows, int64_t ld_self,
                                      const int64_t* rest, double scale, float threshold,
                                      int32_t n_draws, int64_t row0, int32_t draw0, uint64_t seed, double keep,
                                      float* out, int64_t ld_out,
                                      const float* w_head, const float* b_head, int32_t n_classes, float unsure_threshold,
                                      int32_t* votes, int64_t ld_votes, int32_t* unsure, int32_t* empty, double* conf_sum,
                                      int32_t* draw_label, float* draw_prob, int32_t* draw_reads, int32_t* draw_entries,
                                      uint32_t flags, void* stream) {
    static const wgnn::DrawEntry entry{"wgnn_predict_rows_thin", WGNN_THIN_ACCUMULATE,
                                       "only WGNN_FLAG_ROWPTR_I64 and WGNN_THIN_ACCUMULATE are valid flags",
                                       "WGNN_THIN_ACCUMULATE needs a head"};
    const wgnn::DrawCall c{rowptr, col, raw, n_rows, table, ld_table, n_genes, H, alpha, bias, self_rows, ld_self,
                           n_draws, row0, draw0, seed, keep, out, ld_out, w_head, b_head, n_classes, unsure_threshold,
                           votes, ld_votes, unsure, empty, conf_sum, draw_label, draw_prob, flags};
    const wgnn::ThinCall thin{rest, scale, threshold, draw_reads, draw_entries};
    wgnn::error_clear();
    if (const int bad = wgnn::check_draw_call(entry, c, &thin)) return bad;
    if (n_rows == 0) return WGNN_OK;
    TArgs a{};
    wgnn::fill_draw_args(a, c, entry.accumulate);
    a.rest = reinterpret_cast<const long long*>(rest); a.scale = scale; a.vthr = threshold;
    a.draw_reads = draw_reads; a.draw_entries = draw_entries;
    const bool i64 = flags & WGNN_FLAG_ROWPTR_I64;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = wgnn::dispatch_rows(H, w_head != nullptr, self_rows != nullptr, [&](auto lpr, auto hd, auto sf) {
        return launch_lpr<decltype(lpr)::value, decltype(hd)::value, decltype(sf)::value>(a, i64, st);
    });
    return rc == WGNN_OK ? rc : wgnn::fail(rc, entry.fn, "HIP launch failed");
}
