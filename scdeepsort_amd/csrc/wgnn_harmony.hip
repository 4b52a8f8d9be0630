// wgnn_harmony.hip - the device half of ops.harmony_rows / api.ResidentPredictor.harmony: Harmony's soft clustering under a
// batch-diversity penalty and its per-cluster ridge correction (Korsunsky et al. 2019), with the block order a fixed stride
// (include/wgnn.h has the contracts, tests/harmony_reference.py restates them in numpy).  All float64.  Every product, sum,
// difference and quotient named there is rounded on its own - contraction into fused multiply-adds is switched off for the whole
// file - and every sum runs in an order that the data alone fixes: the grid never enters it, there is no atomic of any kind, and
// two calls give the same bits.
//
//   wgnn_harmony_scores        a workgroup per 64 cells, a lane per cell; the centres stream through LDS 64 at a time, the columns 32
//                              at a time, a thread keeps 16 running dot products (j ascending).  dist is written, the row maximum
//                              of -dist / sigma folded over the workgroup, and a second pass over the thread's own dist writes e.
//   wgnn_harmony_assign_block  a workgroup per 64 members of block q (cell i = q + m * n_blocks).  The products e * pen go through
//                              LDS 32 clusters at a time: ONE thread per member adds them, k ascending; the quotients are written
//                              to R and, still in LDS, added member by member into the chunk's [K, S] partial table.
//   wgnn_harmony_fold          one workgroup: T[q] from the chunk partials in chunk order, then O = sum of T without one block
//                              (q ascending), E = rowsum(O) * Pr (s ascending) and pen = pow((E + 1) / (O + 1), theta).
//   wgnn_weighted_group_reduce M[k, s, :] = sum of R[i, k] * X[i, :] over the rows of group s, n[k, s] = sum of R[i, k]: the group's
//                              rows ascending in chunks of 256, a chunk from +0.0 by one owner per (32 clusters, 64 columns),
//                              then a second kernel adds the chunk partials in chunk order.  S = 1 gives the centres.
//   wgnn_harmony_objective     a thread per row adds its three terms k ascending; 256 rows per chunk in row order, then the chunks.
//   wgnn_harmony_apply         Zc = Z0 - sum_k R[i, k] W[k, b_i, :] (k ascending) and U = Zc / sqrt(sum_j Zc_j^2) (j ascending).
#include <limits.h>
#include <math.h>
#include "wgnn_resident_rows.h"

#pragma clang fp contract(off)

namespace {
using namespace wgnn;

constexpr int kMaxK = WGNN_HARMONY_MAX_K;
constexpr int kMaxS = WGNN_HARMONY_MAX_BATCHES;
constexpr int kMaxD = WGNN_HARMONY_MAX_D;
constexpr int kMaxBlocks = WGNN_HARMONY_MAX_BLOCKS;
constexpr int kMaxGrid = 1 << 16;             // the largest grid_blocks an entry takes; 0 = chosen from the sizes
constexpr int kAutoGrid = 4096;               // ... and the most workgroups it chooses on its own (grid-stride beyond)
static_assert(kMaxK == 256 && kMaxS == 64, "the LDS tables below are sized for 256 clusters and 64 batches");

unsigned grid_of(int64_t want, int32_t grid_blocks) {
    const int64_t cap = grid_blocks > 0 ? grid_blocks : kAutoGrid;
    return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
}

// ------------------------------------------------------------------------------------------------------------------ scores
constexpr int kSRows = 64;                    // cells of a workgroup
constexpr int kSCols = 32;                    // columns of a slab
constexpr int kSPitch = kSCols + 1;           // doubles between two rows of a slab (odd: a column's 64 lanes spread over the banks)
constexpr int kSCentres = 64;                 // centres of a tile
constexpr int kSPer = kSCentres / 4;          // running dot products of a thread

struct ScArgs {
    const double* U; long ld_u; const double* Y; long ld_y; long n_rows; int D; int K; double sigma;
    double* dot; double* dist; double* e;
};

__global__ void __launch_bounds__(256) scores_kernel(const ScArgs a) {
    __shared__ double s_u[kSRows * kSPitch];
    __shared__ double s_y[kSCentres * kSPitch];
    __shared__ double s_m[4][kSRows];
    const int tid = threadIdx.x, cell = tid & 63, kg = tid >> 6;
    const long n_blocks = (a.n_rows + kSRows - 1) / kSRows;
    for (long rb = blockIdx.x; rb < n_blocks; rb += gridDim.x) {
        const long row0 = rb * kSRows, row = row0 + cell;
        double mx = -INFINITY;
        for (int k0 = 0; k0 < a.K; k0 += kSCentres) {
            double acc[kSPer];
#pragma unroll
            for (int kk = 0; kk < kSPer; ++kk) acc[kk] = 0.0;
            for (int j0 = 0; j0 < a.D; j0 += kSCols) {
                __syncthreads();                                   // the slab before this one has been read
#pragma unroll
                for (int u = 0; u < kSRows * kSCols / 256; ++u) {
                    const int el = u * 256 + tid, r = el >> 5, c = el & 31;
                    const bool in = j0 + c < a.D;
                    s_u[r * kSPitch + c] = (in && row0 + r < a.n_rows) ? a.U[(size_t)(row0 + r) * a.ld_u + j0 + c] : 0.0;
                    s_y[r * kSPitch + c] = (in && k0 + r < a.K) ? a.Y[(size_t)(k0 + r) * a.ld_y + j0 + c] : 0.0;
                }
                __syncthreads();
                const int jn = min(kSCols, a.D - j0);
                const double* mine = s_u + cell * kSPitch;
                const double* ys = s_y + kg * kSPer * kSPitch;     // wave-uniform: LDS broadcasts
                for (int j = 0; j < jn; ++j) {
                    const double u = mine[j];
#pragma unroll
                    for (int kk = 0; kk < kSPer; ++kk) acc[kk] = acc[kk] + u * ys[kk * kSPitch + j];
                }
            }
#pragma unroll
            for (int kk = 0; kk < kSPer; ++kk) {
                const int k = k0 + kg * kSPer + kk;
                if (row < a.n_rows && k < a.K) {
                    const size_t at = (size_t)row * a.K + k;
                    const double dist = 2.0 * (1.0 - acc[kk]);
                    if (a.dot) a.dot[at] = acc[kk];
                    a.dist[at] = dist;
                    mx = fmax(mx, -dist / a.sigma);
                }
            }
        }
        s_m[kg][cell] = mx;
        __syncthreads();
        mx = fmax(fmax(s_m[0][cell], s_m[1][cell]), fmax(s_m[2][cell], s_m[3][cell]));
        for (int k0 = 0; k0 < a.K; k0 += kSCentres)
            for (int kk = 0; kk < kSPer; ++kk) {
                const int k = k0 + kg * kSPer + kk;
                if (row < a.n_rows && k < a.K) {                   // the thread's own dist
                    const size_t at = (size_t)row * a.K + k;
                    a.e[at] = exp(-a.dist[at] / a.sigma - mx);
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------------------ assign, fold
constexpr int kAChunk = WGNN_HARMONY_T_CHUNK; // members per partial table: part of T's addition order, never tuned per device
constexpr int kAK = 32;                       // clusters of a tile
constexpr int kAPitch = kAK + 1;
static_assert(kAChunk == 64, "a thread per member of a chunk: the first wavefront");

int64_t block_members(int64_t n_rows, int32_t n_blocks, int32_t q) { return q < n_rows ? (n_rows - q + n_blocks - 1) / n_blocks : 0; }
int64_t block_chunks(int64_t n_rows, int32_t n_blocks, int32_t q) { return (block_members(n_rows, n_blocks, q) + kAChunk - 1) / kAChunk; }
int64_t assign_bytes(int64_t n_rows, int32_t K, int32_t S, int32_t n_blocks) {       // block 0 is the largest
    return block_chunks(n_rows, n_blocks, 0) * (int64_t)K * S * 8;
}

struct AArgs {
    const double* e; const int* batch; const double* pen; long n_rows; int K; int S; int n_blocks; int q;
    double* R; double* part; long members; long n_chunks;
};

__global__ void __launch_bounds__(256) assign_kernel(const AArgs a) {
    __shared__ double s_t[kAChunk * kAPitch];
    __shared__ double s_acc[kMaxS * kAK];                          // [s][kk]
    __shared__ double s_sum[kAChunk];
    __shared__ long s_i[kAChunk];
    __shared__ int s_b[kAChunk];
    const int tid = threadIdx.x;
    for (long c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        __syncthreads();                                           // the chunk before this one is done with LDS
        if (tid < kAChunk) {
            const long m = c * kAChunk + tid;
            const long i = m < a.members ? a.q + m * a.n_blocks : -1;
            const bool ok = i >= 0 && i < a.n_rows;
            const int b = ok ? a.batch[i] : -1;
            s_i[tid] = ok ? i : -1;
            s_b[tid] = (unsigned)b < (unsigned)a.S ? b : -1;       // a batch id out of range: pen = 1, no part in T (ops refuses them)
            s_sum[tid] = 0.0;
        }
        __syncthreads();
        const int cnt = (int)min((long)kAChunk, a.members - c * kAChunk);
        // t = e * pen of 64 members x 32 clusters into LDS; `second`: divided by the member's sum, and written to R
        auto stage = [&](int k0, bool second) {
#pragma unroll
            for (int u = 0; u < kAChunk * kAK / 256; ++u) {
                const int el = u * 256 + tid, m = el >> 5, kk = el & 31, k = k0 + kk;
                const long i = s_i[m];
                double t = 0.0;
                if (i >= 0 && k < a.K) {
                    t = a.e[(size_t)i * a.K + k];
                    const int b = s_b[m];
                    if (a.pen && b >= 0) t = t * a.pen[(size_t)k * a.S + b];
                    if (second) {
                        t = t / s_sum[m];
                        a.R[(size_t)i * a.K + k] = t;
                    }
                }
                s_t[m * kAPitch + kk] = t;
            }
        };
        for (int k0 = 0; k0 < a.K; k0 += kAK) {
            stage(k0, false);
            __syncthreads();
            if (tid < kAChunk) {
                const int kn = min(kAK, a.K - k0);
                double sum = s_sum[tid];
                for (int kk = 0; kk < kn; ++kk) sum = sum + s_t[tid * kAPitch + kk];
                s_sum[tid] = sum;
            }
            __syncthreads();
        }
        for (int k0 = 0; k0 < a.K; k0 += kAK) {
            for (int idx = tid; idx < kAK * a.S; idx += 256) s_acc[idx] = 0.0;
            stage(k0, true);
            __syncthreads();
            if (tid < kAK && k0 + tid < a.K)
                for (int m = 0; m < cnt; ++m) {
                    const int b = s_b[m];
                    if (b >= 0) s_acc[b * kAK + tid] = s_acc[b * kAK + tid] + s_t[m * kAPitch + tid];
                }
            __syncthreads();
            for (int idx = tid; idx < kAK * a.S; idx += 256) {
                const int kk = idx / a.S, s = idx % a.S, k = k0 + kk;
                if (k < a.K) a.part[((size_t)c * a.K + k) * a.S + s] = s_acc[s * kAK + kk];
            }
            __syncthreads();                                       // s_acc is zeroed again
        }
    }
}

struct FArgs {
    const double* part; long n_chunks; double* T; const double* Pr; const double* theta; int K; int S; int n_blocks;
    int q_store; int q_skip; double* O; double* E; double* pen;
};

__global__ void __launch_bounds__(256) fold_kernel(const FArgs a) {
    __shared__ double s_rs[kMaxK];
    const int tid = threadIdx.x;
    const int KS = a.K * a.S;
    for (int idx = tid; idx < KS; idx += 256) {
        if (a.q_store >= 0) {
            double sum = 0.0;
            for (long c = 0; c < a.n_chunks; ++c) sum = sum + a.part[(size_t)c * KS + idx];
            a.T[(size_t)a.q_store * KS + idx] = sum;
        }
        double o = 0.0;
        for (int q = 0; q < a.n_blocks; ++q)
            if (q != a.q_skip) o = o + a.T[(size_t)q * KS + idx];  // T[q_store][idx] is this thread's own write
        a.O[idx] = o;
    }
    __syncthreads();
    for (int k = tid; k < a.K; k += 256) {
        double rs = 0.0;
        for (int s = 0; s < a.S; ++s) rs = rs + a.O[(size_t)k * a.S + s];
        s_rs[k] = rs;
    }
    __syncthreads();
    for (int idx = tid; idx < KS; idx += 256) {
        const int k = idx / a.S, s = idx % a.S;
        const double ev = s_rs[k] * a.Pr[s];
        a.E[idx] = ev;
        if (a.pen) a.pen[idx] = pow((ev + 1.0) / (a.O[idx] + 1.0), a.theta[s]);
    }
}

// --------------------------------------------------------------------------------------------------- weighted grouped reduce
constexpr int kWChunk = WGNN_HARMONY_W_CHUNK; // members per chunk: part of the sum's addition order, never tuned per device
constexpr int kWSub = 32;                     // members staged in LDS at a time
constexpr int kWK = 32;                       // clusters of an owner
constexpr int kWD = 64;                       // columns of an owner
constexpr int kWPer = kWK / 4;

struct WArgs {
    const double* X; long ld; const double* R; const int* order; const long long* seg;
    long n_rows; int D; int K; int S; long n_slots; int n_kb; int n_db;
    double* dpart; double* wpart;             // [n_slots][K][D] a chunk's moments, [n_slots][K] its weights
    double* M; double* n;
};

// seg_ptr[s] clamped into [0, n_rows]: a malformed seg_ptr reads no position outside `order` and no slot outside the workspace
__device__ __forceinline__ long wseg_at(const WArgs& a, long s) {
    const long v = a.seg[s];
    return v < 0 ? 0 : (v > a.n_rows ? a.n_rows : v);
}
// chunk w of the workspace belongs to the group s with slot(s) <= w < slot(s + 1) (wgnn_kmeans.hip's scheme)
__device__ __forceinline__ long wslot_at(const WArgs& a, long s) { return wseg_at(a, s) / kWChunk + s; }

__global__ void __launch_bounds__(256) wgr_chunk_kernel(const WArgs a) {
    __shared__ double s_x[kWSub * kWD];
    __shared__ double s_r[kWSub * kWK];
    __shared__ int s_row[kWSub];
    const int tid = threadIdx.x, d = tid & 63, kq = tid >> 6;
    const long per = (long)a.n_kb * a.n_db, total = a.n_slots * per;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {                  // workgroup-uniform
        const long w = item / per;
        const int kb = (int)((item % per) / a.n_db), db = (int)(item % a.n_db);
        if (wslot_at(a, 0) > w) continue;
        long lo = 0, hi = a.S;                                     // the largest s in [0, S] with slot(s) <= w
        while (lo < hi) {
            const long mid = lo + (hi - lo + 1) / 2;
            if (wslot_at(a, mid) <= w) lo = mid; else hi = mid - 1;
        }
        if (lo >= a.S) continue;
        const long c0 = wseg_at(a, lo) + (w - wslot_at(a, lo)) * kWChunk, end = wseg_at(a, lo + 1);
        if (c0 >= end) continue;                                   // a slot the group does not need
        const int cnt = (int)min((long)kWChunk, end - c0);
        double acc[kWPer];
#pragma unroll
        for (int kk = 0; kk < kWPer; ++kk) acc[kk] = 0.0;
        double wacc = 0.0;
        for (int m0 = 0; m0 < cnt; m0 += kWSub) {
            const int mn = min(kWSub, cnt - m0);
            __syncthreads();                                       // the members before these have been read
            if (tid < kWSub) {
                int r = tid < mn ? a.order[c0 + m0 + tid] : -1;
                if ((unsigned long)(long)r >= (unsigned long)a.n_rows) r = -1;       // takes no part
                s_row[tid] = r;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kWSub * kWD / 256; ++u) {
                const int el = u * 256 + tid, m = el >> 6, c = el & 63, col = db * kWD + c, r = s_row[m];
                s_x[el] = (r >= 0 && col < a.D) ? a.X[(size_t)r * a.ld + col] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kWSub * kWK / 256; ++u) {
                const int el = u * 256 + tid, m = el >> 5, k = kb * kWK + (el & 31), r = s_row[m];
                s_r[el] = (r >= 0 && k < a.K) ? a.R[(size_t)r * a.K + k] : 0.0;
            }
            __syncthreads();
            for (int m = 0; m < mn; ++m) {
                if (s_row[m] < 0) continue;
                const double x = s_x[m * kWD + d];
                const double* rs = s_r + m * kWK + kq * kWPer;     // wave-uniform: LDS broadcasts
#pragma unroll
                for (int kk = 0; kk < kWPer; ++kk) acc[kk] = acc[kk] + rs[kk] * x;
            }
            if (db == 0 && tid < kWK)
                for (int m = 0; m < mn; ++m)
                    if (s_row[m] >= 0) wacc = wacc + s_r[m * kWK + tid];
        }
        const int col = db * kWD + d;
#pragma unroll
        for (int kk = 0; kk < kWPer; ++kk) {
            const int k = kb * kWK + kq * kWPer + kk;
            if (k < a.K && col < a.D) a.dpart[((size_t)w * a.K + k) * a.D + col] = acc[kk];
        }
        if (db == 0 && tid < kWK && kb * kWK + tid < a.K) a.wpart[(size_t)w * a.K + kb * kWK + tid] = wacc;
    }
}

// one thread per output element: a group's chunk partials in ascending chunk order
__global__ void __launch_bounds__(256) wgr_finish_kernel(const WArgs a) {
    const long per = (long)a.D + 1, total = (long)a.K * a.S * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long ks = i / per;
        const int j = (int)(i % per);
        const long k = ks / a.S, s = ks % a.S;
        const long b = wseg_at(a, s), e = wseg_at(a, s + 1), first = wslot_at(a, s);
        long chunks = e > b ? (e - b + kWChunk - 1) / kWChunk : 0;
        if (first + chunks > a.n_slots) chunks = first < a.n_slots ? a.n_slots - first : 0;      // malformed seg_ptr only
        double sum = 0.0;
        if (j < a.D) {
            for (long c = 0; c < chunks; ++c) sum = sum + a.dpart[((size_t)(first + c) * a.K + k) * a.D + j];
            a.M[(size_t)ks * a.D + j] = sum;
        } else {
            for (long c = 0; c < chunks; ++c) sum = sum + a.wpart[(size_t)(first + c) * a.K + k];
            a.n[ks] = sum;
        }
    }
}

int64_t wgr_slots(int64_t n_rows, int32_t S) { return n_rows / kWChunk + S; }
int64_t wgr_bytes(int64_t n_rows, int32_t K, int32_t S, int32_t D) { return wgr_slots(n_rows, S) * (int64_t)K * ((int64_t)D + 1) * 8; }

// ---------------------------------------------------------------------------------------------------------------- objective
constexpr int kOChunk = WGNN_HARMONY_OBJ_CHUNK;   // rows per partial: part of the sum's addition order
static_assert(kOChunk == 256, "a thread per row of a chunk");

struct OArgs {
    const double* R; const double* dist; const int* batch; const double* O; const double* E; const double* theta;
    long n_rows; int K; int S; double sigma; double* out; double* part; long n_chunks;
};

__global__ void __launch_bounds__(kOChunk) objective_chunk_kernel(const OArgs a) {
    __shared__ double s_v[3][kOChunk];
    const int tid = threadIdx.x;
    for (long c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        const long row = c * kOChunk + tid;
        double va = 0.0, vb = 0.0, vc = 0.0;
        const int b = row < a.n_rows ? a.batch[row] : -1;
        if ((unsigned)b < (unsigned)a.S) {                         // a batch id out of range takes no part (ops refuses them)
            const double th = a.theta[b];
            const double* r_ = a.R + (size_t)row * a.K;
            const double* d_ = a.dist + (size_t)row * a.K;
            for (int k = 0; k < a.K; ++k) {
                const double r = r_[k];
                const size_t at = (size_t)k * a.S + b;
                va = va + r * d_[k];
                vb = vb + (r > 0.0 ? r * log(r) : 0.0);
                vc = vc + r * (th * log((a.O[at] + 1.0) / (a.E[at] + 1.0)));
            }
        }
        __syncthreads();                                           // the chunk before this one has been added
        s_v[0][tid] = va; s_v[1][tid] = vb; s_v[2][tid] = vc;
        __syncthreads();
        if (tid < 3) {
            double acc = 0.0;
#pragma unroll 16
            for (int i = 0; i < kOChunk; ++i) acc = acc + s_v[tid][i];
            a.part[(size_t)c * 3 + tid] = acc;
        }
    }
}

__global__ void __launch_bounds__(64) objective_finish_kernel(const OArgs a) {
    __shared__ double s_t[3];
    const int tid = threadIdx.x;
    if (tid < 3) {
        double acc = 0.0;
        for (long c = 0; c < a.n_chunks; ++c) acc = acc + a.part[(size_t)c * 3 + tid];
        s_t[tid] = acc;
        a.out[1 + tid] = acc;
    }
    __syncthreads();
    if (tid == 0) a.out[0] = (s_t[0] + a.sigma * s_t[1]) + a.sigma * s_t[2];
}

// -------------------------------------------------------------------------------------------------------------------- apply
constexpr int kPRows = 64;                    // rows of a workgroup: 16 per wavefront, then a thread per row for the norm

struct PArgs {
    const double* Z0; long ld_z; const double* R; const double* W; const int* batch; long n_rows; int D; int K; int S;
    double* Zc; double* U;
};

__global__ void __launch_bounds__(256) apply_kernel(const PArgs a) {
    __shared__ double s_norm[kPRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long n_blocks = (a.n_rows + kPRows - 1) / kPRows;
    for (long rb = blockIdx.x; rb < n_blocks; rb += gridDim.x) {
        const long row0 = rb * kPRows;
        if (a.R)
            for (int rr = 0; rr < kPRows / 4; ++rr) {
                const long row = row0 + wave * (kPRows / 4) + rr;
                if (row >= a.n_rows) break;                        // wave-uniform
                const int b = a.batch[row];
                const bool ok = (unsigned)b < (unsigned)a.S;       // a batch id out of range: no correction (ops refuses them)
                const double* r_ = a.R + (size_t)row * a.K;
                for (int j = lane; j < a.D; j += 64) {
                    double acc = 0.0;
                    if (ok)
                        for (int k = 0; k < a.K; ++k) acc = acc + r_[k] * a.W[((size_t)k * a.S + b) * a.D + j];
                    a.Zc[(size_t)row * a.D + j] = a.Z0[(size_t)row * a.ld_z + j] - acc;
                }
            }
        __syncthreads();                                           // Zc of these rows is written; s_norm has been read
        if (tid < kPRows && row0 + tid < a.n_rows) {
            const double* src = a.R ? a.Zc + (size_t)(row0 + tid) * a.D : a.Z0 + (size_t)(row0 + tid) * a.ld_z;
            double ss = 0.0;
            for (int j = 0; j < a.D; ++j) {
                const double v = src[j];
                ss = ss + v * v;
            }
            s_norm[tid] = sqrt(ss);
        }
        __syncthreads();
        for (int rr = 0; rr < kPRows / 4; ++rr) {
            const int local = wave * (kPRows / 4) + rr;
            const long row = row0 + local;
            if (row >= a.n_rows) break;
            const double* src = a.R ? a.Zc + (size_t)row * a.D : a.Z0 + (size_t)row * a.ld_z;
            const double nv = s_norm[local];
            for (int j = lane; j < a.D; j += 64) a.U[(size_t)row * a.D + j] = src[j] / nv;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- checks
const char* check_sizes(int64_t n_rows, int32_t K, int32_t S, int* code) {
    *code = WGNN_ERR_BAD_ARG;
    if (n_rows < 1 || n_rows > INT32_MAX) return "n_rows must be in [1, 2^31)";
    *code = WGNN_ERR_UNSUPPORTED;
    if (K < 1 || K > kMaxK) return "K must be in [1, 256]";
    if (S < 1 || S > kMaxS) return "S must be in [1, 64]";
    return nullptr;
}
const char* check_d(int32_t D, int* code) {
    *code = WGNN_ERR_UNSUPPORTED;
    if (D < 1 || D > kMaxD) return "D must be in [1, 1024]";
    return nullptr;
}
const char* check_blocks(int32_t n_blocks, int* code) {
    *code = WGNN_ERR_UNSUPPORTED;
    if (n_blocks < 1 || n_blocks > kMaxBlocks) return "n_blocks must be in [1, 64]";
    return nullptr;
}
const char* check_grid(int32_t grid_blocks, uint32_t flags, int* code) {
    *code = WGNN_ERR_BAD_ARG;
    if (flags) return "no flag is defined for this entry (flags must be 0)";
    if (grid_blocks < 0 || grid_blocks > kMaxGrid) return "grid_blocks must be in [0, 65536] (0 = chosen from the sizes)";
    return nullptr;
}
int launched(const char* fn) { return hipGetLastError() == hipSuccess ? WGNN_OK : wgnn::fail(WGNN_ERR_LAUNCH, fn, "HIP launch failed"); }

}  // namespace

#define WGNN_CHECK(expr) do { int code_ = 0; if (const char* what_ = (expr)) return fail(code_, what_); } while (0)
#define WGNN_ENTRY(name)                                                                                             \
    auto fail = [](int code, const char* what) { return wgnn::fail(code, name, what); };                            \
    wgnn::error_clear()

extern "C" int wgnn_harmony_scores(const double* U, int64_t ld_u, const double* Y, int64_t ld_y, int64_t n_rows, int32_t D,
                                   int32_t K, double sigma, double* dot, double* dist, double* e, uint32_t flags,
                                   void* stream) {
    WGNN_ENTRY("wgnn_harmony_scores");
    int code_ = 0;
    if (const char* what = check_sizes(n_rows, K, 1, &code_)) return fail(code_, what);
    if (const char* what = check_d(D, &code_)) return fail(code_, what);
    if (const char* what = check_grid(0, flags, &code_)) return fail(code_, what);
    if (!(sigma > 0.0 && sigma < HUGE_VAL)) return fail(WGNN_ERR_BAD_ARG, "sigma must be positive and finite");
    if (!U || !Y || !dist || !e) return fail(WGNN_ERR_BAD_ARG, "U, Y, dist and e are required");
    if (ld_u < D || ld_y < D) return fail(WGNN_ERR_BAD_ARG, "ld_u and ld_y must be >= D");
    if (!aligned8(U) || !aligned8(Y) || !aligned8(dot) || !aligned8(dist) || !aligned8(e))
        return fail(WGNN_ERR_ALIGNMENT, "U, Y, dot, dist and e must be 8-byte aligned");
    ScArgs a{U, ld_u, Y, ld_y, n_rows, D, K, sigma, dot, dist, e};
    hipLaunchKernelGGL(scores_kernel, dim3(grid_of((n_rows + kSRows - 1) / kSRows, 0)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return launched("wgnn_harmony_scores");
}

extern "C" int wgnn_harmony_assign_workspace_bytes(int64_t n_rows, int32_t K, int32_t S, int32_t n_blocks, int64_t* bytes) {
    WGNN_ENTRY("wgnn_harmony_assign_workspace_bytes");
    if (!bytes) return fail(WGNN_ERR_BAD_ARG, "bytes is required");
    int code_ = 0;
    if (const char* what = check_sizes(n_rows, K, S, &code_)) return fail(code_, what);
    if (const char* what = check_blocks(n_blocks, &code_)) return fail(code_, what);
    *bytes = assign_bytes(n_rows, K, S, n_blocks);
    return WGNN_OK;
}

extern "C" int wgnn_harmony_assign_block(const double* e, const int32_t* batch, const double* pen, int64_t n_rows, int32_t K,
                                         int32_t S, int32_t n_blocks, int32_t q, double* R, void* workspace,
                                         int64_t workspace_bytes, int32_t grid_blocks, uint32_t flags, void* stream) {
    WGNN_ENTRY("wgnn_harmony_assign_block");
    int code_ = 0;
    if (const char* what = check_sizes(n_rows, K, S, &code_)) return fail(code_, what);
    if (const char* what = check_blocks(n_blocks, &code_)) return fail(code_, what);
    if (const char* what = check_grid(grid_blocks, flags, &code_)) return fail(code_, what);
    if (q < 0 || q >= n_blocks) return fail(WGNN_ERR_BAD_ARG, "q must be in [0, n_blocks)");
    if (!e || !batch || !R) return fail(WGNN_ERR_BAD_ARG, "e, batch and R are required");
    if (!aligned8(e) || !aligned8(pen) || !aligned8(R)) return fail(WGNN_ERR_ALIGNMENT, "e, pen and R must be 8-byte aligned");
    if (!aligned4(batch)) return fail(WGNN_ERR_ALIGNMENT, "batch must be 4-byte aligned");
    if (workspace_bytes < 0) return fail(WGNN_ERR_WORKSPACE, "workspace_bytes is negative");
    if (!workspace || workspace_bytes < assign_bytes(n_rows, K, S, n_blocks))
        return fail(WGNN_ERR_WORKSPACE, "workspace is missing or smaller than wgnn_harmony_assign_workspace_bytes asks for");
    if (!aligned8(workspace)) return fail(WGNN_ERR_ALIGNMENT, "workspace must be 8-byte aligned");
    AArgs a{e, batch, pen, n_rows, K, S, n_blocks, q, R, static_cast<double*>(workspace), block_members(n_rows, n_blocks, q),
            block_chunks(n_rows, n_blocks, q)};
    if (a.n_chunks == 0) return WGNN_OK;                           // an empty block: nothing to assign, the fold adds no chunk
    hipLaunchKernelGGL(assign_kernel, dim3(grid_of(a.n_chunks, grid_blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return launched("wgnn_harmony_assign_block");
}

extern "C" int wgnn_harmony_fold(const void* workspace, int64_t workspace_bytes, int64_t n_rows, double* T, const double* Pr,
                                 const double* theta, int32_t K, int32_t S, int32_t n_blocks, int32_t q_store, int32_t q_skip,
                                 double* O, double* E, double* pen, uint32_t flags, void* stream) {
    WGNN_ENTRY("wgnn_harmony_fold");
    int code_ = 0;
    if (const char* what = check_sizes(n_rows, K, S, &code_)) return fail(code_, what);
    if (const char* what = check_blocks(n_blocks, &code_)) return fail(code_, what);
    if (const char* what = check_grid(0, flags, &code_)) return fail(code_, what);
    if (q_store < -1 || q_store >= n_blocks || q_skip < -1 || q_skip >= n_blocks)
        return fail(WGNN_ERR_BAD_ARG, "q_store and q_skip must be in [-1, n_blocks) (-1 = none)");
    if (!T || !Pr || !O || !E) return fail(WGNN_ERR_BAD_ARG, "T, Pr, O and E are required");
    if (pen && !theta) return fail(WGNN_ERR_BAD_ARG, "pen needs theta");
    if (!aligned8(T) || !aligned8(Pr) || !aligned8(theta) || !aligned8(O) || !aligned8(E) || !aligned8(pen))
        return fail(WGNN_ERR_ALIGNMENT, "T, Pr, theta, O, E and pen must be 8-byte aligned");
    if (q_store >= 0) {
        if (workspace_bytes < 0) return fail(WGNN_ERR_WORKSPACE, "workspace_bytes is negative");
        if (!workspace || workspace_bytes < assign_bytes(n_rows, K, S, n_blocks))
            return fail(WGNN_ERR_WORKSPACE, "workspace is missing or smaller than wgnn_harmony_assign_workspace_bytes asks for");
        if (!aligned8(workspace)) return fail(WGNN_ERR_ALIGNMENT, "workspace must be 8-byte aligned");
    }
    FArgs a{static_cast<const double*>(workspace), q_store >= 0 ? block_chunks(n_rows, n_blocks, q_store) : 0, T, Pr, theta, K, S,
            n_blocks, q_store, q_skip, O, E, pen};
    hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return launched("wgnn_harmony_fold");
}

extern "C" int wgnn_weighted_group_reduce_workspace_bytes(int64_t n_rows, int32_t K, int32_t S, int32_t D, int64_t* bytes) {
    WGNN_ENTRY("wgnn_weighted_group_reduce_workspace_bytes");
    if (!bytes) return fail(WGNN_ERR_BAD_ARG, "bytes is required");
    int code_ = 0;
    if (const char* what = check_sizes(n_rows, K, S, &code_)) return fail(code_, what);
    if (const char* what = check_d(D, &code_)) return fail(code_, what);
    *bytes = wgr_bytes(n_rows, K, S, D);
    return WGNN_OK;
}

extern "C" int wgnn_weighted_group_reduce(const double* X, int64_t ld_x, const double* R, const int32_t* order,
                                          const void* seg_ptr, int64_t n_rows, int32_t D, int32_t K, int32_t S, double* M,
                                          double* n, void* workspace, int64_t workspace_bytes, int32_t grid_blocks,
                                          uint32_t flags, void* stream) {
    WGNN_ENTRY("wgnn_weighted_group_reduce");
    int code_ = 0;
    if (const char* what = check_sizes(n_rows, K, S, &code_)) return fail(code_, what);
    if (const char* what = check_d(D, &code_)) return fail(code_, what);
    if (const char* what = check_grid(grid_blocks, flags, &code_)) return fail(code_, what);
    if (!X || !R || !order || !seg_ptr || !M || !n) return fail(WGNN_ERR_BAD_ARG, "X, R, order, seg_ptr, M and n are required");
    if (ld_x < D) return fail(WGNN_ERR_BAD_ARG, "ld_x must be >= D");
    if (!aligned8(X) || !aligned8(R) || !aligned8(seg_ptr) || !aligned8(M) || !aligned8(n))
        return fail(WGNN_ERR_ALIGNMENT, "X, R, seg_ptr, M and n must be 8-byte aligned");
    if (!aligned4(order)) return fail(WGNN_ERR_ALIGNMENT, "order must be 4-byte aligned");
    if (workspace_bytes < 0) return fail(WGNN_ERR_WORKSPACE, "workspace_bytes is negative");
    if (!workspace || workspace_bytes < wgr_bytes(n_rows, K, S, D))
        return fail(WGNN_ERR_WORKSPACE, "workspace is missing or smaller than wgnn_weighted_group_reduce_workspace_bytes asks for");
    if (!aligned8(workspace)) return fail(WGNN_ERR_ALIGNMENT, "workspace must be 8-byte aligned");
    WArgs a{};
    a.X = X; a.ld = ld_x; a.R = R; a.order = order; a.seg = static_cast<const long long*>(seg_ptr);
    a.n_rows = n_rows; a.D = D; a.K = K; a.S = S; a.n_slots = wgr_slots(n_rows, S);
    a.n_kb = (K + kWK - 1) / kWK; a.n_db = (D + kWD - 1) / kWD;
    a.dpart = static_cast<double*>(workspace);
    a.wpart = a.dpart + a.n_slots * (int64_t)K * D;
    a.M = M; a.n = n;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(wgr_chunk_kernel, dim3(grid_of(a.n_slots * a.n_kb * a.n_db, grid_blocks)), dim3(256), 0, st, a);
    if (hipGetLastError() != hipSuccess) return fail(WGNN_ERR_LAUNCH, "HIP launch failed");
    hipLaunchKernelGGL(wgr_finish_kernel, dim3(grid_of(((int64_t)K * S * (D + 1) + 255) / 256, grid_blocks)), dim3(256), 0, st, a);
    return launched("wgnn_weighted_group_reduce");
}

extern "C" int wgnn_harmony_objective_workspace_bytes(int64_t n_rows, int64_t* bytes) {
    WGNN_ENTRY("wgnn_harmony_objective_workspace_bytes");
    if (!bytes) return fail(WGNN_ERR_BAD_ARG, "bytes is required");
    if (n_rows < 1 || n_rows > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [1, 2^31)");
    *bytes = (n_rows + kOChunk - 1) / kOChunk * 24;
    return WGNN_OK;
}

extern "C" int wgnn_harmony_objective(const double* R, const double* dist, const int32_t* batch, const double* O,
                                      const double* E, const double* theta, int64_t n_rows, int32_t K, int32_t S, double sigma,
                                      double* out, void* workspace, int64_t workspace_bytes, uint32_t flags, void* stream) {
    WGNN_ENTRY("wgnn_harmony_objective");
    int code_ = 0;
    if (const char* what = check_sizes(n_rows, K, S, &code_)) return fail(code_, what);
    if (const char* what = check_grid(0, flags, &code_)) return fail(code_, what);
    if (!(sigma > 0.0 && sigma < HUGE_VAL)) return fail(WGNN_ERR_BAD_ARG, "sigma must be positive and finite");
    if (!R || !dist || !batch || !O || !E || !theta || !out)
        return fail(WGNN_ERR_BAD_ARG, "R, dist, batch, O, E, theta and out are required");
    if (!aligned8(R) || !aligned8(dist) || !aligned8(O) || !aligned8(E) || !aligned8(theta) || !aligned8(out))
        return fail(WGNN_ERR_ALIGNMENT, "R, dist, O, E, theta and out must be 8-byte aligned");
    if (!aligned4(batch)) return fail(WGNN_ERR_ALIGNMENT, "batch must be 4-byte aligned");
    const int64_t n_chunks = (n_rows + kOChunk - 1) / kOChunk;
    if (workspace_bytes < 0) return fail(WGNN_ERR_WORKSPACE, "workspace_bytes is negative");
    if (!workspace || workspace_bytes < n_chunks * 24)
        return fail(WGNN_ERR_WORKSPACE, "workspace is missing or smaller than wgnn_harmony_objective_workspace_bytes asks for");
    if (!aligned8(workspace)) return fail(WGNN_ERR_ALIGNMENT, "workspace must be 8-byte aligned");
    OArgs a{R, dist, batch, O, E, theta, n_rows, K, S, sigma, out, static_cast<double*>(workspace), n_chunks};
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(objective_chunk_kernel, dim3(grid_of(n_chunks, 0)), dim3(kOChunk), 0, st, a);
    if (hipGetLastError() != hipSuccess) return fail(WGNN_ERR_LAUNCH, "HIP launch failed");
    hipLaunchKernelGGL(objective_finish_kernel, dim3(1), dim3(64), 0, st, a);
    return launched("wgnn_harmony_objective");
}

extern "C" int wgnn_harmony_apply(const double* Z0, int64_t ld_z, const double* R, const double* W, const int32_t* batch,
                                  int64_t n_rows, int32_t D, int32_t K, int32_t S, double* Zc, double* U, int32_t grid_blocks,
                                  uint32_t flags, void* stream) {
    WGNN_ENTRY("wgnn_harmony_apply");
    int code_ = 0;
    if (const char* what = check_sizes(n_rows, R ? K : 1, R ? S : 1, &code_)) return fail(code_, what);
    if (const char* what = check_d(D, &code_)) return fail(code_, what);
    if (const char* what = check_grid(grid_blocks, flags, &code_)) return fail(code_, what);
    if (!Z0 || !U) return fail(WGNN_ERR_BAD_ARG, "Z0 and U are required");
    if (R && (!W || !batch || !Zc)) return fail(WGNN_ERR_BAD_ARG, "with R, W, batch and Zc are required");
    if (ld_z < D) return fail(WGNN_ERR_BAD_ARG, "ld_z must be >= D");
    if (!aligned8(Z0) || !aligned8(R) || !aligned8(W) || !aligned8(Zc) || !aligned8(U))
        return fail(WGNN_ERR_ALIGNMENT, "Z0, R, W, Zc and U must be 8-byte aligned");
    if (!aligned4(batch)) return fail(WGNN_ERR_ALIGNMENT, "batch must be 4-byte aligned");
    PArgs a{Z0, ld_z, R, W, batch, n_rows, D, K, S, Zc, U};
    hipLaunchKernelGGL(apply_kernel, dim3(grid_of((n_rows + kPRows - 1) / kPRows, grid_blocks)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return launched("wgnn_harmony_apply");
}
