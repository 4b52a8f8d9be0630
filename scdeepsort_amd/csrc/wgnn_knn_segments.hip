// wgnn_knn_segments.hip - wgnn_knn_segments: for every query row its k nearest rows in EACH of n_segs segments of the same matrix
// (include/wgnn.h has the contract) - the search behind a batch-balanced kNN graph.  The segments are given as a permutation of
// the row ids (`order`, segment-major) and its n_segs + 1 bounds; the rows themselves stay where the caller has them.
//
// The search is wgnn_knn.hip's, with a segment where that file has the whole candidate matrix: a workgroup of 256 threads holds
// a tile of 64 queries and streams tiles of 64 candidates of ONE segment past it, 16 columns of D at a time, through two LDS
// buffers; a lane owns a 4 x 4 micro-tile of pairs and carries its 16 distances in registers across the slabs of D,
//     t = q[j] - x[j];  d = fma(t, t, d) in f32;   j = 0 .. D-1 ascending, d = 0 to start
// so that a distance carries the bits wgnn_knn_rows gives the pair.  A loader thread owns one candidate row of the tile and
// fetches it by its id, order[c]: the gather is the loader's address and nothing else.  The tile's 64 ids go to LDS beside the
// slabs; the selection key is (bits(d) << 32 | id) - the ORIGINAL row id, so equal distances go to the lower row id within a
// segment and across segments.  The last tile of a segment stops at the segment's end (the next segment's rows follow directly
// in `order`); an id outside [0, n_rows) is skipped and reported in the status word; the query itself (id == q) is skipped.
//
// A work unit is (query tile, segment, sub-range of the segment's tiles): grid.y = n_segs * splits <= 64.  Every unit writes
// its k sorted keys per query into the workspace; knn_segments_merge - a wavefront per query, a lane per unit - pops the
// smallest head n_segs * k times under a quota of k per segment, and writes every pop at its rank in the merged list and at its
// rank within its segment in the blocked one.  Keys are totally ordered, so the result is a function of the operands alone.
//
// The tile is the shared one (wgnn_pair_tile.h), and so is the staging and merging of survivors (wgnn_topk_select.h has the
// comments): this file passes its run-time staging size where wgnn_knn.hip passes a constant.
#include <limits.h>
#include "wgnn_build_rows.h"
#include "wgnn_pair_tile.h"
#include "wgnn_topk_select.h"

namespace wgnn {
namespace {

constexpr int kMaxStage = 32;           // staging slots per query, at most (stage_slots); a list's pitch is slots + 1 64-bit words (odd:
                                        // the merging lanes spread over banks), and a list that has taken more than half is merged
constexpr int kMaxK = 64;
constexpr int kMaxSegs = WGNN_KNN_SEGMENTS_MAX_SEGS;
constexpr int kMaxList = WGNN_KNN_SEGMENTS_MAX_LIST;      // n_segs * k: the merge gives every entry of a query's lists a lane
constexpr int kMaxUnits = 64;                             // n_segs * splits: the merge gives every unit a lane

struct SArgs {
    const float* X; long ld_x;
    const int* order; const long long* seg_ptr;
    int n_rows; int n_segs; int D; int k;
    int q_first; int n_q; int splits;
    int* idx; float* d2; long ld_out;
    int* m_idx; float* m_d2; long ld_m;
    int* status;
    u64* ws;
    int stage;
};

// Staging slots per query.  The kernel takes 96 registers: five workgroups fit a CU's register files, and 160 KiB of LDS hold
// five only below 32 KiB each.  The slabs take 17 KiB, 32 staging slots 16.5 KiB: with 16 slots the short lists of a balanced
// graph (k <= 8, 0.5 KiB * (k | 1) of sorted keys) leave room for the fifth workgroup; a longer list does not, and keeps 32.
// Measured at k = 3 against 32 slots: 2 % less time at 20 000 and 100 000 rows (profiles/resident_bbknn.md).
inline int stage_slots(int k) { return k <= 8 ? 16 : kMaxStage; }

inline int seg_lds_bytes(int k) {
    return kTQ * sorted_pitch(k) * 8 + kTQ * (stage_slots(k) + 1) * 8 + 2 * kSlabFloats * 4 + kTQ * 4 + kTC * 4 + 16;
}

__global__ void __launch_bounds__(kPairBlock) knn_segments_kernel(const SArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int k = a.k, sp = sorted_pitch(k), stage = a.stage, mark = stage >> 1;
    u64* s_sorted = reinterpret_cast<u64*>(smem);                               // [kTQ][sp]
    u64* s_stage = s_sorted + kTQ * sp;                                         // [kTQ][stage + 1]
    float* s_slab = reinterpret_cast<float*>(s_stage + kTQ * (stage + 1));      // [2][2][kKS][kPitch]; 16-byte aligned: all above is 8 x even
    int* s_cnt = reinterpret_cast<int*>(s_slab + 2 * kSlabFloats);              // [kTQ]
    int* s_id = s_cnt + kTQ;                                                    // [kTC]: the tile's row ids, -1 = no candidate
    int* s_flag = s_id + kTC;

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int ty = tid >> 4, tx = tid & 15;               // the micro-tile: queries ty*4 .. +3, candidates tx*4 .. +3
    const int lrow = tid >> 2, lk4 = tid & 3;             // the loader: row lrow of the tile, its float4 number lk4 of the slab
    const long q0 = (long)blockIdx.x * kTQ;
    const int seg = blockIdx.y / a.splits, part = blockIdx.y - seg * a.splits;
    // the segment's range of `order`, clamped into [0, n_rows] whatever seg_ptr holds
    const long long lo = a.seg_ptr[seg], hi = a.seg_ptr[seg + 1];
    const long c_lo = lo < 0 ? 0 : (lo > a.n_rows ? a.n_rows : (long)lo);
    const long c_hi = hi < c_lo ? c_lo : (hi > a.n_rows ? a.n_rows : (long)hi);
    const long n_tiles = (c_hi - c_lo + kTC - 1) / kTC;
    const long t0 = n_tiles * part / a.splits, t1 = n_tiles * (part + 1) / a.splits;
    const int n_slabs = (a.D + kKS - 1) / kKS;

    for (int i = tid; i < kTQ * sp; i += kPairBlock) s_sorted[i] = kNone;
    if (tid < kTQ) s_cnt[tid] = 0;
    if (tid < 3) s_flag[tid] = 0;                         // "a lane has a survivor", and the two `over` words of the rounds

    const bool q_ok = q0 + lrow < a.n_q;
    const float* q_src = a.X + (size_t)(q_ok ? a.q_first + q0 + lrow : 0) * a.ld_x + lk4 * 4;

    for (long t = t0; t < t1; ++t) {
        const long c = c_lo + t * kTC + lrow;             // the loader's place in `order`: the tile ends where the segment does
        int row = -1;
        if (c < c_hi) {
            row = a.order[c];
            if (row < 0 || row >= a.n_rows) {
                if (lk4 == 0) atomicOr(a.status, WGNN_KNN_SEGMENTS_BAD_ORDER);
                row = -1;
            }
        }
        const bool x_ok = row >= 0;
        const float* x_src = a.X + (size_t)(x_ok ? row : 0) * a.ld_x + lk4 * 4;
        if (lk4 == 0) s_id[lrow] = row;                   // read after this tile's barriers, written again after its selection's
        float acc[4][4];
        pair_tile_d2(acc, s_slab, q_src, q_ok, x_src, x_ok, a.D, n_slabs, tid);

        // selection: which of the 16 pairs beat their query's k-th key (read once; it only tightens).  The ids of the lane's
        // four candidates leave LDS here, before the first barrier of stage_survivors: the next tile's loaders write s_id after it.
        const int4 ids = *reinterpret_cast<const int4*>(s_id + tx * 4);
        const int cid[4] = {ids.x, ids.y, ids.z, ids.w};
        unsigned mask = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long q = q0 + ty * 4 + i;
            const u64 kth = s_sorted[(ty * 4 + i) * sp + k - 1];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u64 key = pair_key(acc[i][j], cid[j]);
                if (q < a.n_q && cid[j] >= 0 && cid[j] != a.q_first + q && key < kth) mask |= 1u << (i * 4 + j);
            }
        }
        stage_survivors(acc, cid, mask, s_sorted, s_stage, s_cnt, s_flag, mark, stage, stage + 1, sp, k, tid);
    }

    __syncthreads();
    merge_marked(s_sorted, s_stage, s_cnt, 0, stage, stage + 1, sp, k, wave, lane);
    __syncthreads();
    for (int e = tid; e < kTQ * k; e += kPairBlock) {
        const int ql = e / k, j = e - ql * k;
        if (q0 + ql >= a.n_q) continue;
        a.ws[((size_t)blockIdx.y * a.n_q + q0 + ql) * k + j] = s_sorted[ql * sp + j];
    }
}

// A wavefront per query.  Lane u walks unit u's sorted list (unit u = segment u / splits); the wave takes the smallest head
// n_segs * k times.  A pop counts against its segment: once a segment has given k keys, all its lanes retire - what they still
// hold is beyond that segment's k-th.  Lane e also keeps entry e of the two outputs in a register and stores it once at the end.
__global__ void __launch_bounds__(256) knn_segments_merge(const SArgs a) {
    const int lane = threadIdx.x & 63;
    const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.n_q) return;                               // wave-uniform
    const int k = a.k, total = a.n_segs * k;
    const bool live = lane < a.n_segs * a.splits;
    const int seg = live ? lane / a.splits : -1;
    const u64* mine = a.ws + ((size_t)(live ? lane : 0) * a.n_q + q) * k;
    int p = 0, taken = 0;                                 // taken: the pops of this lane's segment so far
    u64 head = live ? mine[0] : kNone;
    u64 merged = kNone, blocked = kNone;
    for (int j = 0; j < total; ++j) {
        u64 best = head;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const u64 o = __shfl_xor(best, off, 64);
            best = o < best ? o : best;
        }
        if (best == kNone) break;                         // wave-uniform: every list is used up or retired
        const int winner = __ffsll((long long)__ballot(head == best)) - 1;       // real keys are distinct; the lowest lane of equals
        const int s_win = winner / a.splits;
        const int rank = __shfl(taken, winner, 64);
        if (lane == j) merged = best;
        if (lane == s_win * k + rank) blocked = best;
        if (lane == winner) {
            ++p;
            head = p < k ? mine[p] : kNone;
        }
        if (seg == s_win && ++taken == k) head = kNone;
    }
    if (lane < total) {
        a.idx[(size_t)q * a.ld_out + lane] = blocked == kNone ? -1 : (int)(unsigned)blocked;
        a.d2[(size_t)q * a.ld_out + lane] = __uint_as_float((unsigned)(blocked >> 32));
        if (a.m_idx) {
            a.m_idx[(size_t)q * a.ld_m + lane] = merged == kNone ? -1 : (int)(unsigned)merged;
            a.m_d2[(size_t)q * a.ld_m + lane] = __uint_as_float((unsigned)(merged >> 32));
        }
    }
}

LdsMarks g_seg_lds;

// 0 = chosen here as wgnn_knn_rows chooses: about 4096 workgroups while every sub-range keeps at least two candidate tiles of a
// segment of the mean size (the segments' sizes are on the device).  A request is lowered to what 64 units per query tile leave.
int resolve_seg_splits(int64_t n_q, int64_t n_rows, int32_t n_segs, int32_t n_splits) {
    const int room = kMaxUnits / n_segs;
    if (n_splits > 0) return n_splits < room ? n_splits : room;
    const int64_t q_tiles = (n_q + kTQ - 1) / kTQ, c_tiles = ((n_rows + n_segs - 1) / n_segs + kTC - 1) / kTC;
    int64_t want = q_tiles > 0 ? (4096 + q_tiles * n_segs - 1) / (q_tiles * n_segs) : 1;
    if (want > c_tiles / 2) want = c_tiles / 2;
    if (want > room) want = room;
    return want < 1 ? 1 : (int)want;
}

const char* check_seg_sizes(int64_t n_q, int64_t n_rows, int32_t n_segs, int32_t k, int32_t n_splits, int* code) {
    *code = WGNN_ERR_BAD_ARG;
    if (n_q < 0 || n_q > INT32_MAX) return "n_q must be in [0, 2^31)";
    if (n_rows < 0 || n_rows > INT32_MAX) return "n_rows must be in [0, 2^31)";
    if (n_splits < 0 || n_splits > kMaxUnits) return "n_splits must be in [0, 64] (0 = chosen from the sizes)";
    *code = WGNN_ERR_UNSUPPORTED;
    if (k < 1 || k > kMaxK) return "k must be in [1, 64]";
    if (n_segs < 1 || n_segs > kMaxSegs) return "n_segs must be in [1, 64]";
    if (n_segs * k > kMaxList) return "n_segs * k must be at most 64";
    return nullptr;
}

int64_t seg_workspace_bytes(int64_t n_q, int32_t n_segs, int32_t k, int splits) { return (int64_t)n_segs * splits * n_q * k * 8; }

}  // namespace
}  // namespace wgnn

using namespace wgnn;

extern "C" int wgnn_knn_segments_workspace_bytes(int64_t n_q, int64_t n_rows, int32_t n_segs, int32_t k, int32_t n_splits,
                                                 int64_t* bytes) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_knn_segments_workspace_bytes", what); };
    wgnn::error_clear();
    if (!bytes) return fail(WGNN_ERR_BAD_ARG, "bytes is required");
    int code = 0;
    if (const char* what = check_seg_sizes(n_q, n_rows, n_segs, k, n_splits, &code)) return fail(code, what);
    *bytes = seg_workspace_bytes(n_q, n_segs, k, resolve_seg_splits(n_q, n_rows, n_segs, n_splits));
    return WGNN_OK;
}

extern "C" int wgnn_knn_segments(const float* X, int64_t ld_x, int64_t n_rows, int32_t D,
                                 const int32_t* order, const int64_t* seg_ptr, int32_t n_segs, int32_t k,
                                 int64_t q_first, int64_t n_q, int32_t n_splits,
                                 int32_t* idx, float* d2, int64_t ld_out,
                                 int32_t* merged_idx, float* merged_d2, int64_t ld_merged,
                                 int32_t* status, void* workspace, int64_t workspace_bytes, uint32_t flags, void* stream) {
    auto fail = [](int code, const char* what) { return wgnn::fail(code, "wgnn_knn_segments", what); };
    wgnn::error_clear();
    int code = 0;
    if (const char* what = check_seg_sizes(n_q, n_rows, n_segs, k, n_splits, &code)) return fail(code, what);
    if (flags) return fail(WGNN_ERR_BAD_ARG, "no flag is defined for this entry (flags must be 0)");
    if (int rc = check_row_width("wgnn_knn_segments", D)) return rc;
    if (ld_x < D || ld_x % 4) return fail(WGNN_ERR_ALIGNMENT, "ld_x must be >= D and a multiple of 4");
    if (ld_out < n_segs * k) return fail(WGNN_ERR_BAD_ARG, "ld_out must be >= n_segs * k");
    if ((merged_idx == nullptr) != (merged_d2 == nullptr)) return fail(WGNN_ERR_BAD_ARG, "merged_idx and merged_d2 come together or not at all");
    if (merged_idx && ld_merged < n_segs * k) return fail(WGNN_ERR_BAD_ARG, "ld_merged must be >= n_segs * k");
    if (q_first < 0 || q_first + n_q > n_rows) return fail(WGNN_ERR_BAD_ARG, "q_first must be >= 0 and satisfy q_first + n_q <= n_rows");
    if (workspace_bytes < 0) return fail(WGNN_ERR_WORKSPACE, "workspace_bytes is negative");
    if (n_q == 0) return WGNN_OK;
    if (!X || !order || !seg_ptr || !idx || !d2 || !status) return fail(WGNN_ERR_BAD_ARG, "X, order, seg_ptr, idx, d2 and status are required");
    if (!aligned16(X)) return fail(WGNN_ERR_ALIGNMENT, "X must be 16-byte aligned");
    if (!aligned8(seg_ptr)) return fail(WGNN_ERR_ALIGNMENT, "seg_ptr must be 8-byte aligned");
    if (!aligned4(order) || !aligned4(idx) || !aligned4(d2) || !aligned4(merged_idx) || !aligned4(merged_d2) || !aligned4(status))
        return fail(WGNN_ERR_ALIGNMENT, "order, idx, d2, merged_idx, merged_d2 and status must be 4-byte aligned");
    const int splits = resolve_seg_splits(n_q, n_rows, n_segs, n_splits);
    const int64_t need = seg_workspace_bytes(n_q, n_segs, k, splits);
    if (!workspace || workspace_bytes < need)
        return fail(WGNN_ERR_WORKSPACE, "workspace is smaller than wgnn_knn_segments_workspace_bytes asks for");
    if (!aligned8(workspace)) return fail(WGNN_ERR_ALIGNMENT, "workspace must be 8-byte aligned");

    SArgs a{};
    a.X = X; a.ld_x = ld_x; a.order = order; a.seg_ptr = reinterpret_cast<const long long*>(seg_ptr);
    a.n_rows = (int)n_rows; a.n_segs = n_segs; a.D = D; a.k = k;
    a.q_first = (int)q_first; a.n_q = (int)n_q; a.splits = splits;
    a.idx = idx; a.d2 = d2; a.ld_out = ld_out;
    a.m_idx = merged_idx; a.m_d2 = merged_d2; a.ld_m = ld_merged;
    a.status = status;
    a.ws = reinterpret_cast<u64*>(workspace);
    a.stage = stage_slots(k);
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto failed = [&fail]() { return fail(WGNN_ERR_LAUNCH, "HIP launch failed (or the LDS could not be reserved)"); };
    const int lds = seg_lds_bytes(k);
    if (raise_lds(g_seg_lds, reinterpret_cast<const void*>(knn_segments_kernel), lds) != WGNN_OK) return failed();
    const unsigned q_tiles = (unsigned)((n_q + kTQ - 1) / kTQ);
    hipLaunchKernelGGL(knn_segments_kernel, dim3(q_tiles, (unsigned)(n_segs * splits)), dim3(kPairBlock), lds, st, a);
    if (hipGetLastError() != hipSuccess) return failed();
    hipLaunchKernelGGL(knn_segments_merge, dim3((unsigned)((n_q + 3) / 4)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : failed();
}
