// wgnn_signatures.hip - wgnn_rank_sets_rows: for every (cell, set) pair of a batch the capped, doubled mid-ranks of the set's
// genes inside the cell's own row, added up (api.ResidentPredictor.signatures: UCell's rank-based signature score, Andreatta &
// Carmona 2021).  A set is a GIVEN subset of the genes, bit p of member[g] as wgnn_predict_rows_panels takes it.  The contract is
// the rank-sets block of include/wgnn.h; for one cell r with stored entries 0 .. deg - 1:
//
//   key_i  = the order-preserving integer of the f32 bits of val_i (all bits flipped for a set sign bit, else the sign bit set)
//   R2_j   = 2 * #{i : key_i > key_j} + #{i : key_i == key_j} + 1          twice the tie-averaged rank, rank 1 = the highest value
//   R2c_j  = min(R2_j, 2 * (max_rank + 1))
//   rank2_sum[r, p] = sum of R2c_j over the entries j with bit p of member[col_j];  present[r, p] = their number
//
// Only members need a rank, so the kernel COUNTS and never sorts: (member entries of the cell) x deg integer compares.
//
// Layout: one workgroup of 8 waves per cell, grid-stride.
//   1   the row's keys are staged in an LDS slab (slab = min(n_genes rounded up to 4, 16 384) keys, 64 KiB at most); of a longer
//       row the tail is read from global memory, the same key function applied on the way.
//   2   the row is walked 512 entries at a time; the entries with (member[col] & the launch's set mask) != 0 are compacted (ballot,
//       the waves' counts folded in wave order) into a STASH of 512 (key, masked word) pairs in LDS.  When the next 512 entries'
//       members would not fit, the stash is ranked and emptied first: a row with any number of members runs in passes.
//   3   ranking: the stash is cut into groups of 64, wave w takes the groups w, w + 8, ...  LANE j OWNS entry j of the group and
//       every lane walks ALL staged keys - the same 16-byte address in all lanes, one broadcast ds_read_b128 per four keys -
//       counting gt and eq in its own registers.  There is no cross-lane reduction per entry.
//   4   the group's (R2c, word) pairs are handed round lane by lane (readlane); lane p keeps set p's running sum and count in
//       registers and adds where bit p is set.
//   5   the 8 waves' partials are folded through LDS in wave order, lanes < n_sets store.
// Chosen over "one entry per wave, the 64 lanes stride the keys": that form pays a 64-lane reduction of two counters per entry;
// this one pays idle lanes in a group that is not full, and idle waves for a cell with fewer than 512 members.  Both read the
// slab the same number of times.  Not done: cutting the keys among the idle waves when a cell has few members.
//
// Everything is an integer: the result does not depend on the grid, the slab width, the pass structure or the order of anything,
// and two launches are bit-identical.  No atomics, vector stores only, plain C++.  A gene id outside [0, n_genes) is never used
// as an index: such an entry belongs to no set (it still takes part in the other entries' ranks, as a stored value).

#include "wgnn_align_rows.h"             // below
#include "wgnn_build_rows.h"             // raise_lds

namespace {
using namespace wgnn;

constexpr int kRWaves = 8;
constexpr int kRBlock = 64 * kRWaves;
constexpr int kRMaxBlocks = 1024;             // 256 CUs x 2 resident workgroups, twice: grid-stride beyond that
constexpr int kRMaxSlab = 16384;              // keys staged per row at most: 64 KiB
constexpr int kRStash = kRBlock;              // member entries held between two rankings; one walk step always fits an empty stash
constexpr int kRMaxSets = 64;                 // bits of a member word
// LDS: slab keys | stash keys | stash words | the waves' partial sums | partial counts | the waves' member counts.  With the
// widest slab 65 536 + 2 048 + 4 096 + 4 096 + 2 048 + 64 = 77 888 bytes: two workgroups per CU (160 KiB).
constexpr int kRFixedBytes = kRStash * 4 + kRStash * 8 + kRWaves * 64 * 8 + kRWaves * 64 * 4 + 64;

struct RArgs {
    const void* rowptr; const int* col; const float* val; long n_rows; int n_genes;
    const unsigned long long* member; int n_sets; unsigned long long mask; unsigned cap;
    long long* rank2_sum; long ld_sum; int* present; long ld_present;
    int slab;
};

// the usual order-preserving key of a float's bits: one total order over every bit pattern, the numeric order on finite values
// (with -0.0 below +0.0)
__device__ __forceinline__ unsigned rank_key(float x) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <typename TPtr>
__global__ void __launch_bounds__(kRBlock) rank_sets_rows_kernel(const RArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
    unsigned* s_key = reinterpret_cast<unsigned*>(s_mem);                                       // [slab]
    unsigned char* s_fixed = s_mem + (size_t)a.slab * 4;                                        // slab % 4 == 0: 16-byte aligned
    unsigned* s_skey = reinterpret_cast<unsigned*>(s_fixed);                                    // [kRStash]
    unsigned long long* s_sword = reinterpret_cast<unsigned long long*>(s_fixed + kRStash * 4); // [kRStash]
    unsigned long long* s_psum = s_sword + kRStash;                                             // [kRWaves][64]
    int* s_pcnt = reinterpret_cast<int*>(s_psum + kRWaves * 64);                                // [kRWaves][64]
    int* s_wcnt = s_pcnt + kRWaves * 64;                                                        // [kRWaves]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TPtr* rp = reinterpret_cast<const TPtr*>(a.rowptr);
    const unsigned G = (unsigned)a.n_genes;

    for (long r = blockIdx.x; r < a.n_rows; r += gridDim.x) {                  // everything below is block-uniform but lane / wave
        const long b = rp[r];
        const long e = rp[r + 1] > b ? (long)rp[r + 1] : b;
        const long deg = e - b;
        const int n_st = (int)(deg < a.slab ? deg : a.slab);                   // keys [0, n_st) of the row are in the slab
        for (int i = threadIdx.x; i < n_st; i += kRBlock) s_key[i] = rank_key(a.val[b + i]);
        __syncthreads();                                                       // the slab is staged (and the last row's fold is read)

        unsigned long long sum = 0;                                            // lane p: set p's sum of R2c and its entries,
        int cnt = 0;                                                           // over the groups this wave ranks

        // ranks the stash's m entries and adds them to (sum, cnt); the caller has made the stash visible
        auto rank_stash = [&](int m) {
            for (int g0 = wave * 64; g0 < m; g0 += kRBlock) {                  // wave-uniform
                const int n = m - g0 < 64 ? m - g0 : 64;
                const int i = g0 + (lane < n ? lane : n - 1);
                const unsigned kj = s_skey[i];
                const unsigned long long wj = lane < n ? s_sword[i] : 0ull;
                unsigned gt = 0, eq = 0;
                const uint4* k4 = reinterpret_cast<const uint4*>(s_key);
                const int n4 = n_st >> 2;
                for (int t = 0; t < n4; ++t) {                                 // one address for the wave: a broadcast 16-byte read
                    const uint4 q = k4[t];
                    gt += (q.x > kj) + (q.y > kj) + (q.z > kj) + (q.w > kj);
                    eq += (q.x == kj) + (q.y == kj) + (q.z == kj) + (q.w == kj);
                }
                for (int t = n4 << 2; t < n_st; ++t) {
                    const unsigned k = s_key[t];
                    gt += k > kj; eq += k == kj;
                }
                for (long j = b + n_st; j < e; ++j) {                          // a row beyond the slab: its tail from global memory
                    const unsigned k = rank_key(a.val[j]);
                    gt += k > kj; eq += k == kj;
                }
                const unsigned long long r2 = 2ull * gt + eq + 1ull;
                const unsigned r2c = r2 < a.cap ? (unsigned)r2 : a.cap;
                const unsigned wlo = (unsigned)wj, whi = (unsigned)(wj >> 32);
                for (int j = 0; j < n; ++j) {                                  // entry j's pair to every lane; lane p adds for set p
                    const unsigned rj = (unsigned)__builtin_amdgcn_readlane((int)r2c, j);
                    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)wlo, j);
                    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)whi, j);
                    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
                    const bool in = (w >> lane) & 1ull;
                    sum += in ? rj : 0u;
                    cnt += in ? 1 : 0;
                }
            }
        };

        int fill = 0;                                                          // entries in the stash
        for (long base = b; base < e; base += kRBlock) {
            const long j = base + threadIdx.x;
            const bool on = j < e;
            const unsigned g = on ? (unsigned)a.col[j] : 0u;
            const unsigned long long w = (on && g < G) ? (a.member[g] & a.mask) : 0ull;
            const bool k = w != 0ull;
            unsigned key = 0u;
            if (k) key = j - b < n_st ? s_key[j - b] : rank_key(a.val[j]);
            const unsigned long long km = __ballot(k);
            if (lane == 0) s_wcnt[wave] = __popcll(km);
            __syncthreads();                                                   // the waves' counts
            int before = 0, total = 0;
#pragma unroll
            for (int v = 0; v < kRWaves; ++v) {
                const int c = s_wcnt[v];
                before += v < wave ? c : 0;
                total += c;
            }
            if (fill + total > kRStash) {                                      // block-uniform: rank what is there, then start over
                rank_stash(fill);
                __syncthreads();                                               // every wave has read the stash
                fill = 0;
            }
            if (k) {
                const int s = fill + before + below(km);                       // < kRStash: total <= kRBlock == kRStash
                s_skey[s] = key; s_sword[s] = w;
            }
            fill += total;
            __syncthreads();                                                   // the stash is written, s_wcnt is free again
        }
        rank_stash(fill);

        s_psum[wave * 64 + lane] = sum;
        s_pcnt[wave * 64 + lane] = cnt;
        __syncthreads();                                                       // after it nobody reads the slab or the stash
        if (wave == 0 && lane < a.n_sets) {
            unsigned long long s = 0;
            int c = 0;
#pragma unroll
            for (int v = 0; v < kRWaves; ++v) { s += s_psum[v * 64 + lane]; c += s_pcnt[v * 64 + lane]; }
            a.rank2_sum[(size_t)r * a.ld_sum + lane] = (long long)s;
            a.present[(size_t)r * a.ld_present + lane] = c;
        }
        // no barrier here: the next row writes the partials only after its own barriers, which wave 0 reaches after these reads
    }
}

LdsMarks g_lds[2];                            // the raised LDS limit per rowptr width

template <typename TPtr>
int launch(const RArgs& a, int which, hipStream_t st) {
    const void* fn = reinterpret_cast<const void*>(rank_sets_rows_kernel<TPtr>);
    const int lds = a.slab * 4 + kRFixedBytes;
    if (raise_lds(g_lds[which], fn, lds) != WGNN_OK) return WGNN_ERR_LAUNCH;
    const unsigned nb = (unsigned)(a.n_rows < kRMaxBlocks ? a.n_rows : kRMaxBlocks);
    hipLaunchKernelGGL((rank_sets_rows_kernel<TPtr>), dim3(nb), dim3(kRBlock), lds, st, a);
    return hipGetLastError() == hipSuccess ? WGNN_OK : WGNN_ERR_LAUNCH;
}

}  // namespace

extern "C" int wgnn_rank_sets_rows(const void* rowptr, const int32_t* col, const float* val, int64_t n_rows, int32_t n_genes,
                                   const uint64_t* member, int32_t n_sets, int32_t max_rank,
                                   int64_t* rank2_sum, int64_t ld_sum, int32_t* present, int64_t ld_present,
                                   uint32_t flags, void* stream) {
    const char* fn = "wgnn_rank_sets_rows";
    auto fail = [fn](int code, const char* what) { return wgnn::fail(code, fn, what); };
    wgnn::error_clear();
    if (!rowptr || !col || !val) return fail(WGNN_ERR_BAD_ARG, "rowptr, col and val are required");
    if (!member) return fail(WGNN_ERR_BAD_ARG, "member is required (uint64 [n_genes], bit p = the gene belongs to set p)");
    if (!rank2_sum || !present) return fail(WGNN_ERR_BAD_ARG, "rank2_sum and present are required");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(WGNN_ERR_BAD_ARG, "n_rows must be in [0, 2^31)");
    if (n_sets < 1 || n_sets > kRMaxSets) return fail(WGNN_ERR_BAD_ARG, "n_sets must be in [1, 64] (split the sets)");
    if (max_rank < 1 || max_rank > (1 << 30)) return fail(WGNN_ERR_BAD_ARG, "max_rank must be in [1, 2^30]");
    if (n_genes <= 0) return fail(WGNN_ERR_BAD_ARG, "n_genes must be positive");
    if (ld_sum < n_sets || ld_present < n_sets) return fail(WGNN_ERR_BAD_ARG, "ld_sum and ld_present must be >= n_sets");
    if (int rc = wgnn::check_rowptr_flag(fn, flags)) return rc;
    if (!wgnn::aligned8(member) || !wgnn::aligned8(rank2_sum))
        return fail(WGNN_ERR_ALIGNMENT, "member and rank2_sum must be 8-byte aligned");
    if (int rc = wgnn::check_rowptr_alignment(fn, rowptr, flags)) return rc;
    if (!wgnn::aligned4(col) || !wgnn::aligned4(val) || !wgnn::aligned4(present))
        return fail(WGNN_ERR_ALIGNMENT, "col, val and present must be 4-byte aligned");
    if (n_rows == 0) return WGNN_OK;
    RArgs a{};
    a.rowptr = rowptr; a.col = col; a.val = val; a.n_rows = n_rows; a.n_genes = n_genes;
    a.member = reinterpret_cast<const unsigned long long*>(member); a.n_sets = n_sets;
    a.mask = n_sets == 64 ? ~0ull : (1ull << n_sets) - 1ull;
    a.cap = 2u * ((unsigned)max_rank + 1u);                                    // <= 2^31 + 2
    a.rank2_sum = reinterpret_cast<long long*>(rank2_sum); a.ld_sum = ld_sum; a.present = present; a.ld_present = ld_present;
    const int64_t g4 = ((int64_t)n_genes + 3) & ~(int64_t)3;
    a.slab = (int)(g4 < kRMaxSlab ? g4 : kRMaxSlab);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = (flags & WGNN_FLAG_ROWPTR_I64) ? launch<long long>(a, 1, st) : launch<int>(a, 0, st);
    return rc == WGNN_OK ? rc : fail(rc, "HIP launch failed (or the LDS slab could not be reserved)");
}
