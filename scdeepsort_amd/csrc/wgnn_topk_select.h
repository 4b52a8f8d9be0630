// wgnn_topk_select.h - the top-k selection that wgnn_knn.hip and wgnn_knn_segments.hip run on the distances of a pair tile
// (wgnn_pair_tile.h).  It works on the 64-bit key (bits(d) << 32 | id): d >= +0, so the f32 bits order as unsigned integers,
// every NaN sorts above +inf, and keys of one query are distinct - a total order.  Per query the k smallest keys live in LDS,
// sorted; a distance that beats the k-th of them is appended to the query's staging list (an LDS atomic claims the slot,
// nothing else is atomic).  A list that has taken more than `mark` of its `stage` slots is merged into the sorted list by one
// wavefront, every key placed at its rank in the union, and emptied; a lane whose key found no slot keeps it and appends again
// after the merge.  The order of a staging list depends on the hardware; the sorted set does not.
//
// What a kernel keeps: the LDS carve-up (s_sorted [kTQ][sorted_pitch(k)], s_stage [kTQ][stage_pitch], s_cnt [kTQ], s_flag [3]),
// the staging size (a constant or a launch argument; stage <= 32, stage_pitch = stage + 1: odd, the merging lanes spread over
// banks), and the test that forms a lane's mask of survivors - what a candidate's id is and which id is the query itself.
#pragma once
#include "wgnn_pair_tile.h"

namespace wgnn {

typedef unsigned long long u64;
constexpr u64 kNone = ((u64)0x7f800000u << 32) | 0x7fffffffu;        // (+inf, no candidate): above every selectable key

__host__ __device__ inline int sorted_pitch(int k) { return k | 1; }          // odd, as a staging list's pitch

__device__ __forceinline__ u64 pair_key(float d, int id) { return ((u64)__float_as_uint(d) << 32) | (unsigned)id; }

// Merge the n <= 32 staged keys of one query into its sorted list of k, one WAVEFRONT's work, by rank: a lane takes up to
// two keys of the union (k + n <= 96), counts the keys below each - every lane reads the whole union, one broadcast read per
// key - and stores a real key whose rank is below k at that rank.  Real keys are distinct, so the ranks below k are taken once
// each; kNone is above every real key, keeps its place at the tail (the real keys only grow in number) and is never stored.
// All of a lane's reads are issued before its first store, and a wavefront's LDS operations complete in order.
__device__ __forceinline__ void merge_staged(u64* list, const u64* stage, int n, int k, int lane) {
    const int total = k + n;
    const u64 mine0 = lane < k ? list[lane] : (lane < total ? stage[lane - k] : kNone);
    const u64 mine1 = lane + 64 < total ? stage[lane + 64 - k] : kNone;          // k <= 64: the second key is a staged one
    int r0 = 0, r1 = 0;
    for (int e = 0; e < k; ++e) { const u64 v = list[e]; r0 += v < mine0; r1 += v < mine1; }
    for (int e = 0; e < n; ++e) { const u64 v = stage[e]; r0 += v < mine0; r1 += v < mine1; }
    __builtin_amdgcn_wave_barrier();                      // the compiler keeps the stores below the reads
    if (mine0 != kNone && r0 < k) list[r0] = mine0;
    if (mine1 != kNone && r1 < k) list[r1] = mine1;
}

// Every query of the workgroup whose staging count is above `mark` is merged and its count cleared: wavefront w looks after
// the queries w, w + 4, ...; its first 16 lanes read their counts, a ballot names the lists to merge.  A count above `stage`
// says that appends found no slot (their lanes still hold the keys): the list holds `stage` keys.
__device__ __forceinline__ void merge_marked(u64* s_sorted, const u64* s_stage, int* s_cnt, int mark, int stage, int stage_pitch,
                                             int sp, int k, int wave, int lane) {
    const int mine = wave + (kPairBlock / 64) * (lane & 15);
    const int n = s_cnt[mine];
    unsigned long long todo = __ballot(lane < 16 && n > mark);
    while (todo) {                                        // wave-uniform
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int ql = wave + (kPairBlock / 64) * b;
        merge_staged(s_sorted + ql * sp, s_stage + ql * stage_pitch, min(__shfl(n, b, 64), stage), k, lane);
        if (lane == 0) s_cnt[ql] = 0;
    }
}

// The survivors of one tile go to their queries' staging lists: bit i * 4 + j of `mask` says that the lane's pair (query
// ty * 4 + i, candidate j of its four, whose id is id[j]) beat the query's k-th key.  s_flag: "a lane has a survivor", and the
// two `over` words of the rounds; all three are zero on entry and on return.  Every thread of the workgroup calls this.
__device__ __forceinline__ void stage_survivors(const float (&acc)[4][4], const int (&id)[4], unsigned mask,
                                                u64* s_sorted, u64* s_stage, int* s_cnt, int* s_flag,
                                                int mark, int stage, int stage_pitch, int sp, int k, int tid) {
    const int wave = tid >> 6, lane = tid & 63, ty = tid >> 4;
    if (mask) *s_flag = 1;
    __syncthreads();
    if (*s_flag) {                                        // uniform over the workgroup
        // Rounds of: every lane appends what it still holds; then, if a list passed the merge mark or overflowed, the lists
        // above the mark are merged and emptied and the lanes whose keys found no slot try again.  A round without such a
        // list - the usual one - costs one barrier.  `over` alternates between two words: the one a round clears is set
        // again two rounds (at least one barrier) later.
        unsigned pending = mask;
        for (int round = 0;; ++round) {
            int* over = s_flag + 1 + (round & 1);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (pending & (1u << (i * 4 + j))) {
                        const int ql = ty * 4 + i;
                        const int slot = atomicAdd(&s_cnt[ql], 1);
                        if (slot < stage) {
                            s_stage[ql * stage_pitch + slot] = pair_key(acc[i][j], id[j]);
                            pending &= ~(1u << (i * 4 + j));
                        }
                        if (slot >= mark) *over = 1;
                    }
            __syncthreads();
            if (!*over) break;                            // uniform; no list overflowed, so no lane holds a key any more
            merge_marked(s_sorted, s_stage, s_cnt, mark, stage, stage_pitch, sp, k, wave, lane);
            __syncthreads();
            if (tid == 0) *over = 0;
        }
        if (tid == 0) *s_flag = 0;                        // read again only after the next tile's barriers
    }
}

}  // namespace wgnn
