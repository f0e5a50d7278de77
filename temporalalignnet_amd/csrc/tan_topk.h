// What the matrix-free top-k sweeps share beyond the sorting network (tan_retrieve.hip, tan_coarse.hip): the tile and candidate-buffer
// sizes, the rule that cuts an index into splits, and the launch that folds the splits' lists.  One copy: "bit-identical for every
// `splits`" rests on every sweep cutting and merging the same way.
#pragma once
#include "tan_sort.h"

namespace tal {
namespace {

constexpr int BQ = 128;                     // queries per block: 4 waves x 32
constexpr int BN = 64;                      // index rows per tile
constexpr int CAP = 64;                     // candidate slots per query
constexpr int KMAX = 32;
constexpr int MAX_SPLITS = 256;
constexpr int SENT_ROW = 0x7fffffff;

inline long n_index_tiles(long N) { return (N + BN - 1) / BN; }

inline long max_splits(long N) { return n_index_tiles(N) < MAX_SPLITS ? n_index_tiles(N) : MAX_SPLITS; }

// how many splits a sweep launches (`splits` = 0: chosen from Q and N) and the index tiles each one takes
inline int n_splits(long Q, long N, int splits, long* tiles_per_split) {
    const long n_tiles = n_index_tiles(N), q_tiles = (Q + BQ - 1) / BQ;
    long want = splits > 0 ? splits : (512 + q_tiles - 1) / q_tiles;
    want = want < 1 ? 1 : (want > MAX_SPLITS ? MAX_SPLITS : want);
    want = want > n_tiles ? n_tiles : want;
    *tiles_per_split = (n_tiles + want - 1) / want;
    return (int)((n_tiles + *tiles_per_split - 1) / *tiles_per_split);
}

// launch 3: one wave per query; lanes 0..31 carry the best so far, lanes 32..63 take the next split's list
__global__ void __launch_bounds__(256) rank_merge_kernel(const float* __restrict__ part_s, const int* __restrict__ part_n, long Q, int k,
                                                         int splits, float* __restrict__ top_s, int* __restrict__ top_n) {
    const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= Q) return;
    float s = -INFINITY;
    int n = SENT_ROW;
    for (int sp = 0; sp < splits; ++sp) {
        if (lane >= 32) {
            const bool real = lane - 32 < k;
            const long o = ((long)sp * Q + q) * k + (lane - 32);
            s = real ? part_s[o] : -INFINITY;
            n = real ? part_n[o] : SENT_ROW;
        }
        sort64(s, n, lane);
    }
    if (lane < k) { top_s[q * k + lane] = s; top_n[q * k + lane] = n; }
}

}  // namespace
}  // namespace tal
