// The 64-lane sorting network the top-k kernels share (tan_retrieve.hip, tan_rerank.hip).
#pragma once
#include "tan_common.h"

namespace tal {

__device__ __forceinline__ bool better(float s, int n, float os, int on) { return s > os || (s == os && n < on); }

// 64 (score, row) pairs, one per lane -> lane j holds rank j (score descending, equal scores by ascending row)
__device__ __forceinline__ void sort64(float& s, int& n, int lane) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const float os = __shfl_xor(s, stride, 64);
            const int on = __shfl_xor(n, stride, 64);
            const bool lower = (lane & stride) == 0, desc = (lane & size) == 0;
            const bool mine = better(s, n, os, on);
            const bool keep = (lower == desc) ? mine : !mine;
            if (!keep) { s = os; n = on; }
        }
    }
}

// sort64 under a three-part key, for lists that come from several indices (tan_shard.hip): score descending, then `key` ascending
// (unsigned: (shard << 32) | row, both non-negative).  `src` travels with its entry: give it the lane number and lane j learns
// which lane held rank j before the sort, so any further payload follows by one __shfl per column.
__device__ __forceinline__ void sort64_keyed(float& s, unsigned long long& key, int& src, int lane) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const float os = __shfl_xor(s, stride, 64);
            const unsigned ohi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), stride, 64);
            const unsigned olo = (unsigned)__shfl_xor((int)(unsigned)key, stride, 64);
            const int osrc = __shfl_xor(src, stride, 64);
            const unsigned long long okey = ((unsigned long long)ohi << 32) | olo;
            const bool lower = (lane & stride) == 0, desc = (lane & size) == 0;
            const bool mine = s > os || (s == os && (key < okey || (key == okey && src < osrc)));   // src: equal entries stay 64 entries
            const bool keep = (lower == desc) ? mine : !mine;
            if (!keep) { s = os; key = okey; src = osrc; }
        }
    }
}

}  // namespace tal
