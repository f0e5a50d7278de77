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

}  // namespace tal
