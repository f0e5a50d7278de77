// Sharded search: the device fold of per-shard top-k lists (`search.ShardedIndex`; the contract is in include/tan_hip.h).
//
// An index cut into S shards is searched shard by shard; each sweep leaves a [Q, k_in] list of (score, row) whose rows count from the
// shard's own first row.  tan_topk_fold merges one such list into a running [Q, k] list of (score, shard, row): the k best of the
// union under score descending, shard ascending, row ascending -- the sweeps' own order on the global row row_base[shard] + row, so
// S folds give the list one sweep over the concatenated index gives.  The run list stays on the device (no read-back per shard) and
// its size does not depend on S.
// One wave per query, four queries per workgroup, as rank_merge_kernel: lanes 0..31 hold the run list, lanes 32..63 the incoming
// one, sort64_keyed orders the 64 entries, and up to three int32 payload columns follow their entry by one __shfl each from the
// lane the sort reports.  A lane loads slot `lane` and stores slot `lane`, and every store depends on the sort, which depends on all
// of the wave's loads: the fold is in place.  No atomics, no scratch, no LDS.
#include "tan_sort.h"

namespace tal {
namespace {

constexpr int SENT = 0x7fffffff;            // the row / shard of an empty slot (tan_retrieve.hip's SENT_ROW)
constexpr int MAX_AUX = 3;

struct fold_aux {
    const int* p[MAX_AUX];
};

__global__ void __launch_bounds__(256) topk_fold_kernel(float* run_score, int* run_shard, int* run_row, int* run_aux, long Q, int k,
                                                        int n_aux, int reset, const float* __restrict__ in_score,
                                                        const int* __restrict__ in_row, fold_aux in_aux, int k_in, int shard) {
    const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= Q) return;                                            // wave-uniform
    float s = -INFINITY;
    int sh = SENT, n = SENT;
    int a[MAX_AUX] = {-1, -1, -1};
    if (lane < 32) {
        if (lane < k && !reset) {
            const long o = q * k + lane;
            n = run_row[o];
            if (n != SENT) {
                s = run_score[o];
                sh = run_shard[o];
#pragma unroll
                for (int c = 0; c < MAX_AUX; ++c)
                    if (c < n_aux) a[c] = run_aux[((long)c * Q + q) * k + lane];
            }
        }
    } else if (lane - 32 < k_in) {
        const long o = q * k_in + (lane - 32);
        n = in_row[o];
        if (n != SENT) {                                           // the sweeps' sentinel under a broken v_off: an empty slot
            s = in_score[o];
            sh = shard;
#pragma unroll
            for (int c = 0; c < MAX_AUX; ++c)
                if (c < n_aux) a[c] = in_aux.p[c][o];
        }
    }
    unsigned long long key = ((unsigned long long)(unsigned)sh << 32) | (unsigned)n;
    int src = lane;
    sort64_keyed(s, key, src, lane);
#pragma unroll
    for (int c = 0; c < MAX_AUX; ++c) a[c] = __shfl(a[c], src, 64);
    if (lane < k) {
        const long o = q * k + lane;
        run_score[o] = s;
        run_shard[o] = (int)(unsigned)(key >> 32);
        run_row[o] = (int)(unsigned)key;
#pragma unroll
        for (int c = 0; c < MAX_AUX; ++c)
            if (c < n_aux) run_aux[((long)c * Q + q) * k + lane] = a[c];
    }
}

}  // namespace
}  // namespace tal

using namespace tal;

extern "C" int tan_topk_fold(float* run_score, int* run_shard, int* run_row, int* run_aux, long Q, int k, int n_aux, int reset,
                             const float* in_score, const int* in_row, const int* in_aux0, const int* in_aux1, const int* in_aux2,
                             int k_in, int shard, void* stream) {
    TAN_REQUIRE(Q >= 1 && Q < (1L << 31) && k >= 1 && k <= 32 && k_in >= 1 && k_in <= k && n_aux >= 0 && n_aux <= MAX_AUX);
    TAN_REQUIRE(shard >= 0 && shard < SENT);
    TAN_REQUIRE(run_score && run_shard && run_row && in_score && in_row);
    fold_aux aux = {{in_aux0, in_aux1, in_aux2}};
    TAN_REQUIRE(n_aux == 0 || run_aux);
    for (int c = 0; c < n_aux; ++c) TAN_REQUIRE(aux.p[c]);
    hipLaunchKernelGGL(topk_fold_kernel, dim3(cdiv(Q, 4)), dim3(256), 0, (hipStream_t)stream, run_score, run_shard, run_row, run_aux, Q,
                       k, n_aux, reset, in_score, in_row, aux, k_in, shard);
    TAN_LAUNCH_CHECK();
    return 0;
}
