// Order-preserving timestamps for corpus alignment: a monotonic (non-decreasing) decode over a video's stitched rows.
//
// eval/eval_zeroshot_align.py:222,237 gives every sentence the arg-max of its own row, independently of every other sentence.  ASR
// sentences are spoken in order; this decode picks, for the kept rows r_0 .. r_{m-1} of one video taken in decode order, the
// non-decreasing sequence of seconds with the largest sum of similarities.  With x_i[t] = sim[r_i][t] and V = vlen:
//
//     D_0[t] = x_0[t]                      D_i[t] = x_i[t] + M_{i-1}[t]            (one f32 add, round to nearest, not contracted)
//     M_i[t] = max_{t' <= t} D_i[t']       A_i[t] = the SMALLEST t' <= t with D_i[t'] == M_i[t]
//     t_{m-1} = A_{m-1}[V-1]               t_{i-1} = A_{i-1}[t_i]                  path score = D_{m-1}[t_{m-1}]
//
// The maximum is exact and every cell takes one rounded add, so the result does not depend on the scan order; the tie rule (smallest
// t_{m-1}, then smallest t_{m-2}, ...) is carried by one combine, "keep the left operand unless the right one is strictly greater".
//
// One workgroup per video; rows one after the other; a row is swept in tiles of TILE seconds.  Thread `tid` owns seconds
// [t0 + tid * E, t0 + tid * E + E) of the tile at t0 -- the same seconds in every row -- so M lives in a global scratch row per video
// that is updated in place: a thread reads only the M[t] it wrote itself one row earlier, in program order.  The inclusive
// (max, first-arg) scan runs serially inside the thread, by 64-lane shuffles inside the wave, through LDS across the four waves, and
// a carry pair passes from tile to tile.  The back-pointers A go to global memory ([n_acc] int32, laid out like sim); after a
// workgroup barrier (the writes of one workgroup, read by a thread of the same workgroup) thread 0 walks them backwards.
// No atomics, no host synchronisation, no allocation.
#include "tan_common.h"

#pragma clang fp contract(off)

namespace tal {
namespace {

constexpr int DEC_THREADS = 256;
constexpr int DEC_E = 4;                              // seconds per thread and tile
constexpr int DEC_TILE = DEC_THREADS * DEC_E;
constexpr int DEC_WAVES = DEC_THREADS / WAVE;

__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }      // compiled under this file's contract(off)

struct Best { float m; int a; };                      // a < 0: empty (the identity of the combine)
// the (max, first-arg) combine of a left and a right segment: the left one stays unless the right one is strictly greater
__device__ __forceinline__ Best combine(Best l, Best r) {
    const bool take_r = l.a < 0 || (r.a >= 0 && r.m > l.m);
    return take_r ? r : l;
}

struct Video {
    const int* __restrict__ rows;
    const int* __restrict__ order;
    const unsigned char* __restrict__ keep;
    long n_rows, n_acc;
    int first, cnt, V;
    // the packed row at position j of the video's order list if it takes part in the decode, else -1
    __device__ __forceinline__ int row_at(int j) const {
        const int r = order[first + j];
        if (r < 0 || r >= n_rows || (keep && !keep[r])) return -1;
        const long off = rows[2 * (long)r];
        if (rows[2 * (long)r + 1] != V || off < 0 || off + V > n_acc) return -1;
        return r;
    }
    __device__ __forceinline__ int next_kept(int j) const {
        while (j < cnt && row_at(j) < 0) ++j;
        return j;
    }
};

__device__ __forceinline__ void load_x(const float* __restrict__ p, int t_first, int V, float (&x)[DEC_E]) {
#pragma unroll
    for (int e = 0; e < DEC_E; ++e) x[e] = t_first + e < V ? p[t_first + e] : 0.0f;
}

__global__ void __launch_bounds__(DEC_THREADS) monotonic_decode_kernel(const float* __restrict__ sim, const int* __restrict__ rows,
                                                                       const int* __restrict__ order, const int* __restrict__ vtab,
                                                                       const unsigned char* __restrict__ keep, long n_rows, long n_acc,
                                                                       long n_run, int* __restrict__ bp, float* __restrict__ run,
                                                                       int* __restrict__ ts, float* __restrict__ path) {
    __shared__ float s_m[2][DEC_WAVES];
    __shared__ int s_a[2][DEC_WAVES];
    const int v = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    Video vd{rows, order, keep, n_rows, n_acc, vtab[3 * v], vtab[3 * v + 1], 0};
    const long roff = vtab[3 * v + 2];
    if (tid == 0) path[v] = 0.0f;
    if (vd.first < 0 || vd.cnt <= 0 || (long)vd.first + vd.cnt > n_rows) return;
    for (int j = tid; j < vd.cnt; j += DEC_THREADS) {
        const int r = order[vd.first + j];
        if (r >= 0 && r < n_rows) ts[r] = -1;
    }
    // the video's length: that of its first listed row; a row of another length (a broken table) takes no part
    const int r_first = order[vd.first];
    vd.V = r_first >= 0 && r_first < n_rows ? rows[2 * (long)r_first + 1] : 0;
    const int V = vd.V;
    if (V <= 0 || roff < 0 || roff + V > n_run) return;
    float* __restrict__ M = run + roff;

    int j = vd.next_kept(0);
    if (j >= vd.cnt) return;                          // no kept row: every ts is -1, path 0
    float xn[DEC_E];
    load_x(sim + rows[2 * (long)vd.row_at(j)], tid * DEC_E, V, xn);
    int j_last = j, step = 0;
    for (bool first_row = true; j < vd.cnt; first_row = false) {
        const int jn = vd.next_kept(j + 1);
        const long off = rows[2 * (long)vd.row_at(j)];
        const long off_n = jn < vd.cnt ? (long)rows[2 * (long)vd.row_at(jn)] : 0;
        Best carry{0.0f, -1};
        for (int t0 = 0; t0 < V; t0 += DEC_TILE, ++step) {
            const int tb = t0 + tid * DEC_E;
            float d[DEC_E], mp[DEC_E];
#pragma unroll
            for (int e = 0; e < DEC_E; ++e) {
                d[e] = xn[e];
                mp[e] = !first_row && tb + e < V ? M[tb + e] : 0.0f;
            }
            // the next step's similarities are in flight while this one scans
            if (t0 + DEC_TILE < V) load_x(sim + off, tb + DEC_TILE, V, xn);
            else if (jn < vd.cnt) load_x(sim + off_n, tid * DEC_E, V, xn);
            if (!first_row) {
#pragma unroll
                for (int e = 0; e < DEC_E; ++e) d[e] = add_rn(d[e], mp[e]);
            }
            Best own{0.0f, -1};                       // this thread's seconds
#pragma unroll
            for (int e = 0; e < DEC_E; ++e)
                if (tb + e < V) own = combine(own, Best{d[e], tb + e});
            Best inc = own;                           // inclusive scan over the wave's lanes
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const Best l{__shfl_up(inc.m, o, WAVE), __shfl_up(inc.a, o, WAVE)};
                if (lane >= o) inc = combine(l, inc);
            }
            Best exc{__shfl_up(inc.m, 1, WAVE), __shfl_up(inc.a, 1, WAVE)};       // the lanes to the left of this one
            if (lane == 0) exc.a = -1;
            const int buf = step & 1;                 // two LDS buffers: one barrier per step
            if (lane == WAVE - 1) { s_m[buf][wave] = inc.m; s_a[buf][wave] = inc.a; }
            __syncthreads();
            Best pre = carry;                         // everything to the left of this wave, then of this thread
#pragma unroll
            for (int w = 0; w < DEC_WAVES; ++w) {
                const Best tot{s_m[buf][w], s_a[buf][w]};
                if (w < wave) pre = combine(pre, tot);
                carry = combine(carry, tot);
            }
            pre = combine(pre, exc);
#pragma unroll
            for (int e = 0; e < DEC_E; ++e) {
                if (tb + e < V) {
                    pre = combine(pre, Best{d[e], tb + e});
                    M[tb + e] = pre.m;
                    bp[off + tb + e] = pre.a;
                }
            }
        }
        j_last = j;
        j = jn;
    }
    __syncthreads();                                  // every back-pointer and M of this workgroup is written
    if (tid == 0) {
        path[v] = M[V - 1];                           // = D_{m-1}[t_{m-1}]
        int t = V - 1;
        for (int jj = j_last; jj >= 0; --jj) {
            const int r = vd.row_at(jj);
            if (r < 0) continue;
            t = bp[rows[2 * (long)r] + t];
            if (t < 0 || t >= V) break;               // cannot happen with the pointers written above
            ts[r] = t;
        }
    }
}

}  // namespace
}  // namespace tal

using namespace tal;

extern "C" int tan_monotonic_decode(const float* sim, const int* rows, const int* order, const int* vtab, int n_videos,
                                    const unsigned char* keep, long n_rows, long n_acc, long n_run, int* bp, float* run, int* ts,
                                    float* path, void* stream) {
    TAN_REQUIRE(sim && rows && order && vtab && bp && run && ts && path);
    TAN_REQUIRE(n_videos > 0 && n_rows > 0 && n_acc > 0 && n_run > 0);
    hipLaunchKernelGGL(monotonic_decode_kernel, dim3(n_videos), dim3(DEC_THREADS), 0, (hipStream_t)stream, sim, rows, order, vtab,
                       keep, n_rows, n_acc, n_run, bp, run, ts, path);
    TAN_LAUNCH_CHECK();
    return 0;
}
