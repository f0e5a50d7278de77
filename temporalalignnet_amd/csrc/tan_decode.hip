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
//
// Further down: aligned intervals, a segmental decode over the same rows and tables (tan_segment_decode).
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

// ------------------------------------------------------------------------------------------------------------------------------------
// Aligned intervals: a segmental decode over the same kept rows (include/tan_hip.h, tan_segment_decode, has the definition).  With
// g_i[t] = x_i[t] - bias[r_i]:
//
//     c = G_{i-1}[t-1]   p = E_i[t-1]      E_i[t] = g_i[t] + max(p, c)      S_i[t] = t if c > p, else S_i[t-1]
//     G_i[t] = max(G_i[t-1], E_i[t])       B_i[t] = the smallest t' <= t with E_i[t'] == G_i[t]
//
// Serial in t, parallel in i -- the transpose of the kernel above.  One workgroup per video; the kept rows are compacted in decode
// order and taken in blocks of SEG_THREADS sentences, thread `tid` owning sentence lo + tid.  A block sweeps all V seconds: per second a
// thread takes its left neighbour's G[t-1] by one wave shuffle (lane 0 of waves 1..3 through two alternating LDS words, one barrier per
// second, none when the block fits one wave), does one add and three compares, and keeps E, G, S and the pair (S_i[B_i[t]], B_i[t]) in
// registers.  sim is [K, V] row-major, so rows are staged in tiles of SEG_T seconds: loaded coalesced along t into registers one tile
// ahead, put into LDS as [sentence][SEG_T] with an odd pitch and read transposed (lanes over sentences: conflict-free).  The pair goes
// out the same way: the start pointer overwrites the cell its x was read from, the end pointer has a tile of its own, and both are stored
// coalesced along t into the two planes of bp.  The last sentence of a block leaves its G row in `run` for the first sentence of the next
// block; second t0 + j of that row is loaded and later stored by the same thread j, so no fence orders those accesses.  Thread 0 walks
// the pairs backwards after a workgroup barrier, block by block, with the block's row list in LDS.
constexpr int SEG_THREADS = 256;                      // sentences per block
constexpr int SEG_T = 32;                             // seconds per staged tile
constexpr int SEG_PITCH = SEG_T + 1;                  // odd: lanes over sentences fall on distinct banks
constexpr int SEG_WAVES = SEG_THREADS / WAVE;
constexpr int SEG_ROWS_PER_PASS = SEG_THREADS / SEG_T;               // tile rows one pass of the workgroup's threads covers

struct SegShared {
    float x[SEG_THREADS * SEG_PITCH];                 // the x tile; each cell is overwritten by its start pointer once read
    int e[SEG_THREADS * SEG_PITCH];                   // the end pointers
    int row[SEG_THREADS], off[SEG_THREADS];           // the block's kept rows in decode order: packed row id, offset into sim
    int cnt[2][SEG_WAVES];
    float g[2][SEG_WAVES];                            // G[t] of each wave's last lane, for lane 0 of the next wave
    float cin[2][SEG_T], cout[SEG_T];                 // the previous block's G row (this tile, the tile before) / this block's
};

// The kept rows at positions [lo, lo + SEG_THREADS) of the video's compacted decode order -> sh.row / sh.off.  Returns the number of
// kept rows counted: all of them with `count_all`, else the scan stops once the block is full.  Ends with a barrier.
__device__ int seg_fill_block(const Video& vd, int lo, bool count_all, SegShared& sh) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int base = 0;
    for (int j0 = 0, it = 0; j0 < vd.cnt; j0 += SEG_THREADS, ++it) {
        const int r = j0 + tid < vd.cnt ? vd.row_at(j0 + tid) : -1;
        const unsigned long long mask = __ballot(r >= 0);
        if (lane == 0) sh.cnt[it & 1][wave] = __popcll(mask);
        __syncthreads();                              // two buffers: one barrier per round
        int pos = base - lo + __popcll(mask & ((1ull << lane) - 1));
#pragma unroll
        for (int w = 0; w < SEG_WAVES; ++w) {
            const int c = sh.cnt[it & 1][w];
            if (w < wave) pos += c;
            base += c;
        }
        if (r >= 0 && pos >= 0 && pos < SEG_THREADS) {
            sh.row[pos] = r;
            sh.off[pos] = vd.rows[2 * (long)r];
        }
        if (!count_all && base >= lo + SEG_THREADS) break;
    }
    __syncthreads();
    return base;
}

// the tile at t0 of the block's nb rows, coalesced along t: pass q covers tile rows [q * 8, q * 8 + 8), 32 lanes per row
__device__ __forceinline__ void seg_load_tile(const float* __restrict__ sim, const SegShared& sh, int nb, int t0, int V,
                                              float (&x)[SEG_T]) {
    const int i0 = threadIdx.x / SEG_T, t = t0 + threadIdx.x % SEG_T;
#pragma unroll
    for (int q = 0; q < SEG_T; ++q) {
        const int i = q * SEG_ROWS_PER_PASS + i0;
        x[q] = i < nb && t < V ? sim[(long)sh.off[i] + t] : 0.0f;
    }
}

__global__ void __launch_bounds__(SEG_THREADS) segment_decode_kernel(const float* __restrict__ sim, const int* __restrict__ rows,
                                                                     const int* __restrict__ order, const int* __restrict__ vtab,
                                                                     const unsigned char* __restrict__ keep,
                                                                     const float* __restrict__ bias, long n_rows, long n_acc, long n_run,
                                                                     int* __restrict__ bp, float* __restrict__ run,
                                                                     int* __restrict__ seg, float* __restrict__ path) {
    __shared__ SegShared sh;
    const int v = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    Video vd{rows, order, keep, n_rows, n_acc, vtab[3 * v], vtab[3 * v + 1], 0};
    const long roff = vtab[3 * v + 2];
    if (tid == 0) path[v] = 0.0f;
    if (vd.first < 0 || vd.cnt <= 0 || (long)vd.first + vd.cnt > n_rows) return;
    for (int j = tid; j < vd.cnt; j += SEG_THREADS) {
        const int r = order[vd.first + j];
        if (r >= 0 && r < n_rows) seg[2 * (long)r] = seg[2 * (long)r + 1] = -1;
    }
    // the video's length: that of its first listed row; a row of another length (a broken table) takes no part
    const int r_first = order[vd.first];
    vd.V = r_first >= 0 && r_first < n_rows ? rows[2 * (long)r_first + 1] : 0;
    const int V = vd.V;
    if (V <= 0 || roff < 0 || roff + V > n_run) return;
    float* __restrict__ R = run + roff;
    int* __restrict__ bp_s = bp;                      // plane 0: S_i[B_i[t]], plane 1: B_i[t]; both laid out like sim
    int* __restrict__ bp_e = bp + n_acc;

    const int m = seg_fill_block(vd, 0, true, sh);
    if (m == 0) return;                               // no kept row: every segment is (-1, -1), path 0
    const float NINF = -__builtin_inff();
    if (m > V) {                                      // more sentences than seconds: infeasible
        if (tid == 0) path[v] = NINF;
        return;
    }
    int* const sh_s = reinterpret_cast<int*>(sh.x);
    const int ti = tid / SEG_T, tt_io = tid % SEG_T;  // this thread's place in the coalesced tile passes
    for (int lo = 0; lo < m; lo += SEG_THREADS) {
        if (lo > 0) seg_fill_block(vd, lo, false, sh);
        const int nb = min(SEG_THREADS, m - lo);
        const bool hand_over = lo + SEG_THREADS < m;  // a block follows: it needs this block's last G row
        const float b = tid < nb ? bias[sh.row[tid]] : 0.0f;
        float E = NINF, G = NINF;
        int S = 0, Bs = 0, Be = 0;
        float xn[SEG_T];
        seg_load_tile(sim, sh, nb, 0, V, xn);
        for (int t0 = 0, k = 0; t0 < V; t0 += SEG_T, ++k) {
#pragma unroll
            for (int q = 0; q < SEG_T; ++q) sh.x[(q * SEG_ROWS_PER_PASS + ti) * SEG_PITCH + tt_io] = xn[q];
            if (lo > 0 && tid < SEG_T) sh.cin[k & 1][tid] = t0 + tid < V ? R[t0 + tid] : 0.0f;
            __syncthreads();
            if (t0 + SEG_T < V) seg_load_tile(sim, sh, nb, t0 + SEG_T, V, xn);        // in flight while this tile is swept
            const int nt = min(SEG_T, V - t0);
            for (int tt = 0; tt < nt; ++tt) {
                const int t = t0 + tt;
                float c = __shfl_up(G, 1, WAVE);      // G_{i-1}[t-1]
                if (lane == 0) {
                    if (wave > 0) c = sh.g[(t & 1) ^ 1][wave - 1];
                    else if (lo == 0) c = 0.0f;       // G_{-1} = 0
                    else c = tt > 0 ? sh.cin[k & 1][tt - 1] : sh.cin[(k & 1) ^ 1][SEG_T - 1];
                }
                if (t == 0) c = lo + tid == 0 ? 0.0f : NINF;
                const float g = sh.x[tid * SEG_PITCH + tt] - b;
                const bool open = c > E;              // a tie extends the running segment
                E = add_rn(g, open ? c : E);
                if (open) S = t;
                if (E > G) { G = E; Bs = S; Be = t; }
                sh_s[tid * SEG_PITCH + tt] = Bs;
                sh.e[tid * SEG_PITCH + tt] = Be;
                if (lane == WAVE - 1) sh.g[t & 1][wave] = G;
                if (tid == nb - 1) sh.cout[tt] = G;
                if (nb > WAVE) __syncthreads();       // two buffers of sh.g: one barrier per second
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < SEG_T; ++q) {
                const int i = q * SEG_ROWS_PER_PASS + ti;
                if (i < nb && t0 + tt_io < V) {
                    const long a = (long)sh.off[i] + t0 + tt_io;
                    bp_s[a] = sh_s[i * SEG_PITCH + tt_io];
                    bp_e[a] = sh.e[i * SEG_PITCH + tt_io];
                }
            }
            if (hand_over && tid < SEG_T && t0 + tid < V) R[t0 + tid] = sh.cout[tid];
            __syncthreads();
        }
        if (!hand_over && tid == nb - 1) path[v] = G;                  // = G_{m-1}[V-1]
    }
    // every pair of this workgroup is written (a barrier follows each tile's stores); the last block's row list is still in LDS
    int t = V - 1;
    for (int lo = (m - 1) / SEG_THREADS * SEG_THREADS; lo >= 0; lo -= SEG_THREADS) {
        if (lo + SEG_THREADS < m) seg_fill_block(vd, lo, false, sh);
        if (tid == 0) {
            for (int i = min(SEG_THREADS, m - lo) - 1; i >= 0 && t >= 0; --i) {
                const long a = (long)sh.off[i] + t;
                const int s = bp_s[a], e = bp_e[a];
                if (s < 0 || s > e || e > t) { t = -1; break; }       // cannot happen with the pairs written above
                const long r = sh.row[i];
                seg[2 * r] = s;
                seg[2 * r + 1] = e;
                t = s - 1;
            }
        }
        __syncthreads();                              // the list is read before the next block's overwrites it
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

extern "C" int tan_segment_decode(const float* sim, const int* rows, const int* order, const int* vtab, int n_videos,
                                  const unsigned char* keep, const float* bias, long n_rows, long n_acc, long n_run, int* bp,
                                  float* run, int* seg, float* path, void* stream) {
    TAN_REQUIRE(sim && rows && order && vtab && bias && bp && run && seg && path);
    TAN_REQUIRE(n_videos > 0 && n_rows > 0 && n_acc > 0 && n_run > 0);
    hipLaunchKernelGGL(segment_decode_kernel, dim3(n_videos), dim3(SEG_THREADS), 0, (hipStream_t)stream, sim, rows, order, vtab,
                       keep, bias, n_rows, n_acc, n_run, bp, run, seg, path);
    TAN_LAUNCH_CHECK();
    return 0;
}
