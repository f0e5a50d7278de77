// Chapters: cut a video into contiguous scenes by kernel temporal segmentation (tan_chapter_costs, tan_chapter_decode; the
// definition, bit for bit, is in include/tan_hip.h).  Over a video's own [V, V] block of second-by-second scores, as
// tan_sequence_scores writes it, the cost of making [s, e) one chapter is its within-segment scatter
//
//     J(s,e) = sum_{s<=t<e} fix(x[t][t]) - floor(sum_{s<=i,t<e} fix(x[i][t]) / (e - s)),
//
// and an exact dynamic programme picks the boundaries that minimise the summed cost plus a penalty per boundary.  Everything is a
// 64-bit integer (fix = cover_fix's image, tan_retrieve.hip), so nothing below depends on the order of a sum, on a tile shape or on
// how many waves run.
//
// The diagonal term folds into the square sum: with F'[i][t] = fix(x[i][t]) - fix(x[i][i]) (its diagonal is zero),
//     (e - s) * D(s,e) = sum_{s<=i,t<e} fix(x[i][i]),   so   J(s,e) = -floor(Q'(s,e) / (e - s)),   Q' = the square sum of F'
// exactly (D is an integer; |F'| <= 2^32 and |Q'| < 2^57 under the contract).  Q' splits at the diagonal:
//     lower  L(s,e) = sum_{i=s}^{e-1} RL[i][s],   RL[i][s] = sum_{t=s}^{i}   F'[i][t]     a scan DOWN column s from the diagonal
//     upper  U(s,e) = sum_{i=s}^{e-2} RU[i][e-1], RU[i][c] = sum_{t=i+1}^{c} F'[i][t]     a scan UP column e-1 from the diagonal
// L(s,e) lands at [e-1][s], where J(s,e) belongs; U(s,e) lands at the transposed place [s][e-1], in the half of the block that is
// the kernel's to use.  Three launches over all videos of a call, all in place in the int64 block:
//   1. chapter_rows_kernel: a wave per row; one pass sums the row up to the diagonal, a second scans it in 64-element steps with a
//      carry and writes RL left of the diagonal and RU right of it.  Reads x once more than it must (the second time from L2).
//   2. chapter_upper_kernel: a workgroup per 64-column strip of the upper triangle walks its 64 x 64 tiles from the diagonal up;
//      a thread scans 16 rows of one column, the four waves' partial sums and the carry from the tile below meet in LDS / registers.
//   3. chapter_costs_kernel: a workgroup per 64-column strip of the lower triangle walks its tiles from the diagonal down in the
//      same way, fetches the transposed upper tile THROUGH LDS (coalesced rows in, padded columns out), divides and writes J.
// A strip is a chain of at most 64 tile steps whose loads do not depend on one another; a video of V seconds has ceil(V / 64)
// strips per triangle in flight at once.
//
// The decode is the serial half and has tan_storyboard_select's structure: ONE workgroup of 16 waves per video runs every level,
// dp_{j-1} and dp_j live in LDS (2 x 4097 x 8 bytes), a wave takes an end e and reads row e - 1 of the costs from column
// (j-1) * min_len to e - min_len with 16-byte loads, CH_AHEAD per lane at a time; the first loads of the wave's NEXT row are issued
// before the last chunk of this row is consumed and reduced, so they are in flight across the wave reduction.  arg_j[e] goes into the
// caller's workspace as 16 bits.  Selection, backtrack and the chapter fill happen in the same launch: no scratch, no atomics.
// A video reads about min(k, V / min_len) * V^2 / 2 cost elements of 8 bytes through one workgroup: V and k near their limits
// together are a serial chain of minutes.
#include "tan_common.h"

#pragma clang fp contract(off)

namespace tal {
namespace {

constexpr int CH_MAX_V = 4096;
constexpr int CH_MAX_K = 256;
constexpr int CH_TILE = 64;                           // tile edge of the column scans
constexpr int CH_STRIPS = CH_MAX_V / CH_TILE;         // grid.y of the three cost launches
constexpr int CH_CT = 256;                            // threads of a cost workgroup: 4 waves x 16 rows of a tile
constexpr int CH_ROWS = CH_TILE / (CH_CT / WAVE);     // rows of a tile column one thread scans
constexpr int CH_WAVES = 16;                          // decode
constexpr int CH_THREADS = CH_WAVES * WAVE;
constexpr int CH_AHEAD = 4;                           // 16-byte loads a lane has in flight per chunk
constexpr long long CH_INF = 1LL << 62;
constexpr long long CH_MAX_G = 1LL << 50;

__device__ __forceinline__ long long ch_fix(float x) { return __float2ll_rn(x * 0x1p30f); }

__device__ __forceinline__ long long ch_wave_sum(long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, WAVE);
    return x;
}

// floor(a / n) toward minus infinity, 1 <= n <= 4096, |a| < 2^62: two double estimates (the first is within 2^10 of the quotient, the
// remainder it leaves is below 2^23 and its estimate is within one) and an integer fix-up
__host__ __device__ __forceinline__ long long ch_floor_div(long long a, int n) {
    const double inv = 1.0 / (double)n;
    long long q = (long long)((double)a * inv);
    long long r = a - q * n;
    q += (long long)__builtin_floor((double)r * inv);
    r = a - q * n;
    if (r < 0) { q -= 1; r += n; }
    if (r >= n) q += 1;
    return q;
}

// (block-uniform) the table entry of video p and whether its block lies inside the buffers
__device__ __forceinline__ bool ch_entry(const long* x_off, const int* table, long p, long n_x, int& V, long& off) {
    V = table[2 * p];
    off = x_off[p];
    return V >= 1 && V <= CH_MAX_V && off >= 0 && off <= n_x - (long)V * V;
}

// ---- 1. rows: RL left of the diagonal, RU right of it
__global__ void __launch_bounds__(CH_CT)
chapter_rows_kernel(const float* __restrict__ x, long n_x, const long* __restrict__ x_off, const int* __restrict__ table,
                    long long* __restrict__ cost) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    int V;
    long off;
    if (!ch_entry(x_off, table, blockIdx.x, n_x, V, off) || (int)blockIdx.y * CH_TILE >= V) return;
    for (int r = 0; r < CH_ROWS; ++r) {
        const int i = blockIdx.y * CH_TILE + wave * CH_ROWS + r;                   // wave-uniform
        if (i >= V) break;
        const float* xr = x + off + (long)i * V;
        long long* cr = cost + off + (long)i * V;
        const long long d = ch_fix(xr[i]);
        long long T = 0;                                                           // sum_{t<=i} F'[i][t]
        for (int t = lane; t <= i; t += WAVE) T += ch_fix(xr[t]) - d;
        T = ch_wave_sum(T);
        long long carry = 0;
        for (int c0 = 0; c0 < V; c0 += WAVE) {
            const int t = c0 + lane;
            const long long f = t < V ? ch_fix(xr[t]) - d : 0;
            long long inc = f;                                                     // inclusive scan over the lanes
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const long long up = __shfl_up(inc, o, WAVE);
                if (lane >= o) inc += up;
            }
            if (t < V) cr[t] = t <= i ? T - (carry + inc - f) : carry + inc - T;
            carry += __shfl(inc, WAVE - 1, WAVE);
        }
    }
}

// One 64 x 64 tile at rows r0, columns c0 of a video's block: thread (wave, lane) holds rows r0 + wave * 16 + j of column c0 + lane;
// only cells inside the block and on the wanted side of the diagonal are read, the others count as zero.  The column scan runs DOWN
// (lower = true: cell [r][c] becomes the sum of the cells above it in its column, this tile's and `carry`) or UP; `carry` is per
// column, the same in all four waves, and leaves as the column's total so far.  part: [4][64] in LDS.
template <bool LOWER>
__device__ __forceinline__ void ch_tile_scan(const long long* __restrict__ blk, int V, int r0, int c0, int wave, int lane,
                                             long long (&v)[CH_ROWS], long long& carry, long long (*part)[CH_TILE]) {
    const int c = c0 + lane, rw = r0 + wave * CH_ROWS;
#pragma unroll
    for (int j = 0; j < CH_ROWS; ++j) {
        const int r = rw + j;
        const bool in = r < V && c < V && (LOWER ? r >= c : r < c);
        v[j] = in ? blk[(long)r * V + c] : 0;
    }
    if (LOWER) {
#pragma unroll
        for (int j = 1; j < CH_ROWS; ++j) v[j] += v[j - 1];
    } else {
#pragma unroll
        for (int j = CH_ROWS - 2; j >= 0; --j) v[j] += v[j + 1];
    }
    __syncthreads();                                  // part is free: the tile before has been read by every thread
    part[wave][lane] = LOWER ? v[CH_ROWS - 1] : v[0];
    __syncthreads();
    long long before = carry, all = carry;
#pragma unroll
    for (int w = 0; w < CH_CT / WAVE; ++w) {
        const long long s = part[w][lane];
        all += s;
        if (LOWER ? w < wave : w > wave) before += s;
    }
#pragma unroll
    for (int j = 0; j < CH_ROWS; ++j) v[j] += before;
    carry = all;
}

// ---- 2. the upper triangle: column c from the diagonal up, U at [s][c]
__global__ void __launch_bounds__(CH_CT)
chapter_upper_kernel(long n_x, const long* __restrict__ x_off, const int* __restrict__ table, long long* __restrict__ cost) {
    __shared__ long long part[CH_CT / WAVE][CH_TILE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    int V;
    long off;
    const int c0 = blockIdx.y * CH_TILE;
    if (!ch_entry(x_off, table, blockIdx.x, n_x, V, off) || c0 >= V) return;
    long long* blk = cost + off;
    long long carry = 0, v[CH_ROWS];
    for (int r0 = c0; r0 >= 0; r0 -= CH_TILE) {
        ch_tile_scan<false>(blk, V, r0, c0, wave, lane, v, carry, part);
#pragma unroll
        for (int j = 0; j < CH_ROWS; ++j) {
            const int r = r0 + wave * CH_ROWS + j, c = c0 + lane;
            if (c < V && r < c) blk[(long)r * V + c] = v[j];
        }
    }
}

// ---- 3. the lower triangle: column s from the diagonal down, plus the transposed upper tile, divided: J(s,e) at [e-1][s]
__global__ void __launch_bounds__(CH_CT)
chapter_costs_kernel(long n_x, const long* __restrict__ x_off, const int* __restrict__ table, long long* __restrict__ cost) {
    __shared__ long long part[CH_CT / WAVE][CH_TILE];
    __shared__ long long tr[CH_TILE][CH_TILE + 1];    // the upper tile, row-major; read by columns: the odd stride spreads the banks
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    int V;
    long off;
    const int c0 = blockIdx.y * CH_TILE;
    if (!ch_entry(x_off, table, blockIdx.x, n_x, V, off) || c0 >= V) return;
    long long* blk = cost + off;
    long long carry = 0, v[CH_ROWS];
    for (int r0 = c0; r0 < V; r0 += CH_TILE) {
        // the upper tile at rows c0, columns r0: U(s,e) at [s][e-1]; its cells on or below the diagonal count as zero
        long long u[CH_ROWS];
#pragma unroll
        for (int j = 0; j < CH_ROWS; ++j) {
            const int s = c0 + wave * CH_ROWS + j, c = r0 + lane;
            u[j] = (c < V && s < c) ? blk[(long)s * V + c] : 0;
        }
        ch_tile_scan<true>(blk, V, r0, c0, wave, lane, v, carry, part);           // (its first barrier also frees tr)
#pragma unroll
        for (int j = 0; j < CH_ROWS; ++j) tr[wave * CH_ROWS + j][lane] = u[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CH_ROWS; ++j) {
            const int r = r0 + wave * CH_ROWS + j, s = c0 + lane;
            if (r < V && s <= r) blk[(long)r * V + s] = -ch_floor_div(v[j] + tr[lane][wave * CH_ROWS + j], r + 1 - s);
        }
    }
}

// ---- decode
struct ch_best {
    long long sum;
    int s;
};

__device__ __forceinline__ void ch_take(ch_best& b, long long sum, int s) {
    if (sum < b.sum || (sum == b.sum && s < b.s)) { b.sum = sum; b.s = s; }
}

// the row of end e at level j: columns lo .. e - min_len, from the pair that holds lo on (a pair starts at a 16-byte boundary)
struct ch_row {
    const long long* at;                              // the first pair's first element
    int s0, hi;                                       // its column; the last wanted column
};

__device__ __forceinline__ ch_row ch_row_of(const long long* blk, int V, int e, int lo, int min_len) {
    const long long* p = blk + (long)(e - 1) * V + lo;
    const int back = (int)((reinterpret_cast<uintptr_t>(p) >> 3) & 1u);            // lo >= 1: one column back stays inside the row
    return {p - back, lo - back, e - min_len};
}

__device__ __forceinline__ int ch_chunks(const ch_row& r) { return (r.hi - r.s0 + 2 * WAVE * CH_AHEAD) / (2 * WAVE * CH_AHEAD); }

// chunk c of a row into buf: a pair where both columns are at most hi, the single last column otherwise; nothing beyond hi is read
__device__ __forceinline__ void ch_load(longlong2 (&buf)[CH_AHEAD], const ch_row& r, int c, int lane) {
#pragma unroll
    for (int u = 0; u < CH_AHEAD; ++u) {
        const int i = 2 * ((c * CH_AHEAD + u) * WAVE + lane);
        const int s = r.s0 + i;
        if (s + 1 <= r.hi) buf[u] = *reinterpret_cast<const longlong2*>(r.at + i);
        else if (s <= r.hi) buf[u] = make_longlong2(r.at[i], 0);
    }
}

__global__ void __launch_bounds__(CH_THREADS)
chapter_decode_kernel(const long long* __restrict__ cost, long n_x, const long* __restrict__ x_off, const int* __restrict__ table,
                      long sum_V, int k, int min_len, long long G, int* __restrict__ count, int* __restrict__ start,
                      float* __restrict__ scatter, int* __restrict__ chapter, unsigned short* __restrict__ ws) {
    __shared__ long long dp[2][CH_MAX_V + 1];
    __shared__ long long fin[CH_MAX_K];               // dp_j[V] at [j - 1]
    __shared__ int st[CH_MAX_K + 1];
    __shared__ int n_chap;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const long p = blockIdx.x;
    int V;
    long off;
    const bool in = ch_entry(x_off, table, p, n_x, V, off);
    const long slot = table[2 * p + 1];
    int* sta = start + p * k;
    float* sca = scatter + p * k;
    // (block-uniform) an entry outside the limits: the empty result, its chapter slots untouched
    if (!(in && slot >= 0 && slot <= sum_V - V)) {
        for (int j = tid; j < k; j += CH_THREADS) {
            sta[j] = -1;
            sca[j] = __builtin_inff();
        }
        if (tid == 0) count[p] = 0;
        return;
    }
    const long long* blk = cost + off;
    unsigned short* arg = ws + slot * k;              // arg_j[e] at [(j - 1) * V + e - 1]
    // the levels that can be feasible: j * min_len <= V (j = 1 always is)
    int n_lev = V / min_len;
    n_lev = n_lev < 1 ? 1 : n_lev;
    n_lev = n_lev < k ? n_lev : k;
    for (int e = 1 + tid; e <= V; e += CH_THREADS) dp[0][e] = (e >= min_len || e == V) ? blk[(long)(e - 1) * V] : CH_INF;
    if (tid == 0) dp[0][0] = dp[1][0] = CH_INF;
    __syncthreads();
    if (tid == 0) fin[0] = dp[0][V];
    for (int j = 2; j <= n_lev; ++j) {
        const long long* prev = dp[j & 1];            // level j - 1 sits in dp[(j - 2) & 1]
        long long* next = dp[(j - 1) & 1];
        unsigned short* aj = arg + (long)(j - 1) * V;
        const int lo = (j - 1) * min_len, e_first = j * min_len;                   // 1 <= lo; every end from e_first on has a column
        for (int e = 1 + tid; e < e_first; e += CH_THREADS) {
            next[e] = CH_INF;
            aj[e - 1] = 0;
        }
        int e = e_first + wave;
        longlong2 buf[CH_AHEAD];
        ch_row row = ch_row_of(blk, V, e <= V ? e : V, lo, min_len);
        if (e <= V) ch_load(buf, row, 0, lane);
        while (e <= V) {                              // (wave-uniform)
            const int nc = ch_chunks(row);
            const ch_row cur_row = row;
            ch_best b = {CH_INF, 0xffff};
            for (int c = 0; c < nc; ++c) {
                longlong2 cur[CH_AHEAD];
#pragma unroll
                for (int u = 0; u < CH_AHEAD; ++u) cur[u] = buf[u];
                // the next loads go out before this chunk is consumed: the row's next chunk, or the first of the wave's next row
                if (c + 1 < nc) {
                    ch_load(buf, cur_row, c + 1, lane);
                } else if (e + CH_WAVES <= V) {
                    row = ch_row_of(blk, V, e + CH_WAVES, lo, min_len);
                    ch_load(buf, row, 0, lane);
                }
#pragma unroll
                for (int u = 0; u < CH_AHEAD; ++u) {
                    const int s = cur_row.s0 + 2 * ((c * CH_AHEAD + u) * WAVE + lane);
                    if (s >= lo && s <= cur_row.hi) {
                        const long long d = prev[s];
                        if (d < CH_INF) ch_take(b, d + cur[u].x, s);
                    }
                    if (s + 1 >= lo && s + 1 <= cur_row.hi) {
                        const long long d = prev[s + 1];
                        if (d < CH_INF) ch_take(b, d + cur[u].y, s + 1);
                    }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const long long os = __shfl_xor(b.sum, o, WAVE);
                const int oa = __shfl_xor(b.s, o, WAVE);
                ch_take(b, os, oa);
            }
            if (lane == 0) {
                next[e] = b.sum;
                aj[e - 1] = b.sum < CH_INF ? (unsigned short)b.s : (unsigned short)0;
            }
            e += CH_WAVES;
        }
        __syncthreads();                              // dp_j is complete (and arg_j visible to the block)
        if (tid == 0) fin[j - 1] = next[V];
    }
    __syncthreads();
    for (int j = tid; j < k; j += CH_THREADS)
        sca[j] = (j < n_lev && fin[j] < CH_INF) ? __ll2float_rn(fin[j]) * 0x1p-30f : __builtin_inff();
    if (tid == 0) {
        int best_j = 1;
        long long best = fin[0];
        for (int j = 2; j <= n_lev; ++j) {
            if (fin[j - 1] >= CH_INF) continue;
            const long long t = fin[j - 1] + (long long)(j - 1) * G;
            if (t < best) { best = t; best_j = j; }
        }
        int b = V;
        st[best_j] = V;
        for (int j = best_j; j >= 2; --j) {
            b = arg[(long)(j - 1) * V + b - 1];
            st[j - 1] = b;
        }
        st[0] = 0;
        n_chap = best_j;
        count[p] = best_j;
    }
    __syncthreads();
    const int n = n_chap;
    for (int c = tid; c < k; c += CH_THREADS) sta[c] = c < n ? st[c] : -1;
    int* chap = chapter + slot;
    for (int c = 0; c < n; ++c)
        for (int t = st[c] + tid; t < st[c + 1]; t += CH_THREADS) chap[t] = c;
}

}  // namespace
}  // namespace tal

using namespace tal;

extern "C" int tan_chapter_max_rows(void) { return CH_MAX_V; }

extern "C" int tan_chapter_costs(const float* x, long n_x, const long* x_off, const int* table, long P, long* cost, void* stream) {
    TAN_REQUIRE(x && x_off && table && cost);
    TAN_REQUIRE(n_x >= 1 && P >= 1 && P < (1L << 31));
    const dim3 grid((unsigned)P, CH_STRIPS);
    long long* c = reinterpret_cast<long long*>(cost);
    hipLaunchKernelGGL(chapter_rows_kernel, grid, dim3(CH_CT), 0, (hipStream_t)stream, x, n_x, x_off, table, c);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(chapter_upper_kernel, grid, dim3(CH_CT), 0, (hipStream_t)stream, n_x, x_off, table, c);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(chapter_costs_kernel, grid, dim3(CH_CT), 0, (hipStream_t)stream, n_x, x_off, table, c);
    TAN_LAUNCH_CHECK();
    return 0;
}

extern "C" long tan_chapter_decode_ws_bytes(long P, long sum_V, int k) {
    if (P < 1 || P >= (1L << 31) || sum_V < P || sum_V >= (1L << 31) || k < 1 || k > CH_MAX_K) return TAN_ERR_BAD_ARG;
    return sum_V * k * 2;
}

extern "C" int tan_chapter_decode(const long* cost, long n_x, const long* x_off, const int* table, long P, long sum_V, int k,
                                  int min_len, float penalty, int* count, int* start, float* scatter, int* chapter, void* ws,
                                  void* stream) {
    TAN_REQUIRE(cost && x_off && table && count && start && scatter && chapter && ws);
    TAN_REQUIRE(n_x >= 1 && P >= 1 && P < (1L << 31) && sum_V >= P && sum_V < (1L << 31));
    TAN_REQUIRE(k >= 1 && k <= CH_MAX_K && min_len >= 1 && min_len <= CH_MAX_V);
    TAN_REQUIRE(penalty >= 0.f && penalty - penalty == 0.f);              // finite and not negative
    // G = __float2ll_rn(penalty * 2^30f), clamped (the conversion saturates; host and device agree below 2^63)
    const float scaled = penalty * 0x1p30f;
    const long long G = scaled >= 0x1p50f ? CH_MAX_G : (long long)__builtin_rintf(scaled);
    hipLaunchKernelGGL(chapter_decode_kernel, dim3((unsigned)P), dim3(CH_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(cost), n_x, x_off, table, sum_V, k, min_len, G, count, start, scatter, chapter,
                       static_cast<unsigned short*>(ws));
    TAN_LAUNCH_CHECK();
    return 0;
}
