// Storyboards: the k seconds that together cover a video best (tan_storyboard_select; the definition, bit for bit, is in
// include/tan_hip.h).  Greedy facility location over a video's own [V, V] block of second-by-second scores, as tan_sequence_scores
// writes it: entry j is the row s whose scores, taken together with what the earlier entries already cover, sum highest,
//
//     T_j(s) = sum_t max(fix(x[s][t]), C_{j-1}[t]),      C_j[t] = max(C_{j-1}[t], fix(x[s_j][t])),
//
// in 64-bit fixed point (fix = cover_fix's image, tan_retrieve.hip): every sum is an integer, so nothing below depends on the order
// of a reduction, on the number of waves or on how a row is cut into vector loads.
//
// One WORKGROUP per video (SB_WAVES waves); it runs all k iterations itself: no host round trip, no global atomics, no scratch.
//   * C lives in LDS: 4096 x int64 = 32 KiB.
//   * Candidate pass: wave w takes rows w, w + SB_WAVES, ...; a row is read once per iteration, 16 bytes per lane (up to three
//     leading and three trailing elements, where the row is not 16-byte aligned, go through single lanes), and reduced against C with
//     64-bit integer compares and adds; one wave reduction per row gives T(s).  A wave keeps its best row under strict >: its rows
//     ascend, so that is the lowest s among equals.  The waves' bests meet in LDS and every thread folds them by (T, lowest s).
//   * Update pass: the block walks row s_j once, raises C, writes owner where the row is strictly better, and reduces the new sum
//     of C (the next iteration's stop test and this entry's coverage).
// A video costs min(k, V) * V * V score reads of 4 bytes; k and V near their limits together are a long serial chain on one CU.
#include "tan_common.h"

#pragma clang fp contract(off)

namespace tal {
namespace {

constexpr int SB_MAX_V = 4096;                        // rows of C in LDS
constexpr int SB_MAX_K = 4096;
constexpr int SB_WAVES = 16;
constexpr int SB_THREADS = SB_WAVES * WAVE;
constexpr int SB_AHEAD = 4;                           // 16-byte loads a lane has in flight
constexpr long long SB_FLOOR = -(1LL << 62);          // C_0: below every image
constexpr long long SB_MAX_GMIN = 1LL << 40;          // G_min is clamped here: no gain per second reaches it, and G_min * V < 2^52

// cover_fix's image of a score: the multiply by 2^30 is exact.  For |x| < 2 -- every score of unit rows short of an exact +-2 -- the
// image fits 32 bits and v_cvt_i32_f32 (round to nearest even) makes it; the 64-bit conversion costs a dozen instructions, so a wave
// takes it only when one of its lanes needs it (a wave-uniform branch on a ballot; a NaN goes the wide way too).
__device__ __forceinline__ bool sb_narrow(float y) { return __builtin_fabsf(y) < 0x1p31f; }

__device__ __forceinline__ long long sb_fix(float x) {
    const float y = x * 0x1p30f;
    if (__builtin_amdgcn_ballot_w64(!sb_narrow(y)) == 0) return (long long)__float2int_rn(y);
    return __float2ll_rn(y);
}

__device__ __forceinline__ long long sb_wave_sum(long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, WAVE);
    return x;
}

__device__ __forceinline__ long long sb_max(long long f, long long c) { return f > c ? f : c; }

__device__ __forceinline__ long long sb_term(float x, long long c) { return sb_max(sb_fix(x), c); }

// sum of max(fix(v), c) over four consecutive scores
__device__ __forceinline__ long long sb_term4(const float4 v, const long long* c) {
    const float y0 = v.x * 0x1p30f, y1 = v.y * 0x1p30f, y2 = v.z * 0x1p30f, y3 = v.w * 0x1p30f;
    const bool narrow = sb_narrow(y0) && sb_narrow(y1) && sb_narrow(y2) && sb_narrow(y3);
    long long f0, f1, f2, f3;
    if (__builtin_amdgcn_ballot_w64(!narrow) == 0) {
        f0 = __float2int_rn(y0); f1 = __float2int_rn(y1); f2 = __float2int_rn(y2); f3 = __float2int_rn(y3);
    } else {
        f0 = __float2ll_rn(y0); f1 = __float2ll_rn(y1); f2 = __float2ll_rn(y2); f3 = __float2ll_rn(y3);
    }
    return (sb_max(f0, c[0]) + sb_max(f1, c[1])) + (sb_max(f2, c[2]) + sb_max(f3, c[3]));
}

// sum_t max(fix(row[t]), C[t]) over t < V, by one wave; the result in every lane.  Only addresses inside row[0, V) are read.  The
// loads of a step are issued before anything waits: the unaligned head and tail, and SB_AHEAD vectors per lane (a row of up to
// 1024 + 6 scores is one such step).
__device__ __forceinline__ long long sb_row_sum(const float* __restrict__ row, const long long* C, int V, int lane) {
    int head = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u)) & 3u);      // elements before a 16-byte boundary
    head = head < V ? head : V;
    const int nvec = (V - head) >> 2, tail0 = head + 4 * nvec;
    const float4* body = reinterpret_cast<const float4*>(row + head);
    const int edge = lane < head ? lane : (lane >= 4 && tail0 + lane - 4 < V ? tail0 + lane - 4 : -1);     // lanes 0..2 / 4..6
    const float e = row[edge >= 0 ? edge : 0];       // unconditional (V >= 1) and used last: it is in flight under the vectors
    long long T = 0;
    for (int b0 = 0; b0 < nvec; b0 += SB_AHEAD * WAVE) {              // b0 and the guards on it are wave-uniform
        float4 v[SB_AHEAD];
#pragma unroll
        for (int u = 0; u < SB_AHEAD; ++u) {
            const int i = b0 + u * WAVE + lane;
            if (b0 + u * WAVE < nvec) v[u] = body[i < nvec ? i : nvec - 1];
        }
#pragma unroll
        for (int u = 0; u < SB_AHEAD; ++u) {
            const int i = b0 + u * WAVE + lane;
            if (b0 + u * WAVE < nvec) {
                const long long t = sb_term4(v[u], C + head + 4 * (i < nvec ? i : nvec - 1));
                T += i < nvec ? t : 0;
            }
        }
    }
    if (edge >= 0) T += sb_term(e, C[edge]);
    return sb_wave_sum(T);
}

__global__ void __launch_bounds__(SB_THREADS)
storyboard_select_kernel(const float* __restrict__ x, long n_x, const long* __restrict__ x_off, const int* __restrict__ table, long sum_V,
                         int k, long long g_min, int* __restrict__ second, float* __restrict__ coverage, int* __restrict__ owner) {
    __shared__ long long C[SB_MAX_V];
    __shared__ long long red_t[SB_WAVES];
    __shared__ int red_s[SB_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const long p = blockIdx.x;
    const int V = table[2 * p];
    const long slot = table[2 * p + 1], off = x_off[p];
    int* sec = second + p * k;
    float* cov = coverage + p * k;
    // (block-uniform) an entry outside the limits: the empty result, its owner slots untouched
    const bool ok = V >= 1 && V <= SB_MAX_V && off >= 0 && off <= n_x - (long)V * V && slot >= 0 && slot <= sum_V - V;
    int done = 0;
    if (ok) {
        const float* xb = x + off;
        int* own = owner + slot;
        for (int t = tid; t < V; t += SB_THREADS) C[t] = SB_FLOOR;
        __syncthreads();
        long long sum_c = 0;                          // sum_t C_{j-1}[t]; unused while j == 0
        const int n_it = k < V ? k : V;
        for (int j = 0; j < n_it; ++j) {
            // candidates: this wave's best row under strict >, rows ascending
            long long best = 0;
            int best_s = -1;
            for (int s = wave; s < V; s += SB_WAVES) {
                const long long T = sb_row_sum(xb + (long)s * V, C, V, lane);
                if (best_s < 0 || T > best) { best = T; best_s = s; }
            }
            if (lane == 0) { red_t[wave] = best; red_s[wave] = best_s; }
            __syncthreads();
            best = red_t[0];
            best_s = red_s[0];                        // V >= 1: wave 0 always has row 0
#pragma unroll
            for (int w = 1; w < SB_WAVES; ++w) {
                const long long T = red_t[w];
                const int s = red_s[w];
                if (s >= 0 && (T > best || (T == best && s < best_s))) { best = T; best_s = s; }
            }
            if (j >= 1) {
                const long long gain = best - sum_c;
                if (gain <= 0 || gain < g_min * V) break;              // (block-uniform)
            }
            // row s_j raises C and takes the seconds it shows strictly better
            const float* row = xb + (long)best_s * V;
            long long part = 0;
            for (int t = tid; t < V; t += SB_THREADS) {
                const long long f = sb_fix(row[t]);
                long long c = C[t];
                if (f > c) {
                    C[t] = c = f;
                    own[t] = j;
                }
                part += c;
            }
            part = sb_wave_sum(part);
            __syncthreads();                          // red_t / red_s have been read by every thread
            if (lane == 0) red_t[wave] = part;
            __syncthreads();                          // ... and C is complete before the next candidate pass
            sum_c = 0;
#pragma unroll
            for (int w = 0; w < SB_WAVES; ++w) sum_c += red_t[w];
            if (tid == 0) {
                sec[j] = best_s;
                cov[j] = __fdiv_rn(__ll2float_rn(sum_c) * 0x1p-30f, (float)V);
            }
            done = j + 1;
            __syncthreads();                          // red_t is free for the next iteration's bests
        }
    }
    for (int j = done + tid; j < k; j += SB_THREADS) {
        sec[j] = -1;
        cov[j] = 0.f;
    }
}

}  // namespace
}  // namespace tal

using namespace tal;

extern "C" int tan_storyboard_max_rows(void) { return SB_MAX_V; }

extern "C" int tan_storyboard_select(const float* x, long n_x, const long* x_off, const int* table, long P, long sum_V, int k,
                                     float min_gain, int* second, float* coverage, int* owner, void* stream) {
    TAN_REQUIRE(x && x_off && table && second && coverage && owner);
    TAN_REQUIRE(n_x >= 1 && P >= 1 && P < (1L << 31) && sum_V >= P && sum_V < (1L << 31));
    TAN_REQUIRE(k >= 1 && k <= SB_MAX_K);
    TAN_REQUIRE(min_gain >= 0.f && min_gain - min_gain == 0.f);          // finite and not negative
    // G_min = __float2ll_rn(min_gain * 2^30f), clamped (the conversion saturates; host and device agree below 2^63)
    const float scaled = min_gain * 0x1p30f;
    const long long g_min = scaled >= 0x1p40f ? SB_MAX_GMIN : (long long)__builtin_rintf(scaled);
    hipLaunchKernelGGL(storyboard_select_kernel, dim3((unsigned)P), dim3(SB_THREADS), 0, (hipStream_t)stream, x, n_x, x_off, table, sum_V,
                       k, g_min, second, coverage, owner);
    TAN_LAUNCH_CHECK();
    return 0;
}
