// Temporally consistent labels for corpus annotation: a per-video Viterbi decode over tan_label_topk's lists (tan_label_decode;
// the definition, bit for bit, is in include/tan_hip.h).
//
// Row t of a video has k + 1 states: list position j < k (lab = top_label[t, j], gain = top_score[t, j] - threshold, -inf for a
// score that is not finite) and the background state k (lab = -1, gain = 0).  A path pays switch_penalty wherever its label changes.
//
//     d[0][j] = gain(0, j)
//     m = max_i d[t-1][i]      a = the smallest i attaining it      rel[i] = d[t-1][i] - m
//     i* = the smallest i with lab(t-1, i) == lab(t, j)
//     (c, bp[t][j]) = (rel[i*], i*) if i* exists and rel[i*] >= -switch_penalty, else (-switch_penalty, a)
//     d[t][j] = c + gain(t, j)
//
// Every operation is one f32 add, subtract, max or compare (this file is compiled with contraction off), so the result is the
// same bits whatever the launch looks like.
//
// One WAVE per video, four waves per workgroup, lane j = state j (k + 1 <= 33 of the 64 lanes are live; the dead ones carry
// d = -inf, which never wins the maximum, and store nothing).  The waves of a workgroup share nothing: no barrier, every
// synchronisation below is inside one wave.  Per row:
//   * m by the DPP / permlane maximum of tan_common.h, a = the first set bit of the ballot of d == m;
//   * i* by a loop over the previous row's lanes KP .. 0, unrolled (KP: the smallest of 1, 2, 4, 8, 16, 32 that holds k): all the
//     v_readlanes of the previous labels first, then a compare and a select per lane; rel[i*] is then ONE cross-lane read
//     (ds_bpermute).  The loop is what k costs: 3 vector instructions per state, 13 ns measured;
//   * the lists of the next PF rows are already in registers (a ring of PF (score, label) pairs per lane, refilled as a row is
//     consumed), so the recurrence does not wait for memory -- the chain is latency-bound, not bandwidth-bound;
//   * the back-pointers of the row go to the scratch as k + 1 consecutive bytes, one per live lane.
// The walk back reads the back-pointers in blocks of 64 rows: the wave copies a block (<= 64 * 33 bytes, dword loads from the
// aligned-down address) into its LDS slice, every lane walks the block's 64 dependent LDS bytes (uniform address: a broadcast), lane
// r keeps the state of the block's row r, and the 64 rows' outputs are gathered from the lists and stored coalesced.  A dependent
// GLOBAL load per row would cost a memory latency per second instead of an LDS latency.
// The back-pointers are written and read by the lanes of ONE wave: a workgroup-scope fence (the wave's outstanding stores
// complete; a CU's L1 is write-through and shared by the wave's own later loads) orders the two phases.
// A video of any length works; one very long video is one wave's serial chain (documented in the header).
#include "tan_common.h"

#include <type_traits>

#pragma clang fp contract(off)

namespace tal {
namespace {

constexpr int LD_WAVES = 4;                           // videos per workgroup
constexpr int LD_KMAX = 32;
constexpr int LD_PF = 8;                              // rows of lists in flight per lane
constexpr int LD_BLOCK = 64;                          // rows per back-pointer block of the walk back
constexpr int LD_STAGE_DW = (LD_BLOCK * (LD_KMAX + 1) + 3 + 3) / 4 + 1;      // a block from its aligned-down address, in dwords
constexpr int LD_DEAD = (int)0x80000000;              // the "label" of a lane above k: a match with it is discarded (i* > k)

inline long ld_ws_bytes(long N, int k) { return (N * (k + 1) + 15) / 16 * 16 + 16; }       // + 16: the scratch is aligned inside ws

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// the smallest lane whose d equals the wave's maximum (every lane gets it); dead lanes hold -inf and m is finite
__device__ __forceinline__ int first_max_lane(float d, float& m) {
    m = wave_max(d);
    const unsigned long long at = __ballot(d == m);
    return at ? __builtin_ctzll(at) : 0;              // at == 0 only for a NaN in d (an overflowed gain: caller's error)
}

// KP: the smallest of 1, 2, 4, 8, 16, 32 that is >= k -- the match loop is unrolled over the lanes KP .. 0
template <int KP>
__global__ void __launch_bounds__(LD_WAVES * WAVE)
label_decode_kernel(const float* __restrict__ ts, const int* __restrict__ tl, int k, long N, const int* __restrict__ v_off, int n_videos,
                    float thr, float pen, int* __restrict__ dec_label, float* __restrict__ dec_score, unsigned char* __restrict__ bp) {
    __shared__ unsigned int stage_all[LD_WAVES][LD_STAGE_DW];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const long v = (long)blockIdx.x * LD_WAVES + wave;
    if (v >= n_videos) return;                        // the whole wave: nothing below is shared between waves
    // the video's rows, clamped: whatever v_off holds, [r0, r0 + T) lies inside [0, N)
    long r0 = v_off[v], r1 = v_off[v + 1];
    r0 = r0 < 0 ? 0 : (r0 > N ? N : r0);
    r1 = r1 < r0 ? r0 : (r1 > N ? N : r1);
    const int T = (int)(r1 - r0);
    if (T <= 0) return;
    const int S = k + 1;                              // states per row
    const bool is_list = lane < k, live = lane < S;
    const int col = is_list ? lane : k - 1;           // every lane loads (no branch around a load in flight); the lanes >= k discard
    const float npen = -pen;

    // ---- forward: d over the rows, back-pointers to the scratch ----
    float rs[LD_PF];
    int rl[LD_PF];
#pragma unroll
    for (int u = 0; u < LD_PF; ++u) {
        const long n = r0 + (u < T ? u : T - 1);
        rs[u] = ts[n * k + col];
        rl[u] = tl[n * k + col];
    }
    float d = -INFINITY;
    int plab = LD_DEAD;
    for (int t0 = 0; t0 < T; t0 += LD_PF) {
#pragma unroll
        for (int u = 0; u < LD_PF; ++u) {
            const int t = t0 + u;
            const float sc = rs[u];
            const int lab = is_list ? rl[u] : (live ? -1 : LD_DEAD);
            {                                         // refill the slot with row t + PF (clamped to the video: never out of bounds)
                const long n = r0 + (t + LD_PF < T ? t + LD_PF : T - 1);
                rs[u] = ts[n * k + col];
                rl[u] = tl[n * k + col];
            }
            if (t < T) {                              // uniform
                const float gain = is_list ? (finite_f(sc) ? sc - thr : -INFINITY) : (live ? 0.f : -INFINITY);
                if (t == 0) {
                    d = gain;
                } else {
                    float m;
                    const int a = first_max_lane(d, m);
                    const float rel = d - m;
                    int istar = -1;
                    int pl[KP + 1];                   // all the v_readlanes first: a compare need not wait for its scalar
#pragma unroll
                    for (int i = 0; i <= KP; ++i) pl[i] = __builtin_amdgcn_readlane(plab, i);
#pragma unroll
                    for (int i = KP; i >= 0; --i)     // descending: the smallest matching i is written last
                        istar = pl[i] == lab ? i : istar;
                    istar = istar > k ? -1 : istar;   // a dead lane's LD_DEAD matched a label of that value: no match
                    const float r = __shfl(rel, istar < 0 ? 0 : istar);
                    const bool stay = istar >= 0 && r >= npen;
                    const float c = stay ? r : npen;
                    d = c + gain;
                    if (live) bp[(r0 + t) * S + lane] = (unsigned char)(stay ? istar : a);
                }
                plab = lab;
            }
        }
    }
    float m;
    int s = first_max_lane(d, m);                     // the last row's state: the smallest j attaining max d

    // the wave's back-pointer stores complete before any lane of it loads them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

    // ---- walk back, 64 rows at a time ----
    unsigned int* stage = stage_all[wave];
    const unsigned char* sbytes = reinterpret_cast<const unsigned char*>(stage);
    for (int tb = (T - 1) / LD_BLOCK * LD_BLOCK; tb >= 0; tb -= LD_BLOCK) {
        const int rows = T - tb < LD_BLOCK ? T - tb : LD_BLOCK;
        const unsigned char* first = bp + (r0 + tb) * S;
        const int skew = (int)(reinterpret_cast<uintptr_t>(first) & 3);
        const unsigned int* base = reinterpret_cast<const unsigned int*>(first - skew);      // >= bp (16-byte aligned); the last
        const int ndw = (skew + rows * S + 3) / 4;                                           // dword ends inside ws; <= LD_STAGE_DW
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // the previous block's LDS reads are over
        for (int i = lane; i < ndw; i += WAVE)                      // L2-served loads (sc1): no L1 line decides what the walk reads
            stage[i] = __hip_atomic_load(base + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // the slice is written before it is walked
        int mine = k;
        for (int r = rows - 1; r >= 0; --r) {
            mine = lane == r ? s : mine;
            if (tb + r > 0) {                                       // row 0 has no back-pointer
                const int b = sbytes[skew + r * S + s];
                s = b > k ? k : b;                                  // a byte this wave wrote is <= k; clamped all the same
            }
        }
        if (lane < rows) {
            const long n = r0 + tb + lane;
            const bool bg = mine >= k;
            const int at = bg ? 0 : mine;
            const int lab = tl[n * k + at];
            const float sc = ts[n * k + at];
            dec_label[n] = bg ? -1 : lab;
            dec_score[n] = bg ? -INFINITY : sc;
        }
    }
}

}  // namespace
}  // namespace tal

using namespace tal;

extern "C" long tan_label_decode_ws_bytes(long N, int k) {
    if (N < 1 || N >= (1L << 31) || k < 1 || k > LD_KMAX) return TAN_ERR_BAD_ARG;
    return ld_ws_bytes(N, k);
}

extern "C" int tan_label_decode(const float* top_score, const int* top_label, int k, long N, const int* v_off, long n_videos,
                                float threshold, float switch_penalty, int* dec_label, float* dec_score, void* ws, void* stream) {
    TAN_REQUIRE(top_score && top_label && v_off && dec_label && dec_score && ws);
    TAN_REQUIRE(k >= 1 && k <= LD_KMAX && N >= 1 && N < (1L << 31) && n_videos >= 1 && n_videos <= N);
    TAN_REQUIRE(threshold - threshold == 0.f && switch_penalty >= 0.f);      // a finite threshold; a penalty in [0, +inf], not NaN
    unsigned char* bp = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(ws) + 15) & ~(uintptr_t)15);
    const dim3 grid(cdiv(n_videos, LD_WAVES)), block(LD_WAVES * WAVE);
    auto launch = [&](auto kp) {
        hipLaunchKernelGGL(label_decode_kernel<decltype(kp)::value>, grid, block, 0, (hipStream_t)stream, top_score, top_label, k, N, v_off,
                           (int)n_videos, threshold, switch_penalty, dec_label, dec_score, bp);
    };
    if (k <= 1) launch(std::integral_constant<int, 1>());
    else if (k <= 2) launch(std::integral_constant<int, 2>());
    else if (k <= 4) launch(std::integral_constant<int, 4>());
    else if (k <= 8) launch(std::integral_constant<int, 8>());
    else if (k <= 16) launch(std::integral_constant<int, 16>());
    else launch(std::integral_constant<int, 32>());
    TAN_LAUNCH_CHECK();
    return 0;
}
