// Copy alignment: the best LOCAL alignment of a query's seconds with a video's seconds, steps in either axis allowed
// (tan_local_align; the definition, bit for bit, is in include/tan_hip.h).
//
// A block is a row-major [m, V] f32 matrix x (query second i along the rows, video second j along the columns), as
// tan_sequence_scores writes it for one hit.  With H[-1][*] = H[*][-1] = 0:
//
//     g = x[i][j] - theta;   diag = H[i-1][j-1];   up = H[i-1][j] - skew;   left = H[i][j-1] - skew
//     P = max(diag, up, left), pred = the first of (diag, up, left) attaining it;   H[i][j] = max(0, g + P)
//
// and every positive cell carries the origin of its path and the number of its cells.  Every operation is one f32 add, subtract,
// max or compare (this file is compiled with contraction off), and a cell is a fixed function of three neighbours, so the result is
// the same bits whatever the launch looks like.
//
// One WAVE per block, four waves per workgroup; the waves of a workgroup share nothing: no barrier, every synchronisation below
// is inside one wave.  The query is cut into STRIPS of 64 rows and lane r stands over row r of the strip.  The wave walks the
// strip's anti-diagonals: at step d lane r owns cell (r, d - r).  Then
//   * left is the lane's own previous value, up is lane r - 1's previous value and diag is what the lane received as `up` one step
//     earlier: ONE lane shift per carried quantity per step (DPP wave_shr:1, whose `old` operand feeds lane 0) and no scan;
//   * the carried quantities are H, the origin packed into one word (row << 20 | column: 12 + 20 bits under the limits) and the
//     cell count;
//   * the scores are staged in 64 x 64 slabs: 64 coalesced row loads into registers, stored to the wave's LDS slice at pitch 64 and
//     read back skewed -- lane r reads word 64 r + ((d - r) & 63), so the 64 lanes of a read fall into 64 different banks, as the
//     lanes of the row-wise store do (a pitch of 65 would put every lane of the skewed read into bank d & 63).  Two slabs are live
//     (a diagonal of the strip spans two), and the loads of slab s + 1 are issued before the 64 steps over slab s: the chain is
//     latency-bound and does not wait for memory;
//   * the last live lane of a strip stores (H, origin, cells) of every column to a boundary row in ws, one 16-byte vector store
//     per step; lane 0 of the next strip receives that row as its up / diag, read in blocks of 64 columns one block ahead.  Strips
//     alternate between two boundary rows, so a row is never read and written in the same strip; an agent-scope release / acquire
//     fence between two strips completes the stores and drops the L1 lines before the loads;
//   * every lane keeps a running (best, end, origin, cells) under strict >: columns ascend inside a strip and strips come in
//     ascending rows, so a lane holds the first cell of its rows in (i, j) order that attains its best, and one wave reduction at
//     the end gives max H, then the smallest i (rows of different lanes differ), then that lane's j.
// The strips of one block run one after the other in one wave: a long query is one wave's serial chain (documented in the header).
//
// tan_local_align_path is the same kernel with a TRACE: per (strip, anti-diagonal) one 16-byte entry, the two ballots of the lanes'
// 2-bit codes (0 start, 1 diag, 2 up, 3 left), written by lane 0 with a vector store; the code of cell (i, j) is bit i & 63 of entry
// (i >> 6, j + (i & 63)).  After the last strip's release / acquire the same wave walks the best path back: inside a strip the walk
// only descends in d, so it loads 64 consecutive entries at once, steps through them with v_readlane and reloads when it leaves the
// window or the strip.  The map is collected in the wave's LDS slice (free by then, and exactly 2 x 4096 words) and written coalesced.
#include "tan_common.h"

#pragma clang fp contract(off)

namespace tal {
namespace {

constexpr int LA_WAVES = 4;                           // blocks per workgroup
constexpr int LA_S = 64;                              // rows per strip: one per lane
constexpr int LA_W = 64;                              // columns per slab
constexpr int LA_SLAB = LA_S * LA_W;                  // floats per slab, pitch LA_W
constexpr int LA_MAX_M = 4096;                        // 12 bits of the packed origin
constexpr int LA_COL_BITS = 20;                       // V < 2^20
constexpr unsigned LA_COL_MASK = (1u << LA_COL_BITS) - 1u;
constexpr long LA_MAX_TRACE = 1L << 35;               // trace entries of one launch (16 bytes each)
constexpr int LA_SHR1 = 0x138;                        // DPP wave_shr:1: lane r receives lane r - 1's value, lane 0 keeps `old`

inline long la_ws_bytes(long sum_V) { return 2 * sum_V * 16 + 16; }      // two boundary rows of 16-byte entries; + 16: aligned inside ws

__device__ __forceinline__ int shr1(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, LA_SHR1, 0xf, 0xf, false); }
__device__ __forceinline__ float shr1(float old, float v) { return __int_as_float(shr1(__float_as_int(old), __float_as_int(v))); }

// rows i0 .. i0 + 63, columns c0 .. c0 + 63 of the block, lane = column: 64 coalesced loads.  Rows and columns past the block are
// clamped into it (never out of bounds); their values are never used.
__device__ __forceinline__ void load_slab(float (&pf)[LA_S], const float* __restrict__ xb, int i0, int c0, int m, int V, int lane) {
    const int col = c0 + lane < V ? c0 + lane : V - 1;
#pragma unroll
    for (int k = 0; k < LA_S; ++k) {
        const int row = i0 + k < m ? i0 + k : m - 1;
        pf[k] = xb[(long)row * V + col];
    }
}

// what tan_local_align_path adds to the arguments: path_off / n_map / n_trace / qmap as it takes them, tr: the trace in ws
struct la_path_args {
    const long* path_off;
    long n_map, n_trace;
    int* qmap;
    uint4* tr;
};
template <class T> __device__ __forceinline__ const T& la_first(const T& t) { return t; }

// Both kernels.  local_align_kernel<> is tan_local_align's, with tan_local_align's own argument list; local_align_kernel<la_path_args>
// (TRACE) also records every step's codes, walks the best path back and writes the block's time map.
template <class... PA>
__global__ void __launch_bounds__(LA_WAVES * WAVE)
local_align_kernel(const float* __restrict__ x, long n_x, const long* __restrict__ x_off, const int* __restrict__ table, int P, long sum_V,
                   float theta, float skew, float* __restrict__ score, int* __restrict__ span, uint4* brow, PA... pa) {
    constexpr bool TRACE = sizeof...(PA) != 0;
    __shared__ float slab_all[LA_WAVES][2 * LA_SLAB];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const long p = (long)blockIdx.x * LA_WAVES + wave;
    if (p >= P) return;                               // the whole wave: nothing below is shared between waves
    const int m = table[3 * p], V = table[3 * p + 1];
    const long slot = table[3 * p + 2], off = x_off[p];
    bool ok = m >= 1 && m <= LA_MAX_M && V >= 1 && V <= (int)LA_COL_MASK && (long)m * V < (1L << 31) && off >= 0 &&
              off <= n_x - (long)m * V && slot >= 0 && slot <= sum_V - V;
    long moff = 0;
    uint4* tp = nullptr;                              // the block's trace: entry strip * (V + 63) + d
    if constexpr (TRACE) {
        const la_path_args& a = la_first(pa...);
        moff = a.path_off[2 * p];
        const long toff = a.path_off[2 * p + 1];
        // (ok first: m and V are then inside their limits and the products below are small)
        ok = ok && moff >= 0 && moff <= a.n_map - m && toff >= 0 && toff <= a.n_trace - (long)((m + LA_S - 1) / LA_S) * (V + LA_S - 1);
        tp = a.tr + toff;
    }
    if (!ok) {                                        // (wave-uniform) a skipped entry: the empty result, nothing else touched
        if (lane == 0) {
            score[p] = 0.f;
            span[5 * p] = span[5 * p + 1] = span[5 * p + 2] = span[5 * p + 3] = -1;
            span[5 * p + 4] = 0;
        }
        return;
    }
    const float* xb = x + off;
    float* slab = slab_all[wave];
    float best = 0.f;
    unsigned bend = 0, borg = 0;
    int bcells = 0;

    for (int i0 = 0, strip = 0; i0 < m; i0 += LA_S, ++strip) {
        const int R = m - i0 < LA_S ? m - i0 : LA_S;  // live rows of the strip
        const bool has_prev = strip > 0, has_next = i0 + LA_S < m;
        const uint4* rd = brow + (long)((strip & 1) ^ 1) * sum_V + slot;       // the previous strip's last row
        uint4* wr = brow + (long)(strip & 1) * sum_V + slot;                   // this strip's
        const int row = i0 + lane;
        const bool rowlive = lane < R, writer = has_next && lane == R - 1;
        const int nsteps = V + R - 1;                 // anti-diagonals of the strip
        [[maybe_unused]] uint4* tstrip = TRACE ? tp + (long)strip * (V + LA_S - 1) : nullptr;
        float H = 0.f, dH = 0.f;                      // own previous value (left); the `up` of one step earlier (diag)
        unsigned O = 0, dO = 0;
        int Cn = 0, dC = 0;
        float pf[LA_S];
        load_slab(pf, xb, i0, 0, m, V, lane);
        uint4 bnext = make_uint4(0, 0, 0, 0);
        if (has_prev) bnext = rd[lane < V ? lane : V - 1];
        for (int s = 0; s * LA_W < nsteps; ++s) {
            float* cur = slab + (s & 1) * LA_SLAB;
            const float* prv = slab + ((s & 1) ^ 1) * LA_SLAB;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");       // the reads of slab s - 2 are over
#pragma unroll
            for (int k = 0; k < LA_S; ++k) cur[k * LA_W + lane] = pf[k];
            const uint4 bcur = bnext;
            const int c1 = (s + 1) * LA_W;
            if (c1 < V) {                             // (uniform) the next slab and boundary block, in flight under this slab's steps
                load_slab(pf, xb, i0, c1, m, V, lane);
                if (has_prev) bnext = rd[c1 + lane < V ? c1 + lane : V - 1];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");       // slab s is written before it is read skewed
            const int tend = nsteps - s * LA_W < LA_W ? nsteps - s * LA_W : LA_W;
            const float* mycur = cur + lane * LA_W;
            const float* myprv = prv + lane * LA_W;
            float gnext = (lane == 0 ? mycur : myprv)[-lane & (LA_W - 1)] - theta;      // step 0
            for (int t = 0; t < tend; ++t) {
                const int tr = t - lane;
                const int j = s * LA_W + tr;          // this lane's column at step d = 64 s + t
                const float g = gnext;                // read one step ahead: the LDS latency is not part of the chain
                gnext = (tr + 1 >= 0 ? mycur : myprv)[(tr + 1) & (LA_W - 1)] - theta;
                const bool live = rowlive && j >= 0 && j < V;
                // lane 0's neighbours above: the boundary row's column d (zeros over the first strip)
                const int b_h = __builtin_amdgcn_readlane((int)bcur.x, t), b_o = __builtin_amdgcn_readlane((int)bcur.y, t),
                          b_c = __builtin_amdgcn_readlane((int)bcur.z, t);
                const float uH = shr1(__int_as_float(b_h), H);
                const unsigned uO = (unsigned)shr1(b_o, (int)O);
                const int uC = shr1(b_c, Cn);
                const float upv = uH - skew, leftv = H - skew;
                const bool pd = dH >= upv && dH >= leftv;                // diag first, then up, then left
                const bool pu = !pd && upv >= leftv;
                const float Pm = pd ? dH : (pu ? upv : leftv);
                const float hv = g + Pm;
                const float Hn = hv > 0.f ? hv : 0.f;
                const bool fresh = pd && !(dH > 0.f);                    // a path starts only through a zero diagonal neighbour
                const unsigned On = fresh ? ((unsigned)row << LA_COL_BITS) | (unsigned)j : (pd ? dO : (pu ? uO : O));
                const int Cp = pd ? dC : (pu ? uC : Cn);
                const int Cnew = Hn > 0.f ? (fresh ? 1 : Cp + 1) : 0;
                if constexpr (TRACE) {
                    // the step's codes (0 start, 1 diag, 2 up, 3 left; 0 for a dead lane or H = 0) as two ballots, bit r = lane r:
                    // SGPR pairs, moved to VGPRs and written by ONE lane's 16-byte vector store (d = 64 s + t < V + 63)
                    const bool pos = live && Hn > 0.f;
                    const unsigned long long c0 = __builtin_amdgcn_ballot_w64(pos && (pd ? !fresh : !pu));
                    const unsigned long long c1 = __builtin_amdgcn_ballot_w64(pos && !pd);
                    if (lane == 0)
                        tstrip[s * LA_W + t] = make_uint4((unsigned)c0, (unsigned)(c0 >> 32), (unsigned)c1, (unsigned)(c1 >> 32));
                }
                dH = uH; dO = uO; dC = uC;
                H = live ? Hn : H;
                O = live ? On : O;
                Cn = live ? Cnew : Cn;
                if (live && Hn > best) {
                    best = Hn;
                    bend = ((unsigned)row << LA_COL_BITS) | (unsigned)j;
                    borg = On;
                    bcells = Cnew;
                }
                if (writer && live) wr[j] = make_uint4(__float_as_uint(Hn), On, (unsigned)Cnew, 0u);
            }
        }
        // the boundary stores of this strip complete, and no L1 line of the row survives, before the next strip loads them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }

    const float mx = wave_max(best);
    unsigned key = (best == mx) ? bend : 0xffffffffu;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)key, o, WAVE);
        key = other < key ? other : key;
    }
    if (mx > 0.f) {
        if (best == mx && bend == key) {              // one lane: rows of different lanes differ
            score[p] = mx;
            span[5 * p] = (int)(borg >> LA_COL_BITS);
            span[5 * p + 1] = (int)(bend >> LA_COL_BITS);
            span[5 * p + 2] = (int)(borg & LA_COL_MASK);
            span[5 * p + 3] = (int)(bend & LA_COL_MASK);
            span[5 * p + 4] = bcells;
        }
    } else if (lane == 0) {
        score[p] = 0.f;
        span[5 * p] = span[5 * p + 1] = span[5 * p + 2] = span[5 * p + 3] = -1;
        span[5 * p + 4] = 0;
    }

    if constexpr (TRACE) {
        // The time map.  The slabs are free now: the wave's 8192 LDS words hold the block's m <= 4096 rows of (lo, hi).  They are
        // filled with -1, the walk writes hi when it enters a row and lo when it leaves it (one lane), and the rows go out
        // coalesced: a valid entry writes all its m rows.  The last strip's release / acquire above completed the trace stores
        // and dropped the L1 lines; the explicit wait keeps that true if the fence's own wait is elided.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int* mp = reinterpret_cast<int*>(slab);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");       // the skewed reads of the last slabs are over
        for (int k = lane; k < 2 * m; k += WAVE) mp[k] = -1;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        if (mx > 0.f) {
            // (i, j), the window and the codes are wave-uniform: the walk is scalar, the window a VGPR quadruple per lane
            const unsigned long long win_lane = __builtin_amdgcn_ballot_w64(best == mx && bend == key);
            const int wl = (int)__builtin_ctzll(win_lane);
            const int ncell = __builtin_amdgcn_readlane(bcells, wl);
            int i = __builtin_amdgcn_readfirstlane((int)(key >> LA_COL_BITS));
            int j = __builtin_amdgcn_readfirstlane((int)(key & LA_COL_MASK));
            if (lane == 0) mp[2 * i + 1] = j;
            const int pitch = V + LA_S - 1;
            int wstrip = -1, wlo = 0;                // the window: entries wlo .. wlo + 63 of strip wstrip, lane l holds wlo + l
            uint4 win = make_uint4(0, 0, 0, 0);
            for (int n = 1; ; ++n) {
                const int strip = i >> 6, r = i & (LA_S - 1), d = j + r;
                if (strip != wstrip || d < wlo) {    // inside a strip d only descends: the window ends at d
                    wstrip = strip;
                    wlo = d - (WAVE - 1) > 0 ? d - (WAVE - 1) : 0;
                    // clamped into the strip's V + 63 entries.  Lanes above d - wlo may hold entries past this strip's last step
                    // that the forward pass never wrote (d < 63, a short last strip): no entry above d is ever selected below
                    const int e = wlo + lane < pitch ? wlo + lane : pitch - 1;
                    win = tp[(long)strip * pitch + e];
                }
                const int e = d - wlo;
                const unsigned w0 = (unsigned)__builtin_amdgcn_readlane((int)(r < 32 ? win.x : win.y), e);
                const unsigned w1 = (unsigned)__builtin_amdgcn_readlane((int)(r < 32 ? win.z : win.w), e);
                const int code = (int)((w0 >> (r & 31)) & 1u) | (int)(((w1 >> (r & 31)) & 1u) << 1);
                if (code == 3) {                     // left: the same row
                    if (--j < 0 || n >= ncell) break;                    // (never taken: column 0 has no left, the path has ncell cells)
                    continue;
                }
                if (lane == 0) mp[2 * i] = j;        // the row is left: its first video second
                if (code == 0 || n >= ncell) break;
                --i;
                if (code == 1) --j;
                if (i < 0 || j < 0) break;           // (never taken: row 0 has no up, and a diag out of the matrix is a start)
                if (lane == 0) mp[2 * i + 1] = j;    // the row is entered: its last video second
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        int* qm = la_first(pa...).qmap + 2 * moff;
        for (int k = lane; k < 2 * m; k += WAVE) qm[k] = mp[k];
    }
}

}  // namespace
}  // namespace tal

using namespace tal;

extern "C" long tan_local_align_ws_bytes(long P, long sum_V) {
    if (P < 1 || P >= (1L << 31) || sum_V < P || sum_V >= (1L << 31)) return TAN_ERR_BAD_ARG;
    return la_ws_bytes(sum_V);
}

extern "C" int tan_local_align(const float* x, long n_x, const long* x_off, const int* table, long P, long sum_V, float theta, float skew,
                               float* score, int* span, void* ws, void* stream) {
    TAN_REQUIRE(x && x_off && table && score && span && ws);
    TAN_REQUIRE(n_x >= 1 && P >= 1 && P < (1L << 31) && sum_V >= P && sum_V < (1L << 31));
    TAN_REQUIRE(theta - theta == 0.f && skew >= 0.f && skew - skew == 0.f);      // theta finite; skew in [0, +inf)
    uint4* brow = reinterpret_cast<uint4*>((reinterpret_cast<uintptr_t>(ws) + 15) & ~(uintptr_t)15);
    hipLaunchKernelGGL(local_align_kernel<>, dim3(cdiv(P, LA_WAVES)), dim3(LA_WAVES * WAVE), 0, (hipStream_t)stream, x, n_x, x_off, table,
                       (int)P, sum_V, theta, skew, score, span, brow);
    TAN_LAUNCH_CHECK();
    return 0;
}

extern "C" long tan_local_align_path_ws_bytes(long P, long sum_V, long n_trace) {
    if (P < 1 || P >= (1L << 31) || sum_V < P || sum_V >= (1L << 31) || n_trace < 1 || n_trace >= LA_MAX_TRACE) return TAN_ERR_BAD_ARG;
    return la_ws_bytes(sum_V) + 16 * n_trace;
}

extern "C" int tan_local_align_path(const float* x, long n_x, const long* x_off, const int* table, long P, long sum_V, float theta,
                                    float skew, const long* path_off, long n_map, long n_trace, float* score, int* span, int* qmap,
                                    void* ws, void* stream) {
    TAN_REQUIRE(x && x_off && table && path_off && score && span && qmap && ws);
    TAN_REQUIRE(n_x >= 1 && P >= 1 && P < (1L << 31) && sum_V >= P && sum_V < (1L << 31));
    TAN_REQUIRE(n_map >= 1 && n_map < (1L << 31) && n_trace >= 1 && n_trace < LA_MAX_TRACE);
    TAN_REQUIRE(theta - theta == 0.f && skew >= 0.f && skew - skew == 0.f);
    uint4* brow = reinterpret_cast<uint4*>((reinterpret_cast<uintptr_t>(ws) + 15) & ~(uintptr_t)15);
    const la_path_args pa = {path_off, n_map, n_trace, qmap, brow + 2 * sum_V};
    hipLaunchKernelGGL(local_align_kernel<la_path_args>, dim3(cdiv(P, LA_WAVES)), dim3(LA_WAVES * WAVE), 0, (hipStream_t)stream, x, n_x,
                       x_off, table, (int)P, sum_V, theta, skew, score, span, brow, pa);
    TAN_LAUNCH_CHECK();
    return 0;
}
