// The coarse image of a corpus index: MXFP4 rows (272 bytes per second of video; format: include/tan_hip.h) and the sweep over them.
//
// tan_quantize_rows_mxfp4: one wave per row, 8 channels per lane as tan_quantize_rows_e4m3; a block of 32 elements is four lanes, so
// its amax is two quad_perm DPP steps.  The block scale comes from amax's exponent and fraction bits, the e2m1 code from seven
// compares against the rounding boundaries (strict where the tie goes down to the even code), one 4-byte code store per lane and one
// scale byte per four lanes.
// tan_rank_topk_mxfp4: tan_rank_topk's sweep (tan_retrieve.hip) with another tile routine.  Grid (query tiles of 128, index splits);
// a wave keeps its 32 queries resident as the fp8 B operand of v_mfma_scale_f32_32x32x64_f8f6f4 (8 K steps x 8 VGPRs, as the e4m3
// sweep's 64), and 64-row index tiles stream through LDS as the fp4 A operand -- so a lane's 16 accumulators all belong to ONE query
// (column = lane & 31), which is what the threshold logic below needs.  A tile is ONE stage and ONE barrier: an LDS row is the
// format's own 272 bytes, 256 code bytes and then the 16 scale bytes, and 272 = 17 x 16 makes the 16-byte reads of 32 rows
// conflict-free.  Per wave and tile: 2 x 8 MFMAs of K = 64, two blocks each.
//   operand maps (pinned by tests/test_coarse_gpu.py with exact integer data): lane l, r = l & 31, h = l >> 5, holds for K step j
//     A: the 16 bytes (32 nibbles, low nibble first) of block 2 j + h of tile row r    -- registers 0..3 of the 8
//     B: registers 0..3 the 16 e4m3 bytes k = 64 j + 16 h .. + 15 of query column r, registers 4..7 the bytes k = 64 j + 32 + 16 h ..
//        + 15 -- an 8-bit operand is two runs of 16, NOT the 32 consecutive elements a 4-bit operand's lane holds (measured: byte p
//        of B lane half h' meets nibble 16 h' + (p & 15) of A lane half p >> 4)
//     scale A: byte 0 of the lane's scale register scales the lane's OWN 32 K elements, so lane l passes block 2 j + h's byte
//   The 16 scale bytes of a row are one 16-byte LDS read; K step j's byte is byte 2 (j & 1) + h of word j >> 1, moved to byte 0 by
//   one shift per MFMA.  op_sel stays 0: the instruction is used the one way that does not depend on how it selects another byte.
//   The query's scale operand is 2^0 in every byte.
// The score is acc * q_scale[q], one f32 multiply after the loop.  From there on this is tan_rank_topk: scores at or above the
// query's threshold go to a 64-slot LDS buffer per query, a buffer that would overflow is sorted by the wave (sort64: score
// descending, row ascending), cut to its k best, and the threshold rises to the k-th; tan_rank_topk's own merge launch folds the
// splits' lists, and the tile sizes and the splits rule are its too (tan_topk.h).  The CUTOFF (below_score / below_row) is one more condition on a row's admission, applied before the
// threshold sees the row: the lists are those of the sweep over the admitted rows alone.
#include "tan_mma.h"
#include "tan_sort.h"
#include "tan_topk.h"

namespace tal {
namespace {

constexpr int RC = 512;                     // feature width (the model's)
constexpr int CODE_B = RC / 2;              // code bytes per row
constexpr int SCALE_B = RC / 32;            // scale bytes per row
constexpr int ROW_B = CODE_B + SCALE_B;     // an LDS row: codes, then scales
constexpr int TILE_B = BN * ROW_B;
constexpr int NSTEP = RC / 64;              // K steps of v_mfma_scale_f32_32x32x64_f8f6f4
constexpr int SWEEP_LDS = 2 * TILE_B + 4 * 32 * CAP * 8;
constexpr int FMT_FP8 = 0, FMT_FP4 = 4;     // the instruction's cbsz / blgp operand formats: e4m3, e2m1
constexpr int UNIT_SCALE = 0x7f7f7f7f;      // e8m0 2^0 in every byte

typedef int i32x8 __attribute__((ext_vector_type(8)));

template <typename T> __device__ __forceinline__ f8 load8(const T* p);
template <> __device__ __forceinline__ f8 load8<bf16_t>(const bf16_t* p) { return ld8(p); }
template <> __device__ __forceinline__ f8 load8<float>(const float* p) { return ld8f(p); }

// RNE onto e2m1's magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 (codes 0..7) for 0 <= a <= 6: the code is the number of rounding boundaries
// at or below a, a boundary itself counting only where the tie goes UP to the even code (0.75, 1.75, 3.5)
__device__ __forceinline__ unsigned e2m1_code(float a) {
    return (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
}

// amax = m 2^e with m in [0.5, 1): e = (bits >> 23) - 126 and m <= 0.75 <=> the fraction field <= 0x400000.  A subnormal amax (and
// e = -125) would give s < -127 and takes the clamp; 2^-s is a normal number for every s in [-127, 126].
template <typename T>
__global__ void __launch_bounds__(256) quantize_mxfp4_kernel(const T* __restrict__ x, long n_rows, unsigned* __restrict__ codes,
                                                             unsigned char* __restrict__ scales) {
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n_rows) return;
    const f8 v = load8<T>(x + g * RC + lane * 8);
    float am = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) am = fmaxf(am, fabsf(v.v[i]));
    am = fmaxf(am, dpp_move<0xB1>(am));                            // quad_perm [1,0,3,2]
    am = fmaxf(am, dpp_move<0x4E>(am));                            // quad_perm [2,3,0,1]: the block's four lanes
    const unsigned bits = __float_as_uint(am);
    int s = (int)(bits >> 23) - 129 + ((bits & 0x7fffffu) > 0x400000u ? 1 : 0);
    s = s < -127 ? -127 : s;
    s = am == 0.0f ? 0 : s;
    const float inv = __uint_as_float((unsigned)(127 - s) << 23);
    unsigned w = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned c = e2m1_code(fabsf(v.v[i] * inv)) | ((__float_as_uint(v.v[i]) >> 31) << 3);
        w |= c << (4 * i);                                         // element 2 j: the low nibble of byte j
    }
    codes[g * (CODE_B / 4) + lane] = w;
    if ((lane & 3) == 0) scales[g * SCALE_B + (lane >> 2)] = (unsigned char)(s + 127);
}

// sw: the row's 16 scale bytes; half: lane >> 5.  The upper bytes of the scale operand are not read (op_sel 0).
template <int J>
__device__ __forceinline__ void mma_step(f32x16& acc, const uint4& a, const i32x8& b, const unsigned (&sw)[4], int half) {
    i32x8 av;
    av[0] = (int)a.x; av[1] = (int)a.y; av[2] = (int)a.z; av[3] = (int)a.w;
    av[4] = 0; av[5] = 0; av[6] = 0; av[7] = 0;                    // an fp4 operand is the first four registers
    const int sc = (int)(sw[J >> 1] >> (16 * (J & 1) + 8 * half));
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, b, acc, FMT_FP4, FMT_FP8, 0, sc, 0, UNIT_SCALE);
}

template <int J>
__device__ __forceinline__ void mma_steps(f32x16& acc, const unsigned char* row, const i32x8 (&qf)[NSTEP], const unsigned (&sw)[4],
                                          int half) {
    if constexpr (J < NSTEP) {
        mma_step<J>(acc, *reinterpret_cast<const uint4*>(row + 32 * J + 16 * half), qf[J], sw, half);
        mma_steps<J + 1>(acc, row, qf, sw, half);
    }
}

__global__ void __launch_bounds__(256) coarse_kernel(const unsigned char* __restrict__ Tq, const float* __restrict__ q_scale,
                                                     const unsigned char* __restrict__ codes, const unsigned char* __restrict__ scales,
                                                     long Q, long N, int k, long tiles_per_split, long n_tiles,
                                                     const float* __restrict__ below_s, const int* __restrict__ below_n,
                                                     float* __restrict__ part_s, int* __restrict__ part_n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* bs = reinterpret_cast<float*>(smem + 2 * TILE_B);
    int* bn = reinterpret_cast<int*>(bs + 4 * 32 * CAP);

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5;
    const long qblk = (long)blockIdx.x * BQ;
    const long qme = qblk + wave * 32 + col;
    const bool qok = qme < Q;
    const long qrd = qok ? qme : Q - 1;

    i32x8 qf[NSTEP];                                               // the wave's 32 queries, resident
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) {
        const uint4* p = reinterpret_cast<const uint4*>(Tq + qrd * RC + 64 * j + 16 * half);
        const uint4 lo = p[0], hi = p[2];                          // k = 16 h .. 16 h + 15 and 32 + 16 h .. 32 + 16 h + 15 of the step
        qf[j][0] = (int)lo.x; qf[j][1] = (int)lo.y; qf[j][2] = (int)lo.z; qf[j][3] = (int)lo.w;
        qf[j][4] = (int)hi.x; qf[j][5] = (int)hi.y; qf[j][6] = (int)hi.z; qf[j][7] = (int)hi.w;
    }
    const float qs = q_scale[qrd];
    const bool cut = below_s != nullptr;
    const float cs = cut ? below_s[qrd] : 0.0f;
    const int cn = cut ? below_n[qrd] : 0;

    const long t0 = (long)blockIdx.y * tiles_per_split;
    const long t1 = t0 + tiles_per_split < n_tiles ? t0 + tiles_per_split : n_tiles;

    int fill = 0;
    float thr = -INFINITY;
    const int bbase = (wave * 32 + col) * CAP;

    uint4 pre[4], psc = make_uint4(0, 0, 0, 0);
    auto issue = [&](long t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = tid + 256 * i, row = v >> 4, c16 = v & 15;
            const long n = t * BN + row;
            pre[i] = n < N ? *reinterpret_cast<const uint4*>(codes + n * CODE_B + c16 * 16) : make_uint4(0, 0, 0, 0);
        }
        if (tid < BN) {
            const long n = t * BN + tid;
            psc = n < N ? *reinterpret_cast<const uint4*>(scales + n * SCALE_B) : make_uint4(0, 0, 0, 0);
        }
    };

    // sorts every buffer of the wave that `need` more entries would overflow, keeps its k best and raises the query's threshold
    auto compact = [&](int need) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        for (int qi = 0; qi < 32; ++qi) {
            const int f = __builtin_amdgcn_readlane(fill, qi), nd = __builtin_amdgcn_readlane(need, qi);
            if (f + nd <= CAP) continue;
            const int b = (wave * 32 + qi) * CAP;
            float s = lane < f ? bs[b + lane] : -INFINITY;
            int n = lane < f ? bn[b + lane] : SENT_ROW;
            sort64(s, n, lane);
            const int nf = f < k ? f : k;
            if (lane < nf) { bs[b + lane] = s; bn[b + lane] = n; }
            const float th = __shfl(s, k - 1, 64);
            if (col == qi) { fill = nf; thr = th; }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    };

    if (t0 < t1) issue(t0);
    for (long t = t0; t < t1; ++t) {
        // buffer (t - t0) & 1: its last readers, two tiles back, have all passed the previous tile's barrier
        unsigned char* cur = smem + ((t - t0) & 1) * TILE_B;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = tid + 256 * i, row = v >> 4, c16 = v & 15;
            *reinterpret_cast<uint4*>(cur + row * ROW_B + c16 * 16) = pre[i];
        }
        if (tid < BN) *reinterpret_cast<uint4*>(cur + tid * ROW_B + CODE_B) = psc;
        __syncthreads();
        if (t + 1 < t1) issue(t + 1);
        f32x16 acc[2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            acc_zero(acc[rt]);
            const unsigned char* row = cur + (rt * 32 + col) * ROW_B;
            const uint4 s4 = *reinterpret_cast<const uint4*>(row + CODE_B);
            const unsigned sw[4] = {s4.x, s4.y, s4.z, s4.w};
            mma_steps<0>(acc[rt], row, qf, sw, half);
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            const long nbase = t * BN + rt * 32;
            unsigned mask = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long n = nbase + acc_row(r, lane);
                const float v = acc[rt][r] * qs;
                acc[rt][r] = v;
                bool valid = n < N;
                if (cut) valid = valid && better(cs, cn, v, (int)n);   // strictly after the cutoff entry
                if (valid && v >= thr) mask |= 1u << r;
            }
            const int c_me = __popc(mask), c_pt = __shfl_xor(c_me, 32, 64), need = c_me + c_pt;
            if (__any(fill + need > CAP)) compact(need);
            int off = bbase + fill + (half ? c_pt : 0);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if ((mask >> r) & 1) {
                    bs[off] = acc[rt][r];
                    bn[off] = (int)(nbase + acc_row(r, lane));
                    ++off;
                }
            fill += need;
        }
    }

    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    for (int qi = 0; qi < 32; ++qi) {
        const int f = __builtin_amdgcn_readlane(fill, qi);
        const int b = (wave * 32 + qi) * CAP;
        float s = lane < f ? bs[b + lane] : -INFINITY;
        int n = lane < f ? bn[b + lane] : SENT_ROW;
        sort64(s, n, lane);
        const long q = qblk + wave * 32 + qi;
        if (q < Q && lane < k) {
            const long o = ((long)blockIdx.y * Q + q) * k + lane;
            part_s[o] = s;
            part_n[o] = n;
        }
    }
}

}  // namespace
}  // namespace tal

using namespace tal;

extern "C" int tan_quantize_rows_mxfp4(const void* x, int dtype, long n_rows, int C, void* codes, void* scales, void* stream) {
    TAN_REQUIRE(x && codes && scales && (dtype == TAN_F32 || dtype == TAN_BF16));
    TAN_REQUIRE(C == RC && n_rows >= 1 && n_rows < (1L << 31) && (uintptr_t)x % 16 == 0 && (uintptr_t)codes % 4 == 0);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TAN_BF16)
        hipLaunchKernelGGL(quantize_mxfp4_kernel<bf16_t>, dim3(cdiv(n_rows, 4)), dim3(256), 0, st, (const bf16_t*)x, n_rows,
                           (unsigned*)codes, (unsigned char*)scales);
    else
        hipLaunchKernelGGL(quantize_mxfp4_kernel<float>, dim3(cdiv(n_rows, 4)), dim3(256), 0, st, (const float*)x, n_rows, (unsigned*)codes,
                           (unsigned char*)scales);
    TAN_LAUNCH_CHECK();
    return 0;
}

extern "C" long tan_rank_topk_mxfp4_ws_bytes(long Q, long N, int k) {
    if (Q < 1 || Q >= (1L << 31) || N < 1 || N >= (1L << 31) || k < 1 || k > KMAX) return TAN_ERR_BAD_ARG;
    return max_splits(N) * Q * k * 8;
}

extern "C" int tan_rank_topk_mxfp4(const void* Tq, const float* q_scale, const void* codes, const void* scales, long Q, long N, int C,
                                   int k, int splits, const float* below_score, const int* below_row, float* top_score, int* top_row,
                                   void* ws, void* stream) {
    TAN_REQUIRE(Tq && q_scale && codes && scales && top_score && top_row && ws);
    TAN_REQUIRE((uintptr_t)Tq % 16 == 0 && (uintptr_t)codes % 16 == 0 && (uintptr_t)scales % 16 == 0 && (uintptr_t)ws % 16 == 0);
    TAN_REQUIRE(C == RC && Q >= 1 && Q < (1L << 31) && N >= 1 && N < (1L << 31) && k >= 1 && k <= KMAX && k <= N && splits >= 0);
    TAN_REQUIRE((below_score == nullptr) == (below_row == nullptr));
    hipStream_t st = (hipStream_t)stream;
    const long n_tiles = n_index_tiles(N), q_tiles = (Q + BQ - 1) / BQ;
    long tps;
    const int ns = n_splits(Q, N, splits, &tps);
    float* part_s = (float*)ws;
    int* part_n = (int*)(part_s + (long)ns * Q * k);
    static std::atomic<unsigned long long> lds_done{0};
    const hipError_t attr = ensure_dyn_lds((const void*)coarse_kernel, SWEEP_LDS, lds_done);
    if (attr != hipSuccess) return (int)attr;
    hipLaunchKernelGGL(coarse_kernel, dim3((unsigned)q_tiles, (unsigned)ns), dim3(256), SWEEP_LDS, st, (const unsigned char*)Tq, q_scale,
                       (const unsigned char*)codes, (const unsigned char*)scales, Q, N, k, tps, n_tiles, below_score, below_row, part_s,
                       part_n);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(rank_merge_kernel, dim3(cdiv(Q, 4)), dim3(256), 0, st, (const float*)part_s, (const int*)part_n, Q, k, ns,
                       top_score, top_row);
    TAN_LAUNCH_CHECK();
    return 0;
}
