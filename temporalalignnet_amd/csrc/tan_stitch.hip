// Corpus auto-alignment (HTM-AA inference): window batch packing and window stitching on the device.
//
// The reference's evaluation (eval/eval_zeroshot_align.py:129-223) walks the 64-s windows of ONE video, calls the model per window
// and stitches the last-stage similarities into per-sentence [K, vlen] rows with ~10 small torch ops per window.  Here a pass of up
// to a few hundred windows from MANY videos is packed by one launch (tan_window_pack), evaluated by one `eval_windows` call, and
// folded into the chunk's accumulators by one launch (tan_window_stitch_acc); one more launch per chunk (tan_window_stitch_final)
// turns the accumulators into the stitched rows, timestamps, confidences and scores.
//
// Window table (int32, TAN_WIN_FIELDS per window, in plan order: videos in chunk order, windows by start time within a video):
//   [0] vrow  packed video row of the window's first frame      [1] t     frames (e0 - s0, <= T)
//   [2] krow  packed sentence row of its first sentence         [3] k     sentences (<= Kp)
//   [4] s0    first frame, in the video's own time               [5] vlen  the video's length (accumulator row stride)
//   [6] aoff  the video's first accumulator element             [7] kbase packed sentence row of the video's sentence 0
//
// Exactness: every accumulator element is owned by one thread, which adds the pass's windows in window order onto the value the
// previous pass left -- the host loop's `acc[mt, s0:e0] += sim / 0.07` order, so a video whose windows span passes gives the same
// bits as one pass.  No atomics, no FMA contraction (the host rounds the scaled value before the add).
#include <type_traits>

#include "tan_common.h"

#pragma clang fp contract(off)

namespace tal {
namespace {

constexpr int NF = 8;                       // TAN_WIN_FIELDS
constexpr float INV_TEMP = 1.0f / 0.07f;    // ATen's true-divide by a Python scalar multiplies by the f32 reciprocal
constexpr float EPS_CNT = 1e-5f;            // torch.maximum(cnt, 1e-5) (eval_zeroshot_align.py:199-205)
constexpr float MASKED = -6e4f;             // sim == 0 -> -6e4 (eval_zeroshot_align.py:221)

// separately rounded multiply and add: the HIP headers' __fmul_rn / __fadd_rn are plain operators compiled outside this file's
// `fp contract(off)`, and hipcc fuses them into v_pk_fma_f32; these are compiled under it
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

// ---- tan_window_pack: one block per (row, window); rows [0, T) are frames, [T, T + Kp) sentences
template <int UNIT>
__global__ void __launch_bounds__(256) window_pack_kernel(const char* __restrict__ video, int vrow_bytes, const char* __restrict__ text,
                                                          int trow_bytes, const int* __restrict__ table, int T, int Kp,
                                                          char* __restrict__ out_video, unsigned char* __restrict__ vmask,
                                                          char* __restrict__ out_text, unsigned char* __restrict__ tmask) {
    typedef typename std::conditional<UNIT == 16, uint4, unsigned short>::type U;
    const int w = blockIdx.y, r = blockIdx.x;
    const int* e = table + (long)w * NF;
    const bool is_frame = r < T;
    const int n = is_frame ? min(e[1], T) : min(e[3], Kp);
    const int j = is_frame ? r : r - T;
    const bool real = j < n;
    const int row_bytes = is_frame ? vrow_bytes : trow_bytes;
    const long dst_row = is_frame ? (long)w * T + j : (long)w * Kp + j;
    U* dst = reinterpret_cast<U*>((is_frame ? out_video : out_text) + dst_row * row_bytes);
    const U* src = real ? reinterpret_cast<const U*>((is_frame ? video : text) + (long)(is_frame ? e[0] + j : e[2] + j) * row_bytes)
                        : nullptr;
    const int nu = row_bytes / UNIT;
    for (int i = threadIdx.x; i < nu; i += blockDim.x) dst[i] = real ? src[i] : U{};
    if (threadIdx.x == 0) (is_frame ? vmask : tmask)[is_frame ? (long)w * T + j : (long)w * Kp + j] = real ? 0 : 1;
}

__device__ __forceinline__ bool covers_row(const int* e, int r_local) {      // r_local: sentence index inside the video
    const int left = e[2] - e[7];
    return r_local >= left && r_local < left + e[3];
}

// ---- tan_window_stitch_acc: one block per window, one wave per sentence row, lanes over frames
__global__ void __launch_bounds__(256) window_stitch_acc_kernel(const float* __restrict__ sim_j, const float* __restrict__ sim_d,
                                                                const float* __restrict__ a_joint, const int* __restrict__ table,
                                                                int W, int T, int Kp, float* __restrict__ acc_j,
                                                                float* __restrict__ acc_d, float* __restrict__ cnt, long n_acc,
                                                                float* __restrict__ tcnt, float* __restrict__ a_sum, long n_rows) {
    const int w = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int* e = table + (long)w * NF;
    const int t_w = min(e[1], T), k_w = min(e[3], Kp), s0 = e[4], vlen = e[5], kbase = e[7];
    const long aoff = e[6];
    for (int kk = wave; kk < k_w; kk += 4) {
        const int r = e[2] - kbase + kk;                      // sentence index inside the video
        // the sentence's count and alignability sum: owned by the first window of this pass that holds the sentence
        if (lane == 0) {
            bool owner = true;
            for (int w2 = w - 1; w2 >= 0 && table[(long)w2 * NF + 7] == kbase; --w2)
                if (covers_row(table + (long)w2 * NF, r)) { owner = false; break; }
            const long g = (long)e[2] + kk;
            if (owner && g < n_rows) {
                float c = tcnt[g], a = a_joint ? a_sum[g] : 0.0f;
                for (int w2 = w; w2 < W && table[(long)w2 * NF + 7] == kbase; ++w2) {
                    const int* e2 = table + (long)w2 * NF;
                    if (!covers_row(e2, r)) continue;
                    c = add_rn(c, 1.0f);
                    if (a_joint) a = add_rn(a, a_joint[(long)w2 * Kp + (r - (e2[2] - kbase))]);
                }
                tcnt[g] = c;
                if (a_joint) a_sum[g] = a;
            }
        }
        for (int tt = lane; tt < t_w; tt += 64) {
            const int time = s0 + tt;
            // owner of (r, time): no earlier window of this pass (same video) covers it; windows are ordered by s0, so the ones
            // that can cover `time` are the few whose e0 = s0 + t lies beyond it
            bool owner = true;
            for (int w2 = w - 1; w2 >= 0; --w2) {
                const int* e2 = table + (long)w2 * NF;
                if (e2[7] != kbase || e2[4] + e2[1] <= time) break;
                if (covers_row(e2, r)) { owner = false; break; }
            }
            if (!owner) continue;
            const long idx = aoff + (long)r * vlen + time;
            if (idx < 0 || idx >= n_acc) continue;
            float aj = acc_j[idx], ad = acc_d[idx], c = cnt[idx];
            for (int w2 = w; w2 < W; ++w2) {
                const int* e2 = table + (long)w2 * NF;
                if (e2[7] != kbase || e2[4] > time) break;
                if (!covers_row(e2, r) || time >= e2[4] + min(e2[1], T)) continue;
                const long src = ((long)w2 * T + (time - e2[4])) * Kp + (r - (e2[2] - kbase));
                aj = add_rn(aj, mul_rn(sim_j[src], INV_TEMP));
                ad = add_rn(ad, mul_rn(sim_d[src], INV_TEMP));
                c = add_rn(c, 1.0f);
            }
            acc_j[idx] = aj;
            acc_d[idx] = ad;
            cnt[idx] = c;
        }
    }
}

// ---- tan_window_stitch_final: one wave per sentence row, any vlen
__global__ void __launch_bounds__(256) window_stitch_final_kernel(float* __restrict__ acc_j, const float* __restrict__ acc_d,
                                                                  const float* __restrict__ cnt, const float* __restrict__ tcnt,
                                                                  const float* __restrict__ a_sum, const int* __restrict__ rows,
                                                                  long n_rows, long n_acc, float* __restrict__ res) {
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n_rows) return;
    const long off = rows[2 * g];
    const int vlen = rows[2 * g + 1];
    if (off < 0 || off + vlen > n_acc) return;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int t = lane; t < vlen; t += 64) {
        const float m = fmaxf(cnt[off + t], EPS_CNT);
        float s = mul_rn(add_rn(__fdiv_rn(acc_j[off + t], m), __fdiv_rn(acc_d[off + t], m)), 0.5f);
        if (s == 0.0f) s = MASKED;
        acc_j[off + t] = s;
        if (s > best) { best = s; bidx = t; }                // t increases: a lane keeps its first maximum
    }
    for (int o = 32; o >= 1; o >>= 1) {                      // 64-lane arg-max, lowest index among equal maxima
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bidx, o, 64);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    double sum = 0.0;                                        // softmax denominator; its largest term is exp(0) = 1
    for (int t = lane; t < vlen; t += 64) sum += (double)expf(acc_j[off + t] - best);
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) {
        const float c = tcnt[g];
        res[g] = (float)bidx;
        res[n_rows + g] = (float)(1.0 / sum);
        res[2 * n_rows + g] = a_sum ? __fdiv_rn(a_sum[g], fmaxf(c, EPS_CNT)) : best;
        res[3 * n_rows + g] = c > 0.0f ? 1.0f : 0.0f;
    }
}

}  // namespace
}  // namespace tal

using namespace tal;

extern "C" int tan_window_pack(const void* video, int video_elem_bytes, int Dv, const void* text, int text_elem_bytes, int Dt,
                               const int* table, int W, int T, int Kp, void* out_video, unsigned char* out_vmask, void* out_text,
                               unsigned char* out_tmask, void* stream) {
    TAN_REQUIRE(video && text && table && out_video && out_vmask && out_text && out_tmask);
    TAN_REQUIRE(W > 0 && T > 0 && Kp > 0 && Dv > 0 && Dt > 0 && W <= 65535);
    TAN_REQUIRE((video_elem_bytes == 2 || video_elem_bytes == 4) && (text_elem_bytes == 2 || text_elem_bytes == 4));
    const int vb = Dv * video_elem_bytes, tb = Dt * text_elem_bytes;
    const bool wide = vb % 16 == 0 && tb % 16 == 0 && (uintptr_t)video % 16 == 0 && (uintptr_t)text % 16 == 0 &&
                      (uintptr_t)out_video % 16 == 0 && (uintptr_t)out_text % 16 == 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(T + Kp, W);
    if (wide)
        hipLaunchKernelGGL((window_pack_kernel<16>), grid, dim3(64), 0, st, (const char*)video, vb, (const char*)text, tb, table, T, Kp,
                           (char*)out_video, out_vmask, (char*)out_text, out_tmask);
    else
        hipLaunchKernelGGL((window_pack_kernel<2>), grid, dim3(256), 0, st, (const char*)video, vb, (const char*)text, tb, table, T, Kp,
                           (char*)out_video, out_vmask, (char*)out_text, out_tmask);
    TAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int tan_window_stitch_acc(const float* sim_j, const float* sim_d, const float* a_joint, const int* table, int W, int T,
                                     int Kp, float* acc_j, float* acc_d, float* cnt, long n_acc, float* tcnt, float* a_sum,
                                     long n_rows, void* stream) {
    TAN_REQUIRE(sim_j && sim_d && table && acc_j && acc_d && cnt && tcnt && W > 0 && T > 0 && Kp > 0 && n_acc > 0 && n_rows > 0);
    TAN_REQUIRE(!a_joint == !a_sum);
    hipLaunchKernelGGL(window_stitch_acc_kernel, dim3(W), dim3(256), 0, (hipStream_t)stream, sim_j, sim_d, a_joint, table, W, T,
                       Kp, acc_j, acc_d, cnt, n_acc, tcnt, a_sum, n_rows);
    TAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int tan_window_stitch_final(float* acc_j, const float* acc_d, const float* cnt, const float* tcnt, const float* a_sum,
                                       const int* rows, long n_rows, long n_acc, float* res, void* stream) {
    TAN_REQUIRE(acc_j && acc_d && cnt && tcnt && rows && res && n_rows > 0 && n_acc > 0);
    hipLaunchKernelGGL(window_stitch_final_kernel, dim3(cdiv(n_rows, 4)), dim3(256), 0, (hipStream_t)stream, acc_j, acc_d, cnt,
                       tcnt, a_sum, rows, n_rows, n_acc, res);
    TAN_LAUNCH_CHECK();
    return 0;
}
