// Two-stage search, second stage: what `search.search_rerank` reads off a pass of joint-stack outputs.
//
// tan_rerank_tail turns the joint stack's stage outputs of W windows ([W, L, 512]: T frame rows, then the text rows; the query is
// the text row at position T) into one (score, second, confidence, alignability) per window -- the launches `eval_windows` spends
// on the same quantity are 2 S_d L2 normalisations, S_d batched GEMMs, S_d row copies and the head, and they produce [S, W, T, K].
// One workgroup per window, four waves:
//   * wave 0 loads the query row once (64 lanes x 8 channels, 16-byte loads) and leaves it in LDS as f32; wave 1 the head's row (or
//     takes the query row from LDS when both stages are the same buffer);
//   * every wave takes every fourth frame: 8 products and 8 squares per lane in element order, wave_sum, one division;
//     a frame row is read exactly once, by one wave, so a cosine's bits depend on nothing but its two rows;
//   * wave 0 reduces the window's cosines in LDS: maximum, first arg-max, the softmax maximum, and one 16-byte store.
// tan_rerank_select orders each query's P <= 32 candidates with the sorting network of the rank sweeps (sort64).
// No atomics, no scratch, nothing depends on W or on how windows fall into workgroups.
#include "tan_sort.h"

namespace tal {
namespace {

constexpr int RC = 512;                     // feature width (the model's)
constexpr int T_MAX = 1024;                 // frames per window: the position table's length
constexpr int NF = TAN_WIN_FIELDS;
constexpr float TEMP = 0.07f;               // eval_zeroshot_align.py:197-201

template <typename T> __device__ __forceinline__ f8 ld_row8(const T* p) {
    if constexpr (sizeof(T) == 2) return ld8(p); else return ld8f(p);
}

__device__ __forceinline__ f8 lds_row8(const float* p) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    f8 r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w; r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}

// sum of a lane's 8 products in element order, then the wave's 64 partial sums (wave_sum's fixed tree)
__device__ __forceinline__ float dot8(const f8& a, const f8& b) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += a.v[i] * b.v[i];
    return wave_sum(s);
}

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int stride = 32; stride > 0; stride >>= 1) v = min(v, __shfl_xor(v, stride, 64));
    return v;
}

template <typename T>
__global__ void __launch_bounds__(256) rerank_tail_kernel(const T* last, const T* head, int L, int T_len,
                                                          const int* __restrict__ table, const float* __restrict__ head_w,
                                                          const float* __restrict__ head_b, float* __restrict__ out,
                                                          float* __restrict__ sim) {
    __shared__ __attribute__((aligned(16))) float qs[RC];
    __shared__ float cs[T_MAX];
    __shared__ float hv;
    const int w = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int* e = table + (long)w * NF;
    int t = e[1];
    t = t < 0 ? 0 : (t > T_len ? T_len : t);
    const int s0 = e[4];
    const T* rows = last + (long)w * L * RC;
    if (wave == 0) {
        const f8 q = ld_row8<T>(rows + (long)T_len * RC + lane * 8);
        st4(qs + lane * 8, make_float4(q.v[0], q.v[1], q.v[2], q.v[3]));
        st4(qs + lane * 8 + 4, make_float4(q.v[4], q.v[5], q.v[6], q.v[7]));
    }
    __syncthreads();
    const f8 q = lds_row8(qs + lane * 8);
    if (wave == 1) {                                               // the alignability logit (tan_model.py:148)
        float a = 0.0f;
        if (head) {
            const f8 x = head == last ? q : ld_row8<T>(head + ((long)w * L + T_len) * RC + lane * 8);
            a = dot8(x, ld8f(head_w + lane * 8)) + head_b[0];
        }
        if (lane == 0) hv = a;
    }
    const float nq = sqrtf(dot8(q, q));
    for (int f = wave; f < t; f += 4) {                            // wave-uniform
        const f8 x = ld_row8<T>(rows + (long)f * RC + lane * 8);
        const float d = dot8(x, q), nv = sqrtf(dot8(x, x));
        if (lane == 0) cs[f] = d / (nv * nq);
    }
    __syncthreads();
    if (sim)
        for (int f = threadIdx.x; f < T_len; f += 256) sim[(long)w * T_len + f] = f < t ? cs[f] : -INFINITY;
    if (wave != 0) return;
    float m = -INFINITY;
    int at = 0x7fffffff;
    for (int f = lane; f < t; f += 64) {
        const float c = cs[f];
        if (c > m) { m = c; at = f; }
    }
    const float mx = wave_max(m);
    int first = wave_min_int(m == mx ? at : 0x7fffffff);
    first = first == 0x7fffffff ? 0 : first;                       // no frame, or nothing but NaN
    const float xm = mx / TEMP;
    float z = 0.0f;
    for (int f = lane; f < t; f += 64) z += expf(cs[f] / TEMP - xm);
    z = wave_sum(z);
    if (lane == 0) st4(out + (long)w * 4, make_float4(mx, __int_as_float(s0 + first), t > 0 ? 1.0f / z : 0.0f, hv));
}

// one wave per query: lane i holds candidate i
__global__ void __launch_bounds__(256) rerank_select_kernel(const float* __restrict__ score, long Q, int P, long stride, int k,
                                                            int* __restrict__ out_idx) {
    const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= Q) return;
    float s = -INFINITY;
    int n = 0x7fffffff;
    if (lane < P) {
        s = score[(q * P + lane) * stride];
        s = s == s ? s : -INFINITY;                                // a NaN ranks last among the candidates
        n = lane;
    }
    sort64(s, n, lane);
    if (lane < k) out_idx[q * k + lane] = n;
}

}  // namespace
}  // namespace tal

using namespace tal;

extern "C" int tan_rerank_tail(const void* stage_last, const void* stage_head, int dtype, int L, int T, const int* table, int W,
                               const float* head_w, const float* head_b, float* out, float* sim, void* stream) {
    TAN_REQUIRE(stage_last && table && out && (dtype == TAN_F32 || dtype == TAN_BF16));
    TAN_REQUIRE(W >= 1 && T >= 1 && T <= T_MAX && L > T);
    TAN_REQUIRE(!stage_head || (head_w && head_b));
    TAN_REQUIRE((uintptr_t)stage_last % 16 == 0 && (uintptr_t)stage_head % 16 == 0 && (uintptr_t)head_w % 16 == 0 &&
                (uintptr_t)out % 16 == 0);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TAN_BF16)
        hipLaunchKernelGGL(rerank_tail_kernel<bf16_t>, dim3(W), dim3(256), 0, st, (const bf16_t*)stage_last, (const bf16_t*)stage_head, L,
                           T, table, head_w, head_b, out, sim);
    else
        hipLaunchKernelGGL(rerank_tail_kernel<float>, dim3(W), dim3(256), 0, st, (const float*)stage_last, (const float*)stage_head, L, T,
                           table, head_w, head_b, out, sim);
    TAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int tan_rerank_select(const float* score, long Q, int P, long stride, int k, int* out_idx, void* stream) {
    TAN_REQUIRE(score && out_idx && Q >= 1 && Q < (1L << 31) && P >= 1 && P <= 32 && k >= 1 && k <= P && stride >= 1);
    hipLaunchKernelGGL(rerank_select_kernel, dim3(cdiv(Q, 4)), dim3(256), 0, (hipStream_t)stream, score, Q, P, stride, k, out_idx);
    TAN_LAUNCH_CHECK();
    return 0;
}
