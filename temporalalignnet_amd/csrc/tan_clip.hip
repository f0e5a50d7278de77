// Per-parameter gradient clipping over the flat f32 gradient buffer (gfx950): utils/train_utils.py:3-13, called at train/main.py:115-116.
// Every parameter is a SEGMENT of the buffer, cut into chunks of at most TAN_CLIP_CHUNK elements; two launches, one workgroup per chunk:
//   clip_sumsq_kernel   partials[chunk] = sum of squares of the chunk (per-thread f32 accumulators, wave reduction, four waves through LDS)
//   clip_apply_kernel   norm = sqrt(sum of the segment's partials, in table order, in double) * grad_scale; coef = clip / (norm + 1e-6);
//                       the chunk is multiplied by coef when coef < 1 and not touched otherwise (a NaN norm fails the comparison)
// No atomics: the result does not depend on scheduling.  Pure HBM streaming: two reads of the gradient and at most one write.
#include "tan_common.h"

namespace tal {

constexpr int CLIP_CHUNK = 8192;      // elements per chunk (tan_clip_chunk()): 256 threads x 8 x 16 bytes
constexpr int CLIP_THREADS = 256;

// the chunk's elements [off, off + len) split as head (scalars up to the first 16-byte boundary) | nvec float4 | tail
struct ClipSpan { const float4* body; int head, nvec, tail; };

__device__ __forceinline__ ClipSpan clip_span(const float* p, int len) {
    ClipSpan s;
    s.head = min(len, (int)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    s.nvec = (len - s.head) >> 2;
    s.tail = len - s.head - 4 * s.nvec;
    s.body = reinterpret_cast<const float4*>(p + s.head);
    return s;
}

// chunk_table [n][4] int32 = (off, len, seg, 0); false: an entry that does not lie inside the buffer (nothing is read or written)
__device__ __forceinline__ bool clip_chunk(const int* __restrict__ chunk_table, int c, long n, int& off, int& len, int& seg) {
    const int4 e = *reinterpret_cast<const int4*>(chunk_table + 4 * (long)c);
    off = e.x; len = e.y; seg = e.z;
    return off >= 0 && len > 0 && len <= CLIP_CHUNK && (long)off + len <= n;
}

__global__ __launch_bounds__(CLIP_THREADS) void clip_sumsq_kernel(const float* __restrict__ g, const int* __restrict__ chunk_table, int c0,
                                                                  long n, float* __restrict__ partials) {
    __shared__ float part[CLIP_THREADS / WAVE];
    const int c = c0 + blockIdx.x, tid = threadIdx.x;
    int off, len, seg;
    if (!clip_chunk(chunk_table, c, n, off, len, seg)) return;                  // (block-uniform)
    const float* p = g + off;
    const ClipSpan s = clip_span(p, len);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int i = tid; i < s.nvec; i += CLIP_THREADS) {
        const float4 v = s.body[i];
        a.x = fmaf(v.x, v.x, a.x); a.y = fmaf(v.y, v.y, a.y); a.z = fmaf(v.z, v.z, a.z); a.w = fmaf(v.w, v.w, a.w);
    }
    if (tid < s.head) { const float v = p[tid]; a.x = fmaf(v, v, a.x); }
    if (tid < s.tail) { const float v = p[s.head + 4 * s.nvec + tid]; a.y = fmaf(v, v, a.y); }
    const float w = wave_sum((a.x + a.y) + (a.z + a.w));
    if ((tid & 63) == 0) part[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) partials[c] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(CLIP_THREADS) void clip_apply_kernel(float* __restrict__ g, const int* __restrict__ chunk_table,
                                                                  const int* __restrict__ seg_table, int c0, int c1, int s0, int s1, long n,
                                                                  const float* __restrict__ partials, float clip, float grad_scale,
                                                                  float* __restrict__ norms) {
    const int c = c0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    int off, len, seg;
    if (!clip_chunk(chunk_table, c, n, off, len, seg) || seg < s0 || seg >= s1) return;
    const int first = seg_table[2 * seg], cnt = seg_table[2 * seg + 1];
    if (first < c0 || cnt <= 0 || first > c1 - cnt) return;                   // the segment's partials are this launch's: [first, first + cnt)
    // every wave sums the partials itself, in one fixed order: lane l takes first + l, first + l + 64, ...; then a butterfly over the lanes
    double t = 0.0;
    for (int i = lane; i < cnt; i += WAVE) t += (double)partials[first + i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, WAVE);
    const float norm = (float)sqrt(t) * grad_scale;
    if (c == first && tid == 0) norms[seg] = norm;
    const float coef = clip / (norm + 1e-6f);
    if (!(coef < 1.0f)) return;                                                // not above the threshold, or a NaN norm: nothing is stored
    float* p = g + off;
    const ClipSpan s = clip_span(p, len);
    float4* body = const_cast<float4*>(s.body);
#pragma unroll 4
    for (int i = tid; i < s.nvec; i += CLIP_THREADS) {
        float4 v = body[i];
        v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
        body[i] = v;
    }
    if (tid < s.head) p[tid] *= coef;
    if (tid < s.tail) p[s.head + 4 * s.nvec + tid] *= coef;
}

}  // namespace tal

using namespace tal;

extern "C" int tan_clip_chunk(void) { return CLIP_CHUNK; }

extern "C" int tan_clip_sumsq(const float* g, const int* chunk_table, const int* seg_table, int c0, int c1, int s0, int s1, long n,
                              float* partials, void* stream) {
    TAN_REQUIRE(g && chunk_table && seg_table && partials && 0 <= c0 && c0 <= c1 && 0 <= s0 && s0 <= s1 && n > 0 && n < (1L << 31));
    if (c1 == c0) return 0;
    hipLaunchKernelGGL(clip_sumsq_kernel, dim3((unsigned)(c1 - c0)), dim3(CLIP_THREADS), 0, (hipStream_t)stream, g, chunk_table, c0, n, partials);
    TAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int tan_clip_apply(float* g, const int* chunk_table, const int* seg_table, int c0, int c1, int s0, int s1, long n,
                              const float* partials, float clip, float grad_scale, float* norms, void* stream) {
    TAN_REQUIRE(g && chunk_table && seg_table && partials && norms && 0 <= c0 && c0 <= c1 && 0 <= s0 && s0 <= s1 && n > 0 && n < (1L << 31));
    TAN_REQUIRE(clip > 0.0f);
    if (c1 == c0) return 0;
    hipLaunchKernelGGL(clip_apply_kernel, dim3((unsigned)(c1 - c0)), dim3(CLIP_THREADS), 0, (hipStream_t)stream, g, chunk_table, seg_table, c0, c1,
                       s0, s1, n, partials, clip, grad_scale, norms);
    TAN_LAUNCH_CHECK();
    return 0;
}
