// Step discovery (spherical k-means over the index's seconds): the update half of a Lloyd iteration.  tan_cluster_accumulate adds
// every row into the sums of its cluster, tan_cluster_centroids turns the sums into unit centroids (the definitions, bit for bit,
// are in include/tan_hip.h).  The assignment half is tan_label_topk with k = 1.
//
// The sums are 64-bit FIXED POINT: q = rint(v * 2^30) as an integer, added with wrapping integer arithmetic.  Integer addition is
// associative, so the sums do not depend on the slabs, the shards, the order of the rows or the number of atomics -- where an f32
// atomic sum depends on arrival order.  Nothing else here needs care to be reproducible.
//
// tan_cluster_accumulate: one WAVE per slab of CL_SLAB = 256 positions of `order`, one wave per workgroup (the waves share nothing).
//   * the wave stages its 256 (row, cluster[, scale]) triples in LDS: 4 coalesced loads of `order`, 4 gathers of `assign`;
//   * it then walks the slab's rows one after the other, a row being ONE coalesced wave-instruction (bf16: 16 bytes per lane, 1 KiB;
//     e4m3: 8 bytes per lane; f32: two instructions of 1 KiB), in batches of CL_PF rows (f32: half as many) whose loads are
//     issued together, the next batch's before the current one is consumed (batches of 16 e4m3 rows measured no faster).  A lane
//     owns 8 columns;
//   * while the cluster stays the same (it is uniform over the wave: a scalar branch) a lane adds into 8 registers; when it changes,
//     and at the slab's end, it flushes them with 8 no-return 64-bit integer atomics (global_atomic_add_x2).  With `order` sorted by
//     cluster a launch issues at most (N / 256 + K) * 512 atomics: 16 bytes per row and 4 KiB per cluster against the 1 KiB (bf16)
//     read per row -- the design does not depend on the rate of 8-byte integer atomics.
//   * the running sums of a slab are kept in F64 registers: rint(v * 2^30) is an integer of magnitude <= 2^31 (|v| <= 2) and at most
//     256 of them are added before a flush, so every partial sum is an integer below 2^40 and f64 holds it exactly.  Per element
//     that is v_mul_f32, v_rndne_f32, v_cvt_f64_f32, v_add_f64 -- an f32 -> i64 conversion and a 64-bit integer add are three
//     times as many instructions, and at 516 bytes per row (e4m3) the kernel would be VALU-bound.  The flush converts f64 -> i64
//     once per 8 columns (exact) and the atomics add integers, so the RESULT is the integer sum of the definition.
//   * e4m3: v = decode(code) * v_scale[n].  The kernel multiplies by v_scale[n] * 2^30 instead (one multiply per row): both are
//     exact products by a power of two unless v is subnormal, and then |v * 2^30| < 2^-96 rounds to 0 either way.  The scale is
//     clamped to 2^64 first so that a zero code times a huge scale stays 0 (a non-zero one breaks |v| <= 2 anyway).
// A row or a cluster out of range is skipped (its load goes to row 0 and is discarded): nothing is read or written out of bounds
// whatever assign and order hold.
//
// tan_cluster_centroids: one wave per cluster, four per workgroup; lane l holds columns l, l + 64, ..., l + 448.  Every operation is
// one correctly rounded f32 operation in the header's order (contraction off), so numpy float32 restates it.
#include "tan_common.h"

#pragma clang fp contract(off)

namespace tal {
namespace {

constexpr int CL_SLAB = 256;                          // positions of `order` per wave
constexpr int CL_C = 512;
constexpr int CL_PF = 8;                              // rows per batch of loads
constexpr int CN_WAVES = 4;                           // clusters per workgroup of the centroid kernel
constexpr int FMT_E4M3 = 2;                           // next to TAN_F32 / TAN_BF16

struct cl_e4m3 { unsigned char b; };

// a lane's 8 elements of one row, as loaded (the conversion happens when the row is consumed, not when it is requested)
template <typename T> struct Raw;
template <> struct Raw<float> {                       // columns 4 l .. 4 l + 3 and 256 + 4 l .. 256 + 4 l + 3: two 1 KiB instructions
    float4 a, b;
    static __device__ __forceinline__ int col(int lane, int e) { return (e < 4 ? 0 : 256) + 4 * lane + (e & 3); }
    __device__ __forceinline__ void load(const float* row, int lane) {
        a = *reinterpret_cast<const float4*>(row + 4 * lane);
        b = *reinterpret_cast<const float4*>(row + 256 + 4 * lane);
    }
    __device__ __forceinline__ void get(float (&v)[8]) const {
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
};
template <> struct Raw<bf16_t> {                      // columns 8 l .. 8 l + 7
    uint4 u;
    static __device__ __forceinline__ int col(int lane, int e) { return 8 * lane + e; }
    __device__ __forceinline__ void load(const bf16_t* row, int lane) { u = *reinterpret_cast<const uint4*>(row + 8 * lane); }
    __device__ __forceinline__ void get(float (&v)[8]) const {
        v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
        v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
        v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u);
        v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
    }
};
template <> struct Raw<cl_e4m3> {                     // columns 8 l .. 8 l + 7, OCP e4m3fn codes
    uint2 u;
    static __device__ __forceinline__ int col(int lane, int e) { return 8 * lane + e; }
    __device__ __forceinline__ void load(const cl_e4m3* row, int lane) { u = *reinterpret_cast<const uint2*>(row + 8 * lane); }
    __device__ __forceinline__ void get(float (&v)[8]) const {
        const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)u.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)u.x, true);
        const auto c = __builtin_amdgcn_cvt_pk_f32_fp8((int)u.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)u.y, true);
        v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1]; v[4] = c[0]; v[5] = c[1]; v[6] = d[0]; v[7] = d[1];
    }
};

// an exact integer held in f64 -> i64; a sum poisoned by a non-finite element gives an unspecified, but defined, value
__device__ __forceinline__ long long f64_to_i64(double x) {
    x = x == x ? x : 0.0;
    x = fmin(fmax(x, -0x1p62), 0x1p62);
    return (long long)x;
}

template <typename T>
__global__ void __launch_bounds__(WAVE)
cluster_accumulate_kernel(const T* __restrict__ Vn, const float* __restrict__ v_scale, long N, const int* __restrict__ assign,
                          const int* __restrict__ order, int K, long long* __restrict__ sums) {
    constexpr bool E4M3 = sizeof(T) == 1;
    __shared__ int s_row[CL_SLAB];
    __shared__ int s_cl[CL_SLAB];
    __shared__ float s_mul[CL_SLAB];                  // what a row's elements are multiplied by: [v_scale *] 2^30
    const int lane = threadIdx.x;
    const long p0 = (long)blockIdx.x * CL_SLAB;
    const int n = (int)(N - p0 < CL_SLAB ? N - p0 : CL_SLAB);       // >= 1: the grid is cdiv(N, CL_SLAB)
    // every load below goes to a clamped index, so none sits behind a branch and the four of a kind are in flight together
    int row[CL_SLAB / WAVE], cl[CL_SLAB / WAVE];
    float mul[CL_SLAB / WAVE];
#pragma unroll
    for (int j = 0; j < CL_SLAB / WAVE; ++j) {
        const int i = j * WAVE + lane;
        const int r = order[p0 + (i < n ? i : n - 1)];
        row[j] = i < n && r >= 0 && r < N ? r : -1;
    }
#pragma unroll
    for (int j = 0; j < CL_SLAB / WAVE; ++j) {
        const int r = row[j] < 0 ? 0 : row[j];
        cl[j] = assign[r];
        mul[j] = 0x1p30f;
        if constexpr (E4M3) mul[j] = fminf(v_scale[r], 0x1p64f) * 0x1p30f;
    }
#pragma unroll
    for (int j = 0; j < CL_SLAB / WAVE; ++j) {
        const int i = j * WAVE + lane;
        const bool ok = row[j] >= 0 && cl[j] >= 0 && cl[j] < K;
        s_row[i] = ok ? row[j] : 0;
        s_cl[i] = ok ? cl[j] : -1;
        s_mul[i] = mul[j];
    }
    __syncthreads();                                  // one wave: the LDS writes above are visible to its reads below

    constexpr int PF = sizeof(T) == 4 ? CL_PF / 2 : CL_PF;          // f32 rows take twice the registers
    double acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0;
    int run = -1;                                     // the cluster the registers hold the sums of; -1: none

    auto flush = [&]() {
        if (run >= 0) {
            unsigned long long* dst = reinterpret_cast<unsigned long long*>(sums + (long)run * CL_C);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                __hip_atomic_fetch_add(dst + Raw<T>::col(lane, e), (unsigned long long)f64_to_i64(acc[e]), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                acc[e] = 0.0;
            }
        }
    };
    // the rows of positions i0 .. i0 + PF - 1 (clamped to the slab: never out of bounds), all PF loads issued together
    auto request = [&](Raw<T> (&batch)[PF], int i0) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int i = i0 + u < n ? i0 + u : n - 1;
            batch[u].load(Vn + (long)s_row[i] * CL_C, lane);
        }
    };
    auto consume = [&](const Raw<T> (&batch)[PF], int i0) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int i = i0 + u;
            if (i < n) {                              // uniform
                const int c = __builtin_amdgcn_readfirstlane(s_cl[i]);
                if (c != run) {
                    flush();
                    run = c;
                }
                if (c >= 0) {
                    const float mul = s_mul[i];
                    float v[8];
                    batch[u].get(v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += (double)__builtin_rintf(v[e] * mul);
                }
            }
        }
    };

    // two batches of registers take turns: the next batch's PF loads are issued before the current one is consumed, so a wave has
    // PF to 2 PF rows in flight
    Raw<T> even[PF], odd[PF];
    request(even, 0);
    for (int i0 = 0; i0 < n; i0 += 2 * PF) {
        request(odd, i0 + PF);
        consume(even, i0);
        request(even, i0 + 2 * PF);
        consume(odd, i0 + PF);
    }
    flush();
}

__global__ void __launch_bounds__(CN_WAVES * WAVE)
cluster_centroids_kernel(const long long* __restrict__ sums, const int* __restrict__ counts, const float* prev, int K, float* cent,
                         float* __restrict__ cohesion) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long c = (long)blockIdx.x * CN_WAVES + threadIdx.x / WAVE;
    if (c >= K) return;                               // the whole wave; the waves share nothing
    float x[CL_C / WAVE];
    float n2 = 0.f;
#pragma unroll
    for (int i = 0; i < CL_C / WAVE; ++i) {
        x[i] = (float)sums[c * CL_C + lane + WAVE * i] * 0x1p-30f;     // i64 -> f32 round to nearest even; the scaling is exact
        const float sq = x[i] * x[i];
        n2 = n2 + sq;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n2 = n2 + __shfl_xor(n2, m);
    const float norm = __builtin_sqrtf(n2);
    const int cnt = counts[c];
    const bool keep = cnt <= 0 || !(norm > 0.f) || (__float_as_uint(norm) & 0x7f800000u) == 0x7f800000u;
#pragma unroll
    for (int i = 0; i < CL_C / WAVE; ++i) {
        const long at = c * CL_C + lane + WAVE * i;
        cent[at] = keep ? prev[at] : x[i] / norm;     // prev may be cent: a lane reads an element before it writes it
    }
    if (lane == 0) cohesion[c] = keep ? 0.f : norm / (float)cnt;
}

template <typename T>
int launch_accumulate(const void* Vn, const float* v_scale, long N, const int* assign, const int* order, int K, long* sums, void* stream) {
    hipLaunchKernelGGL(cluster_accumulate_kernel<T>, dim3(cdiv(N, CL_SLAB)), dim3(WAVE), 0, (hipStream_t)stream, static_cast<const T*>(Vn),
                       v_scale, N, assign, order, K, reinterpret_cast<long long*>(sums));
    TAN_LAUNCH_CHECK();
    return 0;
}

int accumulate(const void* Vn, const float* v_scale, int fmt, long N, int C, const int* assign, const int* order, long K, long* sums,
               void* stream) {
    TAN_REQUIRE(Vn && assign && order && sums && (fmt != FMT_E4M3 || v_scale));
    TAN_REQUIRE(C == CL_C && N >= 1 && N < (1L << 31) && K >= 1 && K < (1L << 31));
    TAN_REQUIRE(reinterpret_cast<uintptr_t>(Vn) % 16 == 0 && reinterpret_cast<uintptr_t>(sums) % 8 == 0);
    if (fmt == TAN_F32) return launch_accumulate<float>(Vn, nullptr, N, assign, order, (int)K, sums, stream);
    if (fmt == TAN_BF16) return launch_accumulate<bf16_t>(Vn, nullptr, N, assign, order, (int)K, sums, stream);
    if (fmt == FMT_E4M3) return launch_accumulate<cl_e4m3>(Vn, v_scale, N, assign, order, (int)K, sums, stream);
    return TAN_ERR_BAD_ARG;
}

}  // namespace
}  // namespace tal

using namespace tal;

extern "C" int tan_cluster_slab_rows(void) { return CL_SLAB; }

extern "C" int tan_cluster_accumulate(const void* Vn, int dtype, long N, int C, const int* assign, const int* order, long K, long* sums,
                                      void* stream) {
    TAN_REQUIRE(dtype == TAN_F32 || dtype == TAN_BF16);
    return accumulate(Vn, nullptr, dtype, N, C, assign, order, K, sums, stream);
}

extern "C" int tan_cluster_accumulate_e4m3(const void* Vn, const float* v_scale, long N, int C, const int* assign, const int* order, long K,
                                           long* sums, void* stream) {
    return accumulate(Vn, v_scale, FMT_E4M3, N, C, assign, order, K, sums, stream);
}

extern "C" int tan_cluster_centroids(const long* sums, const int* counts, const float* prev, long K, int C, float* cent, float* cohesion,
                                     void* stream) {
    TAN_REQUIRE(sums && counts && prev && cent && cohesion);
    TAN_REQUIRE(C == CL_C && K >= 1 && K < (1L << 31));
    hipLaunchKernelGGL(cluster_centroids_kernel, dim3(cdiv(K, CN_WAVES)), dim3(CN_WAVES * WAVE), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(sums), counts, prev, (int)K, cent, cohesion);
    TAN_LAUNCH_CHECK();
    return 0;
}
