// Zero-shot retrieval on the device: a matrix-free rank / top-k sweep, clip pooling, and the per-second corpus index.
//
// tan_rank_topk answers, for Q query rows against N index rows of width 512, "how many index rows beat / tie the query's paired row"
// (what eval_zeroshot_retrieval.py:13-27 gets from sorting the whole text x video matrix) and "which k rows score best", without ever
// storing a [Q, N] score.  Three launches:
//   1. pair   : the score of (q, pair[q]) for every query, by the SAME tile routine as the sweep with the paired rows gathered into
//               the index tile -- one MFMA chain per score, in the same order, so the sweep's own entry (q, pair[q]) has the same bits
//               (ties >= 1).  Also zeroes higher / ties.
//   2. sweep  : grid (query tiles of 128, index splits).  A wave keeps the B fragments of its 32 queries in registers for the whole
//               kernel; 64-row index tiles stream through LDS in K chunks (double buffered, one barrier per chunk) as the A operand of
//               32x32 MFMAs.  A lane's 16 accumulators all belong to ONE query (column = lane & 31), so the counts are two compares per
//               score in registers.  Top-k: scores at or above the query's threshold are appended to a 64-slot LDS buffer per query;
//               when a buffer would overflow, the wave sorts it (64-lane bitonic network, order: score descending, then row ascending)
//               keeps the k best and raises the threshold to the k-th.  At the end of the split each query's k best go to scratch.
//   3. merge  : one wave per query folds the splits' lists through the same sorting network.  The order is total (no two entries
//               share a row), so the result is the top k of all N rows whatever the split count; integer counts are summed with
//               integer atomics, whose result does not depend on order.  No float atomics anywhere.
// tan_rank_topk_e4m3 is the same three launches over e4m3 codes with one power-of-two f32 scale per row (the format of
// tan_quantize_rows_e4m3, include/tan_hip.h): a third instantiation of rank_kernel.  The 64 row scales of an index tile ride into
// LDS with the tile's last K chunk, and every accumulator becomes (acc * v_scale[n]) * q_scale[q] -- in the pair launch and in
// the sweep alike -- before anything compares it, so thresholds, candidate buffers, sort64 and the merge see final scores.
// tan_rank_topk_video ranks VIDEOS (contiguous row ranges, v_off) by their best row with the same sweep (rank_kernel's VIDEO mode):
// a candidate slot also holds its video, compaction keeps one entry per video (distinct64), and the merge folds the splits' lists the
// same way.  tan_moment_extent then walks outward from each hit's best row while the score stays within `width` of the peak.
// tan_sequence_topk ranks videos by the best ORDER-PRESERVING path of a sequence of up to 32 query rows (tan_decode.hip's recurrence
// fused into the sweep: seq_kernel, which shares the load / MFMA routine tile_scores with rank_kernel), and tan_sequence_scores
// writes the winners' step x second scores, with the sweep's bits, for tan_monotonic_decode to backtrack.
// tan_clip_topk ranks videos by the best SECOND-FOR-SECOND match of a run of up to 32 query rows -- a diagonal sum over the same
// matrix-free score tile (clip_kernel: seq_kernel's frame with two add chains per lane instead of the scan) -- and returns each
// video's best start; rank_merge_video_kernel folds its splits.
// tan_compound_topk ranks videos by AND / OR / NOT of up to 32 query rows in any order (compound_kernel: the same frame, each term's
// peak over the video in registers, clauses by readlane, the weakest clause by a wave min, the veto by one __any; no LDS beyond the
// tiles), and tan_compound_peaks writes the winners' per-term (peak, row) with the sweep's bits.
// tan_rank_topk_filtered / tan_rank_topk_video_filtered sweep only the rows a FILTER admits (rank_kernel's FILTER mode): the image
// tan_row_filter_build makes from row spans lists the 64-row tiles that hold an admitted row, with a row mask each; a split walks a
// range of that list and masks the other rows, so the lists are the plain sweep's over the gathered admitted rows, bit for bit.
// tan_label_topk / _e4m3 answer the transposed question, the k best LABELS of every index row: label_kernel is the sweep with the
// roles swapped (a tile of index rows resident, the label matrix streamed; tile_scores, the candidate buffers and sort64 carry over),
// one workgroup per 128 rows, no splits, no scratch, no merge.  tan_label_runs compacts the rows' best labels into label segments.
// tan_cover_topk / _e4m3 rank videos by the seconds they share with a SET of up to 4096 query rows in any order: cover_kernel is
// label_kernel's organisation per (video, set) with the score tile reduced along both axes (every row's best second, every second's
// best row; 64-bit fixed-point sums), and cover_select_kernel folds a set's scores into its k best videos.
//
// tan_segment_pool_* and tan_window_feat_* follow tan_stitch.hip's ownership rule: an accumulator row is owned by the first window
// of the launch that touches it, and its owner adds every such window in window order -- no atomics, run-to-run identical bits.
#include <type_traits>

#include "tan_mma.h"
#include "tan_sort.h"
#include "tan_topk.h"

namespace tal {
namespace {

constexpr int RC = 512;                     // feature width (the model's)
constexpr int FILT_HEAD = 4;                // int32 words before a filter image's tile list (include/tan_hip.h)

template <typename T> struct RCfg;
template <> struct RCfg<bf16_t> { static constexpr int KC = 128, LD = 136; };     // 256 B of a row per chunk; 272-B pitch: b128 reads conflict-free
template <> struct RCfg<float> { static constexpr int KC = 64, LD = 65; };        // 256 B of a row per chunk; odd pitch: b32 reads conflict-free
// 256 B of a row per chunk; 264-B pitch = 8 B x 33: the 32 rows a half-wave reads with one ds_read_b64 (all at the same k) start 66 dwords
// apart, i.e. on the dword pairs 2 r mod 64, r = 0..31 -- each of the 64 banks once: b64 reads conflict-free.  The pitch is no multiple
// of 16, so the tile is staged with 8-byte stores.
template <> struct RCfg<e4m3_t> { static constexpr int KC = 256, LD = 264; };

template <typename T> constexpr int scale_bytes() { return sizeof(T) == 1 ? BN * 4 : 0; }   // e4m3: a tile's row scales, after the buffers
template <typename T> constexpr int tile_bytes() { return 2 * BN * RCfg<T>::LD * (int)sizeof(T) + scale_bytes<T>(); }
constexpr int BUF_BYTES = 4 * 32 * CAP * 8;
constexpr int VID_BYTES = 4 * 32 * CAP * 4 + 2 * BN * 4;          // the video sweep: a video per candidate slot, and per row of two tiles
template <typename T, bool VIDEO = false> constexpr int sweep_lds() {
    return (tile_bytes<T>() + 15) / 16 * 16 + BUF_BYTES + (VIDEO ? VID_BYTES : 0);
}

// sort64 with a payload: the entry's video
__device__ __forceinline__ void sort64v(float& s, int& n, int& v, int lane) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const float os = __shfl_xor(s, stride, 64);
            const int on = __shfl_xor(n, stride, 64), ov = __shfl_xor(v, stride, 64);
            const bool lower = (lane & stride) == 0, desc = (lane & size) == 0;
            const bool mine = better(s, n, os, on);
            const bool keep = (lower == desc) ? mine : !mine;
            if (!keep) { s = os; n = on; v = ov; }
        }
    }
}

// sort64v, then every entry whose video already appears at a better rank is dropped: lane j holds the j-th best DISTINCT video's
// best entry, (-inf, SENT_ROW) after the last one.  All 64 lanes must be active.
__device__ __forceinline__ void distinct64(float& s, int& n, int& v, int lane) {
    sort64v(s, n, v, lane);
    bool dup = false;
#pragma unroll
    for (int i = 0; i < 63; ++i) dup |= lane > i && v == __builtin_amdgcn_readlane(v, i);
    if (__any(dup && n != SENT_ROW)) {                             // the empty slots are last already: no duplicate, no second sort
        if (dup) { s = -INFINITY; n = SENT_ROW; }
        sort64v(s, n, v, lane);
    }
}

// the largest v in [lo, hi] with v_off[v] <= n (lo if there is none): whatever v_off holds, the result lies in [lo, hi]
__device__ __forceinline__ int video_search(const int* __restrict__ v_off, long n, int lo, int hi) {
    while (lo < hi) {
        const int mid = (int)(((long)lo + hi + 1) >> 1);
        if (v_off[mid] <= n) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <typename T> struct QFrag;
template <> struct QFrag<bf16_t> {
    static __device__ __forceinline__ bf16x8 load(const bf16_t* row, int j, int lane) {
        return *reinterpret_cast<const bf16x8*>(row + j * 16 + 8 * (lane >> 5));
    }
};
template <> struct QFrag<float> {
    static __device__ __forceinline__ float load(const float* row, int j, int lane) { return row[j * 2 + (lane >> 5)]; }
};

template <> struct QFrag<e4m3_t> {
    static __device__ __forceinline__ long load(const e4m3_t* row, int j, int lane) {
        return *reinterpret_cast<const long*>(row + j * 16 + 8 * (lane >> 5));
    }
};

template <typename T>
__device__ __forceinline__ void stage_store(T* tile, int tid, const uint4 (&pre)[4]) {
    constexpr int LD = RCfg<T>::LD;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = tid + 256 * i, row = v >> 4, c16 = v & 15;
        if constexpr (sizeof(T) == 2) {
            *reinterpret_cast<uint4*>(tile + row * LD + c16 * 8) = pre[i];
        } else if constexpr (sizeof(T) == 1) {
            uint2* d = reinterpret_cast<uint2*>(tile + row * LD + c16 * 16);
            d[0] = make_uint2(pre[i].x, pre[i].y);
            d[1] = make_uint2(pre[i].z, pre[i].w);
        } else {
            float* d = reinterpret_cast<float*>(tile) + row * LD + c16 * 4;
            d[0] = __uint_as_float(pre[i].x); d[1] = __uint_as_float(pre[i].y);
            d[2] = __uint_as_float(pre[i].z); d[3] = __uint_as_float(pre[i].w);
        }
    }
}

// One 64-row index tile against a wave's 32 resident query columns: the load / MFMA loop every sweep of this file shares.  `pre` (and,
// e4m3, `psc`) hold the tile's first K chunk on entry; the chunks stream through the two LDS buffers (one barrier per chunk), and
// after each barrier next(kc) issues the loads that follow chunk kc -- this tile's next chunk or the next tile's first.  On return
// acc[rt][r] is score(column lane & 31, tile row 32 rt + acc_row(r, lane)), for e4m3 already (acc * v_scale[n]) * q_scale[q].  An
// element's MFMA chain and K order do not depend on the tile or on where its row sits in it.  All 256 threads must call it.
template <typename T, typename Next>
__device__ __forceinline__ void tile_scores(T* tile, float* sc, int tid, int lane, const uint4 (&pre)[4], const float& psc,
                                            const typename Mma<T>::frag_t (&qf)[RC / Mma<T>::KS], float qs, f32x16 (&acc)[2],
                                            Next&& next) {
    typedef Mma<T> M;
    typedef typename M::frag_t frag_t;
    constexpr int KC = RCfg<T>::KC, LD = RCfg<T>::LD, KS = M::KS, NCH = RC / KC, SPC = KC / KS;
    constexpr int TS = BN * LD;                                    // elements per tile buffer
    constexpr bool F8 = sizeof(T) == 1;
    acc_zero(acc[0]);
    acc_zero(acc[1]);
#pragma unroll
    for (int kc = 0; kc < NCH; ++kc) {
        T* cur = tile + (kc & 1) * TS;                             // NCH is even: the buffer alternates across tiles too
        stage_store<T>(cur, tid, pre);
        if constexpr (F8) {
            // written before the last chunk's barrier, read after it; the next write comes after the next tile's first barrier,
            // which no wave passes before every wave has left this tile's epilogue: one buffer is enough
            if (kc == NCH - 1 && tid < BN) sc[tid] = psc;
        }
        __syncthreads();
        next(kc);
#pragma unroll
        for (int ks = 0; ks < SPC; ++ks) {
            const frag_t a0 = M::template load<true>(cur, LD, 0, ks * KS, lane);
            const frag_t a1 = M::template load<true>(cur, LD, 32, ks * KS, lane);
            M::mma(acc[0], a0, qf[kc * SPC + ks]);
            M::mma(acc[1], a1, qf[kc * SPC + ks]);
        }
    }
    if constexpr (F8) {
        // a lane's 16 rows of a 32-row half are four runs of four: 8 g + 4 (lane >> 5) + 0..3.  Two f32 multiplies in this order
        // (powers of two: exact), the same in the pair launch and the sweep.
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 s4 = *reinterpret_cast<const float4*>(sc + rt * 32 + 8 * g + 4 * (lane >> 5));
                acc[rt][4 * g + 0] = (acc[rt][4 * g + 0] * s4.x) * qs;
                acc[rt][4 * g + 1] = (acc[rt][4 * g + 1] * s4.y) * qs;
                acc[rt][4 * g + 2] = (acc[rt][4 * g + 2] * s4.z) * qs;
                acc[rt][4 * g + 3] = (acc[rt][4 * g + 3] * s4.w) * qs;
            }
    }
}

// PAIR = true : launch 1 (grid = query tiles); tile t of 2 holds the paired rows of the block's queries 64 t .. 64 t + 63
// PAIR = false: launch 2 (grid = query tiles x splits)
// q_scale / v_scale: the rows' scales, e4m3 only (the other instantiations do not read them)
// VIDEO = true: the sweep of tan_rank_topk_video -- the same tiles and MFMA chains, but a query's list holds at most one entry per
// video, and a candidate slot holds its video next to score and row.  tvid [tiles] holds the videos of every tile's first and last
// row (tile_video_kernel; the next tile's pair is fetched while this tile's MFMAs run).  A tile that lies inside one video (most
// do) gives a query ONE candidate, its (max, first arg-max) over the tile's rows.  A tile with a video boundary takes the per-row
// path: its 64 rows' videos are searched in v_off between the tile's two videos before the MFMA loop and wait in LDS (two
// buffers: a wave may start tile t + 1 while another still reads tile t's).  Compaction keeps the k best distinct videos
// (distinct64) and the threshold is the k-th distinct video's score, -inf while fewer are held: a row below it cannot enter the
// final list, and a dropped entry is dominated by a kept row of its own video.  Nothing in the compaction touches global memory.
// FILTER = true: the sweeps of tan_rank_topk_filtered / _video_filtered.  `pair` carries the filter IMAGE (include/tan_hip.h; these
// sweeps have no paired rows, and the existing instantiations keep their arguments): a split walks a contiguous range of the image's
// tile list -- the loop counter is a LIST position, the tile it names and its row mask are fetched one position ahead -- and a row
// whose mask bit is clear is neither a candidate nor threshold material, in the one-video fast path too.  tvid is indexed by list
// position.  The count of listed tiles is read here, so the grid does not depend on it; a workgroup whose range is empty writes
// empty lists and leaves before it loads its queries.  Every other instantiation is compiled as before (`if constexpr`).
template <typename T, bool PAIR, bool VIDEO = false, bool FILTER = false>
__global__ void __launch_bounds__(256) rank_kernel(const T* __restrict__ Tq, const T* __restrict__ Vn, long Q, long N,
                                                   const int* __restrict__ pair, int k, long tiles_per_split, long n_tiles,
                                                   float* __restrict__ dscore, int* __restrict__ higher, int* __restrict__ ties,
                                                   float* __restrict__ part_s, int* __restrict__ part_n,
                                                   const float* __restrict__ q_scale, const float* __restrict__ v_scale,
                                                   const int2* __restrict__ tvid, const int* __restrict__ v_off,
                                                   int* __restrict__ part_v) {
    typedef Mma<T> M;
    typedef typename M::frag_t frag_t;
    constexpr int KC = RCfg<T>::KC, LD = RCfg<T>::LD, KS = M::KS, NCH = RC / KC, NFR = RC / KS;
    constexpr int TS = BN * LD;                                    // elements per tile buffer
    constexpr long ROWB = (long)RC * sizeof(T);
    constexpr bool F8 = sizeof(T) == 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* tile = reinterpret_cast<T*>(smem);
    float* sc = reinterpret_cast<float*>(smem + 2 * TS * sizeof(T));   // F8: the current tile's 64 row scales
    float* bs = reinterpret_cast<float*>(smem + (tile_bytes<T>() + 15) / 16 * 16);
    int* bn = reinterpret_cast<int*>(bs + 4 * 32 * CAP);
    int* bv = bn + 4 * 32 * CAP;                                   // VIDEO only: the candidates' videos, then the rows' videos of two tiles
    int* vt = bv + 4 * 32 * CAP;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31;
    const long qblk = (long)blockIdx.x * BQ;
    const long qme = qblk + wave * 32 + col;
    const bool qok = qme < Q;

    // FILTER: the split's range [f0, f1) of the image's tile list; whatever the image holds, every position and tile is in range
    long f0 = 0, f1 = 0;
    const int* ftile = nullptr;
    const unsigned long long* fmask = nullptr;
    if constexpr (FILTER) {
        ftile = pair + FILT_HEAD;
        fmask = reinterpret_cast<const unsigned long long*>(pair + FILT_HEAD + (n_tiles + 1) / 2 * 2);
        long nl = pair[0];
        nl = nl < 0 ? 0 : (nl > n_tiles ? n_tiles : nl);
        const long per = (nl + gridDim.y - 1) / gridDim.y;
        f0 = (long)blockIdx.y * per;
        f1 = f0 + per < nl ? f0 + per : nl;
        if (f0 >= f1) {                                            // block-uniform: nothing listed for this split
            for (int e = tid; e < BQ * k; e += 256) {
                const long q = qblk + e / k;
                if (q < Q) {
                    const long o = ((long)blockIdx.y * Q + q) * k + e % k;
                    part_s[o] = -INFINITY;
                    part_n[o] = SENT_ROW;
                    if constexpr (VIDEO) part_v[o] = -1;
                }
            }
            return;
        }
    }

    frag_t qf[NFR];                                                // the wave's 32 queries, resident
    {
        const T* qrow = Tq + (qok ? qme : Q - 1) * RC;
#pragma unroll
        for (int j = 0; j < NFR; ++j) qf[j] = QFrag<T>::load(qrow, j, lane);
    }

    float qs = 1.0f, psc = 0.0f;
    if constexpr (F8) qs = q_scale[qok ? qme : Q - 1];

    long t0, t1;
    if (PAIR) { t0 = 0; t1 = 2; }
    else if (FILTER) { t0 = f0; t1 = f1; }
    else { t0 = (long)blockIdx.y * tiles_per_split; t1 = t0 + tiles_per_split < n_tiles ? t0 + tiles_per_split : n_tiles; }
    auto listed = [&](long it) {                                   // FILTER: the tile at list position `it`
        const long t = ftile[it];
        return t < 0 ? 0 : (t >= n_tiles ? n_tiles - 1 : t);
    };

    const bool counting = !PAIR && !VIDEO && !FILTER && pair != nullptr;
    const float dq = (counting && qok) ? dscore[qme] : 0.0f;
    int hi = 0, eq = 0, fill = 0;
    float thr = -INFINITY, dval = 0.0f;
    const int bbase = (wave * 32 + col) * CAP;

    uint4 pre[4];
    auto issue = [&](long t, int kc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = tid + 256 * i, row = v >> 4, c16 = v & 15;
            long n;
            if (PAIR) {
                const long q = qblk + t * BN + row;
                n = q < Q ? (long)pair[q] : 0;
                n = n < 0 ? 0 : (n >= N ? N - 1 : n);              // memory safety only: a pair outside [0, N) is the caller's error
            } else {
                n = t * BN + row;
            }
            pre[i] = n < N ? *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(Vn) + n * ROWB + kc * 256 + c16 * 16)
                           : make_uint4(0, 0, 0, 0);
        }
        if constexpr (F8) {
            if (kc == NCH - 1 && tid < BN) {                       // the row scales ride with the tile's last chunk
                long n;
                if (PAIR) {
                    const long q = qblk + t * BN + tid;
                    n = q < Q ? (long)pair[q] : 0;
                    n = n < 0 ? 0 : (n >= N ? N - 1 : n);
                } else {
                    n = t * BN + tid;
                }
                psc = n < N ? v_scale[n] : 0.0f;
            }
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
            int nf;
            if constexpr (VIDEO) {
                int v = lane < f ? bv[b + lane] : -1;
                distinct64(s, n, v, lane);
                const int held = __popcll(__ballot(n != SENT_ROW));
                nf = held < k ? held : k;
                if (lane < nf) bv[b + lane] = v;
            } else {
                sort64(s, n, lane);
                nf = f < k ? f : k;
            }
            if (lane < nf) { bs[b + lane] = s; bn[b + lane] = n; }
            const float th = __shfl(s, k - 1, 64);
            if (col == qi) { fill = nf; thr = th; }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    };

    int2 tv_next = make_int2(0, 0);
    if constexpr (VIDEO) {
        if (t0 < t1) tv_next = tvid[t0];
    }
    long ft_next = 0;                                              // FILTER: the next position's tile and row mask
    unsigned long long fm_next = 0;
    if constexpr (FILTER) {
        ft_next = listed(t0);                                      // t0 < t1 here
        fm_next = fmask[t0];
        issue(ft_next, 0);
    } else {
        if (t0 < t1) issue(t0, 0);
    }
    for (long it = t0; it < t1; ++it) {                            // `it`: the tile, or with FILTER its position in the image's list
        const long t = FILTER ? ft_next : it;
        const unsigned long long rows_in = fm_next;                // FILTER: bit r = row 64 t + r is admitted
        if constexpr (FILTER) {
            if (it + 1 < t1) { ft_next = listed(it + 1); fm_next = fmask[it + 1]; }
        }
        const int2 tv = tv_next;
        if constexpr (VIDEO) {
            if (it + 1 < t1) tv_next = tvid[it + 1];
            if (tv.x != tv.y && tid < BN) {                        // a video boundary in the tile: every row's video, for the epilogue
                const long n = t * BN + tid;
                vt[(it & 1) * BN + tid] = video_search(v_off, n < N ? n : N - 1, tv.x, tv.y);
            }
        }
        f32x16 acc[2];
        tile_scores<T>(tile, sc, tid, lane, pre, psc, qf, qs, acc, [&](int kc) {
            if (kc + 1 < NCH) issue(t, kc + 1);
            else if (it + 1 < t1) issue(FILTER ? ft_next : t + 1, 0);
        });
        if (PAIR) {
            if (t == (wave >> 1)) {
                const f32x16 a = (wave & 1) ? acc[1] : acc[0];
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (acc_row(r, lane) == col) dval = a[r];
            }
            continue;
        }
        if constexpr (VIDEO) {
            const long r0 = t * BN;
            if (tv.x == tv.y) {                                    // block-uniform: the tile lies inside one video
                float ms = -INFINITY;
                int mn = SENT_ROW;
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    const unsigned mine = (unsigned)(rows_in >> (rt * 32 + 4 * (lane >> 5)));    // FILTER: bit acc_row(r, 0) = the lane's row r
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const long n = r0 + rt * 32 + acc_row(r, lane);
                        bool valid = n < N;
                        if constexpr (FILTER) valid = valid && ((mine >> acc_row(r, 0)) & 1);
                        if (valid && better(acc[rt][r], (int)n, ms, mn)) { ms = acc[rt][r]; mn = (int)n; }
                    }
                }
                const float os = __shfl_xor(ms, 32, 64);
                const int on = __shfl_xor(mn, 32, 64);
                if (better(os, on, ms, mn)) { ms = os; mn = on; }
                const int need = (mn != SENT_ROW && ms >= thr) ? 1 : 0;
                if (__any(fill + need > CAP)) compact(need);
                if (need && lane < 32) { bs[bbase + fill] = ms; bn[bbase + fill] = mn; bv[bbase + fill] = tv.x; }
                fill += need;
                continue;
            }
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            const long nbase = t * BN + rt * 32;
            unsigned mask = 0;
            const unsigned mine = (unsigned)(rows_in >> (rt * 32 + 4 * (lane >> 5)));            // FILTER: bit acc_row(r, 0) = the lane's row r
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                bool valid = nbase + acc_row(r, lane) < N;
                if constexpr (FILTER) valid = valid && ((mine >> acc_row(r, 0)) & 1);
                const float v = acc[rt][r];
                hi += (valid && v > dq) ? 1 : 0;
                eq += (valid && v == dq) ? 1 : 0;
                if (valid && v >= thr) mask |= 1u << r;
            }
            if (k == 0) continue;
            const int c_me = __popc(mask), c_pt = __shfl_xor(c_me, 32, 64), need = c_me + c_pt;
            if (__any(fill + need > CAP)) compact(need);
            int off = bbase + fill + ((lane >> 5) ? c_pt : 0);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if ((mask >> r) & 1) {
                    bs[off] = acc[rt][r];
                    bn[off] = (int)(nbase + acc_row(r, lane));
                    if constexpr (VIDEO) bv[off] = vt[(it & 1) * BN + rt * 32 + acc_row(r, lane)];
                    ++off;
                }
            fill += need;
        }
    }

    if (PAIR) {
        if ((((col >> 2) & 1) == (lane >> 5)) && qok) {            // the lane that holds row == column of its 32x32 tile
            dscore[qme] = dval;
            if (higher) { higher[qme] = 0; ties[qme] = 0; }
        }
        return;
    }
    if (counting) {
        hi += __shfl_xor(hi, 32, 64);
        eq += __shfl_xor(eq, 32, 64);
        if (lane < 32 && qok) {
            atomicAdd(&higher[qme], hi);
            atomicAdd(&ties[qme], eq);
        }
    }
    if (k > 0) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        for (int qi = 0; qi < 32; ++qi) {
            const int f = __builtin_amdgcn_readlane(fill, qi);
            const int b = (wave * 32 + qi) * CAP;
            float s = lane < f ? bs[b + lane] : -INFINITY;
            int n = lane < f ? bn[b + lane] : SENT_ROW;
            int v = -1;
            if constexpr (VIDEO) {
                v = lane < f ? bv[b + lane] : -1;
                distinct64(s, n, v, lane);
            } else {
                sort64(s, n, lane);
            }
            const long q = qblk + wave * 32 + qi;
            if (q < Q && lane < k) {
                const long o = ((long)blockIdx.y * Q + q) * k + lane;
                part_s[o] = s;
                part_n[o] = n;
                if constexpr (VIDEO) part_v[o] = v;
            }
        }
    }
}

// tan_rank_topk_video's merge: the same fold, each step by distinct64 -- a video that straddles splits is in several lists and keeps
// its best entry.  A video of the global top k is in the list of the split that holds its best row (every video ahead of it in that
// split is ahead of it globally), so the result does not depend on the split count.
__global__ void __launch_bounds__(256) rank_merge_video_kernel(const float* __restrict__ part_s, const int* __restrict__ part_n,
                                                               const int* __restrict__ part_v, long Q, int k, int splits,
                                                               float* __restrict__ top_s, int* __restrict__ top_n, int* __restrict__ top_v) {
    const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= Q) return;
    float s = -INFINITY;
    int n = SENT_ROW, v = -1;
    for (int sp = 0; sp < splits; ++sp) {
        if (lane >= 32) {
            const bool real = lane - 32 < k;
            const long o = ((long)sp * Q + q) * k + (lane - 32);
            s = real ? part_s[o] : -INFINITY;
            n = real ? part_n[o] : SENT_ROW;
            v = real ? part_v[o] : -1;
        }
        distinct64(s, n, v, lane);
    }
    if (lane < k) {                                                // an empty slot (-inf, 0x7fffffff, -1): only under a broken v_off
        top_s[q * k + lane] = s;
        top_n[q * k + lane] = n;
        top_v[q * k + lane] = n != SENT_ROW ? v : -1;
    }
}

// tvid[t] = the videos of tile t's first and last row: the largest v in [0, n_videos) with v_off[v] <= row, so a v_off that breaks
// its contract still gives videos in range
__global__ void __launch_bounds__(256) tile_video_kernel(const int* __restrict__ v_off, int n_videos, long N, long n_tiles,
                                                         int2* __restrict__ tvid) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tiles) return;
    int found[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const long n = e == 0 ? t * BN : (t * BN + BN < N ? t * BN + BN : N) - 1;
        found[e] = video_search(v_off, n, 0, n_videos - 1);
    }
    tvid[t] = make_int2(found[0], found[1]);
}

// tile_video_kernel over a filter image's tile list: tvid[i] = the videos of the first and last row of the tile at list position i
__global__ void __launch_bounds__(256) tile_video_listed_kernel(const int* __restrict__ v_off, int n_videos, long N, long n_tiles,
                                                                const int* __restrict__ filt, int2* __restrict__ tvid) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    long nl = filt[0];
    nl = nl > n_tiles ? n_tiles : nl;
    if (i >= nl) return;
    long t = filt[FILT_HEAD + i];
    t = t < 0 ? 0 : (t >= n_tiles ? n_tiles - 1 : t);
    int found[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const long n = e == 0 ? t * BN : (t * BN + BN < N ? t * BN + BN : N) - 1;
        found[e] = video_search(v_off, n, 0, n_videos - 1);
    }
    tvid[i] = make_int2(found[0], found[1]);
}

// ---- the filter image of tan_row_filter_build (layout: include/tan_hip.h), in int32 words with T tiles, T2 = T rounded up to 2 and
// NB = ceil(T / 256):  [0] listed tiles, [1] T, [2..3] 0 | tile list [T2] | row masks u64 [T] | scratch: every tile's mask u64 [T],
// then NB block counts, scanned in place.  Three launches (counts / scan / fill), no atomics: the image does not depend on timing.
inline long filt_words(long T) { return FILT_HEAD + (T + 1) / 2 * 2 + 4 * T + (T + 255) / 256; }

// launch 1: one thread per tile -- the first span that ends above the tile's first row by binary search, then the spans that begin
// inside the tile (at most 64 when they keep their contract, and never more are looked at); a block's admitted tiles are counted
__global__ void __launch_bounds__(256) filter_mask_kernel(const int* __restrict__ spans, long n_spans, long N, long T,
                                                          int* __restrict__ img) {
    unsigned long long* dense = reinterpret_cast<unsigned long long*>(img + FILT_HEAD + (T + 1) / 2 * 2) + T;
    int* bcnt = img + FILT_HEAD + (T + 1) / 2 * 2 + 4 * T;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long m = 0;
    if (t < T) {
        const long r0 = t * BN, r1 = r0 + BN < N ? r0 + BN : N;
        long lo = 0, hi = n_spans;
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if (spans[2 * mid + 1] > r0) hi = mid; else lo = mid + 1;
        }
        for (int j = 0; j < BN && lo + j < n_spans; ++j) {
            const long a = spans[2 * (lo + j)], b = spans[2 * (lo + j) + 1];
            if (a >= r1) break;
            const long ca = a < r0 ? r0 : a, cb = b > r1 ? r1 : b;  // cut to the tile, which is cut to the index
            if (cb > ca) m |= (cb - ca == 64 ? ~0ull : ((1ull << (cb - ca)) - 1)) << (ca - r0);
        }
        dense[t] = m;
    }
    const int c = __syncthreads_count(m != 0);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = c;
}

// an exclusive scan over the block's 256 values; `total`: their sum.  All 256 threads must call it.
__device__ __forceinline__ int block_scan256(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int l = __shfl_up(inc, o, 64);
        if (lane >= o) inc += l;
    }
    __syncthreads();                                               // the previous call's readers are done
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return before + inc - v;
}

// launch 2: ONE block turns the block counts into each block's first list position and writes the header
__global__ void __launch_bounds__(256) filter_scan_kernel(long T, int* __restrict__ img) {
    __shared__ int wsum[4];
    int* bcnt = img + FILT_HEAD + (T + 1) / 2 * 2 + 4 * T;
    const long NB = (T + 255) / 256;
    int carry = 0;
    for (long b0 = 0; b0 < NB; b0 += 256) {
        const long b = b0 + threadIdx.x;
        int total;
        const int ex = block_scan256(b < NB ? bcnt[b] : 0, wsum, total);
        if (b < NB) bcnt[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) { img[0] = carry; img[1] = (int)T; img[2] = 0; img[3] = 0; }
}

// launch 3: an admitted tile's list position = its block's first position + the admitted tiles before it in the block
__global__ void __launch_bounds__(256) filter_fill_kernel(long T, int* __restrict__ img) {
    __shared__ int wsum[4];
    int* tiles = img + FILT_HEAD;
    unsigned long long* masks = reinterpret_cast<unsigned long long*>(img + FILT_HEAD + (T + 1) / 2 * 2);
    const unsigned long long* dense = masks + T;
    const int* bcnt = img + FILT_HEAD + (T + 1) / 2 * 2 + 4 * T;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long m = t < T ? dense[t] : 0;
    int total;
    const long pos = (long)bcnt[blockIdx.x] + block_scan256(m != 0 ? 1 : 0, wsum, total);
    if (m != 0 && pos >= 0 && pos < T) { tiles[pos] = (int)t; masks[pos] = m; }
}

// ---- ordered-sequence search: videos ranked by the best order-preserving path of a sequence of steps (include/tan_hip.h) ----
// A wave owns ONE sequence: its up to 32 steps are the wave's 32 resident query columns (padded columns are computed and ignored), a
// workgroup of four waves owns four sequences.  A split is a contiguous range of WHOLE videos -- a path needs all of its video: the
// index is cut into equal row ranges and a video goes to the split its first row falls in.  Every video is tiled from its own first
// row by tile_scores, the loop rank_kernel runs; the tail rows of its last tile are masked to -inf.  A lane's 16 accumulators belong
// to one step, so the wave writes its [32 steps][64 seconds] tile to LDS (pitch 65: both directions conflict-free up to the two
// half-waves) and runs tan_monotonic_decode's recurrence with lanes over seconds: per step one LDS read, one add, a 6-round inclusive
// max-scan, a max with the step's carry from the video's previous tile (lane i of `carry` holds step i's) and a readlane for the new
// carry.  The maximum is exact and each cell is one rounded add, so the path's bits do not depend on the tiling.  A finished video
// gives ONE candidate (path, video); the 64 candidates of a sequence live one per lane in registers, sort64 keeps the k best when they
// are full and raises the threshold.  The splits' lists are folded by rank_merge_kernel (row = video: the order is total).
// SCORES = true: tan_sequence_scores -- one workgroup per hit (sequence, video), all four waves hold the hit's sequence, and instead
// of the scan wave w writes the steps i = w mod 4 of the tile to x (lanes over seconds: coalesced).  Same routine, same bits.
constexpr int XS_LD = BN + 1;
constexpr int XS_WAVE = 32 * XS_LD;
template <typename T> constexpr int seq_lds() { return (tile_bytes<T>() + 15) / 16 * 16 + 4 * XS_WAVE * 4; }

// the number of videos whose first row lies below row r (r >= 1): whatever v_off holds, a value in [1, n_videos]
__device__ __forceinline__ int videos_below(const int* __restrict__ v_off, long r, int n_videos) {
    return video_search(v_off, r - 1, 0, n_videos - 1) + 1;
}

template <typename T, bool SCORES>
__global__ void __launch_bounds__(256) seq_kernel(const T* __restrict__ Tq, const T* __restrict__ Vn, long Qt, long N,
                                                  const int* __restrict__ s_off, int n_seq, const int* __restrict__ v_off,
                                                  int n_videos, int k, long rows_per_split, const float* __restrict__ q_scale,
                                                  const float* __restrict__ v_scale, float* __restrict__ part_s,
                                                  int* __restrict__ part_n, const int* __restrict__ hits, int n_hits,
                                                  const long* __restrict__ x_off, float* __restrict__ x, long n_x) {
#pragma clang fp contract(off)
    typedef Mma<T> M;
    typedef typename M::frag_t frag_t;
    constexpr int KC = RCfg<T>::KC, LD = RCfg<T>::LD, NCH = RC / KC, NFR = RC / M::KS;
    constexpr long ROWB = (long)RC * sizeof(T);
    constexpr bool F8 = sizeof(T) == 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* tile = reinterpret_cast<T*>(smem);
    float* sc = reinterpret_cast<float*>(smem + 2 * BN * LD * sizeof(T));
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31;
    float* xw = reinterpret_cast<float*>(smem + (tile_bytes<T>() + 15) / 16 * 16) + wave * XS_WAVE;

    // the wave's sequence and the workgroup's videos [va, vb); every lookup is clamped
    int p, va, vb;
    if constexpr (SCORES) {
        const int h = blockIdx.x;
        p = hits[2 * h];
        va = hits[2 * h + 1];
        va = va < 0 ? 0 : (va >= n_videos ? n_videos - 1 : va);
        vb = va + 1;
    } else {
        p = blockIdx.x * 4 + wave;
        const long r0 = (long)blockIdx.y * rows_per_split, r1 = r0 + rows_per_split;
        va = r0 <= 0 ? 0 : videos_below(v_off, r0, n_videos);
        vb = r1 >= N ? n_videos : videos_below(v_off, r1, n_videos);
    }
    const bool pok = p >= 0 && p < n_seq;
    p = p < 0 ? 0 : (p >= n_seq ? n_seq - 1 : p);
    long q0 = s_off[p];
    q0 = q0 < 0 ? 0 : (q0 >= Qt ? Qt - 1 : q0);
    long m_l = (long)s_off[p + 1] - q0;
    m_l = m_l > Qt - q0 ? Qt - q0 : m_l;
    const int m = m_l < 1 ? 1 : (m_l > 32 ? 32 : (int)m_l);        // wave-uniform

    frag_t qf[NFR];                                                // the sequence's steps, resident; columns >= m repeat the last step
    const long qme = q0 + (col < m ? col : m - 1);
    {
        const T* qrow = Tq + qme * RC;
#pragma unroll
        for (int j = 0; j < NFR; ++j) qf[j] = QFrag<T>::load(qrow, j, lane);
    }
    float qs = 1.0f, psc = 0.0f;
    if constexpr (F8) qs = q_scale[qme];

    long xo = 0;
    if constexpr (SCORES) {
        xo = x_off[blockIdx.x];
        long lo = v_off[va], hi = v_off[va + 1];
        lo = lo < 0 ? 0 : (lo > N ? N : lo);
        hi = hi < lo ? lo : (hi > N ? N : hi);
        if (!pok || xo < 0 || xo + (long)m * (hi - lo) > n_x) return;   // block-uniform: nothing is written outside x
    }

    // the tile under the MFMAs: video v, its rows [lo, hi) cut to the index, tile t of it
    struct Cur { int v; long lo, hi, t; };
    auto open = [&](int v) {
        Cur c{v, 0, 0, 0};
        if (v < vb) {
            c.lo = v_off[v];
            c.hi = v_off[v + 1];
            c.lo = c.lo < 0 ? 0 : (c.lo > N ? N : c.lo);
            c.hi = c.hi < c.lo ? c.lo : (c.hi > N ? N : c.hi);
        }
        return c;
    };
    uint4 pre[4];
    auto issue = [&](const Cur& c, int kc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = tid + 256 * i, row = v >> 4, c16 = v & 15;
            const long n = c.lo + c.t * BN + row;
            pre[i] = n < c.hi ? *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(Vn) + n * ROWB + kc * 256 + c16 * 16)
                              : make_uint4(0, 0, 0, 0);
        }
        if constexpr (F8) {
            if (kc == NCH - 1 && tid < BN) {
                const long n = c.lo + c.t * BN + tid;
                psc = n < c.hi ? v_scale[n] : 0.0f;
            }
        }
    };

    float cs = -INFINITY, thr = -INFINITY, carry = -INFINITY;
    int cn = SENT_ROW, fill = 0;                                   // fill, thr: wave-uniform

    Cur cur = open(va);
    if (cur.v < vb) issue(cur, 0);
    while (cur.v < vb) {                                           // block-uniform
        Cur nxt = cur;
        if ((cur.t + 1) * BN < cur.hi - cur.lo) ++nxt.t; else nxt = open(cur.v + 1);
        f32x16 acc[2];
        tile_scores<T>(tile, sc, tid, lane, pre, psc, qf, qs, acc, [&](int kc) {
            if (kc + 1 < NCH) issue(cur, kc + 1);
            else if (nxt.v < vb) issue(nxt, 0);
        });
        // the wave's tile -> LDS as [step][second]; only this wave reads it back
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) xw[col * XS_LD + rt * 32 + acc_row(r, lane)] = acc[rt][r];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const long V = cur.hi - cur.lo, left = V - cur.t * BN;     // the tile's seconds [0, left) are the video's
        if constexpr (SCORES) {
            if (lane < left)
                for (int i = wave; i < m; i += 4) x[xo + (long)i * V + cur.t * BN + lane] = xw[i * XS_LD + lane];
        } else {
            float mprev = 0.0f;
            for (int i = 0; i < m; ++i) {
                const float xi = lane < left ? xw[i * XS_LD + lane] : -INFINITY;
                float d = i ? xi + mprev : xi;                     // D_i[t]: one add, not contracted
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {                 // inclusive max-scan over the tile's seconds
                    const float l = __shfl_up(d, o, 64);
                    if (lane >= o && l > d) d = l;
                }
                const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(carry), i));
                d = c > d ? c : d;                                 // M_i[t]
                mprev = d;
                const float nc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 63));
                if (lane == i) carry = nc;
            }
            if (nxt.v != cur.v) {                                  // the video is finished: one candidate
                const float path = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(carry), m - 1));
                carry = -INFINITY;
                if (V > 0 && path >= thr) {                        // wave-uniform
                    if (lane == fill) { cs = path; cn = cur.v; }
                    if (++fill == CAP) {
                        sort64(cs, cn, lane);
                        thr = __shfl(cs, k - 1, 64);
                        if (lane >= k) { cs = -INFINITY; cn = SENT_ROW; }
                        fill = k;
                    }
                }
            }
        }
        cur = nxt;
    }
    if constexpr (!SCORES) {
        sort64(cs, cn, lane);
        if (pok && lane < k) {
            const long o = ((long)blockIdx.y * n_seq + p) * k + lane;
            part_s[o] = cs;
            part_n[o] = cn;
        }
    }
}

// ---- clip search: videos ranked by the best second-for-second match of a run of query rows (include/tan_hip.h) ----
// seq_kernel<T, false>'s frame with another epilogue: a wave owns ONE clip (its up to 32 rows are the wave's resident query columns,
// padded columns are computed and ignored), a workgroup four clips, a split the videos whose first row falls into its row range,
// every video is tiled from its own first row by tile_scores (rows past its end load as zero) and the wave's accumulators go to its
// [32][65] LDS block.  Then lanes stand over START seconds.  A diagonal of m <= 32 <= 64 cells crosses at most one tile edge, so a
// lane keeps two partial sums: `cur` for start 64 tile + lane and `prev` for start 64 (tile - 1) + lane.  Step i adds
// xw[i][lane + i] to cur while lane + i < 64 and xw[i][lane + i - 64] to prev afterwards: prev's earlier terms were added in the
// previous tile, so every S(t) is the definition's chain of f32 adds in ascending i whatever the tiling -- and the two chains of a
// lane are independent: no cross-lane scan.  The read address 65 i + lane + i (mod 64 past the edge) is a rotation of the lanes:
// conflict-free.  After the loop exactly one start per lane is complete (prev's where lane + m > 64, cur's otherwise); it feeds the
// lane's running (best, start) under strict >, and a lane meets its starts in ascending order, so the smallest start survives.
// No start is pending after a video's last tile: such a start would end beyond the video.  A finished video gives ONE candidate
// (S, v_off[v] + start, v) by a wave reduction (max score, then min start); the 64 candidates of a clip live one per lane in
// registers, sort64v keeps the k best when they are full and raises the threshold.  rank_merge_video_kernel folds the splits' lists
// (videos are distinct across splits: distinct64 only sorts).
template <typename T>
__global__ void __launch_bounds__(256) clip_kernel(const T* __restrict__ Tq, const T* __restrict__ Vn, long Qt, long N,
                                                   const int* __restrict__ c_off, int n_clip, const int* __restrict__ v_off,
                                                   int n_videos, int k, long rows_per_split, const float* __restrict__ q_scale,
                                                   const float* __restrict__ v_scale, float* __restrict__ part_s,
                                                   int* __restrict__ part_n, int* __restrict__ part_v) {
#pragma clang fp contract(off)
    typedef Mma<T> M;
    typedef typename M::frag_t frag_t;
    constexpr int KC = RCfg<T>::KC, LD = RCfg<T>::LD, NCH = RC / KC, NFR = RC / M::KS;
    constexpr long ROWB = (long)RC * sizeof(T);
    constexpr bool F8 = sizeof(T) == 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* tile = reinterpret_cast<T*>(smem);
    float* sc = reinterpret_cast<float*>(smem + 2 * BN * LD * sizeof(T));
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31;
    float* xw = reinterpret_cast<float*>(smem + (tile_bytes<T>() + 15) / 16 * 16) + wave * XS_WAVE;

    // the wave's clip and the workgroup's videos [va, vb); every lookup is clamped
    int p = blockIdx.x * 4 + wave;
    const long r0 = (long)blockIdx.y * rows_per_split, r1 = r0 + rows_per_split;
    const int va = r0 <= 0 ? 0 : videos_below(v_off, r0, n_videos);
    const int vb = r1 >= N ? n_videos : videos_below(v_off, r1, n_videos);
    const bool pok = p < n_clip;
    p = p >= n_clip ? n_clip - 1 : p;
    long q0 = c_off[p];
    q0 = q0 < 0 ? 0 : (q0 >= Qt ? Qt - 1 : q0);
    long m_l = (long)c_off[p + 1] - q0;
    m_l = m_l > Qt - q0 ? Qt - q0 : m_l;
    const int m = m_l < 1 ? 1 : (m_l > 32 ? 32 : (int)m_l);        // wave-uniform

    frag_t qf[NFR];                                                // the clip's rows, resident; columns >= m repeat the last row
    const long qme = q0 + (col < m ? col : m - 1);
    {
        const T* qrow = Tq + qme * RC;
#pragma unroll
        for (int j = 0; j < NFR; ++j) qf[j] = QFrag<T>::load(qrow, j, lane);
    }
    float qs = 1.0f, psc = 0.0f;
    if constexpr (F8) qs = q_scale[qme];

    // the tile under the MFMAs: video v, its rows [lo, hi) cut to the index, tile t of it
    struct Cur { int v; long lo, hi, t; };
    auto open = [&](int v) {
        Cur c{v, 0, 0, 0};
        if (v < vb) {
            c.lo = v_off[v];
            c.hi = v_off[v + 1];
            c.lo = c.lo < 0 ? 0 : (c.lo > N ? N : c.lo);
            c.hi = c.hi < c.lo ? c.lo : (c.hi > N ? N : c.hi);
        }
        return c;
    };
    uint4 pre[4];
    auto issue = [&](const Cur& c, int kc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = tid + 256 * i, row = v >> 4, c16 = v & 15;
            const long n = c.lo + c.t * BN + row;
            pre[i] = n < c.hi ? *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(Vn) + n * ROWB + kc * 256 + c16 * 16)
                              : make_uint4(0, 0, 0, 0);
        }
        if constexpr (F8) {
            if (kc == NCH - 1 && tid < BN) {
                const long n = c.lo + c.t * BN + tid;
                psc = n < c.hi ? v_scale[n] : 0.0f;
            }
        }
    };

    float cs = -INFINITY, thr = -INFINITY;                         // the candidate registers: (score, row, video), one per lane
    int cn = SENT_ROW, cv = -1, fill = 0;                          // fill, thr: wave-uniform
    float prev = 0.0f, best = -INFINITY;                           // the video under way: the lane's open diagonal and its best start
    int bstart = SENT_ROW;

    Cur cur = open(va);
    if (cur.v < vb) issue(cur, 0);
    while (cur.v < vb) {                                           // block-uniform
        Cur nxt = cur;
        if ((cur.t + 1) * BN < cur.hi - cur.lo) ++nxt.t; else nxt = open(cur.v + 1);
        f32x16 acc[2];
        tile_scores<T>(tile, sc, tid, lane, pre, psc, qf, qs, acc, [&](int kc) {
            if (kc + 1 < NCH) issue(cur, kc + 1);
            else if (nxt.v < vb) issue(nxt, 0);
        });
        // the wave's tile -> LDS as [clip row][second]; only this wave reads it back
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) xw[col * XS_LD + rt * 32 + acc_row(r, lane)] = acc[rt][r];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const long V = cur.hi - cur.lo;
        float sum = xw[lane];                                      // i = 0: the start 64 t + lane opens
#pragma unroll 4
        for (int i = 1; i < m; ++i) {
            const int j = lane + i;
            const bool here = j < BN;
            const float xi = xw[i * XS_LD + (here ? j : j - BN)];
            const float a = (here ? sum : prev) + xi;              // one add per cell, not contracted
            sum = here ? a : sum;
            prev = here ? prev : a;
        }
        {
            const bool done_here = lane + m <= BN;                 // else: the start of the previous tile is complete now
            const long t = (done_here ? cur.t : cur.t - 1) * BN + lane;
            const float s = done_here ? sum : prev;
            if (t >= 0 && t + m <= V && s > best) { best = s; bstart = (int)t; }
        }
        prev = sum;
        if (nxt.v != cur.v) {                                      // the video is finished: one candidate
            float ms = best;
            int mt = bstart;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float os = __shfl_xor(ms, o, 64);
                const int ot = __shfl_xor(mt, o, 64);
                if (better(os, ot, ms, mt)) { ms = os; mt = ot; }
            }
            best = -INFINITY;
            bstart = SENT_ROW;
            if (mt != SENT_ROW && ms >= thr) {                     // wave-uniform; a video shorter than the clip has no start
                if (lane == fill) { cs = ms; cn = (int)(cur.lo + mt); cv = cur.v; }
                if (++fill == CAP) {
                    sort64v(cs, cn, cv, lane);
                    thr = __shfl(cs, k - 1, 64);
                    if (lane >= k) { cs = -INFINITY; cn = SENT_ROW; cv = -1; }
                    fill = k;
                }
            }
        }
        cur = nxt;
    }
    sort64v(cs, cn, cv, lane);
    if (pok && lane < k) {
        const long o = ((long)blockIdx.y * n_clip + p) * k + lane;
        part_s[o] = cs;
        part_n[o] = cn;
        part_v[o] = cv;
    }
}

// ---- compound search: videos ranked by AND / OR / NOT of up to 32 query rows, in any order (include/tan_hip.h) ----
// seq_kernel<T, false>'s frame with a third epilogue, the lightest: a wave owns ONE compound query (its up to 32 terms are the wave's
// resident query columns, padded columns are computed and ignored), a workgroup four queries, a split the videos whose first row
// falls into its row range, every video is tiled from its own first row by tile_scores.  A lane's 32 accumulators belong to one term,
// so per tile the lane takes (max, first row) over its rows BELOW the video's end by better() -- a tail row loads as zero and is no
// candidate: it would beat every row of a video whose scores are all negative -- one __shfl_xor joins the two half-waves, and the
// result feeds the lane's running peak (pk, pr) of the video under strict better(): tiles arrive in ascending row order, so the first
// row that attains the maximum survives, with the bits it has at that row.  At the video's end the veto is one __any over the banned
// columns, a clause's value comes from a readlane loop over the m terms (the first term of the lane's own clause that none beats
// under >), and the score is a 32-lane min over (value, clause) -- the smaller value, equal values by the smaller clause: the fold in
// ascending clause order that replaces only under strict <.  No LDS beyond the tile buffers, no scan.  A finished video gives ONE
// candidate (score, video); the 64 candidates of a query live one per lane in registers, sort64 keeps the k best when they are full
// and raises the threshold.  rank_merge_kernel folds the splits' lists (row = video: the order is total).
// PEAKS = true: tan_compound_peaks -- one workgroup per hit (query, video), all four waves hold the hit's query, and at the video's end
// wave 0 writes the 32 columns' (peak, row), (-inf, 0x7fffffff) for columns >= m.  Same routine, same bits.
// bf16 / e4m3: held to seq_kernel's two waves per SIMD (256 registers a lane); f32's 256 resident fragment registers allow one.
template <typename T, bool PEAKS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sizeof(T) == 4 ? 1 : 2)))
compound_kernel(const T* __restrict__ Tq, const T* __restrict__ Vn, long Qt, long N,
                                                       const int* __restrict__ t_off, const int* __restrict__ role, int n_query,
                                                       const int* __restrict__ v_off, int n_videos, float veto, int k,
                                                       long rows_per_split, const float* __restrict__ q_scale,
                                                       const float* __restrict__ v_scale, float* __restrict__ part_s,
                                                       int* __restrict__ part_n, const int* __restrict__ hits,
                                                       float* __restrict__ peak_s, int* __restrict__ peak_n) {
    typedef Mma<T> M;
    typedef typename M::frag_t frag_t;
    constexpr int KC = RCfg<T>::KC, LD = RCfg<T>::LD, NCH = RC / KC, NFR = RC / M::KS;
    constexpr long ROWB = (long)RC * sizeof(T);
    constexpr bool F8 = sizeof(T) == 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* tile = reinterpret_cast<T*>(smem);
    float* sc = reinterpret_cast<float*>(smem + 2 * BN * LD * sizeof(T));
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31;

    // the wave's query and the workgroup's videos [va, vb); every lookup is clamped
    int p, va, vb;
    bool vok = true;
    if constexpr (PEAKS) {
        const int h = blockIdx.x;
        p = hits[2 * h];
        va = hits[2 * h + 1];
        vok = va >= 0 && va < n_videos;
        va = va < 0 ? 0 : (va >= n_videos ? n_videos - 1 : va);
        vb = va + 1;
    } else {
        p = blockIdx.x * 4 + wave;
        const long r0 = (long)blockIdx.y * rows_per_split, r1 = r0 + rows_per_split;
        va = r0 <= 0 ? 0 : videos_below(v_off, r0, n_videos);
        vb = r1 >= N ? n_videos : videos_below(v_off, r1, n_videos);
    }
    const bool pok = p >= 0 && p < n_query;
    p = p < 0 ? 0 : (p >= n_query ? n_query - 1 : p);
    long q0 = t_off[p];
    q0 = q0 < 0 ? 0 : (q0 >= Qt ? Qt - 1 : q0);
    long m_l = (long)t_off[p + 1] - q0;
    m_l = m_l > Qt - q0 ? Qt - q0 : m_l;
    const int m = m_l < 1 ? 1 : (m_l > 32 ? 32 : (int)m_l);        // wave-uniform

    if constexpr (PEAKS) {
        if (!pok || !vok) {                                        // block-uniform: a hit outside the tables gets the filler alone
            if (tid < 32) { peak_s[(long)blockIdx.x * 32 + tid] = -INFINITY; peak_n[(long)blockIdx.x * 32 + tid] = SENT_ROW; }
            return;
        }
    }

    frag_t qf[NFR];                                                // the query's terms, resident; columns >= m repeat the last term
    const long qme = q0 + (col < m ? col : m - 1);
    {
        const T* qrow = Tq + qme * RC;
#pragma unroll
        for (int j = 0; j < NFR; ++j) qf[j] = QFrag<T>::load(qrow, j, lane);
    }
    float qs = 1.0f, psc = 0.0f;
    if constexpr (F8) qs = q_scale[qme];
    int rl = -1;                                                   // the column's clause; -1: banned
    if constexpr (!PEAKS) rl = role[qme];
    const bool term = col < m;

    // the tile under the MFMAs: video v, its rows [lo, hi) cut to the index, tile t of it
    struct Cur { int v; long lo, hi, t; };
    auto open = [&](int v) {
        Cur c{v, 0, 0, 0};
        if (v < vb) {
            c.lo = v_off[v];
            c.hi = v_off[v + 1];
            c.lo = c.lo < 0 ? 0 : (c.lo > N ? N : c.lo);
            c.hi = c.hi < c.lo ? c.lo : (c.hi > N ? N : c.hi);
        }
        return c;
    };
    uint4 pre[4];
    auto issue = [&](const Cur& c, int kc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = tid + 256 * i, row = v >> 4, c16 = v & 15;
            const long n = c.lo + c.t * BN + row;
            pre[i] = n < c.hi ? *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(Vn) + n * ROWB + kc * 256 + c16 * 16)
                              : make_uint4(0, 0, 0, 0);
        }
        if constexpr (F8) {
            if (kc == NCH - 1 && tid < BN) {
                const long n = c.lo + c.t * BN + tid;
                psc = n < c.hi ? v_scale[n] : 0.0f;
            }
        }
    };

    float cs = -INFINITY, thr = -INFINITY;                         // the candidate registers: (score, video), one per lane
    int cn = SENT_ROW, fill = 0;                                   // fill, thr: wave-uniform
    float pk = -INFINITY;                                          // the video under way: the column's peak and its first row
    int pr = SENT_ROW;

    Cur cur = open(va);
    if (cur.v < vb) issue(cur, 0);
    while (cur.v < vb) {                                           // block-uniform
        Cur nxt = cur;
        if ((cur.t + 1) * BN < cur.hi - cur.lo) ++nxt.t; else nxt = open(cur.v + 1);
        f32x16 acc[2];
        tile_scores<T>(tile, sc, tid, lane, pre, psc, qf, qs, acc, [&](int kc) {
            if (kc + 1 < NCH) issue(cur, kc + 1);
            else if (nxt.v < vb) issue(nxt, 0);
        });
        const long V = cur.hi - cur.lo, left = V - cur.t * BN;     // the tile's rows [0, left) are the video's
        const int nl = left < BN ? (int)left : BN;
        float ms = -INFINITY;
        int mn = SENT_ROW;                                         // a tile row here; the global row below
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = rt * 32 + acc_row(r, lane);
                if (j < nl && better(acc[rt][r], j, ms, mn)) { ms = acc[rt][r]; mn = j; }
            }
        {
            const float os = __shfl_xor(ms, 32, 64);
            const int on = __shfl_xor(mn, 32, 64);
            if (better(os, on, ms, mn)) { ms = os; mn = on; }
        }
        if (mn != SENT_ROW) {
            const int n = (int)(cur.lo + cur.t * BN + mn);
            if (better(ms, n, pk, pr)) { pk = ms; pr = n; }
        }
        if (nxt.v != cur.v) {                                      // the video is finished
            if constexpr (PEAKS) {
                if (wave == 0 && lane < 32) {
                    peak_s[(long)blockIdx.x * 32 + lane] = term ? pk : -INFINITY;
                    peak_n[(long)blockIdx.x * 32 + lane] = term ? pr : SENT_ROW;
                }
            } else {
                const bool vetoed = __any(term && rl < 0 && pk >= veto);
                float g = -INFINITY;                               // the value of the lane's own clause (OR)
                for (int i = 0; i < m; ++i) {
                    const float pi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pk), i));
                    const int ri = __builtin_amdgcn_readlane(rl, i);
                    if (ri == rl && pi > g) g = pi;
                }
                const bool clause = term && rl >= 0;
                float ws = clause ? g : INFINITY;                  // the weakest clause (AND); both half-waves hold the same columns
                int wj = clause ? rl : SENT_ROW;
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) {
                    const float os = __shfl_xor(ws, o, 64);
                    const int oj = __shfl_xor(wj, o, 64);
                    if (os < ws || (os == ws && oj < wj)) { ws = os; wj = oj; }
                }
                if (V > 0 && !vetoed && wj != SENT_ROW && ws >= thr) {     // wave-uniform; one candidate
                    if (lane == fill) { cs = ws; cn = cur.v; }
                    if (++fill == CAP) {
                        sort64(cs, cn, lane);
                        thr = __shfl(cs, k - 1, 64);
                        if (lane >= k) { cs = -INFINITY; cn = SENT_ROW; }
                        fill = k;
                    }
                }
            }
            pk = -INFINITY;
            pr = SENT_ROW;
        }
        cur = nxt;
    }
    if constexpr (!PEAKS) {
        sort64(cs, cn, lane);
        if (pok && lane < k) {
            const long o = ((long)blockIdx.y * n_query + p) * k + lane;
            part_s[o] = cs;
            part_n[o] = cn;
        }
    }
}

// ---- one wave per frame row: 64 lanes x 8 channels
template <typename T> __device__ __forceinline__ f8 ld_row8(const T* p) {
    if constexpr (sizeof(T) == 2) return ld8(p); else return ld8f(p);
}
template <> __device__ __forceinline__ f8 ld_row8<e4m3_t>(const e4m3_t* p) {               // 8 e4m3fn codes -> f32 (exact)
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)u.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)u.x, true);
    const auto c = __builtin_amdgcn_cvt_pk_f32_fp8((int)u.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)u.y, true);
    f8 r;
    r.v[0] = a[0]; r.v[1] = a[1]; r.v[2] = b[0]; r.v[3] = b[1]; r.v[4] = c[0]; r.v[5] = c[1]; r.v[6] = d[0]; r.v[7] = d[1];
    return r;
}

// tan_moment_extent: one wave per hit walks outward from the peak row, EB rows per step (their loads in flight together), and stops
// at the first row below the threshold: the cost follows the moment's length.  s(q, n): a lane's 8 products summed in element order,
// then wave_sum; e4m3: (acc * v_scale[n]) * q_scale[q].  No atomics, no scratch.
constexpr int EB = 4;
template <typename T>
__global__ void __launch_bounds__(256) moment_extent_kernel(const T* __restrict__ Tq, const T* __restrict__ Vn, long Q, long N, int k,
                                                            const int* __restrict__ v_off, int n_videos,
                                                            const float* __restrict__ top_s, const int* __restrict__ top_n,
                                                            const int* __restrict__ top_v, float width,
                                                            const float* __restrict__ q_scale, const float* __restrict__ v_scale,
                                                            int* __restrict__ start, int* __restrict__ end) {
    constexpr bool F8 = sizeof(T) == 1;
    const long h = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (h >= Q * k) return;
    const long q = h / k;
    long p = top_n[h];
    p = p < 0 ? 0 : (p >= N ? N - 1 : p);                          // memory safety only: hits outside the index are the caller's error
    int v = top_v[h];
    v = v < 0 ? 0 : (v >= n_videos ? n_videos - 1 : v);
    long lo = v_off[v], hi = v_off[v + 1];                         // the video's rows [lo, hi), cut to the index and around p
    lo = lo < 0 ? 0 : (lo > p ? p : lo);
    hi = hi > N ? N : hi;
    hi = hi < p + 1 ? p + 1 : hi;
    const float thr = top_s[h] - width;
    const f8 qv = ld_row8<T>(Tq + q * RC + lane * 8);
    float qs = 1.0f;
    if constexpr (F8) qs = q_scale[q];
    auto score = [&](const f8& x, long n) {
        float a = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) a += x.v[i] * qv.v[i];
        a = wave_sum(a);
        if constexpr (F8) a = (a * v_scale[n]) * qs;
        return a;
    };
    long s0 = p, e0 = p;
    while (s0 > lo) {                                              // wave-uniform
        const int nb = s0 - lo < EB ? (int)(s0 - lo) : EB;
        f8 x[EB];
#pragma unroll
        for (int j = 0; j < EB; ++j) x[j] = ld_row8<T>(Vn + (s0 - 1 - (j < nb ? j : nb - 1)) * RC + lane * 8);
        int ok = 0;
        bool open = true;
#pragma unroll
        for (int j = 0; j < EB; ++j) {
            open = open && j < nb && score(x[j], s0 - 1 - (j < nb ? j : nb - 1)) >= thr;
            ok += open ? 1 : 0;
        }
        s0 -= ok;
        if (ok < nb) break;
    }
    while (e0 + 1 < hi) {
        const int nb = hi - 1 - e0 < EB ? (int)(hi - 1 - e0) : EB;
        f8 x[EB];
#pragma unroll
        for (int j = 0; j < EB; ++j) x[j] = ld_row8<T>(Vn + (e0 + 1 + (j < nb ? j : nb - 1)) * RC + lane * 8);
        int ok = 0;
        bool open = true;
#pragma unroll
        for (int j = 0; j < EB; ++j) {
            open = open && j < nb && score(x[j], e0 + 1 + (j < nb ? j : nb - 1)) >= thr;
            ok += open ? 1 : 0;
        }
        e0 += ok;
        if (ok < nb) break;
    }
    if (lane == 0) { start[h] = (int)s0; end[h] = (int)e0; }
}
template <typename T> __device__ __forceinline__ f8 unit_row(const T* row, int lane, bool normalize) {
    f8 x = ld_row8<T>(row + lane * 8);
    if (normalize) {
        float ss = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) ss += x.v[i] * x.v[i];
        const float nrm = sqrtf(wave_sum(ss));
#pragma unroll
        for (int i = 0; i < 8; ++i) x.v[i] = x.v[i] / nrm;
    }
    return x;
}

// one block per window; the first window of the launch that names a clip owns it and adds all of them in window order
template <typename T>
__global__ void __launch_bounds__(256) segment_pool_acc_kernel(const T* __restrict__ stage, long win_stride, int T_len,
                                                               const int* __restrict__ table, int W, int normalize,
                                                               float* __restrict__ sum, float* __restrict__ cnt, int n_clips) {
    __shared__ float part[4][RC];
    const int w = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int clip = table[3 * w];
    if (clip < 0 || clip >= n_clips) return;
    for (int w2 = 0; w2 < w; ++w2)
        if (table[3 * w2] == clip) return;                          // block-uniform
    float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int frames = 0, slot = 0;
    for (int w2 = w; w2 < W; ++w2) {
        if (table[3 * w2] != clip) continue;
        int f0 = table[3 * w2 + 1], nf = table[3 * w2 + 2];
        f0 = f0 < 0 ? 0 : f0;
        nf = f0 + nf > T_len ? T_len - f0 : nf;
        for (int f = 0; f < nf; ++f, ++slot) {
            if ((slot & 3) != wave) continue;
            const f8 x = unit_row<T>(stage + (long)w2 * win_stride + (long)(f0 + f) * RC, lane, normalize != 0);
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] += x.v[i];
        }
        frames += nf > 0 ? nf : 0;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) part[wave][lane * 8 + i] = a[i];
    __syncthreads();
    for (int c = threadIdx.x; c < RC; c += 256)
        sum[(long)clip * RC + c] += ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
    if (threadIdx.x == 0) cnt[clip] += (float)frames;
}

__global__ void __launch_bounds__(256) segment_pool_final_kernel(const float* __restrict__ sum, const float* __restrict__ cnt, int n_clips,
                                                                 int normalize, float* __restrict__ out) {
    const long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= n_clips) return;
    f8 x = ld8f(sum + c * RC + lane * 8);
    const float m = cnt[c];
    float ss = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) { x.v[i] = x.v[i] / m; ss += x.v[i] * x.v[i]; }
    if (normalize) {
        const float nrm = sqrtf(wave_sum(ss));
#pragma unroll
        for (int i = 0; i < 8; ++i) x.v[i] = x.v[i] / nrm;
    }
    st4(out + c * RC + lane * 8, make_float4(x.v[0], x.v[1], x.v[2], x.v[3]));
    st4(out + c * RC + lane * 8 + 4, make_float4(x.v[4], x.v[5], x.v[6], x.v[7]));
}

// one block per window, one wave per frame; index row g = vrow + frame.  Windows are in plan order (packed rows ascending), so the
// windows that can cover g are the neighbours whose [vrow, vrow + t) holds it.
template <typename T>
__global__ void __launch_bounds__(256) window_feat_acc_kernel(const T* __restrict__ feat, long win_stride, const int* __restrict__ table,
                                                              int W, int T_len, float* __restrict__ acc, float* __restrict__ cnt,
                                                              long n_rows) {
    constexpr int NF = TAN_WIN_FIELDS;
    const int w = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int* e = table + (long)w * NF;
    const int t_w = min(e[1], T_len);
    for (int tt = wave; tt < t_w; tt += 4) {
        const long g = (long)e[0] + tt;
        if (g < 0 || g >= n_rows) continue;
        bool owner = true;
        for (int w2 = w - 1; w2 >= 0; --w2) {
            const int* e2 = table + (long)w2 * NF;
            if ((long)e2[0] + min(e2[1], T_len) <= g) break;
            if (e2[0] <= g) { owner = false; break; }
        }
        if (!owner) continue;
        f8 a = ld8f(acc + g * RC + lane * 8);
        float c = cnt[g];
        for (int w2 = w; w2 < W; ++w2) {
            const int* e2 = table + (long)w2 * NF;
            if (e2[0] > g) break;
            if (g >= (long)e2[0] + min(e2[1], T_len)) continue;
            const f8 x = unit_row<T>(feat + (long)w2 * win_stride + (g - e2[0]) * RC, lane, true);
#pragma unroll
            for (int i = 0; i < 8; ++i) a.v[i] += x.v[i];
            c += 1.0f;
        }
        st4(acc + g * RC + lane * 8, make_float4(a.v[0], a.v[1], a.v[2], a.v[3]));
        st4(acc + g * RC + lane * 8 + 4, make_float4(a.v[4], a.v[5], a.v[6], a.v[7]));
        if (lane == 0) cnt[g] = c;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) window_feat_final_kernel(const float* __restrict__ acc, const float* __restrict__ cnt, long n_rows,
                                                                T* __restrict__ out) {
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n_rows) return;
    f8 x = ld8f(acc + g * RC + lane * 8);
    const float m = fmaxf(cnt[g], 1.0f);
#pragma unroll
    for (int i = 0; i < 8; ++i) x.v[i] = x.v[i] / m;
    if constexpr (sizeof(T) == 2) {
        st8(out + g * RC + lane * 8, x);
    } else {
        st4(out + g * RC + lane * 8, make_float4(x.v[0], x.v[1], x.v[2], x.v[3]));
        st4(out + g * RC + lane * 8 + 4, make_float4(x.v[4], x.v[5], x.v[6], x.v[7]));
    }
}

// one wave per row: amax by shuffle-reduce, the power-of-two scale of include/tan_hip.h from amax's bits, v_cvt_pk_fp8_f32 (RNE, OCP
// e4m3fn on gfx950), one 8-byte store per lane.  amax = m 2^e with m in [0.5, 1): e = (bits >> 23) - 126 and m <= 0.875 <=> the
// fraction field <= 0x600000.  A subnormal amax would give s < -126 and takes the clamp.
template <typename T>
__global__ void __launch_bounds__(256) quantize_rows_kernel(const T* __restrict__ x, long n_rows, uint2* __restrict__ codes,
                                                            float* __restrict__ scale) {
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n_rows) return;
    const f8 v = ld_row8<T>(x + g * RC + lane * 8);
    float am = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) am = fmaxf(am, fabsf(v.v[i]));
    am = wave_max(am);
    const unsigned bits = __float_as_uint(am);
    const int eb = (int)(bits >> 23);
    int s = eb - 126 - ((bits & 0x7fffffu) <= 0x600000u ? 9 : 8);
    s = (eb == 0 || s < -126) ? -126 : s;
    s = am == 0.0f ? 0 : s;
    const float inv = __uint_as_float((unsigned)(127 - s) << 23);      // 2^-s; s <= 121 for any bit pattern, so this is a normal number
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(v.v[0] * inv, v.v[1] * inv, lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(v.v[2] * inv, v.v[3] * inv, lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(v.v[4] * inv, v.v[5] * inv, hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(v.v[6] * inv, v.v[7] * inv, hi, true);
    codes[g * (RC / 8) + lane] = make_uint2((unsigned)lo, (unsigned)hi);
    if (lane == 0) scale[g] = __uint_as_float((unsigned)(s + 127) << 23);
}

// a sweep's scratch: VIDEO: tvid [tiles rounded up to 2] int2, otherwise dscore [Q rounded up to 4] f32; then the splits' lists
// (score, row[, video]), 4 bytes per entry each
inline long sweep_ws_head(bool video, long Q, long N) { return video ? (n_index_tiles(N) + 1) / 2 * 2 * 8 : (Q + 3) / 4 * 4 * 4; }

// The four sweeps (tan_rank_topk / _video / _filtered / _video_filtered).  `pair`: FILTER: the filter image, which rides in the
// kernel's `pair` argument; otherwise the paired rows or nullptr (VIDEO: always nullptr).  The pair launch belongs to the plain
// sweep alone; higher / ties are its, v_off / n_videos / top_v the VIDEO sweeps'.  The grid is sized from (Q, N, splits) whatever the
// filter lists.
template <typename T, bool VIDEO, bool FILTER>
int sweep_launch(const void* Tq, const void* Vn, long Q, long N, const int* pair, const int* v_off, int n_videos, int k, int splits,
                 int* higher, int* ties, float* top_s, int* top_n, int* top_v, void* ws, hipStream_t st, const float* q_scale,
                 const float* v_scale) {
    const long n_tiles = n_index_tiles(N), q_tiles = (Q + BQ - 1) / BQ;
    long tps;
    const int ns = n_splits(Q, N, splits, &tps);
    float* dscore = VIDEO || FILTER ? nullptr : (float*)ws;
    int2* tvid = VIDEO ? (int2*)ws : nullptr;
    float* part_s = (float*)((char*)ws + sweep_ws_head(VIDEO, Q, N));
    int* part_n = (int*)(part_s + (long)ns * Q * k);
    int* part_v = VIDEO ? part_n + (long)ns * Q * k : nullptr;
    if constexpr (VIDEO && FILTER) {
        hipLaunchKernelGGL(tile_video_listed_kernel, dim3(cdiv(n_tiles, 256)), dim3(256), 0, st, v_off, n_videos, N, n_tiles, pair, tvid);
        TAN_LAUNCH_CHECK();
    } else if constexpr (VIDEO) {
        hipLaunchKernelGGL(tile_video_kernel, dim3(cdiv(n_tiles, 256)), dim3(256), 0, st, v_off, n_videos, N, n_tiles, tvid);
        TAN_LAUNCH_CHECK();
    } else if constexpr (!FILTER) {
        if (pair) {
            hipLaunchKernelGGL((rank_kernel<T, true>), dim3((unsigned)q_tiles), dim3(256), tile_bytes<T>(), st, (const T*)Tq, (const T*)Vn,
                               Q, N, pair, 0, 0L, 0L, dscore, higher, ties, (float*)nullptr, (int*)nullptr, q_scale, v_scale,
                               (const int2*)nullptr, (const int*)nullptr, (int*)nullptr);
            TAN_LAUNCH_CHECK();
        }
    }
    static std::atomic<unsigned long long> lds_done{0};            // one per instantiation
    constexpr int lds = sweep_lds<T, VIDEO>();
    const hipError_t attr = ensure_dyn_lds((const void*)rank_kernel<T, false, VIDEO, FILTER>, lds, lds_done);
    if (attr != hipSuccess) return (int)attr;
    hipLaunchKernelGGL((rank_kernel<T, false, VIDEO, FILTER>), dim3((unsigned)q_tiles, (unsigned)ns), dim3(256), lds, st, (const T*)Tq,
                       (const T*)Vn, Q, N, pair, k, tps, n_tiles, dscore, higher, ties, part_s, part_n, q_scale, v_scale,
                       (const int2*)tvid, v_off, part_v);
    TAN_LAUNCH_CHECK();
    if constexpr (VIDEO) {
        hipLaunchKernelGGL(rank_merge_video_kernel, dim3(cdiv(Q, 4)), dim3(256), 0, st, part_s, part_n, (const int*)part_v, Q, k, ns, top_s,
                           top_n, top_v);
        TAN_LAUNCH_CHECK();
    } else if (k > 0) {
        hipLaunchKernelGGL(rank_merge_kernel, dim3(cdiv(Q, 4)), dim3(256), 0, st, part_s, part_n, Q, k, ns, top_s, top_n);
        TAN_LAUNCH_CHECK();
    }
    return 0;
}

template <typename T>
int extent_launch(const void* Tq, const void* Vn, long Q, long N, const int* v_off, int n_videos, int k, const float* top_s,
                  const int* top_n, const int* top_v, float width, int* start, int* end, hipStream_t st,
                  const float* q_scale = nullptr, const float* v_scale = nullptr) {
    hipLaunchKernelGGL(moment_extent_kernel<T>, dim3(cdiv(Q * k, 4)), dim3(256), 0, st, (const T*)Tq, (const T*)Vn, Q, N, k, v_off,
                       n_videos, top_s, top_n, top_v, width, q_scale, v_scale, start, end);
    TAN_LAUNCH_CHECK();
    return 0;
}

inline bool video_sizes_ok(long Q, long N, int C, long n_videos, int k) {
    return C == RC && Q >= 1 && Q < (1L << 31) && N >= 1 && N < (1L << 31) && n_videos >= 1 && n_videos <= N && k >= 1 && k <= KMAX &&
           k <= n_videos;
}

// how many splits the sequence sweep launches and the index rows each one covers (a video goes to the split of its first row)
inline int n_seq_splits(long n_seq, long N, int splits, long* rows_per_split) {
    const long blocks = (n_seq + 3) / 4;
    long want = splits > 0 ? splits : (512 + blocks - 1) / blocks;
    want = want < 1 ? 1 : (want > MAX_SPLITS ? MAX_SPLITS : want);
    want = want > n_index_tiles(N) ? n_index_tiles(N) : want;
    *rows_per_split = (N + want - 1) / want;
    return (int)((N + *rows_per_split - 1) / *rows_per_split);
}

inline bool seq_sizes_ok(long Qt, long N, int C, long n_seq, long n_videos) {
    return C == RC && N >= 1 && N < (1L << 31) && n_seq >= 1 && n_seq < (1L << 29) && Qt >= n_seq && Qt <= 32 * n_seq && n_videos >= 1 &&
           n_videos <= N;
}

// ws: the splits' lists (score, video)
template <typename T>
int seq_topk_launch(const void* Tq, const void* Vn, long Qt, long N, const int* s_off, long n_seq, const int* v_off, int n_videos, int k,
                    int splits, float* top_s, int* top_v, void* ws, hipStream_t st, const float* q_scale = nullptr,
                    const float* v_scale = nullptr) {
    long rps;
    const int ns = n_seq_splits(n_seq, N, splits, &rps);
    float* part_s = (float*)ws;
    int* part_n = (int*)(part_s + (long)ns * n_seq * k);
    static std::atomic<unsigned long long> lds_done{0};
    const hipError_t attr = ensure_dyn_lds((const void*)seq_kernel<T, false>, seq_lds<T>(), lds_done);
    if (attr != hipSuccess) return (int)attr;
    hipLaunchKernelGGL((seq_kernel<T, false>), dim3(cdiv(n_seq, 4), (unsigned)ns), dim3(256), seq_lds<T>(), st, (const T*)Tq,
                       (const T*)Vn, Qt, N, s_off, (int)n_seq, v_off, n_videos, k, rps, q_scale, v_scale, part_s, part_n,
                       (const int*)nullptr, 0, (const long*)nullptr, (float*)nullptr, 0L);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(rank_merge_kernel, dim3(cdiv(n_seq, 4)), dim3(256), 0, st, part_s, part_n, n_seq, k, ns, top_s, top_v);
    TAN_LAUNCH_CHECK();
    return 0;
}

// ws: the splits' lists (score, row, video); the splits are the sequence sweep's
template <typename T>
int clip_topk_launch(const void* Tq, const void* Vn, long Qt, long N, const int* c_off, long n_clip, const int* v_off, int n_videos, int k,
                     int splits, float* top_s, int* top_n, int* top_v, void* ws, hipStream_t st, const float* q_scale = nullptr,
                     const float* v_scale = nullptr) {
    long rps;
    const int ns = n_seq_splits(n_clip, N, splits, &rps);
    float* part_s = (float*)ws;
    int* part_n = (int*)(part_s + (long)ns * n_clip * k);
    int* part_v = part_n + (long)ns * n_clip * k;
    static std::atomic<unsigned long long> lds_done{0};
    const hipError_t attr = ensure_dyn_lds((const void*)clip_kernel<T>, seq_lds<T>(), lds_done);
    if (attr != hipSuccess) return (int)attr;
    hipLaunchKernelGGL((clip_kernel<T>), dim3(cdiv(n_clip, 4), (unsigned)ns), dim3(256), seq_lds<T>(), st, (const T*)Tq, (const T*)Vn, Qt,
                       N, c_off, (int)n_clip, v_off, n_videos, k, rps, q_scale, v_scale, part_s, part_n, part_v);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(rank_merge_video_kernel, dim3(cdiv(n_clip, 4)), dim3(256), 0, st, part_s, part_n, (const int*)part_v, n_clip, k, ns,
                       top_s, top_n, top_v);
    TAN_LAUNCH_CHECK();
    return 0;
}

// ws: the splits' lists (score, video); the splits are the sequence sweep's.  The tile buffers are the whole LDS: below the 64 KiB that
// need no attribute.
template <typename T>
int compound_topk_launch(const void* Tq, const void* Vn, long Qt, long N, const int* t_off, const int* role, long n_query,
                         const int* v_off, int n_videos, float veto, int k, int splits, float* top_s, int* top_v, void* ws,
                         hipStream_t st, const float* q_scale = nullptr, const float* v_scale = nullptr) {
    static_assert(tile_bytes<T>() <= 48 * 1024, "compound_kernel's LDS needs the dynamic-LDS attribute");
    long rps;
    const int ns = n_seq_splits(n_query, N, splits, &rps);
    float* part_s = (float*)ws;
    int* part_n = (int*)(part_s + (long)ns * n_query * k);
    hipLaunchKernelGGL((compound_kernel<T, false>), dim3(cdiv(n_query, 4), (unsigned)ns), dim3(256), tile_bytes<T>(), st, (const T*)Tq,
                       (const T*)Vn, Qt, N, t_off, role, (int)n_query, v_off, n_videos, veto, k, rps, q_scale, v_scale, part_s, part_n,
                       (const int*)nullptr, (float*)nullptr, (int*)nullptr);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(rank_merge_kernel, dim3(cdiv(n_query, 4)), dim3(256), 0, st, part_s, part_n, n_query, k, ns, top_s, top_v);
    TAN_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int compound_peaks_launch(const void* Tq, const void* Vn, long Qt, long N, const int* t_off, long n_query, const int* v_off, int n_videos,
                          const int* hits, long P, float* peak_s, int* peak_n, hipStream_t st, const float* q_scale = nullptr,
                          const float* v_scale = nullptr) {
    hipLaunchKernelGGL((compound_kernel<T, true>), dim3((unsigned)P), dim3(256), tile_bytes<T>(), st, (const T*)Tq, (const T*)Vn, Qt, N,
                       t_off, (const int*)nullptr, (int)n_query, v_off, n_videos, 0.0f, 0, 0L, q_scale, v_scale, (float*)nullptr,
                       (int*)nullptr, hits, peak_s, peak_n);
    TAN_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int seq_scores_launch(const void* Tq, const void* Vn, long Qt, long N, const int* s_off, long n_seq, const int* v_off, int n_videos,
                      const int* hits, const long* x_off, long P, float* x, long n_x, hipStream_t st, const float* q_scale = nullptr,
                      const float* v_scale = nullptr) {
    static std::atomic<unsigned long long> lds_done{0};
    const hipError_t attr = ensure_dyn_lds((const void*)seq_kernel<T, true>, seq_lds<T>(), lds_done);
    if (attr != hipSuccess) return (int)attr;
    hipLaunchKernelGGL((seq_kernel<T, true>), dim3((unsigned)P), dim3(256), seq_lds<T>(), st, (const T*)Tq, (const T*)Vn, Qt, N, s_off,
                       (int)n_seq, v_off, n_videos, 0, 0L, q_scale, v_scale, (float*)nullptr, (int*)nullptr, hits, (int)P, x_off, x, n_x);
    TAN_LAUNCH_CHECK();
    return 0;
}

// ---- corpus annotation: the k best LABELS of every index row (include/tan_hip.h) ----
// rank_kernel's sweep with the roles swapped: a workgroup owns one tile of BQ = 128 index rows -- a wave keeps its 32 rows in
// registers as the B fragments, read from HBM once in the whole launch -- and the label matrix streams through LDS in 64-label tiles
// by tile_scores.  A lane's 16 accumulators belong to ONE index row, whose candidates (score, label) at or above its threshold go
// to its 64-slot LDS buffer; sort64 compacts a buffer that would overflow and raises the threshold.  A row's list is complete
// inside its workgroup: no splits, no scratch, no merge -- the epilogue sorts each buffer once more and writes the k best to
// top_s / top_l.  e4m3: tile_scores multiplies by the TILE's scale first and the resident column's second, and the score is defined
// as (acc * v_scale[n]) * l_scale[l] (tan_rank_topk_e4m3's formula with the label as the query), so tile_scores gets a tile scale
// of 1 and the row's scale as the column's -- a multiply by 1 is exact -- and the label tile's 64 scales, loaded with the tile's
// first chunk, wait in a buffer of their own (two, by tile parity: a wave may stage tile t + 1's while another still reads tile
// t's) for the multiply after the MFMA loop.
template <typename T> constexpr int label_lds() { return sweep_lds<T>() + (sizeof(T) == 1 ? 2 * BN * 4 : 0); }

template <typename T>
__global__ void __launch_bounds__(256) label_kernel(const T* __restrict__ Tl, const T* __restrict__ Vn, long L, long N, int k,
                                                    long l_tiles, float* __restrict__ top_s, int* __restrict__ top_l,
                                                    const float* __restrict__ l_scale, const float* __restrict__ v_scale) {
    typedef Mma<T> M;
    typedef typename M::frag_t frag_t;
    constexpr int LD = RCfg<T>::LD, KS = M::KS, NCH = RC / RCfg<T>::KC, NFR = RC / KS;
    constexpr int TS = BN * LD;
    constexpr long ROWB = (long)RC * sizeof(T);
    constexpr bool F8 = sizeof(T) == 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* tile = reinterpret_cast<T*>(smem);
    float* sc = reinterpret_cast<float*>(smem + 2 * TS * sizeof(T));   // F8: tile_scores' tile scales, all 1 here
    float* bs = reinterpret_cast<float*>(smem + (tile_bytes<T>() + 15) / 16 * 16);
    int* bn = reinterpret_cast<int*>(bs + 4 * 32 * CAP);
    float* lsc = reinterpret_cast<float*>(bn + 4 * 32 * CAP);         // F8: the label scales of two tiles

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31;
    const long nblk = (long)blockIdx.x * BQ;
    const long nme = nblk + wave * 32 + col;
    const long nrow = nme < N ? nme : N - 1;                       // a tail column repeats the last row and is not written

    frag_t qf[NFR];                                                // the wave's 32 index rows, resident
    {
        const T* vrow = Vn + nrow * RC;
#pragma unroll
        for (int j = 0; j < NFR; ++j) qf[j] = QFrag<T>::load(vrow, j, lane);
    }
    float vs = 1.0f, pls = 0.0f;
    const float one = 1.0f;
    if constexpr (F8) vs = v_scale[nrow];

    int fill = 0;
    float thr = -INFINITY;
    const int bbase = (wave * 32 + col) * CAP;

    uint4 pre[4];
    auto issue = [&](long t, int kc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = tid + 256 * i, row = v >> 4, c16 = v & 15;
            const long l = t * BN + row;
            pre[i] = l < L ? *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(Tl) + l * ROWB + kc * 256 + c16 * 16)
                           : make_uint4(0, 0, 0, 0);
        }
        if constexpr (F8) {
            if (kc == 0 && tid < BN) {                             // the label scales ride with the tile's first chunk
                const long l = t * BN + tid;
                pls = l < L ? l_scale[l] : 0.0f;
            }
        }
    };

    // rank_kernel's compaction: sorts every buffer of the wave that `need` more entries would overflow, keeps its k best and raises
    // the row's threshold
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

    issue(0, 0);                                                   // l_tiles >= 1
    for (long t = 0; t < l_tiles; ++t) {
        if constexpr (F8) {
            // read after this tile's barriers; the buffer's next write follows tile t + 1's barriers, which no wave passes before
            // every wave has left this tile's epilogue
            if (tid < BN) lsc[(t & 1) * BN + tid] = pls;
        }
        f32x16 acc[2];
        tile_scores<T>(tile, sc, tid, lane, pre, one, qf, vs, acc, [&](int kc) {
            if (kc + 1 < NCH) issue(t, kc + 1);
            else if (t + 1 < l_tiles) issue(t + 1, 0);
        });
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            if constexpr (F8) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 s4 = *reinterpret_cast<const float4*>(lsc + (t & 1) * BN + rt * 32 + 8 * g + 4 * (lane >> 5));
                    acc[rt][4 * g + 0] *= s4.x;
                    acc[rt][4 * g + 1] *= s4.y;
                    acc[rt][4 * g + 2] *= s4.z;
                    acc[rt][4 * g + 3] *= s4.w;
                }
            }
            const long lbase = t * BN + rt * 32;
            unsigned mask = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (lbase + acc_row(r, lane) < L && acc[rt][r] >= thr) mask |= 1u << r;
            const int c_me = __popc(mask), c_pt = __shfl_xor(c_me, 32, 64), need = c_me + c_pt;
            if (__any(fill + need > CAP)) compact(need);
            int off = bbase + fill + ((lane >> 5) ? c_pt : 0);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if ((mask >> r) & 1) {
                    bs[off] = acc[rt][r];
                    bn[off] = (int)(lbase + acc_row(r, lane));
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
        const long row = nblk + wave * 32 + qi;
        if (row < N && lane < k) {
            top_s[row * k + lane] = s;
            top_l[row * k + lane] = n;
        }
    }
}

template <typename T>
int label_launch(const void* Tl, const void* Vn, long L, long N, int k, float* top_s, int* top_l, hipStream_t st,
                 const float* l_scale = nullptr, const float* v_scale = nullptr) {
    static std::atomic<unsigned long long> lds_done{0};
    const hipError_t attr = ensure_dyn_lds((const void*)label_kernel<T>, label_lds<T>(), lds_done);
    if (attr != hipSuccess) return (int)attr;
    hipLaunchKernelGGL((label_kernel<T>), dim3(cdiv(N, BQ)), dim3(256), label_lds<T>(), st, (const T*)Tl, (const T*)Vn, L, N, k,
                       n_index_tiles(L), top_s, top_l, l_scale, v_scale);
    TAN_LAUNCH_CHECK();
    return 0;
}

// ---- cover search: videos ranked by the seconds they share with a SET of query rows, in any order (include/tan_hip.h) ----
// label_kernel's organisation with both reductions of the Chamfer similarity fused into the sweep: grid (video, set).  The workgroup
// walks its video in slabs of BQ = 128 rows -- a wave keeps 32 of them in registers as the B fragments; the tail columns of the last
// slab repeat the video's last row -- and the set's rows stream through LDS in 64-row tiles by tile_scores (rows past the set's end
// load as zero).  A lane's 32 accumulators of a tile belong to ONE video row, so
//   b_t  is a running max in registers over the tile rows that are the set's (a zero-filled tail row is not: 0 beats an all-negative
//        column), finished by one lane ^ 32 exchange per slab; the columns that are the video's go through fix() into a per-lane
//        64-bit sum (a repeated tail column does not), reduced once at the end;
//   a_i  needs, for each of the tile's 64 rows, the max over the wave's 32 columns (a repeated column changes no max): four DPP
//        steps inside a row of 16 lanes and one ds_swizzle across, per accumulator, on order-preserving integer keys (exact, like
//        the float maximum, and one instruction a step); the lane whose column equals the accumulator's
//        index keeps the result, and the wave writes its 64 maxima to its row of the [4][64] staging block.  After the NEXT tile's
//        first barrier (tile_scores' callback) thread r < 64 folds the four waves' values of row r into rowmax[m] -- the same thread
//        for a given row every time, so the fold needs no atomics -- and the stage is free again before any wave passes that tile's
//        second barrier, behind which the next stage writes lie (every format has at least two K chunks).
// rowmax starts at -inf; a tail row of the set's last tile is never folded.  After the last slab one pass sums fix(rowmax[i]); F and
// B are integer sums, so nothing depends on their order, and fwd / bwd leave by two plain stores.  e4m3: label_kernel's scale order
// (tile scale 1, the video row's scale as the column's, the set row's scale after the MFMA loop, two buffers by tile parity).
constexpr int COVER_MAX = 4096;
template <typename T> constexpr int cover_lds() {
    return (tile_bytes<T>() + 15) / 16 * 16 + COVER_MAX * 4 + 4 * BN * 4 + 8 * 8 + (sizeof(T) == 1 ? 2 * BN * 4 : 0);
}

// A float as an int32 whose SIGNED order is the float's (finite values and infinities; -0 sorts just below +0, and fix() sends both
// to 0), and back: the map is its own inverse.  The cross-lane maximum runs on these keys: v_max_i32 takes the DPP operand directly,
// where a float maximum of a lane-crossed value first pays a canonicalising v_max_f32.
__device__ __forceinline__ int order_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

template <int CTRL> __device__ __forceinline__ int dpp_max(int x) {
    const int y = __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, true);
    return x > y ? x : y;
}

// the maximum over the 32 lanes of the caller's half-wave, in every lane of it.  All 64 lanes must be active.
__device__ __forceinline__ int half_wave_max(int x) {
    x = dpp_max<0xB1>(x);                                          // quad_perm [1, 0, 3, 2]: lane ^ 1
    x = dpp_max<0x4E>(x);                                          // quad_perm [2, 3, 0, 1]: lane ^ 2
    x = dpp_max<0x141>(x);                                         // row_half_mirror: the other quad of the 8
    x = dpp_max<0x140>(x);                                         // row_mirror: the other 8 of the 16
    const int y = __builtin_amdgcn_ds_swizzle(x, 0x401F);          // bit mode, xor 16: the other row of the half-wave
    return x > y ? x : y;
}

__device__ __forceinline__ long long wave_sum_ll(long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// tan_cluster_accumulate's image of a value: the multiply by 2^30 is exact
__device__ __forceinline__ long long cover_fix(float x) { return __float2ll_rn(x * 0x1p30f); }

template <typename T>
__global__ void __launch_bounds__(256) cover_kernel(const T* __restrict__ Tq, const T* __restrict__ Vn, long Qt, long N,
                                                    const int* __restrict__ q_off, int n_set, const int* __restrict__ v_off,
                                                    int n_videos, const float* __restrict__ q_scale,
                                                    const float* __restrict__ v_scale, float* __restrict__ fwd,
                                                    float* __restrict__ bwd) {
#pragma clang fp contract(off)
    typedef Mma<T> M;
    typedef typename M::frag_t frag_t;
    constexpr int LD = RCfg<T>::LD, KS = M::KS, NCH = RC / RCfg<T>::KC, NFR = RC / KS;
    constexpr int TS = BN * LD;
    constexpr long ROWB = (long)RC * sizeof(T);
    constexpr bool F8 = sizeof(T) == 1;
    static_assert(NCH >= 2, "the stage is freed between a tile's first and second barrier");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* tile = reinterpret_cast<T*>(smem);
    float* sc = reinterpret_cast<float*>(smem + 2 * TS * sizeof(T));   // F8: tile_scores' tile scales, all 1 here
    float* rowmax = reinterpret_cast<float*>(smem + (tile_bytes<T>() + 15) / 16 * 16);
    float* stage = rowmax + COVER_MAX;                                // [4 waves][64 tile rows]
    long long* red = reinterpret_cast<long long*>(stage + 4 * BN);   // F of the four waves, then B
    float* qsc = reinterpret_cast<float*>(red + 8);                   // F8: the set rows' scales of two tiles

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31;
    const int v = blockIdx.x, p = blockIdx.y;                      // v < n_videos, p < n_set: the grid
    const long o = (long)p * n_videos + v;

    // the video's rows [lo, hi) and the set's rows [q0, q0 + m); every lookup is clamped
    long lo = v_off[v], hi = v_off[v + 1];
    lo = lo < 0 ? 0 : (lo > N ? N : lo);
    hi = hi < lo ? lo : (hi > N ? N : hi);
    const long V = hi - lo;
    long q0 = q_off[p];
    q0 = q0 < 0 ? 0 : (q0 >= Qt ? Qt - 1 : q0);
    long m_l = (long)q_off[p + 1] - q0;
    m_l = m_l > Qt - q0 ? Qt - q0 : m_l;
    const int m = m_l < 1 ? 1 : (m_l > COVER_MAX ? COVER_MAX : (int)m_l);
    if (V < 1) {                                                   // block-uniform; only under a broken v_off
        if (tid == 0) { fwd[o] = 0.0f; bwd[o] = 0.0f; }
        return;
    }
    const int n_t = (m + BN - 1) / BN;
    const long n_slab = (V + BQ - 1) / BQ;

    for (int i = tid; i < m; i += 256) rowmax[i] = -INFINITY;     // read after the second tile's first barrier at the earliest

    uint4 pre[4];
    float pqs = 0.0f;
    const float one = 1.0f;
    auto issue = [&](int t, int kc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, row = e >> 4, c16 = e & 15;
            const int l = t * BN + row;
            pre[i] = l < m ? *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(Tq) + (q0 + l) * ROWB + kc * 256 + c16 * 16)
                           : make_uint4(0, 0, 0, 0);
        }
        if constexpr (F8) {
            if (kc == 0 && tid < BN) {                             // the set rows' scales ride with the tile's first chunk
                const int l = t * BN + tid;
                pqs = l < m ? q_scale[q0 + l] : 0.0f;
            }
        }
    };

    int pend = -1;                                                 // the first set row of the tile whose stage awaits its fold
    auto fold = [&]() {
        if (pend >= 0 && tid < BN && pend + tid < m) {
            const float a = fmaxf(fmaxf(stage[tid], stage[BN + tid]), fmaxf(stage[2 * BN + tid], stage[3 * BN + tid]));
            rowmax[pend + tid] = fmaxf(rowmax[pend + tid], a);
        }
    };
    // the tile row whose maximum this lane keeps: accumulator (rt, r) = (col >> 4, col & 15) of its half-wave
    const int keep_row = 32 * (col >> 4) + acc_row(col & 15, lane);

    long long bsum = 0;                                            // the lane's share of B
    long g = 0;                                                    // tiles so far: the parity of the scale buffers
    issue(0, 0);
    for (long s = 0; s < n_slab; ++s) {
        const long cme = s * BQ + wave * 32 + col;
        const bool cok = cme < V;
        const long nrow = lo + (cok ? cme : V - 1);                // a tail column repeats the video's last row
        frag_t qf[NFR];                                            // the wave's 32 video rows, resident for the slab
        {
            const T* vrow = Vn + nrow * RC;
#pragma unroll
            for (int j = 0; j < NFR; ++j) qf[j] = QFrag<T>::load(vrow, j, lane);
        }
        float vs = 1.0f;
        if constexpr (F8) vs = v_scale[nrow];
        float bmax = -INFINITY;
        for (int t = 0; t < n_t; ++t, ++g) {
            if constexpr (F8) {
                // label_kernel's argument: read after this tile's barriers, written again behind the next tile's
                if (tid < BN) qsc[(g & 1) * BN + tid] = pqs;
            }
            f32x16 acc[2];
            tile_scores<T>(tile, sc, tid, lane, pre, one, qf, vs, acc, [&](int kc) {
                if (kc == 0) fold();
                if (kc + 1 < NCH) issue(t, kc + 1);
                else if (t + 1 < n_t) issue(t + 1, 0);
                else if (s + 1 < n_slab) issue(0, 0);
            });
            if constexpr (F8) {
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        const float4 s4 = *reinterpret_cast<const float4*>(qsc + (g & 1) * BN + rt * 32 + 8 * gq + 4 * (lane >> 5));
                        acc[rt][4 * gq + 0] *= s4.x;
                        acc[rt][4 * gq + 1] *= s4.y;
                        acc[rt][4 * gq + 2] *= s4.z;
                        acc[rt][4 * gq + 3] *= s4.w;
                    }
            }
            const int left = m - t * BN;                           // the tile's rows [0, left) are the set's
            if (left >= BN) {                                      // block-uniform
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) bmax = fmaxf(bmax, acc[rt][r]);
            } else {
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (rt * 32 + acc_row(r, lane) < left) bmax = fmaxf(bmax, acc[rt][r]);
            }
            int w = 0;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int a = half_wave_max(order_key(__float_as_int(acc[rt][r])));
                    w = col == rt * 16 + r ? a : w;
                }
            // behind this tile's last barrier; folded behind the next one
            stage[wave * BN + keep_row] = __int_as_float(order_key(w));
            pend = t * BN;
        }
        bmax = fmaxf(bmax, __shfl_xor(bmax, 32, 64));
        if (lane < 32 && cok) bsum += cover_fix(bmax);
    }
    __syncthreads();
    fold();
    __syncthreads();
    long long fsum = 0;
    for (int i = tid; i < m; i += 256) fsum += cover_fix(rowmax[i]);
    fsum = wave_sum_ll(fsum);
    bsum = wave_sum_ll(bsum);
    if (lane == 0) { red[wave] = fsum; red[4 + wave] = bsum; }
    __syncthreads();
    if (tid == 0) {
        const long long F = red[0] + red[1] + red[2] + red[3], B = red[4] + red[5] + red[6] + red[7];
        fwd[o] = __fdiv_rn(__ll2float_rn(F) * 0x1p-30f, (float)m);
        bwd[o] = __fdiv_rn(__ll2float_rn(B) * 0x1p-30f, (float)V);
    }
}

// one wave per set: lanes 0..31 carry the best so far, lanes 32..63 take the next 32 videos of score[p, :]; sort64v's order is the
// sweeps' (score descending, equal scores by ascending row v_off[v])
__global__ void __launch_bounds__(256) cover_select_kernel(const float* __restrict__ fwd, const float* __restrict__ bwd,
                                                           const int* __restrict__ v_off, long n_set, long n_videos, int rank, int k,
                                                           float* __restrict__ top_s, int* __restrict__ top_n, int* __restrict__ top_v) {
#pragma clang fp contract(off)
    const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= n_set) return;
    float s = -INFINITY;
    int n = SENT_ROW, v = -1;
    for (long c0 = 0; c0 < n_videos; c0 += 32) {
        if (lane >= 32) {
            const long c = c0 + lane - 32;
            s = -INFINITY;
            n = SENT_ROW;
            v = -1;
            if (c < n_videos) {
                const float f = fwd[p * n_videos + c], b = bwd[p * n_videos + c];
                s = rank == TAN_COVER_QUERY ? f : rank == TAN_COVER_VIDEO ? b : (f + b) * 0.5f;
                n = v_off[c];
                v = (int)c;
            }
        }
        sort64v(s, n, v, lane);
    }
    if (lane < k) {
        top_s[p * k + lane] = s;
        top_n[p * k + lane] = n;
        top_v[p * k + lane] = n != SENT_ROW ? v : -1;
    }
}

template <typename T>
int cover_launch(const void* Tq, const void* Vn, long Qt, long N, const int* q_off, long n_set, const int* v_off, long n_videos, int rank,
                 int k, float* fwd, float* bwd, float* top_s, int* top_n, int* top_v, hipStream_t st, const float* q_scale = nullptr,
                 const float* v_scale = nullptr) {
    static std::atomic<unsigned long long> lds_done{0};
    const hipError_t attr = ensure_dyn_lds((const void*)cover_kernel<T>, cover_lds<T>(), lds_done);
    if (attr != hipSuccess) return (int)attr;
    hipLaunchKernelGGL((cover_kernel<T>), dim3((unsigned)n_videos, (unsigned)n_set), dim3(256), cover_lds<T>(), st, (const T*)Tq,
                       (const T*)Vn, Qt, N, q_off, (int)n_set, v_off, (int)n_videos, q_scale, v_scale, fwd, bwd);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(cover_select_kernel, dim3(cdiv(n_set, 4)), dim3(256), 0, st, (const float*)fwd, (const float*)bwd, v_off, n_set,
                       n_videos, rank, k, top_s, top_n, top_v);
    TAN_LAUNCH_CHECK();
    return 0;
}

// ---- tan_label_runs: the rows' best labels -> label segments (include/tan_hip.h) ----
// lab[n] is the row's column-0 label (clamped into [0, L)) if its score is >= threshold, else -1.  A row STARTS a run if lab != -1
// and the row before it is in another video or has another lab, and ENDS one by the same rule on the row after it: every maximal
// run has one start and one end, and the i-th start belongs with the i-th end.  Six launches, all results order-independent:
//   1. flags : per row, its start / end flags (a byte) and the block's counts of each
//   2. scan  : one block per count array turns the block counts into first positions (filter_scan_kernel's loop) and stores the total
//   3. fill  : the i-th start / end row -> rs[i] / re[i]
//   4. keep  : per run, length >= min_len -> its position among the block's kept runs (or -1) and the block's count; the run's
//              length is added to label_rows[label] (integer atomics: order-independent)
//   5. scan  : the kept counts -> first positions; the total is n_runs[0]
//   6. emit  : 16 lanes per run fold its (score, row) by better() -- the largest score, its smallest row -- and lane 0 writes the
//              run at its kept position if that is below cap
// ws (int32 words, NB = ceil(N / 256)): rs [N] | re [N] | kpos [N] | counts 3 x [NB] | totals [4] | flags, N bytes
constexpr int RUN_LANES = 16;
inline long runs_ws_words(long N) { const long NB = (N + 255) / 256; return 3 * N + 3 * NB + 4 + (N + 3) / 4; }

struct RunsWs {
    int *rs, *re, *kpos, *cs, *ce, *ck, *tot;
    unsigned char* flags;
    __host__ __device__ RunsWs(int* w, long N) {
        const long NB = (N + 255) / 256;
        rs = w; re = rs + N; kpos = re + N; cs = kpos + N; ce = cs + NB; ck = ce + NB; tot = ck + NB;
        flags = reinterpret_cast<unsigned char*>(tot + 4);
    }
};

__device__ __forceinline__ int row_lab(const float* __restrict__ ts, const int* __restrict__ tl, int stride, long n, long L, float thr) {
    if (!(ts[n * stride] >= thr)) return -1;                       // NaN: background
    const long l = tl[n * stride];
    return (int)(l < 0 ? 0 : (l >= L ? L - 1 : l));
}

__global__ void __launch_bounds__(256) runs_flag_kernel(const float* __restrict__ ts, const int* __restrict__ tl, int stride, long N, long L,
                                                        const int* __restrict__ v_off, int n_videos, float thr, int* __restrict__ w) {
    const RunsWs ws(w, N);
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    bool st = false, en = false;
    if (n < N) {
        const int lab = row_lab(ts, tl, stride, n, L, thr);
        if (lab != -1) {
            // first(r): row r is the first row of its video -- one function of r, whatever v_off holds
            auto first = [&](long r) { return (long)v_off[video_search(v_off, r, 0, n_videos - 1)] == r; };
            st = n == 0 || row_lab(ts, tl, stride, n - 1, L, thr) != lab || first(n);
            en = n == N - 1 || row_lab(ts, tl, stride, n + 1, L, thr) != lab || first(n + 1);
        }
        ws.flags[n] = (unsigned char)((st ? 1 : 0) | (en ? 2 : 0));
    }
    const int c_st = __syncthreads_count(st), c_en = __syncthreads_count(en);
    if (threadIdx.x == 0) { ws.cs[blockIdx.x] = c_st; ws.ce[blockIdx.x] = c_en; }
}

// block b of the grid scans count array cnt + b * NB in place (exclusive) and stores its total in tot[b] and, if out, in out[0]
__global__ void __launch_bounds__(256) runs_scan_kernel(int* __restrict__ cnt, long NB, int* __restrict__ tot, int* __restrict__ out) {
    __shared__ int wsum[4];
    int* c = cnt + (long)blockIdx.x * NB;
    int carry = 0;
    for (long b0 = 0; b0 < NB; b0 += 256) {
        const long b = b0 + threadIdx.x;
        int total;
        const int ex = block_scan256(b < NB ? c[b] : 0, wsum, total);
        if (b < NB) c[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        tot[blockIdx.x] = carry;
        if (out) out[0] = carry;
    }
}

__global__ void __launch_bounds__(256) runs_fill_kernel(long N, int* __restrict__ w) {
    __shared__ int wsum[4];
    const RunsWs ws(w, N);
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    const int f = n < N ? ws.flags[n] : 0;
    int total;
    const long ps = (long)ws.cs[blockIdx.x] + block_scan256(f & 1, wsum, total);
    const long pe = (long)ws.ce[blockIdx.x] + block_scan256((f >> 1) & 1, wsum, total);
    if ((f & 1) && ps >= 0 && ps < N) ws.rs[ps] = (int)n;
    if ((f & 2) && pe >= 0 && pe < N) ws.re[pe] = (int)n;
}

__global__ void __launch_bounds__(256) runs_keep_kernel(const int* __restrict__ tl, int stride, long N, long L, int min_len,
                                                        int* __restrict__ label_rows, int* __restrict__ w) {
    __shared__ int wsum[4];
    const RunsWs ws(w, N);
    const long R = ws.tot[0] < ws.tot[1] ? ws.tot[0] : ws.tot[1];  // equal: one start and one end per run
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (i < R) {
        const long a = ws.rs[i], b = ws.re[i];
        if (a >= 0 && b >= a && b < N) {
            keep = b - a + 1 >= min_len;
            if (label_rows) {
                const long l = tl[a * stride];
                atomicAdd(&label_rows[l < 0 ? 0 : (l >= L ? L - 1 : l)], (int)(b - a + 1));
            }
        }
    }
    int total;
    const int local = block_scan256(keep ? 1 : 0, wsum, total);
    if (i < N) ws.kpos[i] = keep ? local : -1;
    if (threadIdx.x == 0) ws.ck[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) runs_emit_kernel(const float* __restrict__ ts, const int* __restrict__ tl, int stride, long N, long L,
                                                        const int* __restrict__ v_off, int n_videos, long cap, int* __restrict__ run_video,
                                                        int* __restrict__ run_start, int* __restrict__ run_end, int* __restrict__ run_label,
                                                        int* __restrict__ run_peak_row, float* __restrict__ run_peak_score,
                                                        int* __restrict__ w) {
    const RunsWs ws(w, N);
    const long R = ws.tot[0] < ws.tot[1] ? ws.tot[0] : ws.tot[1];
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) / RUN_LANES;
    const int sub = threadIdx.x % RUN_LANES;
    const int local = i < R ? ws.kpos[i] : -1;                     // the same for a run's 16 lanes
    const long p = local < 0 ? -1 : (long)ws.ck[i / 256] + local;
    const bool live = p >= 0 && p < cap;
    const long a = live ? ws.rs[i] : 0, b = live ? ws.re[i] : -1;  // kept: 0 <= a <= b < N
    float s = -INFINITY;
    int n = SENT_ROW;
    for (long r = a + sub; r <= b; r += RUN_LANES) {
        const float v = ts[r * stride];
        if (better(v, (int)r, s, n)) { s = v; n = (int)r; }
    }
#pragma unroll
    for (int o = RUN_LANES / 2; o > 0; o >>= 1) {
        const float os = __shfl_xor(s, o, 64);
        const int on = __shfl_xor(n, o, 64);
        if (better(os, on, s, n)) { s = os; n = on; }
    }
    if (live && sub == 0) {
        const long l = tl[a * stride];
        run_video[p] = video_search(v_off, a, 0, n_videos - 1);
        run_start[p] = (int)a;
        run_end[p] = (int)b;
        run_label[p] = (int)(l < 0 ? 0 : (l >= L ? L - 1 : l));
        run_peak_row[p] = n;
        run_peak_score[p] = s;
    }
}

}  // namespace
}  // namespace tal

using namespace tal;

// Every plain / _e4m3 pair of entry points shares ONE body, which takes the row format as `fmt`: the plain twin passes its `dtype`
// and no scales, the _e4m3 twin FMT_E4M3 and its scales.  rows_ok is the whole check of the format and the two row matrices;
// by_format calls `launch` with a Rows<T> naming the element type.
namespace {
constexpr int FMT_E4M3 = -1;                 // not a TAN_* dtype: a plain entry point handed it has no scales and is refused
template <typename T> struct Rows { typedef T type; };

inline bool rows_ok(int fmt, const void* Tq, const float* q_scale, const void* Vn, const float* v_scale) {
    return Tq && Vn && (uintptr_t)Tq % 16 == 0 && (uintptr_t)Vn % 16 == 0 &&
           (fmt == FMT_E4M3 ? q_scale && v_scale : fmt == TAN_F32 || fmt == TAN_BF16);
}

template <typename F> int by_format(int fmt, F launch) {
    return fmt == TAN_BF16 ? launch(Rows<bf16_t>()) : fmt == TAN_F32 ? launch(Rows<float>()) : launch(Rows<e4m3_t>());
}

}  // namespace

extern "C" long tan_rank_topk_ws_bytes(long Q, long N, int k) {
    if (Q < 1 || N < 1 || N >= (1L << 31) || k < 0 || k > KMAX) return TAN_ERR_BAD_ARG;
    return sweep_ws_head(false, Q, N) + max_splits(N) * Q * k * 8;
}

static int rank_topk(int fmt, const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q, long N, int C,
              const int* pair, int k, int splits, int* higher, int* ties, float* top_score, int* top_row, void* ws, void* stream) {
    TAN_REQUIRE(rows_ok(fmt, Tq, q_scale, Vn, v_scale) && ws && (uintptr_t)ws % 16 == 0);
    TAN_REQUIRE(C == RC && Q >= 1 && Q < (1L << 31) && N >= 1 && N < (1L << 31) && k >= 0 && k <= KMAX && k <= N);
    TAN_REQUIRE(splits >= 0 && (pair || k > 0));
    TAN_REQUIRE(!pair || (higher && ties));
    TAN_REQUIRE(k == 0 || (top_score && top_row));
    return by_format(fmt, [&](auto r) {
        return sweep_launch<typename decltype(r)::type, false, false>(Tq, Vn, Q, N, pair, nullptr, 0, k, splits, higher, ties, top_score,
                                                                      top_row, nullptr, ws, (hipStream_t)stream, q_scale, v_scale);
    });
}

extern "C" int tan_rank_topk(const void* Tq, const void* Vn, int dtype, long Q, long N, int C, const int* pair, int k, int splits,
                             int* higher, int* ties, float* top_score, int* top_row, void* ws, void* stream) {
    return rank_topk(dtype, Tq, nullptr, Vn, nullptr, Q, N, C, pair, k, splits, higher, ties, top_score, top_row, ws, stream);
}

extern "C" int tan_rank_topk_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q, long N, int C,
                                  const int* pair, int k, int splits, int* higher, int* ties, float* top_score, int* top_row, void* ws,
                                  void* stream) {
    return rank_topk(FMT_E4M3, Tq, q_scale, Vn, v_scale, Q, N, C, pair, k, splits, higher, ties, top_score, top_row, ws, stream);
}

extern "C" long tan_rank_topk_video_ws_bytes(long Q, long N, long n_videos, int k) {
    if (!video_sizes_ok(Q, N, RC, n_videos, k)) return TAN_ERR_BAD_ARG;
    return sweep_ws_head(true, Q, N) + max_splits(N) * Q * k * 12;
}

// FILTER = false: tan_rank_topk_video, filt is nullptr; true: tan_rank_topk_video_filtered
template <bool FILTER>
static int rank_topk_video(int fmt, const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q, long N, int C,
                    const int* v_off, long n_videos, const void* filt, int k, int splits, float* top_score, int* top_row,
                    int* top_video, void* ws, void* stream) {
    TAN_REQUIRE(rows_ok(fmt, Tq, q_scale, Vn, v_scale) && v_off && top_score && top_row && top_video && ws && (uintptr_t)ws % 16 == 0);
    TAN_REQUIRE(video_sizes_ok(Q, N, C, n_videos, k) && splits >= 0);
    TAN_REQUIRE(!FILTER || (filt && (uintptr_t)filt % 16 == 0));
    return by_format(fmt, [&](auto r) {
        return sweep_launch<typename decltype(r)::type, true, FILTER>(Tq, Vn, Q, N, (const int*)filt, v_off, (int)n_videos, k, splits,
                                                                      nullptr, nullptr, top_score, top_row, top_video, ws,
                                                                      (hipStream_t)stream, q_scale, v_scale);
    });
}

extern "C" int tan_rank_topk_video(const void* Tq, const void* Vn, int dtype, long Q, long N, int C, const int* v_off, long n_videos,
                                   int k, int splits, float* top_score, int* top_row, int* top_video, void* ws, void* stream) {
    return rank_topk_video<false>(dtype, Tq, nullptr, Vn, nullptr, Q, N, C, v_off, n_videos, nullptr, k, splits, top_score, top_row,
                                  top_video, ws, stream);
}

extern "C" int tan_rank_topk_video_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q, long N, int C,
                                        const int* v_off, long n_videos, int k, int splits, float* top_score, int* top_row,
                                        int* top_video, void* ws, void* stream) {
    return rank_topk_video<false>(FMT_E4M3, Tq, q_scale, Vn, v_scale, Q, N, C, v_off, n_videos, nullptr, k, splits, top_score, top_row,
                                  top_video, ws, stream);
}

extern "C" long tan_row_filter_bytes(long N) {
    if (N < 1 || N >= (1L << 31)) return TAN_ERR_BAD_ARG;
    return (filt_words(n_index_tiles(N)) * 4 + 15) / 16 * 16;
}

extern "C" int tan_row_filter_build(const int* spans, long n_spans, long N, void* filt, void* stream) {
    TAN_REQUIRE(spans && filt && n_spans >= 1 && n_spans < (1L << 30) && N >= 1 && N < (1L << 31));
    TAN_REQUIRE((uintptr_t)filt % 16 == 0);
    hipStream_t st = (hipStream_t)stream;
    const long T = n_index_tiles(N);
    hipLaunchKernelGGL(filter_mask_kernel, dim3(cdiv(T, 256)), dim3(256), 0, st, spans, n_spans, N, T, (int*)filt);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(256), 0, st, T, (int*)filt);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(filter_fill_kernel, dim3(cdiv(T, 256)), dim3(256), 0, st, T, (int*)filt);
    TAN_LAUNCH_CHECK();
    return 0;
}

static int rank_topk_filtered(int fmt, const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q, long N, int C,
                       const void* filt, int k, int splits, float* top_score, int* top_row, void* ws, void* stream) {
    TAN_REQUIRE(rows_ok(fmt, Tq, q_scale, Vn, v_scale) && filt && top_score && top_row && ws);
    TAN_REQUIRE(C == RC && Q >= 1 && Q < (1L << 31) && N >= 1 && N < (1L << 31) && k >= 1 && k <= KMAX && k <= N && splits >= 0);
    TAN_REQUIRE((uintptr_t)ws % 16 == 0 && (uintptr_t)filt % 16 == 0);
    return by_format(fmt, [&](auto r) {
        return sweep_launch<typename decltype(r)::type, false, true>(Tq, Vn, Q, N, (const int*)filt, nullptr, 0, k, splits, nullptr,
                                                                     nullptr, top_score, top_row, nullptr, ws, (hipStream_t)stream,
                                                                     q_scale, v_scale);
    });
}

extern "C" int tan_rank_topk_filtered(const void* Tq, const void* Vn, int dtype, long Q, long N, int C, const void* filt, int k,
                                      int splits, float* top_score, int* top_row, void* ws, void* stream) {
    return rank_topk_filtered(dtype, Tq, nullptr, Vn, nullptr, Q, N, C, filt, k, splits, top_score, top_row, ws, stream);
}

extern "C" int tan_rank_topk_filtered_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q, long N,
                                           int C, const void* filt, int k, int splits, float* top_score, int* top_row, void* ws,
                                           void* stream) {
    return rank_topk_filtered(FMT_E4M3, Tq, q_scale, Vn, v_scale, Q, N, C, filt, k, splits, top_score, top_row, ws, stream);
}

extern "C" int tan_rank_topk_video_filtered(const void* Tq, const void* Vn, int dtype, long Q, long N, int C, const int* v_off,
                                            long n_videos, const void* filt, int k, int splits, float* top_score, int* top_row,
                                            int* top_video, void* ws, void* stream) {
    return rank_topk_video<true>(dtype, Tq, nullptr, Vn, nullptr, Q, N, C, v_off, n_videos, filt, k, splits, top_score, top_row,
                                 top_video, ws, stream);
}

extern "C" int tan_rank_topk_video_filtered_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q,
                                                 long N, int C, const int* v_off, long n_videos, const void* filt, int k, int splits,
                                                 float* top_score, int* top_row, int* top_video, void* ws, void* stream) {
    return rank_topk_video<true>(FMT_E4M3, Tq, q_scale, Vn, v_scale, Q, N, C, v_off, n_videos, filt, k, splits, top_score, top_row,
                                 top_video, ws, stream);
}

static int moment_extent(int fmt, const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q, long N, int C,
                  const int* v_off, long n_videos, int k, const float* top_score, const int* top_row, const int* top_video, float width,
                  int* start, int* end, void* stream) {
    TAN_REQUIRE(rows_ok(fmt, Tq, q_scale, Vn, v_scale) && v_off && top_score && top_row && top_video && start && end);
    TAN_REQUIRE(video_sizes_ok(Q, N, C, n_videos, k) && width >= 0.0f);
    return by_format(fmt, [&](auto r) {
        return extent_launch<typename decltype(r)::type>(Tq, Vn, Q, N, v_off, (int)n_videos, k, top_score, top_row, top_video, width,
                                                         start, end, (hipStream_t)stream, q_scale, v_scale);
    });
}

extern "C" int tan_moment_extent(const void* Tq, const void* Vn, int dtype, long Q, long N, int C, const int* v_off, long n_videos, int k,
                                 const float* top_score, const int* top_row, const int* top_video, float width, int* start, int* end,
                                 void* stream) {
    return moment_extent(dtype, Tq, nullptr, Vn, nullptr, Q, N, C, v_off, n_videos, k, top_score, top_row, top_video, width, start, end,
                         stream);
}

extern "C" int tan_moment_extent_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q, long N, int C,
                                      const int* v_off, long n_videos, int k, const float* top_score, const int* top_row,
                                      const int* top_video, float width, int* start, int* end, void* stream) {
    return moment_extent(FMT_E4M3, Tq, q_scale, Vn, v_scale, Q, N, C, v_off, n_videos, k, top_score, top_row, top_video, width, start,
                         end, stream);
}

extern "C" long tan_sequence_topk_ws_bytes(long n_seq, long N, int k) {
    if (n_seq < 1 || n_seq >= (1L << 29) || N < 1 || N >= (1L << 31) || k < 1 || k > KMAX) return TAN_ERR_BAD_ARG;
    return max_splits(N) * n_seq * k * 8;
}

static int sequence_topk(int fmt, const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                  const int* s_off, long n_seq, const int* v_off, long n_videos, int k, int splits, float* top_score, int* top_video,
                  void* ws, void* stream) {
    TAN_REQUIRE(rows_ok(fmt, Tq, q_scale, Vn, v_scale) && s_off && v_off && top_score && top_video && ws && (uintptr_t)ws % 16 == 0);
    TAN_REQUIRE(seq_sizes_ok(Qt, N, C, n_seq, n_videos) && k >= 1 && k <= KMAX && k <= n_videos && splits >= 0);
    return by_format(fmt, [&](auto r) {
        return seq_topk_launch<typename decltype(r)::type>(Tq, Vn, Qt, N, s_off, n_seq, v_off, (int)n_videos, k, splits, top_score,
                                                           top_video, ws, (hipStream_t)stream, q_scale, v_scale);
    });
}

extern "C" int tan_sequence_topk(const void* Tq, const void* Vn, int dtype, long Qt, long N, int C, const int* s_off, long n_seq,
                                 const int* v_off, long n_videos, int k, int splits, float* top_score, int* top_video, void* ws,
                                 void* stream) {
    return sequence_topk(dtype, Tq, nullptr, Vn, nullptr, Qt, N, C, s_off, n_seq, v_off, n_videos, k, splits, top_score, top_video, ws,
                         stream);
}

extern "C" int tan_sequence_topk_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                                      const int* s_off, long n_seq, const int* v_off, long n_videos, int k, int splits,
                                      float* top_score, int* top_video, void* ws, void* stream) {
    return sequence_topk(FMT_E4M3, Tq, q_scale, Vn, v_scale, Qt, N, C, s_off, n_seq, v_off, n_videos, k, splits, top_score, top_video,
                         ws, stream);
}

static int sequence_scores(int fmt, const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                    const int* s_off, long n_seq, const int* v_off, long n_videos, const int* hits, const long* x_off, long P, float* x,
                    long n_x, void* stream) {
    TAN_REQUIRE(rows_ok(fmt, Tq, q_scale, Vn, v_scale) && s_off && v_off && hits && x_off && x && (uintptr_t)x_off % 8 == 0);
    TAN_REQUIRE(seq_sizes_ok(Qt, N, C, n_seq, n_videos) && P >= 1 && P < (1L << 31) && n_x >= 1);
    return by_format(fmt, [&](auto r) {
        return seq_scores_launch<typename decltype(r)::type>(Tq, Vn, Qt, N, s_off, n_seq, v_off, (int)n_videos, hits, x_off, P, x, n_x,
                                                             (hipStream_t)stream, q_scale, v_scale);
    });
}

extern "C" int tan_sequence_scores(const void* Tq, const void* Vn, int dtype, long Qt, long N, int C, const int* s_off, long n_seq,
                                   const int* v_off, long n_videos, const int* hits, const long* x_off, long P, float* x, long n_x,
                                   void* stream) {
    return sequence_scores(dtype, Tq, nullptr, Vn, nullptr, Qt, N, C, s_off, n_seq, v_off, n_videos, hits, x_off, P, x, n_x, stream);
}

extern "C" int tan_sequence_scores_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N,
                                        int C, const int* s_off, long n_seq, const int* v_off, long n_videos, const int* hits,
                                        const long* x_off, long P, float* x, long n_x, void* stream) {
    return sequence_scores(FMT_E4M3, Tq, q_scale, Vn, v_scale, Qt, N, C, s_off, n_seq, v_off, n_videos, hits, x_off, P, x, n_x, stream);
}

extern "C" long tan_clip_topk_ws_bytes(long n_clip, long N, int k) {
    if (n_clip < 1 || n_clip >= (1L << 29) || N < 1 || N >= (1L << 31) || k < 1 || k > KMAX) return TAN_ERR_BAD_ARG;
    return max_splits(N) * n_clip * k * 12;
}

static int clip_topk(int fmt, const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
              const int* c_off, long n_clip, const int* v_off, long n_videos, int k, int splits, float* top_score, int* top_row,
              int* top_video, void* ws, void* stream) {
    TAN_REQUIRE(rows_ok(fmt, Tq, q_scale, Vn, v_scale) && c_off && v_off && top_score && top_row && top_video && ws &&
                (uintptr_t)ws % 16 == 0);
    TAN_REQUIRE(seq_sizes_ok(Qt, N, C, n_clip, n_videos) && k >= 1 && k <= KMAX && k <= n_videos && splits >= 0);
    return by_format(fmt, [&](auto r) {
        return clip_topk_launch<typename decltype(r)::type>(Tq, Vn, Qt, N, c_off, n_clip, v_off, (int)n_videos, k, splits, top_score,
                                                            top_row, top_video, ws, (hipStream_t)stream, q_scale, v_scale);
    });
}

extern "C" int tan_clip_topk(const void* Tq, const void* Vn, int dtype, long Qt, long N, int C, const int* c_off, long n_clip,
                             const int* v_off, long n_videos, int k, int splits, float* top_score, int* top_row, int* top_video,
                             void* ws, void* stream) {
    return clip_topk(dtype, Tq, nullptr, Vn, nullptr, Qt, N, C, c_off, n_clip, v_off, n_videos, k, splits, top_score, top_row, top_video,
                     ws, stream);
}

extern "C" int tan_clip_topk_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                                  const int* c_off, long n_clip, const int* v_off, long n_videos, int k, int splits, float* top_score,
                                  int* top_row, int* top_video, void* ws, void* stream) {
    return clip_topk(FMT_E4M3, Tq, q_scale, Vn, v_scale, Qt, N, C, c_off, n_clip, v_off, n_videos, k, splits, top_score, top_row,
                     top_video, ws, stream);
}

extern "C" long tan_compound_topk_ws_bytes(long n_query, long N, int k) {
    if (n_query < 1 || n_query >= (1L << 29) || N < 1 || N >= (1L << 31) || k < 1 || k > KMAX) return TAN_ERR_BAD_ARG;
    return max_splits(N) * n_query * k * 8;
}

static int compound_topk(int fmt, const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                  const int* t_off, const int* role, long n_query, const int* v_off, long n_videos, float veto, int k, int splits,
                  float* top_score, int* top_video, void* ws, void* stream) {
    TAN_REQUIRE(rows_ok(fmt, Tq, q_scale, Vn, v_scale) && t_off && role && v_off && top_score && top_video && ws &&
                (uintptr_t)ws % 16 == 0);
    TAN_REQUIRE(seq_sizes_ok(Qt, N, C, n_query, n_videos) && k >= 1 && k <= KMAX && k <= n_videos && splits >= 0 && veto == veto);
    return by_format(fmt, [&](auto r) {
        return compound_topk_launch<typename decltype(r)::type>(Tq, Vn, Qt, N, t_off, role, n_query, v_off, (int)n_videos, veto, k, splits,
                                                                top_score, top_video, ws, (hipStream_t)stream, q_scale, v_scale);
    });
}

extern "C" int tan_compound_topk(const void* Tq, const void* Vn, int dtype, long Qt, long N, int C, const int* t_off, const int* role,
                                 long n_query, const int* v_off, long n_videos, float veto, int k, int splits, float* top_score,
                                 int* top_video, void* ws, void* stream) {
    return compound_topk(dtype, Tq, nullptr, Vn, nullptr, Qt, N, C, t_off, role, n_query, v_off, n_videos, veto, k, splits, top_score,
                         top_video, ws, stream);
}

extern "C" int tan_compound_topk_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                                      const int* t_off, const int* role, long n_query, const int* v_off, long n_videos, float veto,
                                      int k, int splits, float* top_score, int* top_video, void* ws, void* stream) {
    return compound_topk(FMT_E4M3, Tq, q_scale, Vn, v_scale, Qt, N, C, t_off, role, n_query, v_off, n_videos, veto, k, splits, top_score,
                         top_video, ws, stream);
}

static int compound_peaks(int fmt, const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                   const int* t_off, long n_query, const int* v_off, long n_videos, const int* hits, long n_hits, float* peak_score,
                   int* peak_row, void* stream) {
    TAN_REQUIRE(rows_ok(fmt, Tq, q_scale, Vn, v_scale) && t_off && v_off && hits && peak_score && peak_row);
    TAN_REQUIRE(seq_sizes_ok(Qt, N, C, n_query, n_videos) && n_hits >= 1 && n_hits < (1L << 26));
    return by_format(fmt, [&](auto r) {
        return compound_peaks_launch<typename decltype(r)::type>(Tq, Vn, Qt, N, t_off, n_query, v_off, (int)n_videos, hits, n_hits,
                                                                 peak_score, peak_row, (hipStream_t)stream, q_scale, v_scale);
    });
}

extern "C" int tan_compound_peaks(const void* Tq, const void* Vn, int dtype, long Qt, long N, int C, const int* t_off, long n_query,
                                  const int* v_off, long n_videos, const int* hits, long n_hits, float* peak_score, int* peak_row,
                                  void* stream) {
    return compound_peaks(dtype, Tq, nullptr, Vn, nullptr, Qt, N, C, t_off, n_query, v_off, n_videos, hits, n_hits, peak_score, peak_row,
                          stream);
}

extern "C" int tan_compound_peaks_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                                       const int* t_off, long n_query, const int* v_off, long n_videos, const int* hits, long n_hits,
                                       float* peak_score, int* peak_row, void* stream) {
    return compound_peaks(FMT_E4M3, Tq, q_scale, Vn, v_scale, Qt, N, C, t_off, n_query, v_off, n_videos, hits, n_hits, peak_score,
                          peak_row, stream);
}

extern "C" int tan_cover_max_rows(void) { return COVER_MAX; }

static int cover_topk(int fmt, const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
               const int* q_off, long n_set, const int* v_off, long n_videos, int rank, int k, float* fwd, float* bwd,
               float* top_score, int* top_row, int* top_video, void* stream) {
    TAN_REQUIRE(rows_ok(fmt, Tq, q_scale, Vn, v_scale) && q_off && v_off && fwd && bwd && top_score && top_row && top_video);
    TAN_REQUIRE(C == RC && N >= 1 && N < (1L << 31) && n_set >= 1 && n_set <= 65535 && Qt >= n_set && Qt <= COVER_MAX * n_set &&
                n_videos >= 1 && n_videos <= N && k >= 1 && k <= KMAX && k <= n_videos);
    TAN_REQUIRE(rank == TAN_COVER_QUERY || rank == TAN_COVER_VIDEO || rank == TAN_COVER_BOTH);
    return by_format(fmt, [&](auto r) {
        return cover_launch<typename decltype(r)::type>(Tq, Vn, Qt, N, q_off, n_set, v_off, n_videos, rank, k, fwd, bwd, top_score,
                                                        top_row, top_video, (hipStream_t)stream, q_scale, v_scale);
    });
}

extern "C" int tan_cover_topk(const void* Tq, const void* Vn, int dtype, long Qt, long N, int C, const int* q_off, long n_set,
                              const int* v_off, long n_videos, int rank, int k, float* fwd, float* bwd, float* top_score, int* top_row,
                              int* top_video, void* stream) {
    return cover_topk(dtype, Tq, nullptr, Vn, nullptr, Qt, N, C, q_off, n_set, v_off, n_videos, rank, k, fwd, bwd, top_score, top_row,
                      top_video, stream);
}

extern "C" int tan_cover_topk_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                                   const int* q_off, long n_set, const int* v_off, long n_videos, int rank, int k, float* fwd,
                                   float* bwd, float* top_score, int* top_row, int* top_video, void* stream) {
    return cover_topk(FMT_E4M3, Tq, q_scale, Vn, v_scale, Qt, N, C, q_off, n_set, v_off, n_videos, rank, k, fwd, bwd, top_score,
                      top_row, top_video, stream);
}

static int label_topk(int fmt, const void* Tl, const float* l_scale, const void* Vn, const float* v_scale, long L, long N, int C, int k,
               float* top_score, int* top_label, void* stream) {
    TAN_REQUIRE(rows_ok(fmt, Tl, l_scale, Vn, v_scale) && top_score && top_label);
    TAN_REQUIRE(C == RC && L >= 1 && L < (1L << 31) && N >= 1 && N < (1L << 31) && k >= 1 && k <= KMAX && k <= L);
    return by_format(fmt, [&](auto r) {
        return label_launch<typename decltype(r)::type>(Tl, Vn, L, N, k, top_score, top_label, (hipStream_t)stream, l_scale, v_scale);
    });
}

extern "C" int tan_label_topk(const void* Tl, const void* Vn, int dtype, long L, long N, int C, int k, float* top_score, int* top_label,
                              void* stream) {
    return label_topk(dtype, Tl, nullptr, Vn, nullptr, L, N, C, k, top_score, top_label, stream);
}

extern "C" int tan_label_topk_e4m3(const void* Tl, const float* l_scale, const void* Vn, const float* v_scale, long L, long N, int C,
                                   int k, float* top_score, int* top_label, void* stream) {
    return label_topk(FMT_E4M3, Tl, l_scale, Vn, v_scale, L, N, C, k, top_score, top_label, stream);
}

extern "C" long tan_label_runs_ws_bytes(long N) {
    if (N < 1 || N >= (1L << 31)) return TAN_ERR_BAD_ARG;
    return (runs_ws_words(N) * 4 + 15) / 16 * 16;
}

extern "C" int tan_label_runs(const float* top_score, const int* top_label, int stride, long N, long L, const int* v_off, long n_videos,
                              float threshold, int min_len, long cap, int* n_runs, int* run_video, int* run_start, int* run_end,
                              int* run_label, int* run_peak_row, float* run_peak_score, int* label_rows, void* ws, void* stream) {
    TAN_REQUIRE(top_score && top_label && v_off && n_runs && run_video && run_start && run_end && run_label && run_peak_row &&
                run_peak_score && ws);
    TAN_REQUIRE(stride >= 1 && N >= 1 && N < (1L << 31) && L >= 1 && L < (1L << 31) && n_videos >= 1 && n_videos <= N);
    TAN_REQUIRE(threshold == threshold && min_len >= 1 && cap >= 0 && (uintptr_t)ws % 4 == 0);
    hipStream_t st = (hipStream_t)stream;
    int* w = (int*)ws;
    const RunsWs lay(w, N);
    const long NB = (N + 255) / 256;
    if (label_rows) {
        const hipError_t e = hipMemsetAsync(label_rows, 0, (size_t)L * 4, st);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(runs_flag_kernel, dim3((unsigned)NB), dim3(256), 0, st, top_score, top_label, stride, N, L, v_off, (int)n_videos,
                       threshold, w);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(runs_scan_kernel, dim3(2), dim3(256), 0, st, lay.cs, NB, lay.tot, (int*)nullptr);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(runs_fill_kernel, dim3((unsigned)NB), dim3(256), 0, st, N, w);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(runs_keep_kernel, dim3((unsigned)NB), dim3(256), 0, st, top_label, stride, N, L, min_len, label_rows, w);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(runs_scan_kernel, dim3(1), dim3(256), 0, st, lay.ck, NB, lay.tot + 2, n_runs);
    TAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(runs_emit_kernel, dim3(cdiv(N * RUN_LANES, 256)), dim3(256), 0, st, top_score, top_label, stride, N, L, v_off,
                       (int)n_videos, cap, run_video, run_start, run_end, run_label, run_peak_row, run_peak_score, w);
    TAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int tan_quantize_rows_e4m3(const void* x, int dtype, long n_rows, int C, void* codes, float* scale, void* stream) {
    TAN_REQUIRE(x && codes && scale && (dtype == TAN_F32 || dtype == TAN_BF16));
    TAN_REQUIRE(C == RC && n_rows >= 1 && n_rows < (1L << 31) && (uintptr_t)x % 16 == 0 && (uintptr_t)codes % 8 == 0);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TAN_BF16)
        hipLaunchKernelGGL(quantize_rows_kernel<bf16_t>, dim3(cdiv(n_rows, 4)), dim3(256), 0, st, (const bf16_t*)x, n_rows, (uint2*)codes,
                           scale);
    else
        hipLaunchKernelGGL(quantize_rows_kernel<float>, dim3(cdiv(n_rows, 4)), dim3(256), 0, st, (const float*)x, n_rows, (uint2*)codes,
                           scale);
    TAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int tan_segment_pool_acc(const void* stage, int dtype, long win_stride, int T, const int* table, int W, int normalize,
                                    float* sum, float* cnt, int n_clips, void* stream) {
    TAN_REQUIRE(stage && table && sum && cnt && (dtype == TAN_F32 || dtype == TAN_BF16));
    TAN_REQUIRE(W > 0 && T > 0 && n_clips > 0 && win_stride >= (long)T * RC && win_stride % 8 == 0 && (uintptr_t)stage % 16 == 0);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TAN_BF16)
        hipLaunchKernelGGL(segment_pool_acc_kernel<bf16_t>, dim3(W), dim3(256), 0, st, (const bf16_t*)stage, win_stride, T, table, W,
                           normalize, sum, cnt, n_clips);
    else
        hipLaunchKernelGGL(segment_pool_acc_kernel<float>, dim3(W), dim3(256), 0, st, (const float*)stage, win_stride, T, table, W,
                           normalize, sum, cnt, n_clips);
    TAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int tan_segment_pool_final(const float* sum, const float* cnt, int n_clips, int normalize, float* out, void* stream) {
    TAN_REQUIRE(sum && cnt && out && n_clips > 0);
    hipLaunchKernelGGL(segment_pool_final_kernel, dim3(cdiv(n_clips, 4)), dim3(256), 0, (hipStream_t)stream, sum, cnt, n_clips, normalize,
                       out);
    TAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int tan_window_feat_acc(const void* feat, int dtype, long win_stride, const int* table, int W, int T, float* acc, float* cnt,
                                   long n_rows, void* stream) {
    TAN_REQUIRE(feat && table && acc && cnt && (dtype == TAN_F32 || dtype == TAN_BF16));
    TAN_REQUIRE(W > 0 && T > 0 && n_rows > 0 && win_stride >= (long)T * RC && win_stride % 8 == 0 && (uintptr_t)feat % 16 == 0);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TAN_BF16)
        hipLaunchKernelGGL(window_feat_acc_kernel<bf16_t>, dim3(W), dim3(256), 0, st, (const bf16_t*)feat, win_stride, table, W, T, acc, cnt,
                           n_rows);
    else
        hipLaunchKernelGGL(window_feat_acc_kernel<float>, dim3(W), dim3(256), 0, st, (const float*)feat, win_stride, table, W, T, acc, cnt,
                           n_rows);
    TAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int tan_window_feat_final(const float* acc, const float* cnt, long n_rows, void* out, int out_dtype, void* stream) {
    TAN_REQUIRE(acc && cnt && out && n_rows > 0 && (out_dtype == TAN_F32 || out_dtype == TAN_BF16));
    hipStream_t st = (hipStream_t)stream;
    if (out_dtype == TAN_BF16)
        hipLaunchKernelGGL(window_feat_final_kernel<bf16_t>, dim3(cdiv(n_rows, 4)), dim3(256), 0, st, acc, cnt, n_rows, (bf16_t*)out);
    else
        hipLaunchKernelGGL(window_feat_final_kernel<float>, dim3(cdiv(n_rows, 4)), dim3(256), 0, st, acc, cnt, n_rows, (float*)out);
    TAN_LAUNCH_CHECK();
    return 0;
}
