"""tan_cover_topk's definition (include/tan_hip.h) in numpy, operation by operation: the reference test_cover_gpu.py compares the
kernel with, pinned against a brute force over Python Fractions by test_cover_cpu.py.

A score block is either
  * float32: the device's own bits (tan_sequence_scores), or
  * int64 with a power-of-two `mult`: exact scores X / mult (the exact-arithmetic cases: X * 2^30 / mult is an integer, so fix() is
    that integer and nothing is rounded before the sums).
Per (set, video) block x [m, V]:
    a_i = max_t x[i, t]      b_t = max_i x[i, t]
    F = sum_i fix(a_i)       B = sum_t fix(b_t)        fix(x) = round-half-even(x * 2^30) as int64
    fwd = (f32(F) * 2^-30) / f32(m)                     int64 -> f32 to nearest even, an exact scaling, ONE f32 division
    bwd = (f32(B) * 2^-30) / f32(V)
and score = fwd ("query"), bwd ("video") or (fwd + bwd) * 0.5 ("both": one f32 add, an exact halving)."""
import numpy as np

RANKS = ("query", "video", "both")
EMPTY_ROW = 0x7fffffff
SHIFT = 30


def fix(x, mult=None):
    """int64 image of scores: float32 x -> rint(x * 2^30) (the product is exact in f32, the rounding is to nearest even); int64 x with
    `mult` (a power of two <= 2^30) -> x * (2^30 / mult) exactly"""
    x = np.asarray(x)
    if mult is None:
        assert x.dtype == np.float32
        y = x * np.float32(2.0 ** SHIFT)                            # a power of two: exact
        return np.rint(y.astype(np.float64)).astype(np.int64)       # f32 -> f64 is exact; rint rounds half to even
    m = int(mult)
    assert x.dtype == np.int64 and m == mult and m & (m - 1) == 0 and m <= 1 << SHIFT
    return x * ((1 << SHIFT) // m)


def mean_of_sum(total, n):
    """(f32(total) * 2^-30) / f32(n) with total an int64 (or Python int below 2^63)"""
    f = np.int64(total).astype(np.float32)                          # int64 -> f32: to nearest even
    f = f * np.float32(2.0 ** -SHIFT)                               # exact
    return f / np.float32(n)                                        # one f32 division


def block(x, mult=None):
    """(fwd, bwd) float32 of ONE [m, V] block"""
    x = np.asarray(x)
    m, V = x.shape
    F = int(fix(x.max(axis=1), mult).sum())
    B = int(fix(x.max(axis=0), mult).sum())
    return mean_of_sum(F, m), mean_of_sum(B, V)


def cover(X, q_off, v_off, mult=None):
    """X [Qt, N] -> (fwd, bwd) float32 [n_set, n_videos]"""
    ns, nv = len(q_off) - 1, len(v_off) - 1
    fwd, bwd = np.empty((ns, nv), dtype=np.float32), np.empty((ns, nv), dtype=np.float32)
    for p in range(ns):
        for v in range(nv):
            fwd[p, v], bwd[p, v] = block(X[q_off[p]:q_off[p + 1], v_off[v]:v_off[v + 1]], mult)
    return fwd, bwd


def score(fwd, bwd, rank):
    assert rank in RANKS and fwd.dtype == bwd.dtype == np.float32
    if rank == "query":
        return fwd
    if rank == "video":
        return bwd
    return (fwd + bwd) * np.float32(0.5)


def topk(s, v_off, k):
    """s [n_set, n_videos] float32 -> (top_score f32, top_row int32, top_video int32) [n_set, k]: by descending score, equal scores by
    ascending first row of the video"""
    rows = np.asarray(v_off[:-1], dtype=np.int64)
    ns = s.shape[0]
    top_s, top_r, top_v = np.empty((ns, k), np.float32), np.empty((ns, k), np.int32), np.empty((ns, k), np.int32)
    for p in range(ns):
        order = sorted(range(s.shape[1]), key=lambda v: (-float(s[p, v]), int(rows[v])))[:k]
        top_s[p], top_r[p], top_v[p] = s[p, order], rows[order], order
    return top_s, top_r, top_v
