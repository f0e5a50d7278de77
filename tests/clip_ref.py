"""A numpy restatement of the clip match of include/tan_hip.h (tan_clip_topk), shared by test_clips_cpu.py (which pins it against a
loop over Python ints) and test_clips_gpu.py.

    S(t) = (((x_0[t] + x_1[t + 1]) + x_2[t + 2]) + ...) + x_{m-1}[t + m - 1]      for 0 <= t <= V - m
    match = max_t S(t);   start = the smallest t attaining it;   a video with V < m has neither

Every add is done in x's own dtype, one per term in ascending i (float32: one rounded add per cell, as the kernel; int64 /
float64: a reference)."""
import numpy as np

EMPTY_ROW = 0x7fffffff


def diag_sums(x):
    """x [m, V] -> S [V - m + 1] in x's dtype; empty for V < m"""
    x = np.asarray(x)
    m, V = x.shape
    assert m >= 1
    n = V - m + 1
    if n <= 0:
        return np.empty(0, dtype=x.dtype)
    S = x[0, :n].copy()
    for i in range(1, m):
        S = (S + x[i, i:i + n]).astype(x.dtype)
    return S


def match_and_start(x):
    """x [m, V] -> (match: a scalar of x's dtype, start: int), or None for V < m"""
    S = diag_sums(x)
    if S.size == 0:
        return None
    t = int(np.argmax(S))                                           # the first maximum
    return S[t], t


def matches(X, c_off, v_off):
    """X [Qt, N] scores -> (match [n_clip, n_videos] in X's dtype, start [n_clip, n_videos] int64, -1 where V < m; match is 0 there)"""
    X = np.asarray(X)
    n_clip, nv = len(c_off) - 1, len(v_off) - 1
    match = np.zeros((n_clip, nv), dtype=X.dtype)
    start = np.full((n_clip, nv), -1, dtype=np.int64)
    for p in range(n_clip):
        for v in range(nv):
            got = match_and_start(X[c_off[p]:c_off[p + 1], v_off[v]:v_off[v + 1]])
            if got is not None:
                match[p, v], start[p, v] = got
    return match, start


def topk(match, start, v_off, k):
    """-> (score [n_clip, k] float64, row [n_clip, k] int64, video [n_clip, k] int64): per clip the k eligible videos (start >= 0)
    by descending match, equal matches by ascending row = v_off[v] + start; the slots that are left are (-inf, 0x7fffffff, -1)"""
    n_clip, nv = match.shape
    score = np.full((n_clip, k), -np.inf, dtype=np.float64)
    row = np.full((n_clip, k), EMPTY_ROW, dtype=np.int64)
    video = np.full((n_clip, k), -1, dtype=np.int64)
    for p in range(n_clip):
        order = sorted((v for v in range(nv) if start[p, v] >= 0), key=lambda v: (-match[p, v], int(v_off[v]) + int(start[p, v])))[:k]
        for j, v in enumerate(order):
            score[p, j], row[p, j], video[p, j] = match[p, v], int(v_off[v]) + int(start[p, v]), v
    return score, row, video


def brute_force(x):
    """The same by a loop over t and i in Python ints (exact for integer-valued x): (match, start) or None for V < m"""
    x = np.asarray(x)
    m, V = x.shape
    best = None
    for t in range(V - m + 1):
        s = 0
        for i in range(m):
            s += int(x[i, t + i])
        if best is None or s > best[0]:
            best = (s, t)
    return best
