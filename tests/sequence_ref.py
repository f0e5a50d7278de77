"""A numpy restatement of the ordered-sequence path of include/tan_hip.h (tan_sequence_topk / tan_monotonic_decode) and of its
backtrack, shared by test_sequences_cpu.py (which pins it against exhaustive enumeration) and test_sequences_gpu.py.

    D_0[t] = x_0[t]      D_i[t] = x_i[t] + M_{i-1}[t]      M_i[t] = max_{t' <= t} D_i[t']      path = M_{m-1}[V - 1]
    A_i[t] = the smallest t' <= t with D_i[t'] == M_i[t];   t_{m-1} = A_{m-1}[V - 1];   t_{i-1} = A_{i-1}[t_i]

Every add is done in x's own dtype (float32: one rounded add per cell, as the kernels; int64 / float64: a reference)."""
import itertools

import numpy as np


def path_and_seconds(x):
    """x [m, V] -> (path: a scalar of x's dtype, seconds: m ints, non-decreasing)"""
    x = np.asarray(x)
    m, V = x.shape
    assert m >= 1 and V >= 1
    t_all = np.arange(V)
    M, A = None, []
    for i in range(m):
        d = x[i] if i == 0 else (x[i] + M).astype(x.dtype)
        M = np.maximum.accumulate(d)
        record = np.concatenate([[True], d[1:] > M[:-1]])                   # a strictly larger value than everything to its left
        A.append(np.maximum.accumulate(np.where(record, t_all, 0)))
    t, seconds = V - 1, []
    for i in range(m - 1, -1, -1):
        t = int(A[i][t])
        seconds.append(t)
    return M[V - 1], tuple(seconds[::-1])


def paths(X, s_off, v_off):
    """X [Qt, N] scores -> path [n_seq, n_videos] in X's dtype"""
    X = np.asarray(X)
    out = np.empty((len(s_off) - 1, len(v_off) - 1), dtype=X.dtype)
    for p in range(out.shape[0]):
        for v in range(out.shape[1]):
            out[p, v] = path_and_seconds(X[s_off[p]:s_off[p + 1], v_off[v]:v_off[v + 1]])[0]
    return out


def topk(path, k):
    """path [n_seq, n_videos] -> (scores [n_seq, k], videos [n_seq, k]): descending path, equal paths by ascending video"""
    order = np.stack([np.array(sorted(range(path.shape[1]), key=lambda v: (-row[v], v))[:k]) for row in path])
    return np.take_along_axis(path, order, 1), order


def brute_force(x):
    """The same by enumerating every non-decreasing assignment (exact for integer-valued x): the largest sum; among the
    assignments that reach it the smallest last second, then the smallest second to last, and so on."""
    x = np.asarray(x)
    m, V = x.shape
    best = None
    for ts in itertools.combinations_with_replacement(range(V), m):
        key = (-sum(x[i, t] for i, t in enumerate(ts)), ts[::-1])
        if best is None or key < best:
            best = key
    return -best[0], tuple(best[1][::-1])
