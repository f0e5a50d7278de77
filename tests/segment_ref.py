"""The numpy restatement of tan_segment_decode's recurrence (include/tan_hip.h): the oracle of test_segments_cpu.py, which pins it
against exhaustive enumeration, and of test_segments_gpu.py, which compares the kernel with it bit for bit."""
import numpy as np

NINF = np.float32(-np.inf)


def np_tables(x, bias):
    """x [m, V] f32, the kept rows in decode order; bias [m] f32 -> (S [m, V], B [m, V] int64, path f32).  One step per second, every
    sentence at once: E_i[t] = g_i[t] + max(E_i[t-1], G_{i-1}[t-1]) is one f32 add, the maxima are exact."""
    x, bias = np.asarray(x, dtype=np.float32), np.asarray(bias, dtype=np.float32)
    m, V = x.shape
    g = x - bias[:, None]                                         # one f32 subtraction
    assert g.dtype == np.float32
    E, G = np.full(m, NINF), np.full(m, NINF)
    s, b = np.zeros(m, np.int64), np.zeros(m, np.int64)
    S, B = np.empty((m, V), np.int64), np.empty((m, V), np.int64)
    for t in range(V):
        c = np.concatenate([np.zeros(1, np.float32), G[:-1]])     # G_{i-1}[t-1]; G_{-1} = 0
        opens = c > E                                             # a tie extends the running segment
        E = g[:, t] + np.where(opens, c, E)
        s = np.where(opens, t, s)
        new = E > G                                               # strictly greater: B is the smallest arg-max
        G, b = np.where(new, E, G), np.where(new, t, b)
        S[:, t], B[:, t] = s, b
    assert E.dtype == G.dtype == np.float32
    return S, B, G[-1]


def np_segments(x, bias):
    """-> (seg [m, 2] int64 inclusive (s, e), path f32); m > V: all (-1, -1), -inf."""
    m, V = np.shape(x)
    seg = np.full((m, 2), -1, np.int64)
    if m > V:
        return seg, NINF
    S, B, path = np_tables(x, bias)
    t = V - 1
    for i in range(m - 1, -1, -1):
        e = B[i, t]
        seg[i] = S[i, e], e
        t = S[i, e] - 1
    return seg, path


def np_segments_video(sim, order, bias, keep=None):
    """One video: sim [K, V], order [K] (row ids in decode order), bias [K], keep [K] bool or None -> (seg [K, 2] with (-1, -1) where not
    kept, path); no kept row: path 0."""
    K = len(sim)
    keep = np.ones(K, bool) if keep is None else np.asarray(keep).astype(bool)
    ids = [int(r) for r in order if keep[r]]
    seg = np.full((K, 2), -1, np.int64)
    if not ids:
        return seg, np.float32(0)
    seg[ids], path = np_segments(np.asarray(sim, dtype=np.float32)[ids], np.asarray(bias, dtype=np.float32)[ids])
    return seg, path


def np_segments_prefix(x, bias):
    """The same optimum written with prefix sums, P_i[t] = sum_{t' <= t} g_i[t']: E_i[t] = P_i[t] + max_{s <= t} (G_{i-1}[s-1] - P_i[s-1]).
    Equal in exact arithmetic, NOT in f32 (the adds are re-associated): what the kernel must not do.  -> path f32."""
    x, bias = np.asarray(x, dtype=np.float32), np.asarray(bias, dtype=np.float32)
    m, V = x.shape
    if m > V:
        return NINF
    Gp = np.zeros(V + 1, np.float32)                              # G_{i-1}[t-1] at index t
    for i in range(m):
        P = np.concatenate([np.zeros(1, np.float32), np.cumsum(x[i] - bias[i], dtype=np.float32)])      # P[t-1] at index t
        E = P[1:] + np.maximum.accumulate(Gp[:V] - P[:V])
        Gp = np.concatenate([[NINF], np.maximum.accumulate(E)]).astype(np.float32)
    return Gp[V]
