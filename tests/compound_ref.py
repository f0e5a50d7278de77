"""A numpy restatement of the compound score of include/tan_hip.h (tan_compound_topk / tan_compound_peaks), shared by
test_compound_cpu.py (which pins it against a brute force over Python numbers) and test_compound_gpu.py (which compares the kernels
with it).  It works on a score matrix X [Qt, N] of any dtype:
  * int64: exact-arithmetic tests, where mult x score is an integer (veto is then given on the same scale), or
  * float32: the device's own bits (tan_sequence_scores), where every comparison is the kernel's float comparison.
Nothing here adds or multiplies: peaks, clause values and scores are ELEMENTS of X, picked by >, < and first-wins rules, so the
bits of a float32 X (the sign of a zero included) pass through unchanged."""
import numpy as np

SENT = 0x7fffffff


def peaks(X, t_off, v_off):
    """(p [Qt, n_videos] of X's dtype, r [Qt, n_videos] int64): per term and video the score of the first row of the video,
    ascending, that no other row of it beats under >, and that row (global).  A video without rows: (0, SENT); see `scores`."""
    Qt, nv = X.shape[0], len(v_off) - 1
    p, r = np.zeros((Qt, nv), dtype=X.dtype), np.full((Qt, nv), SENT, dtype=np.int64)
    for v in range(nv):
        lo, hi = int(v_off[v]), int(v_off[v + 1])
        if hi > lo:
            first = np.argmax(X[:, lo:hi], axis=1)                  # numpy's argmax: the first of the maxima, compared by >
            p[:, v], r[:, v] = X[np.arange(Qt), lo + first], lo + first
    return p, r


def scores(p, r, t_off, role, veto):
    """(score [n_query, n_videos] of p's dtype, candidate bool [n_query, n_videos], weakest int64 [n_query, n_videos]): the fold of
    the definition, written as loops -- a clause is worth the first of its terms, in term order, that none beats under >; the score
    starts at the first occupied clause, ascending, and is replaced only under strict <; a banned term with p >= veto, or a video
    without rows, makes the video no candidate."""
    nq, nv = len(t_off) - 1, p.shape[1]
    score = np.zeros((nq, nv), dtype=p.dtype)
    cand = np.zeros((nq, nv), dtype=bool)
    weakest = np.full((nq, nv), -1, dtype=np.int64)
    for q in range(nq):
        terms = range(int(t_off[q]), int(t_off[q + 1]))
        clauses = sorted({int(role[t]) for t in terms if role[t] >= 0})
        assert clauses, "a query needs a clause term"
        for v in range(nv):
            if r[terms[0], v] == SENT:
                continue
            s = w = None
            for j in clauses:
                g = None
                for t in terms:
                    if role[t] == j and (g is None or p[t, v] > g):
                        g = p[t, v]
                if s is None or g < s:
                    s, w = g, j
            score[q, v], weakest[q, v] = s, w
            cand[q, v] = not any(role[t] < 0 and p[t, v] >= veto for t in terms)
    return score, cand, weakest


def topk(score, cand, k):
    """(top_s [n_query, k] -- float64 for an integer score matrix, else its dtype --, top_v [n_query, k] int32): the k best
    candidates by descending score, equal scores by ascending video; the tail is (-inf, SENT)."""
    nq = score.shape[0]
    top_s = np.full((nq, k), -np.inf, dtype=np.float64 if score.dtype.kind == "i" else score.dtype)
    top_v = np.full((nq, k), SENT, dtype=np.int32)
    for q in range(nq):
        vs = np.flatnonzero(cand[q])
        order = vs[np.argsort(-score[q, vs].astype(np.float64) if score.dtype.kind == "i" else -score[q, vs], kind="stable")][:k]
        top_s[q, :len(order)], top_v[q, :len(order)] = score[q, order], order
    return top_s, top_v


def compound(X, t_off, role, v_off, veto, k):
    """Everything at once: (top_s, top_v, p, r, score, cand, weakest)"""
    p, r = peaks(X, t_off, v_off)
    score, cand, weakest = scores(p, r, t_off, role, veto)
    return (*topk(score, cand, k), p, r, score, cand, weakest)
