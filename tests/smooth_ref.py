"""The reference of the label decode (tan_label_decode, include/tan_hip.h), three times over:
  * `decode_f32`: the header's recurrence, row by row, every operation a numpy float32 one, in the header's order;
  * `decode_i64`: the same Viterbi over int64 (the caller scales exact inputs to integers), with the same tie rules;
  * `brute_force`: the objective maximised over ALL paths, for tiny cases.
Nothing here knows how the kernel works."""
import itertools

import numpy as np

F = np.float32
NEG = F(-np.inf)
FAR = -(1 << 60)                                                       # the int64 stand-in for -inf: below every finite sum


def _video(decode_rows, score, label, v_off, *args):
    N = len(score)
    dec_label, dec_score = np.full(N, -1, dtype=np.int64), np.full(N, NEG, dtype=np.float32)
    for v in range(len(v_off) - 1):
        a, b = int(v_off[v]), int(v_off[v + 1])
        states = decode_rows(score[a:b], label[a:b], *args)
        for t, s in enumerate(states):
            if s < score.shape[1]:
                dec_label[a + t], dec_score[a + t] = label[a + t, s], score[a + t, s]
    return dec_label, dec_score


def _labels(label_row):
    return [int(x) for x in label_row] + [-1]                          # state k: background


def _walk(bp, last):
    states = [last]
    for t in range(len(bp) - 1, 0, -1):
        states.append(bp[t][states[-1]])
    return states[::-1]


def _first_match(prev_labs, lab):
    for i, p in enumerate(prev_labs):
        if p == lab:
            return i
    return None


def states_f32(score, label, threshold, switch):
    """one video: score f32 / label [T, k] -> the chosen state of every row (k = background), by the header's recurrence"""
    thr, pen = F(threshold), F(switch)
    T, k = score.shape

    def gains(t):
        with np.errstate(over="ignore"):
            return [F(score[t, j]) - thr if np.isfinite(score[t, j]) else NEG for j in range(k)] + [F(0)]
    d = gains(0)
    bp = [None]
    for t in range(1, T):
        m = d[0]
        for x in d[1:]:
            m = np.maximum(m, x)
        a = next(i for i, x in enumerate(d) if x == m)
        rel = [x - m for x in d]
        prev, cur, g = _labels(label[t - 1]), _labels(label[t]), gains(t)
        nd, row = [], []
        for j in range(k + 1):
            i = _first_match(prev, cur[j])
            if i is not None and rel[i] >= -pen:
                c, b = rel[i], i
            else:
                c, b = -pen, a
            nd.append(F(c + g[j]))
            row.append(b)
        d = nd
        bp.append(row)
    m = max(d)
    return _walk(bp, next(j for j, x in enumerate(d) if x == m))


def states_i64(score, label, threshold, switch):
    """the same over Python integers: score int [T, k] with None for a score that is not finite; switch None for +inf"""
    T, k = len(score), len(score[0])

    def gains(t):
        return [FAR if score[t][j] is None else score[t][j] - threshold for j in range(k)] + [0]

    def add(c, g):
        return FAR if c == FAR or g == FAR else c + g
    d = gains(0)
    bp = [None]
    for t in range(1, T):
        m = max(d)
        a = d.index(m)
        rel = [FAR if x == FAR else x - m for x in d]
        npen = FAR if switch is None else -switch
        prev, cur, g = _labels(label[t - 1]), _labels(label[t]), gains(t)
        nd, row = [], []
        for j in range(k + 1):
            i = _first_match(prev, cur[j])
            if i is not None and rel[i] >= npen:
                c, b = rel[i], i
            else:
                c, b = npen, a
            nd.append(add(c, g[j]))
            row.append(b)
        d = nd
        bp.append(row)
    return _walk(bp, d.index(max(d)))


def decode_f32(score, label, v_off, threshold, switch):
    """score f32 / label [N, k], v_off [n_videos + 1] -> (dec_label int64 [N], dec_score f32 [N]) as tan_label_decode defines them"""
    score, label = np.asarray(score, dtype=np.float32), np.asarray(label, dtype=np.int64)
    return _video(states_f32, score, label, v_off, threshold, switch)


def decode_i64(score, label, v_off, threshold, switch, unit):
    """The int64 Viterbi on inputs that are exact multiples of `unit` (a power of two): scores, threshold and switch are scaled
    to integers, so no sum rounds; switch may be +inf.  Returns what `decode_f32` returns."""
    score, label = np.asarray(score, dtype=np.float32), np.asarray(label, dtype=np.int64)

    def scaled(x):
        q = float(x) / unit
        assert q == int(q), (x, unit)
        return int(q)

    def rows(sc, lab, thr, pen):
        return states_i64([[scaled(x) if np.isfinite(x) else None for x in r] for r in sc], lab, thr, pen)
    return _video(rows, score, label, v_off, scaled(threshold), None if np.isinf(switch) else scaled(switch))


def objective(states, score, label, threshold, switch):
    """the objective of one path over one video, in Python floats (exact for the eighths the tests use); -inf for a path through a
    score that is not finite, or one that changes label under an infinite penalty"""
    T, k = score.shape
    total, prev = 0.0, None
    for t, s in enumerate(states):
        lab = -1 if s == k else int(label[t, s])
        if s < k:
            if not np.isfinite(score[t, s]):
                return -np.inf
            total += float(score[t, s]) - threshold
        if t and lab != prev:
            if np.isinf(switch):
                return -np.inf
            total -= switch
        prev = lab
    return total


def brute_force(score, label, threshold, switch):
    """the largest objective over all (k + 1)^T paths of one video"""
    T, k = score.shape
    return max(objective(p, score, label, threshold, switch) for p in itertools.product(range(k + 1), repeat=T))
