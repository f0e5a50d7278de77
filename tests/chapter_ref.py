"""tan_chapter_costs' and tan_chapter_decode's definition (include/tan_hip.h) in numpy over int64: the reference
test_chapters_gpu.py compares the kernels with, pinned against a plain-Python brute force over Python ints by test_chapters_cpu.py.

A score block x [V, V] is float32 -- the device's own bits, or hand-made bit patterns.  With F = fix(x) (cover_ref.fix):
    D(s,e) = sum_{s<=t<e} F[t][t];   Q(s,e) = sum_{s<=i,t<e} F[i][t];   J(s,e) = D(s,e) - Q(s,e) // (e - s)        (numpy's //)
    dp_1[e] = J(0,e) if e >= min_len or e == V else INF
    dp_j[e] = min over s in [1, e - min_len], dp_{j-1}[s] < INF, of dp_{j-1}[s] + J(s,e); equal sums: the lowest s = arg_j[e]
    count = the lowest feasible j with the smallest dp_j[V] + (j - 1) * G;   b_count = V, b_{j-1} = arg_j[b_j]
    start[c] = b_c;  chapter[t] = c for start[c] <= t < start[c+1];  scatter[j-1] = f32(dp_j[V]) * 2^-30, +inf where infeasible"""
import numpy as np

from cover_ref import SHIFT, fix

MAX_ROWS = 4096
MAX_K = 256
INF = 1 << 62
MAX_G = 1 << 50


def g_of(penalty):
    """min(__float2ll_rn(penalty * 2^30f), 2^50): the f32 product (it may round, and overflow to inf), to nearest even, clamped"""
    with np.errstate(over="ignore"):
        y = float(np.float32(penalty) * np.float32(2.0 ** SHIFT))
    return MAX_G if y >= MAX_G else int(np.rint(y))


def costs(x):
    """ONE block x f32 [V, V] -> J int64 [V + 1, V + 1]: J[s, e] for 0 <= s < e <= V, 0 elsewhere.  The square sums by cumsum over
    both axes and the four-corner difference."""
    x = np.asarray(x)
    V = x.shape[0]
    assert x.shape == (V, V) and x.dtype == np.float32 and V >= 1
    F = fix(x)
    S = np.zeros((V + 1, V + 1), dtype=np.int64)
    S[1:, 1:] = F.cumsum(axis=0).cumsum(axis=1)
    d = np.concatenate([[0], np.cumsum(np.diagonal(F))]).astype(np.int64)
    ends = np.arange(V + 1)
    diag = np.diagonal(S)
    Q = diag[None, :] - S - S.T + diag[:, None]                     # at [s, e]: S[e,e] - S[s,e] - S[e,s] + S[s,s]
    n = ends[None, :] - ends[:, None]
    J = (d[None, :] - d[:, None]) - Q // np.maximum(n, 1)
    return np.where(n > 0, J, 0)


def cost_block(x):
    """the defined triangle as the kernel lays it out: int64 [V, V] with [e-1, s] = J(s, e) for s < e, and a mask of those cells"""
    J = costs(x)
    V = J.shape[0] - 1
    out = J[:V, 1:].T.copy()                                        # [e-1, s] = J[s, e]
    mask = np.tril(np.ones((V, V), dtype=bool))
    return np.where(mask, out, 0), mask


def decode(J, k, min_len=1, penalty=0.0):
    """J from `costs` -> (count, start int32 [k], scatter f32 [k], chapter int32 [V])"""
    V = J.shape[0] - 1
    assert k >= 1 and min_len >= 1
    G = g_of(penalty)
    m = min(k, V)
    ends = np.arange(V + 1)
    dp = np.where((ends >= min_len) | (ends == V), J[0], INF).astype(np.int64)
    dp[0] = INF
    finals, args = [int(dp[V])], [None]
    for j in range(2, m + 1):
        # cand[s, e] = dp_{j-1}[s] + J[s, e] for 1 <= s <= e - min_len, dp_{j-1}[s] < INF
        ok = (ends[:, None] >= 1) & (ends[:, None] <= ends[None, :] - min_len) & (dp[:, None] < INF)
        cand = np.where(ok, dp[:, None] + J, INF)
        arg = cand.argmin(axis=0)                                   # the first of equal minima: the lowest s
        new = cand[arg, ends]
        if int(new[V]) >= INF:                                      # a level that cannot reach V: neither can a later one
            break
        dp = new
        finals.append(int(dp[V]))
        args.append(arg)
    totals = [f + j * G for j, f in enumerate(finals)]
    count = int(np.argmin(totals)) + 1                              # the first of equal minima: the lowest j
    start, scatter = np.full(k, -1, np.int32), np.full(k, np.inf, np.float32)
    for j, f in enumerate(finals):
        scatter[j] = np.int64(f).astype(np.float32) * np.float32(2.0 ** -SHIFT)
    b = V
    for j in range(count, 1, -1):
        b = int(args[j - 1][b])
        start[j - 1] = b
    start[0] = 0
    edges = np.concatenate([start[:count], [V]])
    chapter = np.repeat(np.arange(count, dtype=np.int32), np.diff(edges))
    return count, start, scatter, chapter


def decode_many(Js, k, min_len=1, penalty=0.0):
    """a list of J -> (count [P], start [P, k], scatter [P, k], chapter [sum V])"""
    out = [decode(J, k, min_len, penalty) for J in Js]
    return (np.array([o[0] for o in out], np.int32), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
            np.concatenate([o[3] for o in out]))


def brute(F, k, min_len, G):
    """The same over Python ints, nothing vectorised: F is a list of lists of ALREADY FIXED integers.  Every composition of V into at
    most min(k, V) parts of at least min_len seconds (one part: always allowed) with its exact summed cost; returns
    (count: the lowest j with the smallest total, {j: the smallest summed cost of j parts})."""
    V = len(F)

    def J(s, e):
        D = sum(F[t][t] for t in range(s, e))
        Q = sum(F[i][t] for i in range(s, e) for t in range(s, e))
        return D - Q // (e - s)

    best = {}                                                       # j -> (cost, starts)

    def walk(starts, cost):
        s = starts[-1]
        j = len(starts)
        if V - s >= min_len or j == 1:                              # close the last part at V (one part: whatever its length)
            total = cost + J(s, V)
            if j not in best or total < best[j][0]:
                best[j] = (total, list(starts))
        if j < min(k, V):
            for nxt in range(s + min_len, V):
                walk(starts + [nxt], cost + J(s, nxt))

    walk([0], 0)
    levels = {j: c for j, (c, _) in best.items()}
    count = min(levels, key=lambda j: (levels[j] + (j - 1) * G, j))
    return count, levels


def dp_starts(F, count, min_len):
    """the definition's backtrack over Python ints: level by level with the lowest s among equal sums"""
    V = len(F)

    def J(s, e):
        return sum(F[t][t] for t in range(s, e)) - sum(F[i][t] for i in range(s, e) for t in range(s, e)) // (e - s)

    dp = [INF] + [J(0, e) if (e >= min_len or e == V) else INF for e in range(1, V + 1)]
    args = [None]
    for j in range(2, count + 1):
        new, arg = [INF] * (V + 1), [0] * (V + 1)
        for e in range(1, V + 1):
            for s in range(1, e - min_len + 1):
                if dp[s] < INF and dp[s] + J(s, e) < new[e]:
                    new[e], arg[e] = dp[s] + J(s, e), s
        dp = new
        args.append(arg)
    b, starts = V, []
    for j in range(count, 1, -1):
        b = args[j - 1][b]
        starts.append(b)
    return [0] + starts[::-1], dp[V]


def scenes_aba(seed):
    """A scenes-style video (storyboard_ref.scenes) of three scenes whose third repeats the first direction: rows f32 [V, 512],
    scene int [V] = 0 / 1 / 0.  A's two stretches hold 10 to 39 seconds each and B 5 to 19, so A is the larger scene."""
    rng = np.random.default_rng(seed)
    dirs = rng.standard_normal((2, 512))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    lens = (rng.integers(10, 40), rng.integers(5, 20), rng.integers(10, 40))
    scene = np.repeat(np.array([0, 1, 0]), lens)
    rows = dirs[scene] + rng.standard_normal((len(scene), 512)) * (0.3 / np.sqrt(512))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    return rows.astype(np.float32), scene
