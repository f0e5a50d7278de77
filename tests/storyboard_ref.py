"""tan_storyboard_select's definition (include/tan_hip.h) in numpy over int64, operation by operation: the reference
test_storyboard_gpu.py compares the kernel with, pinned against a plain-Python brute force over Python ints by test_storyboard_cpu.py.

A score block x [V, V] (row s = the candidate second, column t = the second it is to show) is either float32 -- the device's own
bits, or hand-made bit patterns -- or int64 with a power-of-two `mult`: exact scores x / mult (cover_ref.fix).
    C_0[t] = -2^62;   T_j(s) = sum_t max(fix(x[s, t]), C_{j-1}[t]);   s_j = the lowest s with the largest T_j
    stop before entry j >= 2 when gain = T_j(s_j) - sum C_{j-1} <= 0 or gain < G_min * V
    C_j = max(C_{j-1}, fix(x[s_j]));   owner[t] = j where fix(x[s_j, t]) > C_{j-1}[t];   coverage[j] = (f32(sum C_j) * 2^-30) / f32(V)
Entries are stored 0-based; entries after a stop and beyond V hold second = -1, coverage = 0."""
import numpy as np

from cover_ref import SHIFT, fix, mean_of_sum

MAX_ROWS = 4096
MAX_K = 4096
FLOOR = -(1 << 62)
MAX_GMIN = 1 << 40


def g_min(min_gain):
    """min(__float2ll_rn(min_gain * 2^30f), 2^40): the f32 product (it may round, and overflow to inf), to nearest even, clamped"""
    with np.errstate(over="ignore"):
        y = float(np.float32(min_gain) * np.float32(2.0 ** SHIFT))
    return MAX_GMIN if y >= MAX_GMIN else int(np.rint(y))


def select(x, k, min_gain=0.0, mult=None):
    """ONE block x [V, V] -> (second int32 [k], coverage f32 [k], owner int32 [V])"""
    x = np.asarray(x)
    V = x.shape[0]
    assert x.shape == (V, V) and 1 <= V and k >= 1
    F = fix(x, mult)                                                # int64 [V, V]
    gm = g_min(min_gain)
    C = np.full(V, FLOOR, dtype=np.int64)
    second, coverage, owner = np.full(k, -1, np.int32), np.zeros(k, np.float32), np.zeros(V, np.int32)
    for j in range(min(k, V)):
        T = np.maximum(F, C[None, :]).sum(axis=1)                   # int64, exact
        s = int(np.argmax(T))                                       # the first of equal maxima
        if j >= 1:
            gain = int(T[s]) - int(C.sum())
            if gain <= 0 or gain < gm * V:
                break
        better = F[s] > C
        owner[better] = j
        C = np.where(better, F[s], C)
        second[j], coverage[j] = s, mean_of_sum(int(C.sum()), V)
    return second, coverage, owner


def select_many(blocks, k, min_gain=0.0, mult=None):
    """blocks: a list of [V, V] arrays -> (second [P, k], coverage [P, k], owner [sum V])"""
    out = [select(b, k, min_gain, mult) for b in blocks]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.concatenate([o[2] for o in out]))


def brute(x, k, min_gain_fixed=0):
    """The same over Python ints, nothing vectorised: x is a list of lists of ALREADY FIXED integers (fix applied), min_gain_fixed is
    G_min.  Returns (seconds list, C-sums list, owner list): the entries made, the exact integer sum of C after each, owner per t."""
    V = len(x)
    C = [FLOOR] * V
    seconds, sums, owner = [], [], [0] * V
    for j in range(min(k, V)):
        best_s, best_T = None, None
        for s in range(V):
            T = sum(max(x[s][t], C[t]) for t in range(V))
            if best_T is None or T > best_T:
                best_s, best_T = s, T
        if j >= 1:
            gain = best_T - sum(C)
            if gain <= 0 or gain < min_gain_fixed * V:
                break
        for t in range(V):
            if x[best_s][t] > C[t]:
                C[t], owner[t] = x[best_s][t], j
        seconds.append(best_s)
        sums.append(sum(C))
    return seconds, sums, owner


def scenes(seed, n_scenes=6):
    """The 'meaning' input: a video of `n_scenes` scenes, each a random unit direction held 5 to 39 seconds with noise of
    0.3 / sqrt(512) per component, renormalised.  Returns (rows f32 [V, 512], scene int [V]: every second's scene)."""
    rng = np.random.default_rng(seed)
    dirs = rng.standard_normal((n_scenes, 512))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    lens = rng.integers(5, 40, n_scenes)
    scene = np.repeat(np.arange(n_scenes), lens)
    rows = dirs[scene] + rng.standard_normal((len(scene), 512)) * (0.3 / np.sqrt(512))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    return rows.astype(np.float32), scene
