"""tan_local_align restated (include/tan_hip.h): the best local alignment of a block x [m, V], steps in either axis allowed.

    g = x[i][j] - theta;  diag = H[i-1][j-1];  up = H[i-1][j] - skew;  left = H[i][j-1] - skew      (H = 0 outside the matrix)
    P = max(diag, up, left), pred = the FIRST of (diag, up, left) attaining it;  H[i][j] = max(0, g + P)

`align` works in x's own dtype -- float32 as the kernel does (every - and + one rounded f32 operation), int64 / float64 as
references -- by anti-diagonals, one vector operation per quantity and diagonal.  `align_loop` is the plain loop over Python ints
that test_align_cpu.py pins it against.  Both return (score, (a_first, a_last, b_first, b_last, cells)): the largest H, the cell
attaining it with the smallest i, then the smallest j, its path's first cell and its number of cells; (0, (-1, -1, -1, -1, 0))
when no cell is positive."""
import numpy as np

EMPTY = (-1, -1, -1, -1, 0)


def align(x, theta, skew):
    x = np.asarray(x)
    m, V = x.shape
    dt = x.dtype.type
    theta, skew, zero = dt(theta), dt(skew), dt(0)
    # index r + 1 = row r; index 0 = the row above the matrix, always 0.  cur: every row's latest value (0 before its first
    # column); old: the same one diagonal earlier
    cur, old = np.zeros(m + 1, dtype=x.dtype), np.zeros(m + 1, dtype=x.dtype)
    cur_o, old_o = np.zeros((m + 1, 2), dtype=np.int64), np.zeros((m + 1, 2), dtype=np.int64)
    cur_c, old_c = np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    best = np.zeros(m, dtype=x.dtype)                  # per row, under strict >: its first column attaining its maximum
    best_j, best_c = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    best_o = np.zeros((m, 2), dtype=np.int64)
    for d in range(m + V - 1):
        i = np.arange(max(0, d - V + 1), min(m - 1, d) + 1)
        j = d - i
        g = x[i, j] - theta
        diag, up, left = old[i], cur[i] - skew, cur[i + 1] - skew
        pd = (diag >= up) & (diag >= left)
        pu = ~pd & (up >= left)
        P = np.where(pd, diag, np.where(pu, up, left))
        h = g + P
        h = np.where(h > zero, h, zero)
        fresh = pd & ~(diag > zero)
        o = np.where(pd[:, None], old_o[i], np.where(pu[:, None], cur_o[i], cur_o[i + 1]))
        o = np.where(fresh[:, None], np.stack((i, j), 1), o)
        c = np.where(pd, old_c[i], np.where(pu, cur_c[i], cur_c[i + 1])) + 1
        c = np.where(h > zero, np.where(fresh, 1, c), 0)
        new, new_o, new_c = cur.copy(), cur_o.copy(), cur_c.copy()
        new[i + 1], new_o[i + 1], new_c[i + 1] = h, o, c
        old, old_o, old_c, cur, cur_o, cur_c = cur, cur_o, cur_c, new, new_o, new_c
        win = h > best[i]
        iw = i[win]
        best[iw], best_j[iw], best_c[iw], best_o[iw] = h[win], j[win], c[win], o[win]
    top = best.max()
    if not top > zero:
        return zero, EMPTY
    r = int(np.argmax(best))                            # the first row attaining it
    return top, (int(best_o[r, 0]), r, int(best_o[r, 1]), int(best_j[r]), int(best_c[r]))


def align_loop(x, theta, skew):
    """x: rows of Python ints; theta, skew ints"""
    m, V = len(x), len(x[0])
    H = [[0] * (V + 1) for _ in range(m + 1)]           # H[i + 1][j + 1] = cell (i, j)
    org = [[None] * (V + 1) for _ in range(m + 1)]
    cnt = [[0] * (V + 1) for _ in range(m + 1)]
    top, end = 0, None
    for i in range(m):
        for j in range(V):
            g = x[i][j] - theta
            diag, up, left = H[i][j], H[i][j + 1] - skew, H[i + 1][j] - skew
            P = max(diag, up, left)
            if diag == P:
                pi, pj = i, j
            elif up == P:
                pi, pj = i, j + 1
            else:
                pi, pj = i + 1, j
            h = max(0, g + P)
            H[i + 1][j + 1] = h
            if h > 0:
                if (pi, pj) == (i, j) and H[pi][pj] == 0:
                    org[i + 1][j + 1], cnt[i + 1][j + 1] = (i, j), 1
                else:
                    org[i + 1][j + 1], cnt[i + 1][j + 1] = org[pi][pj], cnt[pi][pj] + 1
                if h > top:                             # (i, j) ascending: the first cell attaining the maximum
                    top, end = h, (i, j)
    if end is None:
        return 0, EMPTY
    i, j = end
    return top, (org[i + 1][j + 1][0], i, org[i + 1][j + 1][1], j, cnt[i + 1][j + 1])


def piece_table(m, V, n_before=0, x_before=0, pieces=32):
    """The hits of one (query, video) pair for tan_sequence_scores when the query's m rows are sequences of `pieces` rows (the last
    one shorter), numbered from n_before: [(sequence, x offset)] with consecutive offsets from x_before, so the pieces' [len, V]
    blocks ARE the [m, V] block."""
    return [(n_before + a // pieces, x_before + a * V) for a in range(0, m, pieces)]
