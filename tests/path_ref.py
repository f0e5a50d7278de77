"""tan_local_align_path restated (include/tan_hip.h): tan_local_align's recurrence with one code per positive cell and the walk back
along the codes, by a plain loop.

    g = x[i][j] - theta;  diag = H[i-1][j-1];  up = H[i-1][j] - skew;  left = H[i][j-1] - skew      (H = 0 outside the matrix)
    P = max(diag, up, left), pred = the FIRST of (diag, up, left) attaining it;  H[i][j] = max(0, g + P)
    code: 0 start (pred is diag and that H is 0), 1 diag, 2 up, 3 left

`align_path` works in x's own dtype: int64 and float64 as Python ints / floats (the same arithmetic), float32 as numpy float32 scalars,
every - and + one rounded operation.  It returns (score, (a_first, a_last, b_first, b_last, cells), qmap int32 [m, 2]): the span is
READ OFF THE WALK (its last cell, its length), not carried forward as align_ref.align carries it, so the two agree only if the codes
and the carried origins say the same.  qmap[i] = (first, last video second of query second i) on the path, (-1, -1) elsewhere.
`staircase` plants a path of known cells."""
import numpy as np

EMPTY = (-1, -1, -1, -1, 0)
START, DIAG, UP, LEFT = 0, 1, 2, 3
PATTERN = (("d", 5), ("l", 3), ("u", 2), ("d", 1), ("l", 1), ("u", 1))


def codes(x, theta, skew):
    """(H as nested lists [m + 1][V + 1] with H[i + 1][j + 1] = cell (i, j), code [m][V], best, end)"""
    x = np.asarray(x)
    m, V = x.shape
    if x.dtype == np.float32:
        conv, rows = np.float32, [list(r) for r in x]
    else:
        assert x.dtype in (np.int64, np.float64), x.dtype
        conv, rows = (int if x.dtype == np.int64 else float), x.tolist()
    theta, skew, zero = conv(theta), conv(skew), conv(0)
    H = [[zero] * (V + 1) for _ in range(m + 1)]
    code = [[START] * V for _ in range(m)]
    top, end = zero, None
    for i in range(m):
        above, here, row, crow = H[i], H[i + 1], rows[i], code[i]
        for j in range(V):
            g = row[j] - theta
            diag, up, left = above[j], above[j + 1] - skew, here[j] - skew
            if diag >= up and diag >= left:
                P, c = diag, (DIAG if diag > zero else START)
            elif up >= left:
                P, c = up, UP
            else:
                P, c = left, LEFT
            h = g + P
            if h > zero:
                here[j + 1], crow[j] = h, c
                if h > top:                             # (i, j) ascending: the first cell attaining the maximum
                    top, end = h, (i, j)
    return H, code, top, end


def walk(code, end):
    """the path's cells from `end` back to its start, in walk order"""
    i, j = end
    cells = [(i, j)]
    while code[i][j] != START:
        c = code[i][j]
        i, j = (i - 1, j - 1) if c == DIAG else (i - 1, j) if c == UP else (i, j - 1)
        assert i >= 0 and j >= 0
        cells.append((i, j))
    return cells


def map_of(cells, m):
    """qmap int32 [m, 2] of a list of path cells"""
    qmap = np.full((m, 2), -1, dtype=np.int32)
    for i, j in cells:
        qmap[i, 0] = j if qmap[i, 0] < 0 else min(qmap[i, 0], j)
        qmap[i, 1] = max(qmap[i, 1], j)
    return qmap


def align_path(x, theta, skew):
    x = np.asarray(x)
    _, code, top, end = codes(x, theta, skew)
    if end is None:
        return x.dtype.type(0), EMPTY, map_of([], x.shape[0])
    cells = walk(code, end)
    (a0, b0), (a1, b1) = cells[-1], cells[0]
    return x.dtype.type(top), (a0, a1, b0, b1, len(cells)), map_of(cells, x.shape[0])


def staircase(m, V, start, pattern=PATTERN, on=24, off=-8):
    """An int64 block [m, V] of sixteenths, `on` along a staircase and `off` elsewhere, and the staircase's cells in path order: from
    `start` the runs of `pattern` -- ("d", n): n diagonal steps, ("l", n): n steps whose predecessor is LEFT (the column advances),
    ("u", n): n whose predecessor is UP (the row advances) -- over and over until the next step would leave the block."""
    x = np.full((m, V), off, dtype=np.int64)
    i, j = start
    cells = [(i, j)]
    step = {"d": (1, 1), "l": (0, 1), "u": (1, 0)}
    while True:
        for kind, n in pattern:
            for _ in range(n):
                i, j = i + step[kind][0], j + step[kind][1]
                if i >= m or j >= V:
                    for a, b in cells:
                        x[a, b] = on
                    return x, cells
                cells.append((i, j))


STAIR_SHAPES = ((129, 200), (200, 129), (65, 65), (64, 64), (130, 131))
STAIR_STARTS = ((0, 0), (3, 7), (1, 0), (60, 59), (2, 0))             # from (2, 0) the pattern's up step lands on row 128
STAIR_PRICES = tuple((theta, skew) for theta in (8, 7) for skew in (0, 2, 7))       # sixteenths
STAIR_CASES = tuple((mv, start) for mv in STAIR_SHAPES for start in STAIR_STARTS)


def steps(cells):
    """[((i, j), (i', j'))] of consecutive path cells"""
    return list(zip(cells[:-1], cells[1:]))
