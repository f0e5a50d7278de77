"""numpy restatement of step discovery (include/tan_hip.h: tan_cluster_accumulate, tan_cluster_centroids; search.discover_steps).

  * `fixed_point` / `accumulate`: the int64 image q = rint(v * 2^30) of f32 values and the per-cluster integer sums (np.add.at);
  * `centroids`: the centroid arithmetic in float32, every operation rounded on its own, in the header's order;
  * `update`: the two together -- one Lloyd update from (rows, assign, prev);
  * `lloyd`: an independent Lloyd loop: fp64 scores of the stored rows against the stored centroid image, argmax with equal scores
    to the lower cluster, `update`, under `discover_steps`' stopping rule.  It also reports every pass's smallest best-minus-second
    margin, so a test can show that no assignment of its input is within reach of the kernels' rounding.
"""
import numpy as np

SCALE = 2.0 ** 30
WIDTH = 512


def fixed_point(v):
    """f32 values -> int64: round-to-nearest-even of v * 2^30 (the product is exact in fp64)"""
    v = np.asarray(v)
    assert v.dtype == np.float32
    return np.rint(v.astype(np.float64) * SCALE).astype(np.int64)


def accumulate(rows, assign, K, sums=None):
    """rows f32 [N, 512] (the VALUES of the stored rows), assign int [N] -> int64 [K, 512]: sums (zeros if None) plus every row's
    image in the row of its cluster; a row whose assign lies outside [0, K) is skipped.  int64 wraps as the kernel's adds do."""
    assign = np.asarray(assign, dtype=np.int64)
    sums = np.zeros((K, WIDTH), dtype=np.int64) if sums is None else sums.copy()
    ok = (assign >= 0) & (assign < K)
    np.add.at(sums, assign[ok], fixed_point(rows)[ok])
    return sums


def centroids(sums, counts, prev):
    """int64 [K, 512], int [K], f32 [K, 512] -> (cent f32 [K, 512], cohesion f32 [K]) in float32, operation by operation"""
    sums, counts, prev = np.asarray(sums, dtype=np.int64), np.asarray(counts), np.asarray(prev, dtype=np.float32)
    K = sums.shape[0]
    x = sums.astype(np.float32) * np.float32(2.0 ** -30)               # int64 -> f32 rounds to nearest even; the scaling is exact
    lanes = np.arange(64)
    p = np.zeros((K, 64), dtype=np.float32)
    for i in range(WIDTH // 64):                                       # lane l: j = l, l + 64, ..., l + 448, in that order
        xi = x[:, 64 * i:64 * i + 64]
        p = p + xi * xi                                                # a rounded multiply, then a rounded add
    for d in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lanes ^ d]
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = np.sqrt(p[:, 0])
        cent = x / norm[:, None]
        cohesion = norm / counts.astype(np.float32)
    keep = (counts <= 0) | ~(norm > 0) | ~np.isfinite(norm)
    cent[keep] = prev[keep]
    cohesion[keep] = 0
    assert cent.dtype == np.float32 and cohesion.dtype == np.float32
    return cent, cohesion


def update(rows, assign, prev):
    """One Lloyd update: (cent, cohesion) from the rows' values, their clusters and the centroids before"""
    K = prev.shape[0]
    assign = np.asarray(assign, dtype=np.int64)
    return centroids(accumulate(rows, assign, K), np.bincount(assign[(assign >= 0) & (assign < K)], minlength=K), prev)


def lloyd(rows, image, init, iters):
    """rows f32 [N, 512]: the stored rows' values; image(cent f32 [K, 512]) -> fp64 [K, 512]: the values of the centroids as the
    sweep sees them; init f32 [K, 512].  Returns dict(assign, score (fp64), sizes, centroids, cohesion, moved, margin): margin[t]
    is pass t's smallest (best - second best) score over the rows (inf for K = 1)."""
    rows64 = np.asarray(rows, dtype=np.float64)
    cent = np.asarray(init, dtype=np.float32).copy()
    before = np.full(len(rows), -1, dtype=np.int64)
    moved, margin = [], []
    while True:
        S = rows64 @ image(cent).T                                     # [N, K]
        assign = S.argmax(1)                                           # the first maximum: equal scores to the lower cluster
        top2 = np.sort(S, axis=1)[:, -2:]
        margin.append(float((top2[:, -1] - top2[:, 0]).min()) if S.shape[1] > 1 else float("inf"))
        new, cohesion = update(rows, assign, cent)
        moved.append(int((assign != before).sum()))
        if len(moved) > iters or (len(moved) > 1 and moved[-1] == 0):
            break
        cent, before = new, assign
    return dict(assign=assign, score=S.max(1), sizes=np.bincount(assign, minlength=len(cent)), centroids=cent, cohesion=cohesion,
                moved=moved, margin=margin)
