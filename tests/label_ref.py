"""The reference of corpus annotation (tan_label_topk / tan_label_runs, include/tan_hip.h), stated row by row in numpy / torch
fp64.  Nothing here knows how the kernels work."""
import numpy as np
import torch


def label_topk(S, k):
    """S [L, N] fp64 scores (label x row, any device) -> (score [N, k] fp64, label [N, k] int64): per row the k best labels by
    descending score, equal scores by ascending label (a stable sort of the whole score matrix)."""
    St = S.T.contiguous()
    order = torch.sort(St, dim=1, descending=True, stable=True).indices[:, :k]
    return St.gather(1, order), order


def row_labels(score0, label0, threshold):
    """lab[n]: the row's best label if its score is >= threshold, else -1 (a NaN score compares false: background)"""
    score0, label0 = np.asarray(score0, dtype=np.float32), np.asarray(label0, dtype=np.int64)
    return np.where(score0 >= np.float32(threshold), label0, -1)


def label_runs(score0, label0, v_off, threshold, min_len=1):
    """score0 / label0 [N]: column 0 of the lists; v_off [n_videos + 1].  Returns the kept runs, in ascending first row, as a list
    of (video, first row, last row (inclusive), label, peak row, peak score): a run is a maximal range of rows of ONE video whose
    lab is constant and not -1; runs of fewer than min_len rows are dropped; the peak is the run's largest score and the smallest
    row that attains it."""
    score0 = np.asarray(score0, dtype=np.float32)
    lab = row_labels(score0, label0, threshold)
    runs = []
    for v in range(len(v_off) - 1):
        n = int(v_off[v])
        end = int(v_off[v + 1])
        while n < end:
            if lab[n] == -1:
                n += 1
                continue
            b = n
            while b + 1 < end and lab[b + 1] == lab[n]:
                b += 1
            if b - n + 1 >= min_len:
                peak = n
                for r in range(n, b + 1):
                    if score0[r] > score0[peak]:
                        peak = r
                runs.append((v, n, b, int(lab[n]), peak, float(score0[peak])))
            n = b + 1
    return runs


def label_rows(score0, label0, threshold, L):
    """[L] int64: how many rows have lab == l, whatever min_len is"""
    lab = row_labels(score0, label0, threshold)
    return np.bincount(lab[lab >= 0], minlength=L).astype(np.int64)


def runs_fast(score0, label0, v_off, threshold, min_len=1):
    """`label_runs` with numpy for large N (checked against it in test_annotate_cpu.py): the same tuples as arrays
    (video, start, end, label, peak_row int64; peak_score f32)."""
    score0 = np.asarray(score0, dtype=np.float32)
    N = len(score0)
    lab = row_labels(score0, label0, threshold)
    video = np.searchsorted(np.asarray(v_off), np.arange(N), side="right") - 1
    new = np.ones(N, dtype=bool)
    new[1:] = (lab[1:] != lab[:-1]) | (video[1:] != video[:-1])
    start = np.flatnonzero(new & (lab != -1))
    last = np.ones(N, dtype=bool)
    last[:-1] = new[1:]
    end = np.flatnonzero(last & (lab != -1))
    keep = end - start + 1 >= min_len
    start, end = start[keep], end[keep]
    if len(start) == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z, z, np.zeros(0, dtype=np.float32)
    safe = np.where(lab != -1, score0, -np.inf).astype(np.float32)
    # reduceat over the cuts start_0, end_0 + 1, start_1, ...: the even pieces are the runs, the odd ones what lies between them
    peak = np.maximum.reduceat(np.concatenate([safe, [-np.inf]]).astype(np.float32), np.stack((start, end + 1), 1).reshape(-1))[::2]
    run_of_row = np.full(N, -1, dtype=np.int64)
    run_of_row[start] = np.arange(len(start))
    run_id = np.maximum.accumulate(run_of_row)                         # the last kept run that began at or before the row
    inside = np.zeros(N + 1, dtype=np.int64)
    inside[start] += 1                                                 # starts are distinct rows, and so are ends
    inside[end + 1] -= 1
    at_peak = np.flatnonzero((np.cumsum(inside[:N]) > 0) & (safe == peak[np.maximum(run_id, 0)]))
    _, first = np.unique(run_id[at_peak], return_index=True)           # run_id ascends: the first row at the peak of every run
    return video[start], start, end, lab[start], at_peak[first], peak
