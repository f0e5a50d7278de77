"""Order-preserving timestamps, host side (no GPU): the numpy restatement of the decode that the GPU tests compare the kernel with,
pinned against exhaustive enumeration; the chunk's decode tables; the csv rows; the C entry point's argument check."""
import csv
import io
import itertools

import numpy as np
import torch

from temporalalignnet_amd import _lib
from temporalalignnet_amd.infer_align import _Chunk, write_rows


def np_decode(x):
    """include/tan_hip.h, tan_monotonic_decode, restated: x [m, V] f32, the kept rows in decode order -> (seconds [m], score f32).
    D_0 = x_0, D_i = x_i + M_{i-1} (one f32 add); M_i[t] = max D_i[:t+1]; A_i[t] = the smallest t' <= t with D_i[t'] == M_i[t];
    t_{m-1} = A_{m-1}[V-1], t_{i-1} = A_{i-1}[t_i]; score = D_{m-1}[t_{m-1}]."""
    x = np.asarray(x, dtype=np.float32)
    m, V = x.shape
    A = np.empty((m, V), dtype=np.int64)
    M = None
    for i in range(m):
        D = x[i] if i == 0 else (x[i] + M).astype(np.float32)
        run = np.maximum.accumulate(D)
        new = np.r_[True, D[1:] > run[:-1]]                   # a strictly greater value: the running maximum moves here
        A[i] = np.maximum.accumulate(np.where(new, np.arange(V), 0))
        M = D[A[i]]
    t = np.empty(m, dtype=np.int64)
    t[-1] = A[-1, V - 1]
    for i in range(m - 1, 0, -1):
        t[i - 1] = A[i - 1, t[i]]
    return t, M[V - 1]


def np_decode_video(sim, order, keep=None):
    """One video: sim [K, V], order [K] (row ids in decode order), keep [K] bool or None -> (ts [K] with -1 where not kept, score);
    no kept row: all -1, score 0."""
    K = len(sim)
    keep = np.ones(K, bool) if keep is None else np.asarray(keep).astype(bool)
    ids = [int(r) for r in order if keep[r]]
    ts = np.full(K, -1, dtype=np.int64)
    if not ids:
        return ts, np.float32(0)
    ts[ids], score = np_decode(np.asarray(sim, dtype=np.float32)[ids])
    return ts, score


def test_numpy_decode_is_the_exhaustive_optimum():
    rng = np.random.default_rng(0)
    n_ties = 0
    for case in range(300):
        m, V = int(rng.integers(1, 5)), int(rng.integers(1, 7))
        x = rng.integers(-3, 4, (m, V)).astype(np.float32)       # integers: every sum is exact, ties are common
        t, score = np_decode(x)
        assert (np.diff(t) >= 0).all() and t.min() >= 0 and t.max() < V
        assert x[np.arange(m), t].sum() == score
        paths = [p for p in itertools.product(range(V), repeat=m) if all(a <= b for a, b in zip(p, p[1:]))]
        sums = [sum(x[i, s] for i, s in enumerate(p)) for p in paths]
        assert score == max(sums), case
        # the tie rule: smallest t_{m-1}, then smallest t_{m-2}, ...
        best = [p for p, s in zip(paths, sums) if s == score]
        n_ties += len(best) > 1
        assert tuple(t) == min(best, key=lambda p: p[::-1]), case
    assert n_ties > 75                                           # the tie rule was exercised in at least a quarter of the cases


def test_numpy_decode_moves_independent_argmaxes_and_keeps_ordered_ones():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((37, 5000)) * 5).astype(np.float32)
    t, score = np_decode(x)
    assert (np.diff(t) >= 0).all() and (t != x.argmax(-1)).sum() > 20
    # rows whose own first arg-maxes are already in order decode to exactly them
    y = rng.integers(0, 3, (9, 40)).astype(np.float32)
    peaks = np.sort(rng.integers(0, 40, 9))
    y[np.arange(9), peaks] = 5
    t, score = np_decode(y)
    assert (t == peaks).all() and score == 45
    # masked cells are ordinary finite values: the only monotone path may run through them
    z = np.full((2, 6), -6e4, np.float32)
    z[0, 4:] = [1, 2]
    z[1, :2] = [3, 1]
    t, score = np_decode(z)
    assert list(t) == [0, 0] and score == np.float32(-6e4) + np.float32(3)
    ts, s = np_decode_video(z, [1, 0], keep=[1, 1])               # the other order: row 1 first
    assert list(ts) == [5, 0] and s == 5
    ts, s = np_decode_video(z, [1, 0], keep=[0, 0])
    assert list(ts) == [-1, -1] and s == 0


def _item(vid, start, vlen):
    start = np.asarray(start, dtype=np.float64)
    return {"vid": vid, "vlen": vlen, "start": start, "end": start + 2, "str": [f"{vid}s{k}" for k in range(len(start))]}


def test_chunk_order_and_vtab():
    items = [_item("a", [5.0, 1.0, 3.0], 100),                   # starts out of order
             _item("b", [], 50),                                  # a video with no sentence
             _item("c", [2.0, 2.0, 0.5, 2.0, 0.5], 70),           # equal starts: by sentence index
             _item("d", [7.0], 33)]
    ch = _Chunk(items, [[(0, 64, 0, len(it["str"]))] if it["str"] else [] for it in items], 64, 4)
    assert ch.order.dtype == torch.int32 and ch.vtab.dtype == torch.int32
    assert ch.order.tolist() == [1, 2, 0, 3 + 2, 3 + 4, 3 + 0, 3 + 1, 3 + 3, 8]
    assert ch.vtab.tolist() == [[0, 3, 0], [3, 0, 100], [3, 5, 150], [8, 1, 220]]
    assert ch.order.shape == (ch.n_rows,) and ch.vtab.shape == (4, 3)
    # the table rows the decode reads together with them: each row's accumulator offset and vlen
    assert ch.rows[ch.order[3:8].long(), 1].tolist() == [70] * 5
    # one video, no sentence at all
    ch = _Chunk([_item("e", [], 40)], [[]], 64, 4)
    assert ch.order.shape == (0,) and ch.vtab.tolist() == [[0, 0, 0]]


def _rows(res, threshold=None):
    buf = io.StringIO(newline="")
    n = write_rows(csv.writer(buf), res, threshold)
    rows = list(csv.reader(io.StringIO(buf.getvalue(), newline="")))
    assert n == len(rows)
    return rows


def test_write_rows_takes_the_ordered_timestamps():
    res = {"vid": "v", "str": ["a", "b", "c", "d"], "timestamp": np.array([30, 10, 20, 5]),
           "score": np.array([0.5, 2.0, 1.0, 9.0], np.float32), "confidence": np.array([0.1, 0.2, 0.3, 0.4], np.float32),
           "covered": np.array([1, 1, 1, 0], bool)}
    plain = _rows(res)
    assert [r[1] for r in plain] == ["30", "10", "20"]
    dec = dict(res, ordered_timestamp=np.array([10, 10, 20, -1]), ordered=np.array([1, 1, 1, 0], bool), path_score=3.5)
    got = _rows(dec)
    assert [r[1] for r in got] == ["10", "10", "20"]
    assert [r[:1] + r[2:] for r in got] == [r[:1] + r[2:] for r in plain]           # same rows, same other columns
    # decoded under a threshold: the rows written are the rows decoded
    dec_t = dict(res, ordered_timestamp=np.array([-1, 12, 20, -1]), ordered=np.array([0, 1, 1, 0], bool), path_score=2.0)
    got = _rows(dec_t, threshold=0.5)
    assert [(r[1], r[2]) for r in got] == [("12", "b"), ("20", "c")]
    assert [r[2] for r in _rows(res, threshold=0.5)] == ["b", "c"]


def test_decode_is_rejected_without_touching_a_device():
    L = _lib.lib()
    assert "tan_monotonic_decode" in _lib.declared_symbols()
    assert L.tan_monotonic_decode(None, None, None, None, 0, None, 0, 0, 0, None, None, None, None, None) == -1
    # non-positive counts with every pointer set (never dereferenced: nothing is launched)
    p = 4096
    assert L.tan_monotonic_decode(p, p, p, p, 0, None, 1, 1, 1, p, p, p, p, None) == -1
    assert L.tan_monotonic_decode(p, p, p, p, 1, None, 0, 1, 1, p, p, p, p, None) == -1
    assert L.tan_monotonic_decode(p, p, p, p, 1, None, 1, 1, 0, p, p, p, p, None) == -1
    assert L.tan_monotonic_decode(p, p, p, p, 1, None, 1, 1, 1, None, p, p, p, None) == -1


def test_cli_knows_decode_and_rejects_other_values():
    import pytest
    from temporalalignnet_amd import infer_align
    base = ["--checkpoint", "c", "--feature-dir", "f", "--asr-json", "a", "--vlen-csv", "v", "--vocab", "x", "--out", "o"]
    with pytest.raises(SystemExit) as e:
        infer_align.main(base + ["--decode", "viterbi"])
    assert e.value.code == 2
    with pytest.raises(ValueError, match="decode"):
        next(infer_align.align_corpus(None, [], None, decode="viterbi"))
