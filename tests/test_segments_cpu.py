"""Aligned intervals, host side (no GPU): the numpy restatement of tan_segment_decode (segment_ref.py) against exhaustive enumeration
and its tie rule; the exactness clause; the C entry point's argument check; the command line; the IoU arithmetic; the csv rows."""
import csv
import io
import itertools

import numpy as np
import pytest

from segment_ref import NINF, np_segments, np_segments_prefix, np_segments_video
from temporalalignnet_amd import _lib
from temporalalignnet_amd.eval_align import temporal_iou
from temporalalignnet_amd.infer_align import CSV_COLUMNS, SEGMENT_COLUMNS, parse_args, write_rows


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def all_segmentations(m, V):
    """Every ((s_0, e_0), ..., (s_{m-1}, e_{m-1})) with s_i <= e_i < s_{i+1}, seconds in [0, V)."""
    for cut in itertools.combinations_with_replacement(range(V), 2 * m):
        segs = tuple(zip(cut[0::2], cut[1::2]))
        if all(a[1] < b[0] for a, b in zip(segs, segs[1:])):
            yield segs


def cases():
    rng = np.random.default_rng(0)
    for case in range(400):
        m, V = int(rng.integers(1, 4)), int(rng.integers(1, 8))
        yield case, rng.integers(-3, 4, (m, V)).astype(np.float32)       # integer gains: every sum is exact, ties are common


def test_restatement_is_the_exhaustive_optimum_with_the_tie_rule():
    n_feasible = n_infeasible = n_ties = 0
    for case, g in cases():
        m, V = g.shape
        seg, path = np_segments(g, np.zeros(m, np.float32))
        if m > V:
            assert path == NINF and (seg == -1).all(), case
            assert not list(all_segmentations(m, V))
            n_infeasible += 1
            continue
        n_feasible += 1
        assert (seg[:, 0] <= seg[:, 1]).all() and (seg[:-1, 1] < seg[1:, 0]).all() and seg.min() >= 0 and seg.max() < V, case
        assert sum(g[i, s:e + 1].sum() for i, (s, e) in enumerate(seg)) == path, case
        every = list(all_segmentations(m, V))
        sums = [sum(g[i, s:e + 1].sum() for i, (s, e) in enumerate(segs)) for segs in every]
        assert path == max(sums), case
        # the tie rule: smallest e_{m-1}, then smallest s_{m-1}, then smallest e_{m-2}, ...
        best = [segs for segs, s in zip(every, sums) if s == path]
        n_ties += len(best) > 1
        key = lambda segs: tuple(x for s, e in segs[::-1] for x in (e, s))      # noqa: E731
        assert tuple(map(tuple, seg)) == min(best, key=key), case
    assert (n_feasible, n_infeasible, n_ties) == (348, 52, 105)  # what this generator gives
    assert 4 * n_ties >= n_feasible                              # the tie rule was exercised in at least a quarter of the feasible cases


def test_one_sentence_is_the_maximum_sum_run():
    rng = np.random.default_rng(1)
    for case in range(100):
        V = int(rng.integers(1, 40))
        g = rng.integers(-4, 5, (1, V)).astype(np.float32)
        seg, path = np_segments(g, np.zeros(1, np.float32))
        runs = [(g[0, s:e + 1].sum(), e, s) for s in range(V) for e in range(s, V)]
        best = max(r[0] for r in runs)
        _, e, s = min(r for r in runs if r[0] == best)           # among the best runs: the smallest end, then the smallest start
        assert path == best and tuple(seg[0]) == (s, e), case


def test_bias_and_keep_and_order():
    x = np.array([[5, 5, 1, 0, 0, 0], [0, 0, 0, 4, 5, 4], [9, 9, 9, 9, 9, 9]], np.float32)
    bias = x.max(-1) - np.float32(1.5)
    seg, path = np_segments_video(x, [0, 1, 2], bias, keep=[1, 1, 0])
    assert seg.tolist() == [[0, 1], [3, 5], [-1, -1]] and path == np.float32(3 + 2.5)
    seg, path = np_segments_video(x, [1, 0, 2], bias, keep=[1, 1, 0])          # row 1 first: the two peaks are out of order
    assert (seg[1, 1] < seg[0, 0]) and (seg[2] == -1).all()
    seg, path = np_segments_video(x, [0, 1, 2], bias, keep=[0, 0, 0])
    assert (seg == -1).all() and path == 0
    # a bias above every value: every gain is negative, so every segment is one second; seven rows do not fit six seconds
    seg, path = np_segments_video(np.tile(x, (2, 1)), np.arange(6), np.full(6, 100, np.float32))
    assert (seg[:, 0] == seg[:, 1]).all() and seg[:, 0].tolist() == list(range(6))
    seg, path = np_segments_video(np.tile(x, (3, 1))[:7], np.arange(7), np.full(7, 100, np.float32))
    assert (seg == -1).all() and path == NINF


def test_a_prefix_sum_form_gives_other_bits():
    """The exactness clause is not vacuous: the same optimum written with prefix sums re-associates the adds and differs in f32."""
    rng = np.random.default_rng(2)
    differ = same_on_integers = 0
    for case in range(50):
        m, V = int(rng.integers(1, 6)), int(rng.integers(20, 200))
        x = (rng.standard_normal((m, V)) * 5).astype(np.float32)
        bias = x.max(-1) - np.float32(6)
        _, path = np_segments(x, bias)
        other = np_segments_prefix(x, bias)
        assert abs(float(path) - float(other)) <= 1e-3 * max(1.0, abs(float(path)))          # the same optimum ...
        differ += bits(path) != bits(other)                                                     # ... in other bits
        xi = rng.integers(-3, 4, (m, V)).astype(np.float32)
        same_on_integers += bits(np_segments(xi, np.zeros(m, np.float32))[1]) == bits(np_segments_prefix(xi, np.zeros(m, np.float32)))
    assert differ >= 10 and same_on_integers == 50


def test_segment_decode_is_rejected_without_touching_a_device():
    L = _lib.lib()
    assert "tan_segment_decode" in _lib.declared_symbols()
    assert L.tan_segment_decode(None, None, None, None, 0, None, None, 0, 0, 0, None, None, None, None, None) == -1
    p = 4096                                                     # never dereferenced: nothing is launched
    ok = dict(sim=p, rows=p, order=p, vtab=p, n_videos=1, keep=None, bias=p, n_rows=1, n_acc=1, n_run=1, bp=p, run=p, seg=p, path=p,
              stream=None)
    for name in ("sim", "rows", "order", "vtab", "bias", "bp", "run", "seg", "path"):
        assert L.tan_segment_decode(*dict(ok, **{name: None}).values()) == -1, name
    for name in ("n_videos", "n_rows", "n_acc", "n_run"):
        for bad in (0, -1):
            assert L.tan_segment_decode(*dict(ok, **{name: bad}).values()) == -1, name


def test_cli_parses_segments_and_width():
    base = ["--checkpoint", "c", "--feature-dir", "f", "--asr-json", "a", "--vlen-csv", "v", "--vocab", "x", "--out", "o"]
    a = parse_args(base + ["--decode", "segments", "--width", "2.5"])
    assert a.decode == "segments" and a.width == 2.5
    a = parse_args(base + ["--decode", "segments"])
    assert a.width == 1.0
    assert parse_args(base).decode == "argmax"
    for bad in (["--width", "-1"], ["--width", "nan"], ["--decode", "viterbi"]):
        with pytest.raises(SystemExit) as e:
            parse_args(base + ["--decode", "segments"] + bad)
        assert e.value.code == 2
    from temporalalignnet_amd import infer_align
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="width"):
            next(infer_align.align_corpus(None, [], None, decode="segments", width=bad))


def test_temporal_iou_by_hand():
    # seconds 10..14 are [10, 15); the annotation 11.5 .. 16.2 is [11, 17]: they share [11, 15) = 4 of 5 + 6 - 4 = 7
    assert temporal_iou(10, 14, 11.5, 16.2) == 4 / 7
    assert temporal_iou(3, 3, 3.0, 4.0) == 1.0                   # one second, exactly the annotation
    assert temporal_iou(0, 4, 5.0, 9.0) == 0.0                   # [0, 5) and [5, 9] touch: nothing shared
    assert temporal_iou(0, 9, 2.2, 3.9) == 2 / 10                # the annotation [2, 4] inside the segment
    assert temporal_iou(-1, -1, 2.0, 3.0) == 0.0                 # no segment


def _rows(res, threshold=None):
    buf = io.StringIO(newline="")
    n = write_rows(csv.writer(buf), res, threshold)
    rows = list(csv.reader(io.StringIO(buf.getvalue(), newline="")))
    assert n == len(rows)
    return rows


def test_write_rows_appends_start_and_end():
    assert CSV_COLUMNS == ("vid", "timestamp", "text", "score", "confidence") and SEGMENT_COLUMNS == ("start", "end")
    res = {"vid": "v", "str": ["a", "b", "c", "d"], "timestamp": np.array([30, 10, 20, 5]),
           "score": np.array([0.5, 2.0, 1.0, 9.0], np.float32), "confidence": np.array([0.1, 0.2, 0.3, 0.4], np.float32),
           "covered": np.array([1, 1, 1, 0], bool)}
    plain = _rows(res)
    assert all(len(r) == 5 for r in plain)
    dec = dict(res, segment_start=np.array([28, 9, 15, -1]), segment_end=np.array([33, 12, 22, -1]),
               segmented=np.array([1, 1, 1, 0], bool), path_score=3.5)
    got = _rows(dec)
    assert [r[:5] for r in got] == plain                         # the columns of the plain mode, unchanged
    assert [r[5:] for r in got] == [["28", "33"], ["9", "12"], ["15", "22"]]
    dec_t = dict(res, segment_start=np.array([-1, 9, 15, -1]), segment_end=np.array([-1, 12, 22, -1]),
                 segmented=np.array([0, 1, 1, 0], bool), path_score=2.0)
    got = _rows(dec_t, threshold=0.5)                            # decoded under a threshold: the rows written are the rows decoded
    assert [(r[2], r[5], r[6]) for r in got] == [("b", "9", "12"), ("c", "15", "22")]
