"""Aligned intervals on the GPU: tan_segment_decode against its numpy restatement (segment_ref.py, pinned against exhaustive
enumeration in test_segments_cpu.py) -- segments and path score bit for bit, no tolerance anywhere -- then through align_corpus, the
HTM-Align harness and the command line."""
import csv
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from segment_ref import NINF, np_segments_video
from temporalalignnet_amd import ops, synth
from temporalalignnet_amd.eval_align import temporal_iou
from temporalalignnet_amd.infer_align import align_corpus
from test_infer_align_gpu import _g6_embed, cli_setup  # noqa: F401  (cli_setup: a fixture)
from test_monotonic_cpu import np_decode_video
from test_monotonic_gpu import _model, _order, _shuffled_videos

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# seconds: the staged tile (32) and multiples of it around the wave width, one second, many tiles
VLENS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1025)
# sentences: the wave (64), the block of 256 sentences and the hand-over of a G row to the next block
MS = (1, 2, 63, 64, 65, 255, 256, 257, 300)
MASKED = np.float32(-6e4)
GUARD = 64


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def guarded(n, fill, dtype):
    """A device buffer of n elements between two guard bands: (the whole buffer, the view in the middle)."""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def launch(sim, rows, order, vtab, keep, bias, n_run):
    """One launch over host tables as they are.  Scratch and outputs start as garbage between guard bands; the launch runs twice
    (once more over what the first left) and must give the same bits.  -> (seg [n_rows, 2] int64, path [n_videos] f32)"""
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()      # noqa: E731
    sim_d, bias_d = dev(sim, np.float32), dev(bias, np.float32)
    rows_d, order_d, vtab_d = dev(rows, np.int32), dev(order, np.int32), dev(vtab, np.int32)
    keep_d = None if keep is None else dev(keep, bool)
    n_rows, n_videos = len(rows), len(vtab)
    bufs = {"bp": guarded(2 * sim_d.numel(), -7, torch.int32), "run": guarded(n_run, float("nan"), torch.float32),
            "seg": guarded(2 * n_rows, -7, torch.int32), "path": guarded(n_videos, float("nan"), torch.float32)}
    out = []
    for rep in range(2):
        ops.segment_decode(sim_d, rows_d, order_d, vtab_d, keep_d, bias_d, bufs["bp"][1], bufs["run"][1],
                           bufs["seg"][1].view(n_rows, 2), bufs["path"][1])
        out.append((bufs["seg"][1].view(n_rows, 2).cpu().numpy().astype(np.int64), bufs["path"][1].cpu().numpy()))
    assert (out[0][0] == out[1][0]).all() and (bits(out[0][1]) == bits(out[1][1])).all()
    for name, (whole, _) in bufs.items():
        for band in (whole[:GUARD], whole[-GUARD:]):
            intact = band == -7 if whole.dtype == torch.int32 else band.isnan()
            assert bool(intact.all()), name
    return out[0]


def tables(videos, orders=None, video_perm=None):
    n = len(videos)
    k_off = np.concatenate([[0], np.cumsum([len(x) for x in videos])])
    a_off = np.concatenate([[0], np.cumsum([x.size for x in videos])])
    v_off = np.concatenate([[0], np.cumsum([x.shape[1] for x in videos])])
    rows = np.concatenate([np.stack([a_off[i] + np.arange(len(x)) * x.shape[1], np.full(len(x), x.shape[1])], 1)
                           for i, x in enumerate(videos)]).astype(np.int32)
    orders = [np.arange(len(x)) for x in videos] if orders is None else orders
    order, vtab, at = [], np.zeros((n, 3), np.int32), 0
    for i in (range(n) if video_perm is None else video_perm):
        order.append(k_off[i] + np.asarray(orders[i]))
        vtab[i] = (at, len(videos[i]), v_off[i])
        at += len(videos[i])
    return rows, np.concatenate(order).astype(np.int32), vtab, k_off, int(v_off[-1])


def check(videos, biases, orders=None, keep=None, video_perm=None):
    """videos: list of [m, V] f32; biases: per video [m] f32; orders: per video a permutation of its rows (decode order); keep: per
    video bool [m] or None; video_perm: the order in which the videos' runs appear in `order`.  One launch against the restatement."""
    rows, order, vtab, k_off, n_run = tables(videos, orders, video_perm)
    seg, path = launch(np.concatenate([x.ravel() for x in videos]), rows, order, vtab, None if keep is None else np.concatenate(keep),
                       np.concatenate(biases), n_run)
    got = []
    for i, x in enumerate(videos):
        o = np.arange(len(x)) if orders is None else orders[i]
        kp = np.ones(len(x), bool) if keep is None else keep[i]
        want_seg, want_path = np_segments_video(x, o, biases[i], kp)
        s, tag = seg[k_off[i]:k_off[i + 1]], f"video {i}: m = {len(x)} ({int(kp.sum())} kept), vlen = {x.shape[1]}"
        assert (s == want_seg).all(), tag
        assert bits(path[i]) == bits(want_path), tag
        assert (s[~kp] == -1).all() and (s < x.shape[1]).all(), tag
        if kp.sum() > x.shape[1]:
            assert path[i] == NINF and (s == -1).all(), tag
        elif kp.any():
            d = s[o][kp[o]]                                       # in decode order: s <= e, e < the next s
            assert (d >= 0).all() and (d[:, 0] <= d[:, 1]).all() and (d[:-1, 1] < d[1:, 0]).all(), tag
        got.append((s, path[i]))
    return got


def values(kind, rng, m, V):
    """-> (rows, bias): 'ties' has integer gains in -2 .. 2 (every sum exact, ties everywhere), 'normal' 5 * randn under the bias
    align_corpus uses, the row's maximum minus a width."""
    if kind == "ties":
        return rng.integers(0, 5, (m, V)).astype(np.float32), np.full(m, 2, np.float32)
    x = (rng.standard_normal((m, V)) * 5).astype(np.float32)
    return x, x.max(-1) - rng.uniform(2, 12, m).astype(np.float32)


@pytest.mark.parametrize("kind", ["ties", "normal"])
def test_every_time_and_sentence_edge_in_one_launch(kind):
    """VLENS x MS and m == V, V + 1, 3 V: the tile, wave and block edges; whatever has more sentences than seconds is -inf."""
    rng = np.random.default_rng(7)
    shapes = [(m, V) for V in VLENS for m in MS] + [(m, V) for V in (2, 33, 65, 257) for m in (V, V + 1, 3 * V)]
    # three blocks: the middle one both reads the G row the block before it left in `run` and overwrites it for the block after it
    shapes += [(600, 1025), (513, 520)]
    vb = [values(kind, rng, m, V) for m, V in shapes]
    got = check([x for x, _ in vb], [b for _, b in vb])
    n_inf = sum(m > V for m, V in shapes)
    assert n_inf >= 20 and sum(p == NINF for _, p in got) == n_inf
    # non-vacuity: segments longer than a second, gaps between segments, and several blocks in one video
    seg = got[shapes.index((300, 1025))][0]
    assert (seg[:, 1] > seg[:, 0]).any() and (seg[1:, 0] > seg[:-1, 1] + 1).any()


def test_orders_keeps_and_shuffled_videos():
    rng = np.random.default_rng(9)
    shapes = [(5, 40), (70, 33), (300, 400), (37, 65), (64, 64), (20, 9), (257, 300), (12, 128), (30, 31)]
    vb = [values("normal" if i % 2 else "ties", rng, m, V) for i, (m, V) in enumerate(shapes)]
    videos, biases = [x for x, _ in vb], [b for _, b in vb]
    orders = [rng.permutation(len(x)) for x in videos]
    keep = [rng.random(len(x)) >= 1 / 3 for x in videos]
    keep[0][:] = False                                            # none kept: path 0
    keep[1][:] = True
    keep[1][orders[1][:40]] = False                               # 70 rows over 33 seconds: infeasible until 40 rows are dropped
    keep[2][:] = True
    keep[2][orders[2][0]] = keep[2][orders[2][-1]] = False        # the first and the last row of the decode order dropped
    keep[3][:] = True
    keep[3][orders[3][::2]] = False                               # alternate rows dropped
    keep[5][:] = True                                             # 20 rows over 9 seconds stay infeasible
    got = check(videos, biases, orders, keep, video_perm=rng.permutation(len(videos)))
    assert (got[0][0] == -1).all() and bits(got[0][1]) == bits(0.0)
    assert np.isfinite(got[1][1]) and (got[1][0][keep[1]] >= 0).all()
    assert got[5][1] == NINF
    check(videos, biases, orders, None, video_perm=rng.permutation(len(videos)))          # keep == NULL
    assert check(videos[1:2], biases[1:2], orders[1:2])[0][1] == NINF                      # the same video with every row kept


def test_blocks_of_masked_seconds():
    rng = np.random.default_rng(8)
    videos, biases = [], []
    for m, V in ((12, 65), (12, 300), (70, 1200)):
        x, b = values("normal", rng, m, V)
        for r in range(m):                                            # no window covered the left part of some rows, the right of others
            cut = int(rng.integers(1, V))
            if r % 3 == 0:
                x[r, :cut] = MASKED
            elif r % 3 == 1:
                x[r, cut:] = MASKED
        videos.append(x)
        biases.append(b)
    # the only ordered segmentation runs through uncovered cells: the first row is covered late only, the second early only
    x, b = values("normal", rng, 2, 500)
    x[0, :400], x[1, 300:] = MASKED, MASKED
    got = check(videos + [x], biases + [b])
    assert got[-1][1] < -5e4


def test_a_bias_above_and_below_every_value():
    rng = np.random.default_rng(10)
    shapes = [(5, 40), (64, 64), (257, 300), (100, 1025)]
    videos = [values("normal", rng, m, V)[0] for m, V in shapes]
    for seg, _ in check(videos, [np.full(len(x), 1e3, np.float32) for x in videos]):
        assert (seg[:, 0] == seg[:, 1]).all() and (np.diff(seg[:, 0]) > 0).all()          # every gain negative: one second each
    for (seg, _), x in zip(check(videos, [np.full(len(x), -1e3, np.float32) for x in videos]), videos):
        assert seg[0, 0] == 0 and seg[-1, 1] == x.shape[1] - 1 and (seg[1:, 0] == seg[:-1, 1] + 1).all()      # every gain positive


def test_broken_table_entries_take_no_part():
    rng = np.random.default_rng(12)
    shapes = [(6, 50), (9, 70), (4, 33), (5, 20), (3, 45)]
    vb = [values("normal", rng, m, V) for m, V in shapes]
    videos, biases = [x for x, _ in vb], [b for _, b in vb]
    rows, order, vtab, k_off, n_run = tables(videos)
    sim = np.concatenate([x.ravel() for x in videos])
    keep = [np.ones(len(x), bool) for x in videos]
    # video 0 (vlen 50): its sentence 2 is replaced by a row of another vlen, its sentence 4 by a negative and 5 by a too large row
    # id.  The foreign row is kept (keep == NULL) and its 50 seconds would lie inside sim, so only the vlen check holds it back; it
    # is a row of video 4 (vlen 45), whose workgroup returns before it writes anything: video 0 alone writes its (-1, -1).
    foreign = k_off[4] + 1
    assert rows[foreign, 1] == 45 and rows[foreign, 0] + 50 <= sim.size
    order[k_off[0] + 2], order[k_off[0] + 4], order[k_off[0] + 5] = foreign, -3, len(rows) + 7
    keep[0][[2, 4, 5]] = False
    # video 1: row offsets outside [0, n_acc - vlen]
    rows[k_off[1] + 1, 0], rows[k_off[1] + 6, 0] = -5, sim.size - 69
    keep[1][[1, 6]] = False
    vtab[2, 2] = n_run - 32                                       # video 2: its run row would end outside n_run
    vtab[3, 2] = -1                                               # video 3: a negative run offset
    vtab[4, 1] = len(rows)                                        # video 4: first + count beyond n_rows
    seg, path = launch(sim, rows, order, vtab, None, np.concatenate(biases), n_run)
    for i in (0, 1):                                              # the restatement over the rows that remain, bit for bit
        want_seg, want_path = np_segments_video(videos[i], np.arange(len(videos[i])), biases[i], keep[i])
        got = seg[k_off[i]:k_off[i + 1]]
        assert (got[keep[i]] == want_seg[keep[i]]).all() and bits(path[i]) == bits(want_path), i
    assert (seg[k_off[0] + 2] == -7).all() and (seg[k_off[0] + 4:k_off[0] + 6] == -7).all()     # listed by no video: not written
    assert (seg[foreign] == -1).all()                             # listed by video 0, of another vlen: no segment
    assert (seg[k_off[1] + 1] == -1).all() and (seg[k_off[1] + 6] == -1).all()
    for i in (2, 3):
        assert (seg[k_off[i]:k_off[i + 1]] == -1).all() and bits(path[i]) == bits(0.0), i
    assert (seg[[k_off[4], k_off[4] + 2]] == -7).all() and bits(path[4]) == bits(0.0)            # video 4 itself wrote nothing


# ------------------------------------------------------------------------------------------------------------ through align_corpus
def _bias(r, width):
    return r["sim"][np.arange(len(r["timestamp"])), r["timestamp"]] - np.float32(width)


@pytest.mark.parametrize("dtype,head", [("fp32", True), ("bf16", False)])
def test_align_corpus_segments_its_own_stitched_rows(dtype, head):
    """Every run against the restatement over its own returned sim and against the plain run with the same `windows_per_pass`.  In
    fp32 the stitched rows do not depend on how the windows are cut into passes, so there the two `windows_per_pass` values must
    agree in every bit as well; the bf16 stacks' bits depend on the batch they run in, with or without a decode."""
    m = _model(dtype, head)
    videos = _shuffled_videos()
    embed = _g6_embed(videos)
    plain = {wpp: list(align_corpus(m, videos, embed, windows_per_pass=wpp, return_sim=True)) for wpp in (256, 5)}
    if dtype == "bf16":                               # the reason for the exemption, shown: the plain rows differ with the pass cut
        assert any(p["sim"].tobytes() != p5["sim"].tobytes() for p, p5 in zip(plain[256], plain[5]))
    mono = list(align_corpus(m, videos, embed, return_sim=True, decode="monotonic"))
    thr = float(np.median(np.concatenate([r["score"] for r in plain[256]])))
    # the last width is above every spread of a covered row: every covered second pays, so segments run over many seconds
    for keep_threshold, width in ((None, 1.0), (thr, 1.0), (None, 1e3)):
        runs = {wpp: list(align_corpus(m, videos, embed, decode="segments", keep_threshold=keep_threshold, width=width,
                                       windows_per_pass=wpp, return_sim=True)) for wpp in (256, 5)}
        long_ones = 0
        for wpp in (256, 5):
            for v, p, d in zip(videos, plain[wpp], runs[wpp]):
                assert set(p) == {"vid", "str", "timestamp", "confidence", "score", "covered", "sim"}
                assert set(d) == set(p) | {"segment_start", "segment_end", "segmented", "path_score"}
                for key in ("timestamp", "confidence", "score", "covered", "sim"):       # what there is without `decode`: unchanged
                    assert p[key].dtype == d[key].dtype and p[key].tobytes() == d[key].tobytes(), key
                keep = d["covered"] if keep_threshold is None else d["covered"] & (d["score"].astype(np.float64) > keep_threshold)
                want_seg, want_path = np_segments_video(d["sim"], _order(v), _bias(d, width), keep)
                assert d["segment_start"].dtype == d["segment_end"].dtype == np.int64
                assert (d["segment_start"] == want_seg[:, 0]).all() and (d["segment_end"] == want_seg[:, 1]).all()
                assert d["segmented"].dtype == np.bool_ and (d["segmented"] == keep).all()
                assert isinstance(d["path_score"], float) and bits(d["path_score"]) == bits(want_path)
                long_ones += int((d["segment_end"] > d["segment_start"]).sum())
        if dtype == "fp32":
            for d, d5 in zip(runs[256], runs[5]):
                for key in ("sim", "segment_start", "segment_end", "segmented"):
                    assert d[key].tobytes() == d5[key].tobytes(), key
                assert bits(d["path_score"]) == bits(d5["path_score"])
        assert long_ones >= 1 or width < 1e3
        if keep_threshold is not None:
            assert any(not r["segmented"].all() for r in runs[256]) and any(r["segmented"].any() for r in runs[256])
    for v, p, mo in zip(videos, plain[256], mono):                                       # the monotonic decode, in the same run
        assert set(mo) == set(p) | {"ordered_timestamp", "ordered", "path_score"}
        for key in ("timestamp", "confidence", "score", "covered", "sim"):
            assert p[key].tobytes() == mo[key].tobytes(), key
        want_ts, want_score = np_decode_video(mo["sim"], _order(v), mo["covered"])
        assert (mo["ordered_timestamp"] == want_ts).all() and bits(mo["path_score"]) == bits(want_score)


def test_align_corpus_segments_without_sentences_and_bad_arguments():
    m = _model("fp32", False)
    v = {"vid": "empty", "start": np.zeros(0), "end": np.zeros(0), "str": [], "video": np.zeros((40, 1024), np.float32)}
    (r,) = list(align_corpus(m, [v], lambda s: torch.zeros(0, 512, device="cuda"), decode="segments"))
    for key in ("segment_start", "segment_end"):
        assert r[key].shape == (0,) and r[key].dtype == np.int64
    assert r["segmented"].shape == (0,) and r["segmented"].dtype == np.bool_ and r["path_score"] == 0.0
    with pytest.raises(ValueError, match="width"):
        next(align_corpus(m, [v], None, decode="segments", width=-0.5))
    with pytest.raises(ValueError, match="decode"):
        next(align_corpus(m, [v], None, decode="viterbi"))


# ----------------------------------------------------------------------------------------------------------- the HTM-Align harness
def test_alignment_htm_segments_the_aligned_sentences():
    from temporalalignnet_amd.eval_align import make_batched_sim_fn, make_sim_fn, test_alignment_htm
    m = _model("fp32", True)
    videos = synth.align_videos()
    embed = _g6_embed(videos)
    batched, fn = make_batched_sim_fn(m, embed), make_sim_fn(m, embed)
    for method, bs, width in (("overlap-seq", batched, 1.0), ("overlap-seq", None, 1.0), ("global", None, 3.0)):
        base, pv0 = test_alignment_htm(fn, videos, method=method, return_per_video=True, batched_sim=bs)
        dec, pv1 = test_alignment_htm(fn, videos, method=method, return_per_video=True, batched_sim=bs, decode="segments", width=width)
        assert set(base) == {"Recall", "AUC"} and set(dec) == {"Recall", "AUC", "IoU"} and dec["AUC"] == base["AUC"]
        recall, ious = [], []
        for v, h0, h1 in zip(videos, pv0, pv1):
            al = np.asarray(v["aligned"]).astype(bool)
            assert torch.equal(h0["sim"], h1["sim"]) and "segments" not in h0
            sim = h1["sim"].numpy()
            want, _ = np_segments_video(sim, _order(v), sim.max(-1) - np.float32(width), al)
            assert h1["segments"].dtype == torch.int64 and (h1["segments"].numpy() == want[al]).all()
            best = [s + int(np.argmax(sim[k, s:e + 1])) for k, (s, e) in zip(np.flatnonzero(al), want[al])]
            assert h1["argmax"].tolist() == best
            for (s, e), t, a, b in zip(want[al].tolist(), best, np.asarray(v["start"])[al], np.asarray(v["end"])[al]):
                recall.append(np.floor(a) <= t <= np.ceil(b))
                ious.append(temporal_iou(s, e, a, b))
        assert dec["Recall"] == float(np.mean(recall)) and dec["IoU"] == float(np.mean(ious))
        assert 0.0 <= dec["IoU"] <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_decode_segments(cli_setup):  # noqa: F811
    from temporalalignnet_amd import infer_align
    from temporalalignnet_amd.word2vec_model import Word2VecTokenizer
    tmp, paths, args = cli_setup
    out = str(tmp / "segments.csv")
    p = subprocess.run([sys.executable, "-m", "temporalalignnet_amd.infer_align", *args, "--out", out, "--decode", "segments",
                        "--width", "2.0"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["vid", "timestamp", "text", "score", "confidence", "start", "end"]
    rows = rows[1:]
    vocab = np.load(str(tmp / "s3d_dict.npy"))
    model = infer_align.build_aligner(args[1], vocab, "init", "bf16")
    embed = infer_align.make_embed_text(model, Word2VecTokenizer(max_words=32, vocab=vocab))
    corpus = list(infer_align.read_corpus(paths["features"], paths["asr"], paths["vlen"]))
    results = list(align_corpus(model, corpus, embed, decode="segments", width=2.0, return_sim=True))
    buf, plain = io.StringIO(newline=""), io.StringIO(newline="")
    for it, r in zip(corpus, results):
        infer_align.write_rows(csv.writer(buf), r)
        infer_align.write_rows(csv.writer(plain), {k: r[k] for k in ("vid", "str", "timestamp", "confidence", "score", "covered")})
        want, _ = np_segments_video(r["sim"], _order(it), _bias(r, 2.0), r["covered"])
        assert (r["segment_start"] == want[:, 0]).all() and (r["segment_end"] == want[:, 1]).all()
    assert list(csv.reader(io.StringIO(buf.getvalue(), newline=""))) == rows
    # the plain mode's rows and columns, and two more columns: per video ordered, disjoint inclusive seconds
    assert [r[:5] for r in rows] == list(csv.reader(io.StringIO(plain.getvalue(), newline="")))
    at = n_checked = 0
    for it, r in zip(corpus, results):
        n = int(r["covered"].sum())
        se = np.full((len(r["str"]), 2), -1)
        se[r["covered"]] = [[int(row[5]), int(row[6])] for row in rows[at:at + n]]
        at += n
        d = se[_order(it)]
        d = d[d[:, 0] >= 0]
        assert (d[:, 0] <= d[:, 1]).all() and (d[:-1, 1] < d[1:, 0]).all() and (d < it["vlen"]).all(), it["vid"]
        n_checked += len(d) > 1
    assert at == len(rows) and n_checked >= 3
