"""Order-preserving timestamps on the GPU: tan_monotonic_decode against its numpy restatement (test_monotonic_cpu.np_decode, pinned
there against exhaustive enumeration) -- seconds and path score bit for bit, no tolerance anywhere -- then through align_corpus,
the HTM-Align harness and the command line."""
import csv
import io

import numpy as np
import pytest
import torch

from temporalalignnet_amd import ops, synth
from temporalalignnet_amd.infer_align import align_corpus
from test_infer_align_gpu import _g6_embed, _run_cli, cli_setup  # noqa: F401  (cli_setup: a fixture)
from test_monotonic_cpu import np_decode_video

pytestmark = pytest.mark.gpu

# the wave (64 lanes x 4 seconds = 256), the thread (4), the tile (1024 seconds) and several tiles with a carry
VLENS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1200, 5000)
MS = (1, 2, 37)
MASKED = np.float32(-6e4)


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def gpu_decode(videos, orders=None, keep=None, video_perm=None):
    """videos: list of [m, V] f32; orders: per video a permutation of its rows (decode order), default 0..m-1; keep: per video
    bool [m] or None; video_perm: the order in which the videos' runs appear in `order`.  One launch.  -> [(ts [m], score)]"""
    n = len(videos)
    k_off = np.concatenate([[0], np.cumsum([len(x) for x in videos])])
    a_off = np.concatenate([[0], np.cumsum([x.size for x in videos])])
    v_off = np.concatenate([[0], np.cumsum([x.shape[1] for x in videos])])
    rows = np.concatenate([np.stack([a_off[i] + np.arange(len(x)) * x.shape[1], np.full(len(x), x.shape[1])], 1)
                           for i, x in enumerate(videos)]).astype(np.int32)
    orders = [np.arange(len(x)) for x in videos] if orders is None else orders
    video_perm = range(n) if video_perm is None else video_perm
    order, vtab, at = [], np.zeros((n, 3), np.int32), 0
    for i in video_perm:
        order.append(k_off[i] + np.asarray(orders[i]))
        vtab[i] = (at, len(videos[i]), v_off[i])
        at += len(videos[i])
    dev = "cuda"
    sim = torch.from_numpy(np.concatenate([x.ravel() for x in videos]).astype(np.float32)).to(dev)
    keep_d = None if keep is None else torch.from_numpy(np.concatenate(keep).astype(bool)).to(dev)
    # scratch and outputs start as garbage: nothing relies on their contents
    bp = torch.full((sim.numel(),), -7, dtype=torch.int32, device=dev)
    run = torch.full((int(v_off[-1]),), float("nan"), device=dev)
    ts = torch.full((int(k_off[-1]),), -7, dtype=torch.int32, device=dev)
    path = torch.full((n,), float("nan"), device=dev)
    ops.monotonic_decode(sim, torch.from_numpy(rows).to(dev), torch.from_numpy(np.concatenate(order).astype(np.int32)).to(dev),
                         torch.from_numpy(vtab).to(dev), keep_d, bp, run, ts, path)
    ts, path = ts.cpu().numpy().astype(np.int64), path.cpu().numpy()
    return [(ts[k_off[i]:k_off[i + 1]], path[i]) for i in range(n)]


def check(videos, orders=None, keep=None, video_perm=None):
    got = gpu_decode(videos, orders, keep, video_perm)
    moved = 0
    for i, (x, (ts, score)) in enumerate(zip(videos, got)):
        order = np.arange(len(x)) if orders is None else orders[i]
        kp = np.ones(len(x), bool) if keep is None else keep[i]
        want_ts, want_score = np_decode_video(x, order, kp)
        tag = f"video {i}: m = {len(x)}, vlen = {x.shape[1]}"
        assert (ts == want_ts).all(), tag
        assert bits(score) == bits(want_score), tag
        assert (ts[~kp] == -1).all() and (ts[kp] >= 0).all() and (ts < x.shape[1]).all(), tag
        in_order = ts[order][kp[order]]
        assert (np.diff(in_order) >= 0).all(), tag
        moved += bool((ts[kp] != x.argmax(-1)[kp]).any())
    return got, moved


def values(kind, rng, m, V):
    if kind == "ties":
        return rng.integers(0, 4, (m, V)).astype(np.float32)              # ties everywhere, every add exact
    return (rng.standard_normal((m, V)) * 5).astype(np.float32)


@pytest.fixture(scope="module", params=["ties", "normal"])
def grid(request):
    rng = np.random.default_rng(7)
    return [values(request.param, rng, m, V) for V in VLENS for m in MS]


def test_time_edges_and_ties(grid):
    """Every vlen edge x m in {1, 2, 37} in one launch; the decode is not the independent arg-max (non-vacuity, asserted)."""
    _, moved = check(grid)
    assert moved >= 1
    big = [x for x in grid if x.shape == (37, 5000)][0]
    ts, _ = np_decode_video(big, np.arange(37))
    assert (ts != big.argmax(-1)).sum() >= 10


def test_blocks_of_masked_seconds():
    rng = np.random.default_rng(8)
    videos = []
    for V in (65, 300, 1200, 2100):
        x = values("normal", rng, 12, V)
        for r in range(12):                                           # no window covered the left part of some rows, the right of others
            cut = int(rng.integers(1, V))
            if r % 3 == 0:
                x[r, :cut] = MASKED
            elif r % 3 == 1:
                x[r, cut:] = MASKED
        videos.append(x)
    # the only monotone path runs through uncovered cells: the first row is covered late only, the second early only
    x = values("normal", rng, 2, 1500)
    x[0, :1100], x[1, 1000:] = MASKED, MASKED
    videos.append(x)
    got, moved = check(videos)
    assert moved >= 1
    assert got[-1][1] < -5e4


@pytest.mark.parametrize("use_keep", [True, False])
def test_order_and_keep(grid, use_keep):
    rng = np.random.default_rng(9)
    videos = [x for x in grid if x.shape[1] in (2, 65, 257, 1025, 1200)]
    orders = [rng.permutation(len(x)) for x in videos]
    assert any((o != np.arange(len(o))).any() for o in orders)
    keep = None
    if use_keep:
        keep = [rng.random(len(x)) >= 1 / 3 for x in videos]
        dead = [i for i, x in enumerate(videos) if len(x) == 37][1]
        keep[dead][:] = False                                         # one video with every row dropped
        assert any(k.any() and not k.all() for k in keep)
    got, moved = check(videos, orders, keep, video_perm=rng.permutation(len(videos)))
    assert moved >= 1
    if use_keep:
        assert (got[dead][0] == -1).all() and bits(got[dead][1]) == bits(0.0)


def test_rows_already_in_order_come_back_unchanged():
    rng = np.random.default_rng(10)
    videos = []
    for m, V in ((5, 64), (37, 257), (37, 1200), (20, 3000)):
        x = rng.integers(0, 3, (m, V)).astype(np.float32)
        peaks = np.sort(rng.integers(0, V, m))
        x[np.arange(m), peaks] = 5
        assert (x.argmax(-1) == peaks).all()
        videos.append(x)
    got, moved = check(videos)
    assert moved == 0
    for x, (ts, score) in zip(videos, got):
        assert (ts == x.argmax(-1)).all() and score == 5 * len(x)


# ------------------------------------------------------------------------------------------------------------ through align_corpus
def _model(dtype, head):
    from temporalalignnet_amd.tan_model import TemporalAligner
    m = TemporalAligner(1, 3, use_alignability_head=int(head), random_pos_start=0, language_model=None, compute_dtype=dtype)
    sd = m.state_dict()
    for k, v in synth.make_params(108, 1, 3, head).items():
        sd[k].copy_(torch.from_numpy(v))
    return m.cuda().eval()


def _shuffled_videos():
    """synth.align_videos with each video's sentences permuted, so that ASR start order is not sentence order, and two equal starts."""
    rng = np.random.default_rng(11)
    out = []
    for v in synth.align_videos():
        p = rng.permutation(len(v["str"]))
        w = dict(v, start=np.asarray(v["start"], dtype=np.float64)[p], end=np.asarray(v["end"], dtype=np.float64)[p],
                 aligned=np.asarray(v["aligned"])[p], str=[v["str"][k] for k in p], emb=np.asarray(v["emb"])[p])
        w["start"][3] = w["start"][9]
        out.append(w)
    return out


def _order(v):
    return np.argsort(np.asarray(v["start"], dtype=np.float64), kind="stable")


@pytest.mark.parametrize("windows_per_pass", [256, 5])
@pytest.mark.parametrize("head", [True, False])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_align_corpus_decodes_its_own_stitched_rows(dtype, head, windows_per_pass):
    m = _model(dtype, head)
    videos = _shuffled_videos()
    embed = _g6_embed(videos)
    kw = dict(windows_per_pass=windows_per_pass, return_sim=True)
    plain = list(align_corpus(m, videos, embed, **kw))
    thr = float(np.median(np.concatenate([r["score"] for r in plain])))
    for keep_threshold in (None, thr):
        dec = list(align_corpus(m, videos, embed, decode="monotonic", keep_threshold=keep_threshold, **kw))
        moved = 0
        for v, p, d in zip(videos, plain, dec):
            assert set(p) == {"vid", "str", "timestamp", "confidence", "score", "covered", "sim"}
            assert set(d) == set(p) | {"ordered_timestamp", "ordered", "path_score"}
            for key in ("timestamp", "confidence", "score", "covered", "sim"):
                assert p[key].dtype == d[key].dtype and p[key].tobytes() == d[key].tobytes(), key
            keep = d["covered"] if keep_threshold is None else d["covered"] & (d["score"].astype(np.float64) > keep_threshold)
            want_ts, want_score = np_decode_video(d["sim"], _order(v), keep)
            assert d["ordered_timestamp"].dtype == np.int64 and (d["ordered_timestamp"] == want_ts).all()
            assert d["ordered"].dtype == np.bool_ and (d["ordered"] == keep).all()
            assert isinstance(d["path_score"], float) and bits(d["path_score"]) == bits(want_score)
            moved += bool((d["ordered_timestamp"][keep] != d["timestamp"][keep]).any())
        assert moved >= 1
        if keep_threshold is not None:
            assert any(not r["ordered"].all() for r in dec) and any(r["ordered"].any() for r in dec)


def test_align_corpus_without_sentences_has_the_same_keys():
    m = _model("fp32", False)
    v = {"vid": "empty", "start": np.zeros(0), "end": np.zeros(0), "str": [], "video": np.zeros((40, 1024), np.float32)}
    (r,) = list(align_corpus(m, [v], lambda s: torch.zeros(0, 512, device="cuda"), decode="monotonic"))
    assert r["ordered_timestamp"].shape == (0,) and r["ordered_timestamp"].dtype == np.int64
    assert r["ordered"].shape == (0,) and r["ordered"].dtype == np.bool_ and r["path_score"] == 0.0
    (r,) = list(align_corpus(m, [v], lambda s: torch.zeros(0, 512, device="cuda")))
    assert set(r) == {"vid", "str", "timestamp", "confidence", "score", "covered"}


# ----------------------------------------------------------------------------------------------------------- the HTM-Align harness
def test_alignment_htm_decodes_the_aligned_sentences(golden):
    from temporalalignnet_amd.eval_align import make_batched_sim_fn, make_sim_fn, test_alignment_htm
    g = golden("g6_eval_harness")
    m = _model("fp32", True)
    videos = synth.align_videos()
    embed = _g6_embed(videos)
    batched = make_batched_sim_fn(m, embed)
    metric, pv = test_alignment_htm(None, videos, return_per_video=True, batched_sim=batched)
    assert metric["Recall"] == pytest.approx(float(g["Recall"]), abs=1e-12)           # without decode: the G6 numbers
    assert metric["AUC"] == pytest.approx(float(g["AUC"]), abs=1e-9)
    for i, h in enumerate(pv):
        assert (h["argmax"].numpy() == g[f"v{i}/argmax"]).all()
    for method, fn in (("overlap-seq", None), ("global", make_sim_fn(m, embed))):
        base, pv0 = test_alignment_htm(fn, videos, method=method, return_per_video=True, batched_sim=batched)
        dec, pv1 = test_alignment_htm(fn, videos, method=method, return_per_video=True, batched_sim=batched, decode="monotonic")
        assert dec["AUC"] == base["AUC"]
        recall, moved = [], 0
        for v, h0, h1 in zip(videos, pv0, pv1):
            al = np.asarray(v["aligned"]).astype(bool)
            assert torch.equal(h0["sim"], h1["sim"])
            want, _ = np_decode_video(h1["sim"].numpy(), _order(v), al)
            assert (h1["argmax"].numpy() == want[al]).all()
            moved += bool((h1["argmax"] != h0["argmax"]).any())
            recall += [np.floor(s) <= t <= np.ceil(e) for s, e, t in zip(np.asarray(v["start"])[al], np.asarray(v["end"])[al], want[al])]
        assert dec["Recall"] == float(np.mean(recall))
        assert moved >= 1, method


# ---------------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_decode_monotonic(cli_setup):  # noqa: F811
    from temporalalignnet_amd import infer_align
    from temporalalignnet_amd.word2vec_model import Word2VecTokenizer
    tmp, paths, args = cli_setup
    rows = _run_cli(args + ["--decode", "monotonic"], str(tmp / "mono.csv"))
    vocab = np.load(str(tmp / "s3d_dict.npy"))
    model = infer_align.build_aligner(args[1], vocab, "init", "bf16")
    embed = infer_align.make_embed_text(model, Word2VecTokenizer(max_words=32, vocab=vocab))
    corpus = list(infer_align.read_corpus(paths["features"], paths["asr"], paths["vlen"]))
    buf, plain = io.StringIO(newline=""), io.StringIO(newline="")
    n_checked = moved = 0
    results = list(align_corpus(model, corpus, embed, decode="monotonic"))
    for it, r in zip(corpus, results):
        assert it["vid"] == r["vid"]
        infer_align.write_rows(csv.writer(buf), r)
        infer_align.write_rows(csv.writer(plain), {k: r[k] for k in ("vid", "str", "timestamp", "confidence", "score", "covered")})
        assert (r["ordered"] == r["covered"]).all()
    mine = list(csv.reader(io.StringIO(buf.getvalue(), newline="")))
    assert mine == rows and len(rows) == sum(int(r["covered"].sum()) for r in results)
    # per video, the written timestamps are non-decreasing in ASR start order
    at = 0
    for it, r in zip(corpus, results):
        n = int(r["covered"].sum())
        stamps = np.full(len(r["str"]), -1)
        stamps[r["covered"]] = [int(row[1]) for row in rows[at:at + n]]
        assert {row[0] for row in rows[at:at + n]} <= {it["vid"]}
        at += n
        in_order = stamps[_order(it)]
        in_order = in_order[in_order >= 0]
        assert (np.diff(in_order) >= 0).all(), it["vid"]
        n_checked += len(in_order) > 1
    assert n_checked >= 3
    # against the arg-max rows: the same rows and columns, another timestamp somewhere
    argmax_rows = list(csv.reader(io.StringIO(plain.getvalue(), newline="")))
    assert [r[:1] + r[2:] for r in argmax_rows] == [r[:1] + r[2:] for r in rows]
    assert [r[1] for r in argmax_rows] != [r[1] for r in rows]
