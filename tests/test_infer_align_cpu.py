"""Corpus auto-alignment, host side: the window planner against the CPU oracle's evaluation loop, sharding, the corpus reader and
the HTM-AA csv (no GPU)."""
import csv
import io
import json
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import eval_ref
from temporalalignnet_amd import synth
from temporalalignnet_amd.eval_align import plan_windows
from temporalalignnet_amd.infer_align import CSV_COLUMNS, read_corpus, write_rows


def oracle_windows(start, end, vlen, aligned, seq_len=64):
    """The windows oracle/eval_ref.test_alignment forms, recorded through its model callback: frame features carry their own
    time index and sentences their index, the callback returns zeros of the shapes the loop reads."""
    K = len(start)
    seen = []

    def cb(video, text_str, interpolate_from=None, abs_text_pos=None):
        s0, t, k = int(video[0, 0, 0]), video.shape[1], len(text_str)
        idx = [int(s[1:]) for s in text_str]
        assert idx == list(range(idx[0], idx[0] + k))           # a window holds a contiguous range of sentences
        seen.append((s0, s0 + t, idx[0], idx[0] + k))
        z = torch.zeros(1, 3, k, t)
        return {"sim": z, "dual-sim": z, "alignability-dual": torch.zeros(1, k, 1), "alignability-joint": torch.zeros(1, 3, k, 1)}

    item = {"video": np.repeat(np.arange(vlen, dtype=np.float32)[:, None], 2, 1), "start": np.asarray(start, np.float32),
            "end": np.asarray(end, np.float32), "aligned": np.asarray(aligned).astype(np.int64), "str": [f"s{k}" for k in range(K)]}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                         # metrics over an empty / one-class set are NaN here
        with np.errstate(all="ignore"):
            eval_ref.test_alignment([item], cb, seq_len=seq_len)
    return seen


def check(start, end, vlen, aligned=None, seq_len=64):
    K = len(start)
    aligned = np.zeros(K, bool) if aligned is None else np.asarray(aligned).astype(bool)
    want = oracle_windows(start, end, vlen, aligned, seq_len)
    cand = None if not aligned.any() else ~aligned
    got = plan_windows(np.asarray(start, np.float32), np.asarray(end, np.float32), vlen, seq_len, candidates=cand)
    assert got == want
    return got


@pytest.mark.parametrize("mode", ["not_aligned", "all"])
def test_plan_windows_matches_the_oracle_loop_on_align_videos(mode):
    for v in synth.align_videos():
        al = np.asarray(v["aligned"]).astype(bool) if mode == "not_aligned" else None
        w = check(v["start"], v["end"], len(v["video"]), al)
        assert len(w) > 4


def test_plan_windows_edge_cases():
    assert check([3.0, 10.0], [5.0, 12.0], 32) == []                     # vlen <= 32: no window start
    assert check([3.0], [5.0], 20) == []
    w = check([3.0, 10.0, 50.0], [5.0, 12.0, 60.0], 64)                   # vlen == 64
    assert w and all(e0 <= 64 for _, e0, _, _ in w)
    assert check([30.0], [40.0], 200) != []                               # K == 1
    # sentences past vlen (starts >= vlen): the last windows' `right = vlen` edge rule takes them
    w = check([10.0, 100.0, 150.0, 230.0, 260.0], [20.0, 110.0, 160.0, 240.0, 270.0], 200)
    assert w[-1][3] == 5
    # K > vlen + 1: `right = vlen` stops at sentence vlen
    K = 150
    s = np.linspace(1, 40, K)
    w = check(s, s + 1, 100)
    assert w[0][3] == K and w[-1][3] == 101
    # no candidate in reach of a window start: no window at all
    assert check([10.0, 12.0], [11.0, 13.0], 300, aligned=[1, 1]) == []
    # a mixed pattern with a gap in the middle of a long video
    s = np.concatenate([np.linspace(5, 100, 12), np.linspace(600, 700, 9)])
    check(s, s + 3, 800, aligned=(np.arange(21) % 3 == 0))


def test_plan_windows_rejects_oversize_windows_by_vid():
    s = np.linspace(0, 60, 40)
    ok = plan_windows(s, s + 1, 300, max_sentences=40)
    assert max(r - l for *_, l, r in ok) == 40
    with pytest.raises(ValueError, match="vidX.*41 sentences"):
        plan_windows(np.r_[s, 61.0], np.r_[s + 1, 62.0], 300, max_sentences=40, vid="vidX")


def test_plan_windows_is_the_rule_of_the_evaluation():
    """test_alignment_htm forms its windows through plan_windows (recorded through its batched callback)."""
    from temporalalignnet_amd.eval_align import test_alignment_htm
    v = synth.align_videos(n_videos=1)[0]
    got = []

    def batched(video, text, windows, seq_len):
        got.extend((s0, e0, int(np.flatnonzero(m)[0]), int(np.flatnonzero(m)[-1]) + 1) for s0, e0, m in windows)
        K, out = len(text), []
        for s0, e0, m in windows:
            k = int(m.sum())
            out.append({"sim": torch.zeros(1, 3, k, e0 - s0), "dual-sim": torch.zeros(1, 3, k, e0 - s0),
                        "alignability-dual": torch.zeros(1, k, 1), "alignability-joint": torch.zeros(1, 3, k, 1)})
        return out

    test_alignment_htm(None, [v], device="cpu", batched_sim=batched)
    al = np.asarray(v["aligned"]).astype(bool)
    assert got == plan_windows(v["start"], v["end"], len(v["video"]), candidates=~al)
    assert got == oracle_windows(v["start"], v["end"], len(v["video"]), al)


# ------------------------------------------------------------------------------------------------------------------ corpus reader
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("htm"))
    fx = synth.htm_fixture()
    paths = synth.write_htm_fixture(root, fx)
    # half the videos stored as float16, as some feature dumps are
    for vid in list(fx["vlen"])[::2]:
        p = os.path.join(paths["features"], f"{vid}.{'webm' if vid in fx['webm'] else 'mp4'}.npy")
        np.save(p, np.load(p).astype(np.float16))
    return fx, paths


def test_reader_formats_webm_fallback_and_f16(corpus):
    fx, paths = corpus
    items = list(read_corpus(paths["features"], paths["asr"], paths["vlen"]))
    assert [it["vid"] for it in items] == sorted(fx["vlen"])
    dtypes = set()
    for it in items:
        vid, n = it["vid"], fx["vlen"][it["vid"]]
        asr = fx["asr"][vid]
        keep = [i for i, s in enumerate(asr["start"]) if s < n]
        assert it["vlen"] == n and it["str"] == [asr["text"][i] for i in keep]
        assert len(keep) < len(asr["start"]) or vid == "vidE0005"          # the fixture runs captions past the end
        np.testing.assert_array_equal(it["start"], [asr["start"][i] for i in keep])
        f = it["video"]()
        assert f.shape == (n, 1024)
        dtypes.add(f.dtype)
        np.testing.assert_allclose(f.astype(np.float32), synth.htm_features(vid, n), rtol=1e-3, atol=1e-3)
    assert dtypes == {np.dtype(np.float32), np.dtype(np.float16)}
    assert "vidI0009" in fx["webm"]                                        # read through the .webm.npy fallback above


def test_shards_are_disjoint_and_cover_the_corpus(corpus):
    fx, paths = corpus
    every = [it["vid"] for it in read_corpus(paths["features"], paths["asr"], paths["vlen"])]
    for n in (1, 2, 3, 4):
        shards = [[it["vid"] for it in read_corpus(paths["features"], paths["asr"], paths["vlen"], i, n)] for i in range(n)]
        flat = [v for s in shards for v in s]
        assert sorted(flat) == every and len(set(flat)) == len(flat)
        assert shards[0] == every[::n]


def test_reader_skips_videos_without_features_listing(tmp_path, corpus):
    fx, paths = corpus
    asr = dict(fx["asr"])
    asr["onlyInJson"] = {"text": ["a"], "start": [1.0], "end": [2.0]}
    p = tmp_path / "asr.json"
    p.write_text(json.dumps(asr))
    assert "onlyInJson" not in [it["vid"] for it in read_corpus(paths["features"], str(p), paths["vlen"])]


def test_csv_round_trips_text_and_filters_rows():
    texts = ['plain words', 'a, comma', 'say "hi"', 'two\nlines', 'all, of "it"\nhere', 'uncovered one']
    res = {"vid": "v,1", "str": texts, "timestamp": np.arange(6) * 7, "score": np.array([0.5, -1.0, 2.0, 0.1, 3.0, 9.0], np.float32),
           "confidence": np.linspace(0.1, 0.6, 6).astype(np.float32), "covered": np.array([1, 1, 1, 1, 1, 0], bool)}
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(CSV_COLUMNS)
    assert write_rows(w, res) == 5
    rows = list(csv.reader(io.StringIO(buf.getvalue(), newline="")))
    assert rows[0] == list(CSV_COLUMNS)
    assert [r[2] for r in rows[1:]] == texts[:5] and all(r[0] == "v,1" for r in rows[1:])
    assert [int(r[1]) for r in rows[1:]] == [0, 7, 14, 21, 28]
    assert [np.float32(r[3]) for r in rows[1:]] == list(res["score"][:5])
    pd = pytest.importorskip("pandas")
    df = pd.read_csv(io.StringIO(buf.getvalue()))
    assert list(df.columns) == list(CSV_COLUMNS)
    assert df.iloc[3].to_dict()["text"] == "two\nlines" and int(df.iloc[2]["timestamp"]) == 14
    # threshold: score > t only
    buf = io.StringIO(newline="")
    assert write_rows(csv.writer(buf), res, threshold=0.5) == 2
    assert [r[2] for r in csv.reader(io.StringIO(buf.getvalue(), newline=""))] == [texts[2], texts[4]]


def test_cli_help_and_argument_errors():
    from temporalalignnet_amd import infer_align
    with pytest.raises(SystemExit) as e:
        infer_align.main(["--help"])
    assert e.value.code == 0
    with pytest.raises(SystemExit):
        infer_align.main(["--checkpoint", "c", "--feature-dir", "f", "--asr-json", "a", "--vlen-csv", "v", "--vocab", "x",
                          "--out", "o", "--worker-id", "2", "--num-workers", "2"])
