"""Clip search on the host: clip_ref.py (the numpy restatement of tan_clip_topk's match that test_clips_gpu.py compares the kernel
with) pinned against a loop over Python ints, and the host logic of `search.clip_features` / `search_clips` / `similar`: the clip
checks over a CPU `VideoIndex` made from tensors, the `exclude_source` list surgery, the command line.  No device is used."""
import numpy as np
import pytest
import torch

import clip_ref as ref
from temporalalignnet_amd import search


# ----------------------------------------------------------------------------------------------------------------- the reference
def test_diag_sums_equal_the_brute_force_on_integers():
    rng = np.random.default_rng(0)
    for m, V in ((1, 1), (1, 7), (3, 2), (3, 3), (3, 4), (5, 64), (5, 65), (32, 31), (32, 32), (32, 33), (32, 200), (7, 129)):
        x = rng.integers(-50, 51, (m, V))
        S = ref.diag_sums(x)
        assert S.dtype == x.dtype and S.shape == (max(V - m + 1, 0),), (m, V)
        got = ref.match_and_start(x)
        if V < m:
            assert got is None and ref.brute_force(x) is None
            continue
        for t in range(V - m + 1):
            assert int(S[t]) == sum(int(x[i, t + i]) for i in range(m)), (m, V, t)
        assert (int(got[0]), got[1]) == ref.brute_force(x), (m, V)
    # V == m: one start; V == m + 1: two
    x = np.arange(12).reshape(3, 4)
    assert ref.diag_sums(x[:, :3]).tolist() == [0 + 5 + 10] and ref.diag_sums(x).tolist() == [0 + 5 + 10, 1 + 6 + 11]
    # m == 1: the row itself, its first maximum
    assert ref.match_and_start(np.array([[3, 9, 2, 9]])) == (9, 1) == ref.brute_force(np.array([[3, 9, 2, 9]]))


def test_ties_go_to_the_first_start():
    x = np.zeros((2, 6), dtype=np.int64)
    x[0, 1] = x[1, 2] = 4                                           # start 1: 8
    x[0, 3] = 5
    x[1, 4] = 3                                                     # start 3: 8 again
    assert ref.diag_sums(x).tolist() == [0, 8, 0, 8, 0]
    assert ref.match_and_start(x) == (8, 1) == ref.brute_force(x)


def test_diag_sums_add_in_ascending_order_in_the_input_dtype():
    x = np.diag(np.array([2.0 ** 24, 1.0, 1.0, -2.0 ** 24], dtype=np.float32))    # [4, 4]: one start, its terms on the diagonal
    S = ref.diag_sums(x)
    assert S.dtype == np.float32 and S.tolist() == [0.0]            # ((2^24 + 1) + 1) - 2^24 in f32: both ones are rounded away
    assert ref.diag_sums(x.astype(np.float64)).tolist() == [2.0]


def test_topk_orders_and_leaves_empty_slots():
    v_off = np.array([0, 4, 6, 16, 19, 29])                         # V = 4, 2, 10, 3, 10
    X = np.zeros((3 + 1, 29), dtype=np.int64)
    c_off = np.array([0, 3, 4])                                     # a clip of 3 rows and one of 1
    X[0, 1], X[1, 2], X[2, 3] = 2, 2, 2                             # video 0: start 1, match 6
    X[0, 8], X[1, 9], X[2, 10] = 2, 2, 2                            # video 2: start 2, match 6 -- a tie, the lower row first
    X[0, 25], X[1, 26], X[2, 27] = 3, 3, 3                          # video 4: start 6, match 9
    X[3, 5] = 7                                                     # the one-row clip: video 1, its second row
    match, start = ref.matches(X, c_off, v_off)
    assert start[0].tolist() == [1, -1, 2, 0, 6] and match[0].tolist() == [6, 0, 6, 0, 9]
    assert start[1].tolist() == [0, 1, 0, 0, 0] and match[1, 1] == 7
    s, r, v = ref.topk(match, start, v_off, 5)
    assert v[0].tolist() == [4, 0, 2, 3, -1] and r[0].tolist() == [25, 1, 8, 16, ref.EMPTY_ROW]
    assert s[0].tolist() == [9.0, 6.0, 6.0, 0.0, -np.inf]
    assert v[1].tolist() == [1, 0, 2, 3, 4] and r[1].tolist() == [5, 0, 6, 16, 19]
    s, r, v = ref.topk(match, start, v_off, 2)
    assert v.tolist() == [[4, 0], [1, 0]]


# ------------------------------------------------------------------------------------------------------------------ the host logic
def _cpu_index(e4m3=False):
    g = torch.Generator().manual_seed(5)
    feat = torch.randn(60, 512, generator=g)
    vids = ["a", "b", "c", "b"]                                     # equal names are distinct videos
    v_off = [0, 10, 50, 55, 60]
    if e4m3:
        return search.VideoIndex(torch.zeros(60, 512, dtype=torch.uint8), v_off, vids, torch.ones(60))
    return search.VideoIndex(feat, v_off, vids)


def test_clip_spans_resolve_and_check_every_clip():
    idx = _cpu_index()
    rows = torch.zeros(7, 512)
    got = search.clip_spans(idx, [("a", 0, 9), ("b", 5, 5), (2, 1, 4), ("c", 0, 4), rows, rows.bfloat16()[:1], ("b", 0, 31)])
    assert got == [(10, (0, 0)), (1, (1, 5)), (4, (2, 1)), (5, (2, 0)), (7, None), (1, None), (32, (1, 0))]   # "b": the first one
    sharded = search.ShardedIndex([search.VideoIndex(idx.feat[:50], [0, 10, 50], ["a", "b"]),
                                   search.VideoIndex(idx.feat[50:], [0, 5, 10], ["c", "b"])])
    assert search.clip_spans(sharded, [("c", 0, 4), (3, 2, 3)]) == [(5, (2, 0)), (2, (3, 2))]
    bad = [("nope", 0, 1),                                          # an unknown vid
           (4, 0, 1), (-1, 0, 1), (1.5, 0, 1),                      # ... or video number
           ("a", 5, 4),                                             # first > last
           ("a", 0, 10), ("a", -1, 3), ("c", 3, 5),                 # seconds outside the video
           ("b", 0, 32),                                            # 33 seconds
           torch.zeros(33, 512), torch.zeros(0, 512),               # m outside [1, 32]
           torch.zeros(4, 256), torch.zeros(512), torch.zeros(4, 512, dtype=torch.int32),   # not float [m, 512]
           ("a", 1), "a:1-2", ("a", "x", 2)]                        # not a clip at all
    for clip in bad:
        for index in (idx, sharded, _cpu_index(e4m3=True)):
            with pytest.raises(ValueError):
                search.clip_spans(index, [("a", 0, 3), clip])
            with pytest.raises(ValueError):                         # and before anything touches a device
                search.clip_features(index, [clip])
            with pytest.raises(ValueError):
                search.search_clips(index, [clip])
    with pytest.raises(ValueError):
        search.clip_features(idx, [])
    assert search.search_clips(idx, []) == []
    for k, kw in ((0, {}), (-1, {}), (0, dict(exclude_source=True))):
        with pytest.raises(ValueError):
            search.search_clips(idx, [("a", 0, 3)], k=k, **kw)
    big = search.VideoIndex(torch.zeros(40, 512), np.arange(41), [f"v{i}" for i in range(40)])
    for k, kw in ((33, {}), (32, dict(exclude_source=True))):
        with pytest.raises(ValueError):
            search.search_clips(big, [("v0", 0, 0)], k=k, **kw)


def test_drop_source_is_the_top_k_of_the_other_videos():
    e = [(4, 0, 9.0), (7, 3, 8.0), (1, 2, 7.0), (9, 1, 6.0)]        # out of a sweep asked for k + 1 = 4
    assert search.drop_source(e, 7, 3) == [e[0], e[2], e[3]]        # listed: removed
    assert search.drop_source(e, 4, 3) == e[1:]
    assert search.drop_source(e, 5, 3) == e[:3]                     # not listed: the last hit goes
    assert search.drop_source(e, None, 3) == e[:3]                  # a tensor clip has no source
    assert search.drop_source(e[:2], 5, 3) == e[:2]                 # fewer than k + 1 eligible videos: nothing to cut
    assert search.drop_source(e[:2], 4, 3) == e[1:2]
    assert search.drop_source([], 4, 3) == []


def test_similar_command_line():
    argv = ["similar", "--index", "i.npz", "--clip", "vid:10-29"]
    a = search.parse_args(argv)
    assert a.cmd == "similar" and a.clip == [("vid", 10, 29)] and a.k == 10 and not a.keep_source
    assert a.shard is None and not a.host_resident
    assert not hasattr(a, "checkpoint") and not hasattr(a, "vocab")            # no checkpoint, no model
    a = search.parse_args(argv + ["--clip", "a:b:0-31", "--keep-source", "-k", "32", "--shard", "j.npz", "--host-resident"])
    assert a.clip == [("vid", 10, 29), ("a:b", 0, 31)] and a.keep_source and a.k == 32 and a.shard == ["j.npz"] and a.host_resident
    assert search.parse_args(argv + ["-k", "31"]).k == 31
    for bad in (["--clip", "vid:0-32"],                             # 33 seconds
                ["--clip", "vid:5-4"], ["--clip", "vid"], ["--clip", "vid:3"], ["--clip", ":1-2"], ["--clip", "vid:a-b"],
                ["-k", "0"], ["-k", "32"], ["-k", "33", "--keep-source"], ["--checkpoint", "c"], ["whisk"]):
        with pytest.raises(SystemExit):
            search.parse_args(argv + bad)
    with pytest.raises(SystemExit):
        search.parse_args(["similar", "--index", "i.npz"])          # no clip
    with pytest.raises(SystemExit):
        search.parse_args(["similar", "--clip", "vid:1-2"])         # no index


def test_a_clip_of_33_seconds_is_told_to_be_cut(capsys):
    with pytest.raises(SystemExit):
        search.parse_args(["similar", "--index", "i.npz", "--clip", "vid:100-132"])
    err = capsys.readouterr().err
    assert "33 seconds" in err and "cut" in err
    assert search.parse_within("v:1-2") == ("v", 1, 2)
    with pytest.raises(ValueError, match="--within"):
        search.parse_within("v")
