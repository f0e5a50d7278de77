"""Host-side pieces of the GPU retrieval path (temporalalignnet_amd/eval_retrieval.py additions, search.py) and the C ABI of
csrc/tan_retrieve.hip: metrics from counts against golden G12 and the oracle, the window grouping against `clip_windows`, the index
window plan, row -> (video, second) mapping, and the exported entry points.  No device needed."""
import ctypes as C

import numpy as np
import pytest

from temporalalignnet_amd import _lib, synth
from temporalalignnet_amd.eval_retrieval import clip_windows, compute_metrics, metrics_from_counts, plan_clip_groups

NEW_SYMBOLS = ("tan_rank_topk", "tan_rank_topk_ws_bytes", "tan_segment_pool_acc", "tan_segment_pool_final", "tan_window_feat_acc",
               "tan_window_feat_final")


def _counts(x):
    x = np.asarray(x)
    d = np.diag(x)[:, None]
    return (x > d).sum(1), (x == d).sum(1)


def _same(a, b):
    for k in ("R1", "R5", "R10", "MR"):
        assert float(a[k]) == float(b[k]), k


def test_metrics_from_counts_match_golden_and_oracle(golden):
    from oracle import retrieval_ref
    g = golden("g12_compute_metrics")
    got = metrics_from_counts(*_counts(g["x"]))
    orc = retrieval_ref.metrics(g["x"])
    for k in ("R1", "R5", "R10", "MR"):
        assert float(got[k]) == float(g[k]) == orc[k], k
    _same(got, compute_metrics(g["x"]))


def test_metrics_from_counts_with_constructed_ties():
    from oracle import retrieval_ref
    rng = np.random.default_rng(3)
    x = rng.standard_normal((23, 23))
    x[:, 7] = x[:, 3]                      # duplicate columns: rows 3 and 7 tie with each other's column
    x[:, 19] = x[:, 3]
    x[11, :] = 0.25                        # a row of all-equal scores: 23 hits at positions 0..22
    x[5, 2] = x[5, 5]                      # a single off-diagonal tie
    got = metrics_from_counts(*_counts(x))
    _same(got, compute_metrics(x))
    _same(got, retrieval_ref.metrics(x))
    h, t = _counts(x)
    assert t[11] == 23 and h[11] == 0 and t[3] == 3 and t[5] == 2
    # small integers: many ties everywhere
    y = rng.integers(0, 4, (31, 31)).astype(np.float64)
    _same(metrics_from_counts(*_counts(y)), compute_metrics(y))
    _same(metrics_from_counts(*_counts(y)), retrieval_ref.metrics(y))


def _check_plan(clips, num_clips, max_windows):
    calls = plan_clip_groups(clips, num_clips, max_windows)
    seen = np.zeros((len(clips), num_clips), dtype=np.int64)
    for call in calls:
        w, win = call["idx"].shape
        assert 1 <= w <= max_windows and win == call["win"]
        assert call["clip"].shape == call["window"].shape == call["s_idx"].shape == call["e_idx"].shape == (w,)
        for j in range(w):
            c, i = int(call["clip"][j]), int(call["window"][j])
            seen[c, i] += 1
            item = clips[c]
            vlen = item["vlen"] if "vlen" in item else item["feature"].shape[0]
            idx, s_idx, e_idx = clip_windows(vlen, item["start"], item["end"], num_clips, -1)
            assert idx.shape[1] == win                                       # one window length per call
            assert (call["idx"][j] == idx[i]).all() and call["s_idx"][j] == s_idx[i] and call["e_idx"][j] == e_idx[i]
    assert (seen == 1).all()                                                 # every window of every clip exactly once
    return calls


def test_plan_clip_groups_on_the_fixture():
    fx = synth.yc2_fixture()
    feats = {vid: np.zeros((vlen, 4), np.float32) for vid, vlen in fx["videos"].items()}
    clips = [{"feature": feats[c["vid"]], "start": c["segment"][0], "end": c["segment"][1], "str": c["sentence"]} for c in fx["clips"]]
    for mw in (256, 16, 7, 1):
        calls = _check_plan(clips, 10, mw)
        assert [c["win"] for c in calls] == sorted(c["win"] for c in calls)


def test_plan_clip_groups_on_synthetic_clips():
    rng = np.random.default_rng(11)
    clips = []
    for _ in range(300):
        vlen = int(rng.integers(40, 900))
        s = int(rng.integers(0, vlen - 4))
        e = int(min(vlen - 1, s + rng.integers(2, 400)))
        clips.append({"vlen": vlen, "start": s, "end": max(e, s + 1), "str": "x"})
    for num_clips, mw in ((10, 256), (10, 37), (4, 64)):
        calls = _check_plan(clips, num_clips, mw)
        lens = {c["win"] for c in calls}
        # a group's calls are all full except its last
        for win in lens:
            sizes = [len(c["clip"]) for c in calls if c["win"] == win]
            assert all(s == mw for s in sizes[:-1])
    with pytest.raises(ValueError):
        plan_clip_groups(clips, 10, 0)


def test_index_windows_cover_every_second():
    from temporalalignnet_amd.eval_align import plan_windows
    from temporalalignnet_amd.search import plan_index_windows
    for vlen in (1, 5, 20, 31, 32, 33, 47, 48, 49, 64, 65, 100, 777, 1200):
        plan = plan_index_windows(vlen, 64)
        cover = np.zeros(vlen, int)
        for s0, e0 in plan:
            assert 0 <= s0 < e0 <= vlen and e0 - s0 <= 64
            cover[s0:e0] += 1
        assert (cover >= 1).all(), vlen
        assert [s for s, _ in plan] == sorted(s for s, _ in plan)
        if vlen > 32:       # the alignment evaluation's stepping, with one sentence that activates every window
            ref = plan_windows(np.array([0.0]), np.array([float(vlen)]), vlen, 64, None)
            want = [(int(s0), int(min(vlen, s0 + 64))) for s0 in np.arange(0, vlen - 32, 16)]
            assert plan == want and {(a, b) for a, b, _, _ in ref} <= set(plan)


def test_index_rows_map_to_video_and_second():
    import torch
    from temporalalignnet_amd.search import VideoIndex
    idx = VideoIndex(torch.zeros(10 + 1 + 25, 512), [0, 10, 11, 36], ["a", "b", "c"])
    v, sec = idx.locate(np.array([[0, 9, 10], [11, 35, 12]]))
    assert v.tolist() == [[0, 0, 1], [2, 2, 2]] and sec.tolist() == [[0, 9, 0], [0, 24, 1]]


def test_index_save_load_roundtrip_on_the_host(tmp_path):
    import torch
    from temporalalignnet_amd.search import VideoIndex
    for dt in (torch.bfloat16, torch.float32):
        f = torch.randn(17, 512).to(dt)
        p = str(tmp_path / f"i_{dt}.npz".replace("torch.", ""))
        VideoIndex(f, [0, 5, 17], ["x", "y"]).save(p)
        back = VideoIndex.load(p, device="cpu")
        assert back.feat.dtype == dt and torch.equal(back.feat, f) and back.v_off.tolist() == [0, 5, 17] and back.vids == ["x", "y"]


def test_library_exports_the_retrieval_entry_points():
    names = _lib.declared_symbols()
    L = _lib.lib()
    protos = _lib.declared_prototypes()
    for n in NEW_SYMBOLS:
        assert n in names and getattr(L, n) is not None, n
    assert protos["tan_rank_topk_ws_bytes"] == (C.c_long, [C.c_long, C.c_long, C.c_int])
    assert protos["tan_rank_topk"][1][3:9] == [C.c_long, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int]


def test_scratch_size_and_bad_arguments_without_a_device():
    L = _lib.lib()
    # 2 048 queries, 2 M rows, k = 10: scratch + outputs stay far below the 16 GB the explicit matrix would take
    ws = L.tan_rank_topk_ws_bytes(2048, 2_000_000, 10)
    assert 0 < ws + 2048 * 10 * 8 + 2048 * 8 < 64 * 2 ** 20
    assert L.tan_rank_topk_ws_bytes(1, 1, 0) > 0
    assert L.tan_rank_topk_ws_bytes(1 << 33, 5, 1) > 1 << 33                  # a `long` result comes back whole
    for bad in ((0, 5, 1), (5, 0, 1), (5, 1 << 31, 1), (5, 5, 33), (5, 5, -1)):
        assert L.tan_rank_topk_ws_bytes(*bad) == -1, bad
    assert L.tan_rank_topk(None, None, 0, 4, 4, 512, None, 1, 0, None, None, None, None, None, None) == -1
    assert L.tan_segment_pool_acc(None, 0, 512 * 4, 4, None, 1, 1, None, None, 1, None) == -1
    assert L.tan_segment_pool_final(None, None, 1, 1, None, None) == -1
    assert L.tan_window_feat_acc(None, 0, 512 * 4, None, 1, 4, None, None, 4, None) == -1
    assert L.tan_window_feat_final(None, None, 4, None, 0, None) == -1
