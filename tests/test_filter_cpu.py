"""Host-side pieces of filtered search: `restrict()` on a `VideoIndex` and a `ShardedIndex` against the numpy statement
(filter_ref.py), the per-shard cut of a `RowFilter`, the `query --only / --exclude / --within` command line, and the C ABI of the
new entry points with their argument checks.  No device needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import filter_ref as ref
from temporalalignnet_amd import _lib

i, l, p = C.c_int, C.c_long, C.c_void_p

ENTRY_POINTS = {
    "tan_row_filter_bytes": (l, [l]),
    "tan_row_filter_build": (i, [p, l, l, p, p]),
    "tan_rank_topk_filtered": (i, [p, p, i, l, l, i, p, i, i, p, p, p, p]),
    "tan_rank_topk_filtered_e4m3": (i, [p, p, p, p, l, l, i, p, i, i, p, p, p, p]),
    "tan_rank_topk_video_filtered": (i, [p, p, i, l, l, i, p, l, p, i, i, p, p, p, p, p]),
    "tan_rank_topk_video_filtered_e4m3": (i, [p, p, p, p, l, l, i, p, l, p, i, i, p, p, p, p, p]),
}


# ------------------------------------------------------------------------------------------------------------------- the C ABI
def test_library_exports_the_entry_points_with_the_headers_prototypes():
    names, protos, L = _lib.declared_symbols(), _lib.declared_prototypes(), _lib.lib()
    for name, proto in ENTRY_POINTS.items():
        assert name in names and getattr(L, name) is not None
        assert protos[name] == proto, name
        assert getattr(L, name).argtypes == proto[1] and getattr(L, name).restype == proto[0]


def test_image_size_is_the_documented_layout():
    L = _lib.lib()
    for N in (1, 63, 64, 65, 64 * 300 + 17, 64 * 256, 64 * 256 + 1, 2 ** 31 - 1):
        assert L.tan_row_filter_bytes(N) == ref.image_bytes(N), N
        assert L.tan_row_filter_bytes(N) % 16 == 0
    for N in (0, -1, 2 ** 31):
        assert L.tan_row_filter_bytes(N) == -1


def test_bad_arguments_are_rejected_without_touching_a_device():
    L = _lib.lib()
    a = C.c_void_p(1 << 20)                            # never dereferenced: every call below fails its argument checks
    odd = C.c_void_p((1 << 20) + 8)

    def build(spans=a, n=3, N=1000, filt=a):
        return L.tan_row_filter_build(spans, n, N, filt, None)

    for kw in (dict(spans=None), dict(filt=None), dict(n=0), dict(n=-1), dict(n=1 << 30), dict(N=0), dict(N=1 << 31), dict(filt=odd)):
        assert build(**kw) == -1, kw

    def rows(e4m3, tq=a, vn=a, qs=a, vs=a, dtype=1, Q=4, N=1000, Cw=512, filt=a, k=10, splits=0, ts=a, tr=a, ws=a):
        if e4m3:
            return L.tan_rank_topk_filtered_e4m3(tq, qs, vn, vs, Q, N, Cw, filt, k, splits, ts, tr, ws, None)
        return L.tan_rank_topk_filtered(tq, vn, dtype, Q, N, Cw, filt, k, splits, ts, tr, ws, None)

    def videos(e4m3, tq=a, vn=a, qs=a, vs=a, dtype=1, Q=4, N=1000, Cw=512, v_off=a, nv=50, filt=a, k=10, splits=0, ts=a, tr=a, tv=a,
               ws=a):
        if e4m3:
            return L.tan_rank_topk_video_filtered_e4m3(tq, qs, vn, vs, Q, N, Cw, v_off, nv, filt, k, splits, ts, tr, tv, ws, None)
        return L.tan_rank_topk_video_filtered(tq, vn, dtype, Q, N, Cw, v_off, nv, filt, k, splits, ts, tr, tv, ws, None)

    common = (dict(tq=None), dict(vn=None), dict(filt=None), dict(ts=None), dict(tr=None), dict(ws=None), dict(k=0), dict(k=33),
              dict(Q=0), dict(N=0), dict(N=1 << 31), dict(Cw=256), dict(splits=-1), dict(filt=odd), dict(ws=odd), dict(tq=odd))
    for e4m3 in (False, True):
        more = (dict(qs=None), dict(vs=None)) if e4m3 else (dict(dtype=2),)
        for kw in common + more + (dict(k=11, N=10),):
            assert rows(e4m3, **kw) == -1, (e4m3, kw)
        for kw in common + more + (dict(v_off=None), dict(tv=None), dict(nv=0), dict(nv=1001), dict(k=11, nv=10)):
            assert videos(e4m3, **kw) == -1, (e4m3, kw)


# ------------------------------------------------------------------------------------------------------- the reference, by hand
def test_reference_tile_image_by_hand():
    # N = 130: tiles 0, 1 and a tail tile of 2 rows.  Spans: rows 63..64 (the tile edge), and the last row alone.
    tiles, masks = ref.tile_image(np.array([[63, 65], [129, 130]]), 130)
    assert tiles.tolist() == [0, 1, 2] and masks.tolist() == [1 << 63, 1, 1 << 1]
    tiles, masks = ref.tile_image(np.array([[64, 128]]), 130)
    assert tiles.tolist() == [1] and masks.tolist() == [2 ** 64 - 1]
    tiles, masks = ref.tile_image(np.array([[0, 130]]), 130)
    assert tiles.tolist() == [0, 1, 2] and masks.tolist() == [2 ** 64 - 1, 2 ** 64 - 1, 3]
    assert ref.spans_of([False, True, True, False, True]).tolist() == [[1, 3], [4, 5]]
    rows = ref.admitted_rows([[1, 3], [4, 5]])
    assert rows.tolist() == [1, 2, 4]
    v_off, kept = ref.gathered_videos(rows, [0, 1, 2, 4, 5])                       # video 0 has no admitted row
    assert v_off.tolist() == [0, 1, 2, 3] and kept.tolist() == [1, 2, 3]
    assert ref.map_back([2, ref.SENT, 0], rows).tolist() == [4, ref.SENT, 1]


# --------------------------------------------------------------------------------------------------------------- restrict()
VLENS = (7, 3, 1, 20, 64, 2, 130)                                      # v_off 0 7 10 11 31 95 97 227
VIDS = ["a", "b", "a", "c", "d", "e", "f"]                             # "a" names videos 0 and 2


def _index(vlens=VLENS, vids=VIDS, seed=1):
    from temporalalignnet_amd.search import VideoIndex
    g = torch.Generator().manual_seed(seed)
    n = int(sum(vlens))
    return VideoIndex(torch.randint(-16, 17, (n, 512), generator=g).float() / 16, np.concatenate([[0], np.cumsum(vlens)]), list(vids))


CASES = {
    "duplicate vid strings":        dict(videos=["a"]),
    "a number and a string":        dict(videos=[3, "e", np.int64(0)]),
    "exclude overlapping videos":   dict(videos=["a", "b", "c"], exclude=["b", "a"]),
    "exclude alone":                dict(exclude=["d", 6]),
    "adjacent videos, one span":    dict(videos=["b", "a", "c"]),                          # videos 0..3: rows [0, 31)
    "windows clamped":              dict(videos=["c", "f"], windows=[("c", -5, 4), ("f", 120, 10 ** 6)]),
    "windows merged":               dict(windows=[("f", 10, 20), ("f", 15, 30), ("f", 31, 40), ("f", 50, 50), ("d", 0, 63)]),
    "windows on a duplicate name":  dict(windows=[("a", 0, 0)]),                           # narrows BOTH videos "a"
    "a window outside the video":   dict(videos=["b", "c"], windows=[("c", 20, 25), ("c", 3, 1)]),   # "c" keeps nothing
    "a window of an excluded one":  dict(exclude=["c"], windows=[("c", 0, 5), ("e", 1, 1)]),
    "everything":                   dict(),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restrict_equals_the_row_by_row_statement(name):
    from temporalalignnet_amd.search import RowFilter
    idx, kw = _index(), CASES[name]
    f = idx.restrict(**kw)
    mask = ref.admitted_mask(idx.v_off, idx.vids, **kw)
    assert isinstance(f, RowFilter) and f.spans.dtype == np.int64 and f.spans.tolist() == ref.spans_of(mask).tolist(), name
    assert f.n_rows == int(mask.sum()) and f.n_videos == len(ref.videos_with_a_row(mask, idx.v_off))
    assert f.windowed == ("windows" in kw)
    assert f.shards() == [0] and f.shard_spans(0).tolist() == f.spans.tolist()
    assert f.shard_rows(0) == f.n_rows and f.shard_videos(0) == f.n_videos
    f.check(idx)


def test_restrict_by_hand():
    idx = _index()
    assert idx.restrict(videos=["b", "a", "c"]).spans.tolist() == [[0, 31]]
    assert idx.restrict(videos=["a"]).spans.tolist() == [[0, 7], [10, 11]]
    f = idx.restrict(windows=[("f", 10, 20), ("f", 15, 30), ("f", 31, 40), ("f", 50, 50), ("f", 129, 500)])
    assert f.spans.tolist() == [[0, 97], [107, 138], [147, 148], [226, 227]] and f.n_videos == 7 and f.n_rows == 97 + 31 + 1 + 1
    start, end = f.clip(np.array([110, 147, 5]), np.array([100, 140, 0]), np.array([150, 160, 96]))
    assert start.tolist() == [107, 147, 0] and end.tolist() == [137, 147, 96]


def test_restrict_errors():
    idx, other = _index(), _index(seed=2)
    for kw in (dict(videos=["zz"]), dict(exclude=["zz"]), dict(windows=[("zz", 0, 1)]), dict(videos=[7]), dict(videos=[-1])):
        with pytest.raises(KeyError):
            idx.restrict(**kw)
    for kw in (dict(videos=[]), dict(videos=["b"], exclude=["b"]), dict(videos=["b"], windows=[("b", 3, 9)]),
               dict(exclude=list(range(7)))):
        with pytest.raises(ValueError, match="admits no row"):
            idx.restrict(**kw)
    f = idx.restrict(videos=["b"])
    with pytest.raises(ValueError, match="another index"):
        f.check(other)
    from temporalalignnet_amd import search
    for call in (search.search, search.search_moments, search.search_rerank):
        with pytest.raises(ValueError, match="another index"):
            call(other, None, None, ["whisk"], restrict=f)              # refused before the model or the device is touched
    stem = search.VideoIndex(idx.feat, idx.v_off, idx.vids, None, idx.feat.clone())
    with pytest.raises(ValueError, match="windows"):
        search.search_rerank(stem, None, None, ["whisk"], restrict=stem.restrict(windows=[("b", 0, 1)]))
    assert "restrict" in search.search_sequences.__doc__ and "restrict" not in search.search_sequences.__code__.co_varnames


# ------------------------------------------------------------------------------------------------------------------- shards
def _sharded():
    from temporalalignnet_amd.search import ShardedIndex, VideoIndex
    cuts = ((0, 1), (1, 4), (4, 5), (5, 7))                             # shards of 1, 3, 1 and 2 videos: rows 7, 24, 64, 132
    whole = _index()
    parts = []
    for a, b in cuts:
        lo, hi = whole.v_off[a], whole.v_off[b]
        parts.append(VideoIndex(whole.feat[lo:hi], whole.v_off[a:b + 1] - lo, whole.vids[a:b]))
    return whole, ShardedIndex(parts)


@pytest.mark.parametrize("name", sorted(CASES))
def test_sharded_restrict_is_the_concatenated_filter_cut_per_shard(name):
    whole, sh = _sharded()
    kw = CASES[name]
    f, g = sh.restrict(**kw), whole.restrict(**kw)
    assert f.spans.tolist() == g.spans.tolist() and (f.n_rows, f.n_videos, f.windowed) == (g.n_rows, g.n_videos, g.windowed)
    mask = ref.admitted_mask(whole.v_off, whole.vids, **kw)
    want = []
    for s in range(4):
        part = mask[sh.row_base[s]:sh.row_base[s + 1]]
        if part.any():
            want.append(s)
            assert f.shard_spans(s).tolist() == ref.spans_of(part).tolist(), (name, s)
            assert f.shard_rows(s) == int(part.sum())
            assert f.shard_videos(s) == len(ref.videos_with_a_row(part, sh.shards[s].v_off))
    assert f.shards() == want                                            # ascending, the empty shards left out
    assert sum(f.shard_rows(s) for s in want) == f.n_rows and sum(f.shard_videos(s) for s in want) == f.n_videos
    assert [s for s, *_ in sh.shard_views(f.shards())] == want
    with pytest.raises(ValueError, match="another index"):
        f.check(whole)


def test_sharded_restrict_leaves_out_empty_shards_by_hand():
    _, sh = _sharded()
    f = sh.restrict(videos=["a", "f"])                                   # videos 0, 2 (shards 0, 1) and 6 (shard 3)
    assert f.shards() == [0, 1, 3]
    assert f.shard_spans(0).tolist() == [[0, 7]] and f.shard_spans(1).tolist() == [[3, 4]] and f.shard_spans(3).tolist() == [[2, 132]]
    f = sh.restrict(videos=["b", "a", "c", "d"])                         # one global span over three shards
    assert f.spans.tolist() == [[0, 95]] and f.shards() == [0, 1, 2]
    assert [f.shard_spans(s).tolist() for s in (0, 1, 2)] == [[[0, 7]], [[0, 24]], [[0, 64]]]
    assert [f.shard_videos(s) for s in (0, 1, 2)] == [1, 3, 1]


# ------------------------------------------------------------------------------------------------------------- command line
def test_cli_takes_the_filter_options_and_refuses_the_conflicts(tmp_path):
    from temporalalignnet_amd import search
    argv = ["query", "--checkpoint", "c", "--vocab", "/nonexistent/s3d_dict.npy", "--index", "i.npz"]
    a = search.parse_args(argv + ["--only", "v1", "--only", "v2", "--exclude", "v3", "--within", "v1:30-90", "--within", "a:b:0-5",
                                  "--only-file", "p.txt", "--exclude-file", "q.txt", "whisk"])
    assert a.only == ["v1", "v2"] and a.exclude == ["v3"] and a.only_file == "p.txt" and a.exclude_file == "q.txt"
    assert a.within == [("v1", 30, 90), ("a:b", 0, 5)] and a.sentences == ["whisk"]
    a = search.parse_args(argv + ["whisk"])
    assert a.only is None and a.exclude is None and a.within is None and a.only_file is None and a.exclude_file is None
    assert search.parse_args(argv + ["--moments", "--within", "v:1-2", "whisk"]).within == [("v", 1, 2)]
    assert search.parse_args(argv + ["--rerank", "--only", "v", "--exclude-file", "q", "whisk"]).rerank
    assert search.parse_args(argv + ["--shard", "a.npz", "--host-resident", "--only", "v", "whisk"]).only == ["v"]
    for bad in (["--sequence", "--only", "v", "whisk"], ["--sequence", "--only-file", "p", "whisk"], ["--sequence", "--exclude", "v", "whisk"],
                ["--sequence", "--exclude-file", "p", "whisk"], ["--sequence", "--within", "v:1-2", "whisk"],
                ["--rerank", "--within", "v:1-2", "whisk"], ["--within", "v", "whisk"], ["--within", "v:1", "whisk"],
                ["--within", ":1-2", "whisk"], ["--within", "v:a-2", "whisk"], ["--within", "v:1-", "whisk"]):
        with pytest.raises(SystemExit):
            search.parse_args(argv + bad)
    # the options -> restrict(): files are read one vid per line, blank lines skipped
    idx = _index()
    (tmp_path / "only.txt").write_text("a\n\nf\n")
    (tmp_path / "not.txt").write_text("f\n")
    a = search.parse_args(argv + ["--only", "c", "--only-file", str(tmp_path / "only.txt"), "--exclude-file", str(tmp_path / "not.txt"),
                                  "--within", "c:2-4", "whisk"])
    f = search.restrict_from_args(idx, a)
    assert f.spans.tolist() == idx.restrict(videos=["c", "a", "f"], exclude=["f"], windows=[("c", 2, 4)]).spans.tolist()
    assert f.spans.tolist() == [[0, 7], [10, 11], [13, 16]] and f.windowed
    assert search.restrict_from_args(idx, search.parse_args(argv + ["whisk"])) is None
    assert search.restrict_from_args(idx, search.parse_args(argv + ["--exclude", "a", "whisk"])).n_videos == 5
    with pytest.raises(KeyError):
        search.restrict_from_args(idx, search.parse_args(argv + ["--only", "nope", "whisk"]))
