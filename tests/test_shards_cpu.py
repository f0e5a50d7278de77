"""Host-side pieces of sharded search: the C ABI of tan_topk_fold and its argument checks, the numpy statement of the fold
(shard_ref.py) against a global sort, `VideoIndex.concat`, `ShardedIndex` bookkeeping, the `merge` command and the `query --shard /
--host-resident` command line.  No device needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import shard_ref as ref
from temporalalignnet_amd import _lib

i, l, p = C.c_int, C.c_long, C.c_void_p


def test_library_exports_the_fold_with_the_headers_prototype():
    names, protos, L = _lib.declared_symbols(), _lib.declared_prototypes(), _lib.lib()
    assert "tan_topk_fold" in names and L.tan_topk_fold is not None
    assert protos["tan_topk_fold"] == (i, [p, p, p, p, l, i, i, i, p, p, p, p, p, i, i, p])
    assert L.tan_topk_fold.argtypes == protos["tan_topk_fold"][1]


def test_bad_arguments_are_rejected_without_touching_a_device():
    L = _lib.lib()
    a = C.c_void_p(1 << 20)                            # never dereferenced: every call below fails its argument checks

    def fold(Q=4, k=10, n_aux=0, k_in=5, shard=0, run=(a, a, a, a), inc=(a, a), aux=(a, a, a)):
        return L.tan_topk_fold(*run, Q, k, n_aux, 0, *inc, *aux, k_in, shard, None)

    assert L.tan_topk_fold(None, None, None, None, 4, 10, 0, 0, None, None, None, None, None, 5, 0, None) == -1
    for kw in (dict(k=0), dict(k=33), dict(k=4, k_in=5), dict(k_in=0), dict(n_aux=4), dict(n_aux=-1), dict(shard=-1),
               dict(shard=ref.SENT), dict(Q=0), dict(n_aux=2, aux=(a, None, a)), dict(n_aux=3, aux=(a, a, None)),
               dict(n_aux=1, run=(a, a, a, None)), dict(run=(None, a, a, a)), dict(run=(a, None, a, a)), dict(run=(a, a, None, a)),
               dict(inc=(None, a)), dict(inc=(a, None))):
        assert fold(**kw) == -1, kw


@pytest.mark.parametrize("k", (1, 10, 32))
@pytest.mark.parametrize("S", (1, 2, 5))
def test_reference_fold_in_any_order_is_the_global_sort(S, k):
    for k_in in sorted({1, k // 2 or 1, k}):
        for n_aux, kw in ((0, {}), (3, {}), (1, dict(all_equal=True)), (2, dict(sentinels=True))):
            Q = 7
            lists = ref.make_lists(Q, k_in, n_aux, range(S), seed=1000 * S + 10 * k + k_in, **kw)
            want = ref.best_of_all(lists, k)
            # the statement itself, once by hand: query 0's entries through Python's own sort
            ent = [(-float(sc), s, int(r)) for s, (score, row, _) in lists.items() for sc, r in zip(score[0], row[0]) if r != ref.SENT]
            ent = sorted(ent)[:k]
            assert [e[2] for e in ent] == want[2][0, :len(ent)].tolist() and [e[1] for e in ent] == want[1][0, :len(ent)].tolist()
            assert (want[2][0, len(ent):] == ref.SENT).all() and np.isinf(want[0][0, len(ent):]).all()
            rng = np.random.default_rng(S + k)
            for order in (list(range(S)), list(range(S))[::-1], list(rng.permutation(S))):
                run = tuple(np.full_like(t, 77) for t in ref.empty(Q, k, n_aux))           # poisoned: the first fold resets
                for n, s in enumerate(order):
                    run = ref.fold(run, lists[s], s, reset=n == 0)
                assert ref.same(run, want), (k_in, n_aux, order)
            if n_aux:                                                                       # the payload is its key's
                real = want[2] != ref.SENT
                for c in range(n_aux):
                    assert np.array_equal(want[3][c][real], ref.aux_of(want[1].astype(np.int64), want[2].astype(np.int64), c)[real])
                    assert (want[3][c][~real] == -1).all()


# ------------------------------------------------------------------------------------------------------------ indices on the host
def _rows(n, fmt, seed):
    g = torch.Generator().manual_seed(seed)
    if fmt == "e4m3":
        return torch.randint(0, 256, (n, 512), generator=g, dtype=torch.uint8), torch.ldexp(torch.ones(n), torch.randint(-6, 4, (n,), generator=g))
    x = torch.randint(-16, 17, (n, 512), generator=g).float() / 16
    return (x if fmt == "f32" else x.bfloat16()), None


def _index(vlens, fmt, seed, stem=None, tag="v"):
    from temporalalignnet_amd.search import VideoIndex
    n = int(sum(vlens))
    feat, scale = _rows(n, fmt, seed)
    st = None if stem is None else _rows(n, stem, seed + 500)[0]
    return VideoIndex(feat, np.concatenate([[0], np.cumsum(vlens)]), [f"{tag}{j}" for j in range(len(vlens))], scale, st)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


SHARD_VLENS = ([7], [3, 1, 20], [64, 2])                               # shards of 1, 3 and 2 videos


@pytest.mark.parametrize("stem", (None, "bf16", "f32"))
@pytest.mark.parametrize("fmt", ("f32", "bf16", "e4m3"))
def test_concat_is_the_concatenation_and_round_trips(fmt, stem, tmp_path):
    from temporalalignnet_amd.search import VideoIndex
    parts = [_index(v, fmt, 10 + n, stem, tag=f"s{n}_") for n, v in enumerate(SHARD_VLENS)]
    parts[2].vids[0] = parts[0].vids[0]                                # equal vid strings stay two videos
    idx = VideoIndex.concat(parts)
    assert len(idx) == 97 and idx.e4m3 == (fmt == "e4m3") and idx.feat.dtype == parts[0].feat.dtype
    assert torch.equal(_bits(idx.feat), torch.cat([_bits(x.feat) for x in parts]))
    assert idx.v_off.dtype == np.int64 and idx.v_off.tolist() == [0, 7, 10, 11, 31, 95, 97]
    assert idx.vids == [v for x in parts for v in x.vids] and len(idx.vids) == 6
    assert (idx.scale is None) if fmt != "e4m3" else torch.equal(idx.scale, torch.cat([x.scale for x in parts]))
    assert (idx.stem is None) if stem is None else torch.equal(_bits(idx.stem), torch.cat([_bits(x.stem) for x in parts]))
    path = str(tmp_path / "i.npz")
    idx.save(path)
    back = VideoIndex.load(path, device="cpu")
    assert back.feat.dtype == idx.feat.dtype and torch.equal(_bits(back.feat), _bits(idx.feat)) and back.vids == idx.vids
    assert back.v_off.tolist() == idx.v_off.tolist()
    assert (back.scale is None) if fmt != "e4m3" else torch.equal(back.scale, idx.scale)
    assert (back.stem is None) if stem is None else (back.stem.dtype == idx.stem.dtype and torch.equal(_bits(back.stem), _bits(idx.stem)))
    one = VideoIndex.concat([parts[1]])
    assert torch.equal(_bits(one.feat), _bits(parts[1].feat)) and one.v_off.tolist() == parts[1].v_off.tolist()


def test_concat_refuses_what_does_not_fit_together():
    from temporalalignnet_amd.search import VideoIndex
    a, b, c = _index([3], "f32", 1), _index([4], "bf16", 2), _index([5], "e4m3", 3)
    for pair in ((a, b), (a, c), (b, c), (c, a)):
        with pytest.raises(ValueError):
            VideoIndex.concat(pair)
    with pytest.raises(ValueError):
        VideoIndex.concat([a, _index([4], "f32", 4, stem="bf16")])     # a stem here, none there
    with pytest.raises(ValueError):
        VideoIndex.concat([_index([4], "f32", 4, stem="f32"), _index([4], "f32", 5, stem="bf16")])
    with pytest.raises(ValueError):
        VideoIndex.concat([])


def test_sharded_index_bookkeeping():
    from temporalalignnet_amd.search import ShardedIndex, VideoIndex
    parts = [_index(v, "bf16", 20 + n, tag=f"s{n}_") for n, v in enumerate(SHARD_VLENS)]
    sh = ShardedIndex(parts, resident="device")
    whole = VideoIndex.concat(parts)
    assert len(sh) == 97 and not sh.e4m3 and sh.resident == "device" and sh.device == torch.device("cpu")
    assert sh.row_base.dtype == np.int64 and sh.row_base.tolist()[:3] == [0, 7, 31] and sh.row_base[-1] == 97
    assert sh.video_base.dtype == np.int64 and sh.video_base.tolist()[:3] == [0, 1, 4] and sh.video_base[-1] == 6
    assert sh.vids == ["s0_0", "s1_0", "s1_1", "s1_2", "s2_0", "s2_1"] == whole.vids
    assert sh.v_off.dtype == np.int64 and sh.v_off.tolist() == whole.v_off.tolist()
    for s, x in enumerate(parts):
        rows = np.arange(len(x))
        v, sec = sh.locate(np.full(len(x), s), rows)
        wv, wsec = whole.locate(sh.row_base[s] + rows)
        assert v.tolist() == wv.tolist() and sec.tolist() == wsec.tolist()
    v, sec = sh.locate(np.array([[2, 0], [1, 1]]), np.array([[64, 6], [3, 4]]))            # any shape, as the searches' [Q, k]
    assert v.tolist() == [[5, 0], [2, 3]] and sec.tolist() == [[0, 6], [0, 0]]
    assert [s for s, *_ in sh.shard_views()] == [0, 1, 2] and [s for s, *_ in sh.shard_views([2, 0])] == [2, 0]
    s, feat, scale, v_off = next(iter(sh.shard_views([1])))
    assert feat is parts[1].feat and scale is None and v_off.dtype == torch.int32 and v_off.tolist() == [0, 3, 4, 24]
    assert ShardedIndex([_index([2], "e4m3", 1), _index([3], "e4m3", 2)]).e4m3
    with pytest.raises(ValueError):
        ShardedIndex([parts[0], _index([3], "f32", 9)])                # mixed row formats
    with pytest.raises(ValueError):
        ShardedIndex([parts[0], _index([3], "e4m3", 9)])
    with pytest.raises(ValueError):
        ShardedIndex([])
    with pytest.raises(ValueError):
        ShardedIndex(parts, resident="disk")


def test_hit_coordinates_match_a_walk_over_the_concatenation():
    """What the searches map their shard-local hits with: every (shard, row) -> (video, second) and every (shard, video) -> (global
    video, first row), against a brute-force walk over `VideoIndex.concat`'s v_off."""
    from temporalalignnet_amd.search import ShardedIndex, VideoIndex
    from temporalalignnet_amd.search.index import _locate_videos
    vlens = ([5, 3], [9], [2, 2])
    parts = [_index(v, "f32", 40 + n) for n, v in enumerate(vlens)]    # tag "v": shards 0 and 2 share the vid strings v0, v1
    sh, whole = ShardedIndex(parts, resident="device"), VideoIndex.concat(parts)
    assert whole.vids == ["v0", "v1", "v0", "v0", "v1"] and whole.v_off.tolist() == [0, 5, 8, 17, 19, 21]
    walk = []                                                          # global row -> (video number, second, the video's first row)
    for v in range(len(whole.vids)):
        walk += [(v, g - int(whole.v_off[v]), int(whole.v_off[v])) for g in range(int(whole.v_off[v]), int(whole.v_off[v + 1]))]
    assert len(walk) == len(whole) == len(sh) == 21
    g = gv = 0
    for s, lens in enumerate(vlens):
        for row in range(sum(lens)):                                   # every row: each video's and each shard's first and last
            for index, at in ((sh, (s, row)), (whole, (g,))):
                v, sec = index.locate(*(np.array([a]) for a in at))
                assert (int(v[0]), int(sec[0])) == walk[g][:2], (s, row)
            g += 1
        for video in range(len(lens)):
            for index, at, base in ((sh, (s, video), int(sh.row_base[s])), (whole, (0, gv), 0)):
                v, first = _locate_videos(index, *(np.array([a]) for a in at))
                assert (int(v[0]), base + int(first[0])) == (gv, int(whole.v_off[gv])), (s, video)
            assert walk[int(whole.v_off[gv])] == (gv, 0, int(whole.v_off[gv]))
            gv += 1
    assert (g, gv) == (21, 5)
    # whole arrays at once, as the searches pass their [Q, k] lists
    shard, video = np.array([[0, 2], [1, 2]]), np.array([[1, 0], [0, 1]])
    v, first = _locate_videos(sh, shard, video)
    assert v.tolist() == [[1, 3], [2, 4]] and first.tolist() == [[5, 0], [0, 2]]
    v, sec = sh.locate(shard, first + 1)
    assert v.tolist() == [[1, 3], [2, 4]] and sec.tolist() == [[1, 1], [1, 1]]


def test_search_rerank_refuses_a_sharded_index():
    from temporalalignnet_amd import search
    sh = search.ShardedIndex([_index([4], "bf16", 1, stem="bf16")])
    with pytest.raises(ValueError, match="search_rerank: not built for a ShardedIndex; merge the shards"):
        search.search_rerank(sh, None, None, ["whisk"])


# ------------------------------------------------------------------------------------------------------------------ command line
@pytest.mark.parametrize("fmt,stem", (("bf16", None), ("e4m3", "bf16"), ("f32", None)))
def test_merge_writes_the_concatenation(fmt, stem, tmp_path, capsys):
    from temporalalignnet_amd import search
    parts = [_index(v, fmt, 30 + n, stem, tag=f"s{n}_") for n, v in enumerate(SHARD_VLENS)]
    paths = [str(tmp_path / f"w{n}.npz") for n in range(3)]
    for x, path in zip(parts, paths):
        x.save(path)
    out = str(tmp_path / "all.npz")
    assert search.main(["merge", "--out", out] + paths) == 0            # no checkpoint, no vocabulary, no device
    assert capsys.readouterr().out == ""
    got, want = search.VideoIndex.load(out, device="cpu"), search.VideoIndex.concat(parts)
    assert got.feat.dtype == want.feat.dtype and torch.equal(_bits(got.feat), _bits(want.feat))
    assert got.v_off.tolist() == want.v_off.tolist() and got.vids == want.vids
    assert (got.scale is None) if fmt != "e4m3" else torch.equal(got.scale, want.scale)
    assert (got.stem is None) if stem is None else torch.equal(_bits(got.stem), _bits(want.stem))
    sh = search.ShardedIndex.load(paths, device="cpu")
    assert len(sh) == len(want) and sh.vids == want.vids and sh.v_off.tolist() == want.v_off.tolist()
    for bad in (["merge", "--out", out], ["merge"] + paths, ["merge", "--out", out, "--checkpoint", "c"] + paths):
        with pytest.raises(SystemExit):
            search.parse_args(bad)


def test_cli_takes_shards_and_host_resident():
    from temporalalignnet_amd import search
    argv = ["query", "--checkpoint", "c", "--vocab", "/nonexistent/s3d_dict.npy", "--index", "i.npz"]
    a = search.parse_args(argv + ["--shard", "a.npz", "--shard", "b.npz", "whisk"])
    assert a.index == "i.npz" and a.shard == ["a.npz", "b.npz"] and not a.host_resident and a.sentences == ["whisk"]
    a = search.parse_args(argv + ["--host-resident", "whisk"])
    assert a.host_resident and not a.shard and a.index == "i.npz"
    a = search.parse_args(argv + ["--moments", "--shard", "a.npz", "--host-resident", "whisk"])
    assert a.moments and a.shard == ["a.npz"] and a.host_resident
    a = search.parse_args(argv + ["--sequence", "--shard", "a.npz", "crack", "whisk"])
    assert a.sequence and a.shard == ["a.npz"]
    a = search.parse_args(argv + ["whisk"])
    assert isinstance(a.index, str) and a.index == "i.npz" and not a.shard and not a.host_resident
    for bad in (["--rerank", "--shard", "a.npz", "whisk"], ["--rerank", "--host-resident", "whisk"]):
        with pytest.raises(SystemExit):
            search.parse_args(argv + bad)
    assert search.parse_args(argv + ["--rerank", "whisk"]).rerank
    with pytest.raises(FileNotFoundError):
        search.main(argv + ["--shard", "a.npz", "whisk"])               # parsed; the run stops at the missing vocabulary
