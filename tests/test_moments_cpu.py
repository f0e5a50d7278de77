"""Host-side pieces of moment search: the C ABI of tan_rank_topk_video / tan_moment_extent, the scratch size, `search.Moment`, and
the `query --moments` command line.  No device needed."""
import ctypes as C

import pytest

from temporalalignnet_amd import _lib

i, l, f, p = C.c_int, C.c_long, C.c_float, C.c_void_p
PROTOS = {
    "tan_rank_topk_video_ws_bytes": (l, [l, l, l, i]),
    "tan_rank_topk_video": (i, [p, p, i, l, l, i, p, l, i, i, p, p, p, p, p]),
    "tan_rank_topk_video_e4m3": (i, [p, p, p, p, l, l, i, p, l, i, i, p, p, p, p, p]),
    "tan_moment_extent": (i, [p, p, i, l, l, i, p, l, i, p, p, p, f, p, p, p]),
    "tan_moment_extent_e4m3": (i, [p, p, p, p, l, l, i, p, l, i, p, p, p, f, p, p, p]),
}


def test_library_exports_the_moment_entry_points():
    names, protos, L = _lib.declared_symbols(), _lib.declared_prototypes(), _lib.lib()
    for n, proto in PROTOS.items():
        assert n in names and getattr(L, n) is not None, n
        assert protos[n] == proto, n


def test_bad_arguments_are_rejected_without_touching_a_device():
    L = _lib.lib()
    assert L.tan_rank_topk_video(None, None, 0, 4, 4, 512, None, 2, 1, 0, None, None, None, None, None) == -1
    assert L.tan_rank_topk_video_e4m3(None, None, None, None, 4, 4, 512, None, 2, 1, 0, None, None, None, None, None) == -1
    assert L.tan_moment_extent(None, None, 0, 4, 4, 512, None, 2, 1, None, None, None, 0.07, None, None, None) == -1
    assert L.tan_moment_extent_e4m3(None, None, None, None, 4, 4, 512, None, 2, 1, None, None, None, 0.07, None, None, None) == -1
    a = C.c_void_p(1 << 20)                            # never dereferenced: every call below fails its argument checks

    def sweep(Q=4, N=40, Cc=512, nv=4, k=3, splits=0, dtype=0):
        return L.tan_rank_topk_video(a, a, dtype, Q, N, Cc, a, nv, k, splits, a, a, a, a, None)

    def extent(Q=4, N=40, Cc=512, nv=4, k=3, width=0.07, dtype=0):
        return L.tan_moment_extent(a, a, dtype, Q, N, Cc, a, nv, k, a, a, a, width, a, a, None)

    sizes = (dict(Cc=256), dict(k=0), dict(k=33), dict(k=5), dict(Q=0), dict(N=0), dict(N=1 << 31), dict(nv=0), dict(nv=41), dict(dtype=2))
    for kw in sizes + (dict(splits=-1),):
        assert sweep(**kw) == -1, kw
    for kw in sizes + (dict(width=-1.0), dict(width=float("nan"))):
        assert extent(**kw) == -1, kw
    assert L.tan_rank_topk_video(C.c_void_p((1 << 20) + 8), a, 0, 4, 40, 512, a, 4, 3, 0, a, a, a, a, None) == -1       # Tq not 16-byte aligned


def test_scratch_size_does_not_grow_with_the_score_matrix():
    L = _lib.lib()
    ws = L.tan_rank_topk_video_ws_bytes
    for bad in ((0, 5, 5, 1), (5, 0, 1, 1), (5, 1 << 31, 5, 1), (5, 5, 5, 33), (5, 5, 5, 0), (5, 5, 5, -1), (5, 5, 0, 1), (5, 5, 6, 1),
                (5, 40, 4, 5)):
        assert ws(*bad) == -1, bad
    SPLITS_MAX = 256
    for Q, N, nv, k in ((1, 1, 1, 1), (1, 4 << 20, 8000, 10), (2048, 2_000_000, 3000, 10), (2048, 2_000_000, 2_000_000, 32),
                        (130, 200003, 1, 1), (100_000, 1 << 30, 1 << 20, 32)):
        got = ws(Q, N, nv, k)
        assert 0 < got <= 12 * Q * k * SPLITS_MAX + 4 * N + 16, (Q, N, nv, k, got)       # the lists, and a row -> video map
        assert got == ws(Q, N, max(k, 1 + nv // 2), k)                                  # no term in n_videos at all
    assert ws(2048, 2_000_000, 3000, 10) + 2048 * 10 * 20 < 96 * 2 ** 20                # against 16 GB for the explicit matrix


def test_moment_fields():
    from temporalalignnet_amd.search import Moment
    assert Moment._fields == ("vid", "start", "end", "second", "score")
    m = Moment("v", 3, 9, 5, 0.5)
    assert (m.vid, m.start, m.end, m.second, m.score) == ("v", 3, 9, 5, 0.5) and tuple(m) == ("v", 3, 9, 5, 0.5)


def test_cli_takes_moments_and_width():
    from temporalalignnet_amd import search
    argv = ["query", "--checkpoint", "c", "--vocab", "/nonexistent/s3d_dict.npy", "--index", "i.npz", "-k", "7"]
    a = search.parse_args(argv + ["--moments", "--width", "0.1", "crack two eggs"])
    assert a.moments and a.width == 0.1 and a.k == 7 and a.sentences == ["crack two eggs"]
    a = search.parse_args(argv + ["--moments", "whisk"])
    assert a.moments and a.width is None
    a = search.parse_args(argv + ["whisk"])
    assert not a.moments and a.width is None
    for bad in (["--width", "0.1", "whisk"], ["--moments", "--width", "-1", "whisk"], ["--moments", "--width", "nan", "whisk"]):
        with pytest.raises(SystemExit):
            search.parse_args(argv + bad)
    with pytest.raises(SystemExit):
        search.main(argv + ["--width", "0.1", "whisk"])                                 # refused before anything is loaded
    with pytest.raises(FileNotFoundError):
        search.main(argv + ["--moments", "--width", "0.1", "whisk"])                    # parsed; the run stops at the missing vocabulary


def test_video_index_keeps_one_device_copy_of_v_off():
    import torch
    from temporalalignnet_amd.search import VideoIndex
    idx = VideoIndex(torch.zeros(17, 512), [0, 5, 17], ["x", "y"])
    v = idx.v_off_device
    assert v.dtype == torch.int32 and v.tolist() == [0, 5, 17] and idx.v_off_device is v and idx.v_off.dtype.kind == "i"
