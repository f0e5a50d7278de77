"""Host-side pieces of ordered-sequence search: the C ABI of tan_sequence_topk / tan_sequence_scores, the scratch size,
`search.SequenceHit`, the `query --sequence` command line, and the numpy restatement of the path (sequence_ref.py) pinned against
exhaustive enumeration.  No device needed."""
import ctypes as C
import itertools

import numpy as np
import pytest

import sequence_ref as ref
from temporalalignnet_amd import _lib

i, l, p = C.c_int, C.c_long, C.c_void_p
PROTOS = {
    "tan_sequence_topk_ws_bytes": (l, [l, l, i]),
    "tan_sequence_topk": (i, [p, p, i, l, l, i, p, l, p, l, i, i, p, p, p, p]),
    "tan_sequence_topk_e4m3": (i, [p, p, p, p, l, l, i, p, l, p, l, i, i, p, p, p, p]),
    "tan_sequence_scores": (i, [p, p, i, l, l, i, p, l, p, l, p, p, l, p, l, p]),
    "tan_sequence_scores_e4m3": (i, [p, p, p, p, l, l, i, p, l, p, l, p, p, l, p, l, p]),
}


def test_library_exports_the_sequence_entry_points():
    names, protos, L = _lib.declared_symbols(), _lib.declared_prototypes(), _lib.lib()
    for n, proto in PROTOS.items():
        assert n in names and getattr(L, n) is not None, n
        assert protos[n] == proto, n


def test_bad_arguments_are_rejected_without_touching_a_device():
    L = _lib.lib()
    assert L.tan_sequence_topk(None, None, 0, 8, 40, 512, None, 2, None, 4, 3, 0, None, None, None, None) == -1
    assert L.tan_sequence_topk_e4m3(None, None, None, None, 8, 40, 512, None, 2, None, 4, 3, 0, None, None, None, None) == -1
    assert L.tan_sequence_scores(None, None, 0, 8, 40, 512, None, 2, None, 4, None, None, 3, None, 100, None) == -1
    assert L.tan_sequence_scores_e4m3(None, None, None, None, 8, 40, 512, None, 2, None, 4, None, None, 3, None, 100, None) == -1
    a = C.c_void_p(1 << 20)                            # never dereferenced: every call below fails its argument checks
    odd = C.c_void_p((1 << 20) + 8)
    ptrs = dict(tq=a, vn=a, so=a, vo=a, s=a, v=a, w=a, qs=a, vs=a, hits=a, xo=a, x=a)

    def topk(e4m3=False, Qt=8, N=40, Cc=512, n_seq=2, nv=4, k=3, splits=0, dtype=0, **kw):
        q = dict(ptrs, **kw)
        if e4m3:
            return L.tan_sequence_topk_e4m3(q["tq"], q["qs"], q["vn"], q["vs"], Qt, N, Cc, q["so"], n_seq, q["vo"], nv, k, splits,
                                            q["s"], q["v"], q["w"], None)
        return L.tan_sequence_topk(q["tq"], q["vn"], dtype, Qt, N, Cc, q["so"], n_seq, q["vo"], nv, k, splits, q["s"], q["v"], q["w"], None)

    def scores(e4m3=False, Qt=8, N=40, Cc=512, n_seq=2, nv=4, P=3, n_x=100, dtype=0, **kw):
        q = dict(ptrs, **kw)
        if e4m3:
            return L.tan_sequence_scores_e4m3(q["tq"], q["qs"], q["vn"], q["vs"], Qt, N, Cc, q["so"], n_seq, q["vo"], nv, q["hits"],
                                              q["xo"], P, q["x"], n_x, None)
        return L.tan_sequence_scores(q["tq"], q["vn"], dtype, Qt, N, Cc, q["so"], n_seq, q["vo"], nv, q["hits"], q["xo"], P, q["x"], n_x, None)

    # a width other than 512; n_seq < 1; Qt outside [n_seq, 32 n_seq]; n_videos outside [1, N]; N outside [1, 2^31)
    sizes = (dict(Cc=256), dict(Cc=1024), dict(n_seq=0), dict(n_seq=-1), dict(Qt=1), dict(Qt=65), dict(Qt=0), dict(nv=0), dict(nv=41),
             dict(nv=-1), dict(N=0), dict(N=1 << 31))
    for e4m3 in (False, True):
        for kw in sizes + (dict(k=0), dict(k=33), dict(k=5), dict(k=-1), dict(splits=-1), dict(tq=None), dict(vn=None), dict(so=None),
                           dict(vo=None), dict(s=None), dict(v=None), dict(w=None), dict(tq=odd), dict(vn=odd), dict(w=odd)):
            assert topk(e4m3, **kw) == -1, (e4m3, kw)
        for kw in sizes + (dict(P=0), dict(n_x=0), dict(tq=None), dict(vn=None), dict(so=None), dict(vo=None), dict(hits=None),
                           dict(xo=None), dict(x=None), dict(tq=odd), dict(vn=odd)):
            assert scores(e4m3, **kw) == -1, (e4m3, kw)
    for kw in (dict(qs=None), dict(vs=None)):
        assert topk(True, **kw) == -1 and scores(True, **kw) == -1
    assert topk(dtype=2) == -1 and scores(dtype=2) == -1


def test_scratch_size_does_not_grow_with_the_score_matrix():
    ws = _lib.lib().tan_sequence_topk_ws_bytes
    for bad in ((0, 5, 1), (-1, 5, 1), (5, 0, 1), (5, 1 << 31, 1), (5, 5, 33), (5, 5, 0), (5, 5, -1)):
        assert ws(*bad) == -1, bad
    SPLITS_MAX = 256
    for n_seq, N, k in ((1, 1, 1), (1, 4 << 20, 10), (32, 4 << 20, 10), (2048, 2_000_000, 32), (5, 200003, 1), (100_000, 1 << 30, 32)):
        got = ws(n_seq, N, k)
        assert 0 < got <= 8 * n_seq * k * SPLITS_MAX, (n_seq, N, k, got)                 # the splits' lists and nothing else
    # no Qt x N, n_seq x N or n_seq x n_videos term: beyond 256 tiles of index the size does not move with N at all
    assert ws(32, 1 << 20, 10) == ws(32, 1 << 30, 10) == 8 * 32 * 10 * SPLITS_MAX
    assert ws(32, 4 << 20, 10) < 2 ** 20                                                 # against 16 GiB for 1024 x 4 Mi f32 scores


def test_sequence_hit_fields():
    from temporalalignnet_amd.search import SequenceHit
    assert SequenceHit._fields == ("vid", "seconds", "score")
    h = SequenceHit("v", (3, 3, 9), 1.5)
    assert (h.vid, h.seconds, h.score) == ("v", (3, 3, 9), 1.5) and tuple(h) == ("v", (3, 3, 9), 1.5)


def test_cli_takes_sequence():
    from temporalalignnet_amd import search
    argv = ["query", "--checkpoint", "c", "--vocab", "/nonexistent/s3d_dict.npy", "--index", "i.npz", "-k", "7"]
    a = search.parse_args(argv + ["--sequence", "crack two eggs", "whisk them", "pour into the pan"])
    assert a.sequence and not a.moments and a.k == 7 and a.sentences == ["crack two eggs", "whisk them", "pour into the pan"]
    assert not search.parse_args(argv + ["whisk"]).sequence and not search.parse_args(argv + ["--moments", "whisk"]).sequence
    assert len(search.parse_args(argv + ["--sequence"] + ["s"] * 32).sentences) == 32
    for bad in (["--sequence", "--moments", "whisk"], ["--sequence", "--width", "0.1", "whisk"],
                ["--sequence", "--moments", "--width", "0.1", "whisk"], ["--sequence"], ["--sequence"] + ["s"] * 33):
        with pytest.raises(SystemExit):
            search.parse_args(argv + bad)
    with pytest.raises(SystemExit):
        search.main(argv + ["--sequence", "--moments", "whisk"])                          # refused before anything is loaded
    with pytest.raises(FileNotFoundError):
        search.main(argv + ["--sequence", "whisk", "pour"])                              # parsed; the run stops at the missing vocabulary


def test_search_sequences_checks_its_arguments_before_any_device_work():
    from temporalalignnet_amd import search
    import torch
    idx = search.VideoIndex(torch.zeros(17, 512), [0, 5, 17], ["x", "y"])
    assert search.search_sequences(idx, None, None, []) == []
    for bad in ([[]], [["a"], []], [["s"] * 33]):
        with pytest.raises(ValueError):
            search.search_sequences(idx, None, None, bad)
    with pytest.raises(ValueError):
        search.search_sequences(idx, None, None, [["a"]], k=0)


def test_numpy_path_equals_exhaustive_enumeration():
    """All non-decreasing assignments for m <= 4, V <= 6, integer scores from a range small enough that ties are the rule."""
    rng = np.random.default_rng(11)
    n_ties = 0
    for m in range(1, 5):
        for V in range(1, 7):
            for trial in range(12):
                x = rng.integers(-2, 3, size=(m, V)).astype(np.float32 if trial % 2 else np.int64)
                if trial == 0:
                    x[:] = 1                                                             # every assignment ties
                want = ref.brute_force(x)
                got = ref.path_and_seconds(x)
                assert got[0] == want[0] and got[1] == want[1], (m, V, x, got, want)
                assert all(a <= b for a, b in zip(got[1], got[1][1:])) and len(got[1]) == m
                assert got[0] == sum(x[j, t] for j, t in enumerate(got[1]))
                n_ties += sum(1 for ts in itertools.combinations_with_replacement(range(V), m)
                              if sum(x[j, t] for j, t in enumerate(ts)) == want[0]) > 1
    assert n_ties > 100
    assert ref.path_and_seconds(np.ones((3, 5), dtype=np.float32)) == (3.0, (0, 0, 0))
    assert ref.path_and_seconds(np.array([[0, 5, 0, 5], [5, 0, 0, 5]], dtype=np.float32)) == (10.0, (1, 3))
    assert ref.path_and_seconds(np.array([[1, 2, 3]], dtype=np.int64)) == (3, (2,))
    assert ref.path_and_seconds(np.array([[4], [5], [6]], dtype=np.int64)) == (15, (0, 0, 0))          # V < m


def test_numpy_topk_orders_equal_paths_by_video():
    path = np.array([[1.0, 3.0, 3.0, -np.inf, 2.0], [0.0, 0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    s, v = ref.topk(path, 3)
    assert v.tolist() == [[1, 2, 4], [0, 1, 2]] and s.tolist() == [[3.0, 3.0, 2.0], [0.0, 0.0, 0.0]]
    X = np.arange(12, dtype=np.int64).reshape(3, 4)
    assert ref.paths(X, [0, 1, 3], [0, 1, 4]).tolist() == [[0, 3], [4 + 8, 7 + 11]]
