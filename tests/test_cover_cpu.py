"""Cover search on the host: cover_ref.py (the numpy restatement of tan_cover_topk's definition that test_cover_gpu.py compares the
kernel with) pinned against a brute force over Python Fractions, the C entry points' argument checks, and the host logic of
`ops.cover_topk` / `search.search_cover` / `similar --cover` over CPU indices.  No device is used."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import cover_ref as ref
from temporalalignnet_amd import _lib, ops, search


# ----------------------------------------------------------------------------------------------------------------- the reference
def _to_f32(q):
    """A Fraction rounded to the nearest float32, ties to even (normal range), as a Fraction"""
    if q == 0:
        return Fraction(0)
    e = 0
    while abs(q) / Fraction(2) ** e >= 2 ** 24:
        e += 1
    while abs(q) / Fraction(2) ** e < 2 ** 23:
        e -= 1
    assert e > -126 - 23
    return round(q / Fraction(2) ** e) * Fraction(2) ** e           # round(Fraction): half to even


def _brute(x):
    """x: a list of rows of Fractions -> (fwd, bwd, both) as Fractions, every step of the definition spelled out"""
    m, V = len(x), len(x[0])
    F = sum(round(max(row) * 2 ** 30) for row in x)
    B = sum(round(max(x[i][t] for i in range(m)) * 2 ** 30) for t in range(V))
    fwd = _to_f32(_to_f32(Fraction(F)) / 2 ** 30 / m)
    bwd = _to_f32(_to_f32(Fraction(B)) / 2 ** 30 / V)
    return fwd, bwd, _to_f32(fwd + bwd) / 2


def _as_fraction(f):
    return Fraction(float(f))                                       # exact: every float is a dyadic rational


@pytest.mark.parametrize("negative", (False, True))
def test_cover_ref_equals_the_brute_force_over_fractions(negative):
    rng = np.random.default_rng(3 + negative)
    for trial in range(20):
        # exact inputs: int64 X with score = X / 256
        X = rng.integers(-2 * 256, 2 * 256 + 1, (5, 7)).astype(np.int64)
        if negative:
            X = -np.abs(X) - 1
        want = _brute([[Fraction(int(v), 256) for v in row] for row in X])
        fwd, bwd = ref.block(X, 256)
        got = (fwd, bwd, ref.score(np.float32(fwd).reshape(1), np.float32(bwd).reshape(1), "both")[0])
        assert tuple(_as_fraction(g) for g in got) == want, trial
        if negative:
            assert fwd < 0 and bwd < 0
        # float32 bit patterns, ties of fix() included: multiples of 2^-31 round half to even
        x = (rng.standard_normal((5, 7)) * (0.7 if trial % 2 else 2.0 ** -20)).astype(np.float32)
        x[0, 0] = np.float32(3 * 2.0 ** -31)                        # x * 2^30 = 1.5 -> 2
        x[1, 1] = np.float32(5 * 2.0 ** -31)                        # 2.5 -> 2
        if negative:
            x = -np.abs(x) - np.float32(2.0 ** -31)
        want = _brute([[_as_fraction(v) for v in row] for row in x])
        fwd, bwd = ref.block(x)
        got = (fwd, bwd, ref.score(np.float32(fwd).reshape(1), np.float32(bwd).reshape(1), "both")[0])
        assert tuple(_as_fraction(g) for g in got) == want, trial


def test_fix_rounds_half_to_even_and_the_exact_image_is_a_product():
    assert ref.fix(np.array([1.5, 2.5, -1.5, -2.5, 0.25], dtype=np.float32) * np.float32(2.0 ** -30)).tolist() == [2, 2, -2, -2, 0]
    assert ref.fix(np.array([1.0, -2.0], dtype=np.float32)).tolist() == [1 << 30, -(2 << 30)]
    assert ref.fix(np.array([3, -5], dtype=np.int64), 512).tolist() == [3 << 21, -(5 << 21)]
    x = np.array([[0.5, -0.25]], dtype=np.float32)
    assert ref.block(x) == ref.block((x * 256).astype(np.int64), 256) == (np.float32(0.5), np.float32(0.125))


def test_cover_and_topk_order():
    v_off = np.array([0, 2, 3, 6, 8])                               # V = 2, 1, 3, 2
    q_off = np.array([0, 2, 3])
    X = np.full((3, 8), -256, dtype=np.int64)
    X[0, 3], X[1, 5] = 256, 256                                     # set 0 is in video 2 whole: fwd 1, bwd (1 - 1 + 1) / 3
    X[2, 0], X[2, 1], X[2, 6], X[2, 7] = 128, 128, 128, 128         # set 1 ties on videos 0 and 3
    fwd, bwd = ref.cover(X, q_off, v_off, 256)
    assert fwd[0].tolist() == [-1, -1, 1, -1] and bwd[0, 2] == np.float32(1 / 3)
    assert fwd[1].tolist() == [0.5, -1, -1, 0.5] and bwd[1].tolist() == [0.5, -1, -1, 0.5]
    for rank in ref.RANKS:
        s, r, v = ref.topk(ref.score(fwd, bwd, rank), v_off, 4)
        assert v[0, 0] == 2 and v[1].tolist() == [0, 3, 1, 2] and r[1].tolist() == [0, 6, 2, 3], rank   # ties: the lower row first
        assert s[1, 0] == s[1, 1] == 0.5
    assert ref.topk(ref.score(fwd, bwd, "both"), v_off, 2)[2].tolist() == [[2, 0], [0, 3]]


# ------------------------------------------------------------------------------------------------------------- the C entry points
def test_the_header_declares_what_the_library_exports():
    i, l, p = C.c_int, C.c_long, C.c_void_p
    names, protos, L = _lib.declared_symbols(), _lib.declared_prototypes(), _lib.lib()
    tail = [l, l, i, p, l, p, l, i, i, p, p, p, p, p, p]            # Qt N C q_off n_set v_off n_videos rank k fwd bwd top_* stream
    want = {"tan_cover_max_rows": (i, []), "tan_cover_topk": (i, [p, p, i] + tail), "tan_cover_topk_e4m3": (i, [p, p, p, p] + tail)}
    for n, proto in want.items():
        assert n in names and protos[n] == proto, n
        assert getattr(L, n).argtypes == proto[1] and getattr(L, n).restype == proto[0], n
    assert L.tan_version() >= 107
    assert L.tan_cover_max_rows() == 4096 == ops.COVER_MAX_ROWS == search.MAX_COVER_SECONDS
    assert ops.COVER_RANKS == {"query": 0, "video": 1, "both": 2}


def test_entry_points_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    p = 4096                                                        # a non-NULL, aligned address: every call is refused before use
    good = dict(Tq=p, Vn=p, dtype=1, Qt=40, N=100, C=512, q_off=p, n_set=2, v_off=p, n_videos=5, rank=2, k=3, fwd=p, bwd=p,
                top_score=p, top_row=p, top_video=p)
    bad = [dict(Tq=None), dict(Vn=None), dict(q_off=None), dict(v_off=None), dict(fwd=None), dict(bwd=None), dict(top_score=None),
           dict(top_row=None), dict(top_video=None),
           dict(Tq=p + 8), dict(Vn=p + 4),                          # rows are 16-byte aligned
           dict(C=256), dict(dtype=2), dict(dtype=-1),              # another width, an unknown dtype (-1: the e4m3 twin's, no scales)
           dict(rank=3), dict(rank=-1),
           dict(k=0), dict(k=33), dict(k=6),                        # k in [1, min(32, n_videos)]
           dict(n_set=0), dict(n_set=65536, Qt=65536), dict(Qt=1), dict(Qt=2 * 4096 + 1),
           dict(N=0), dict(N=1 << 31), dict(n_videos=0), dict(n_videos=101)]
    for b in bad:
        a = {**good, **b}
        assert L.tan_cover_topk(*a.values(), None) == -1, b
        e = dict(Tq=a["Tq"], q_scale=p, Vn=a["Vn"], v_scale=p, **{n: a[n] for n in list(a)[3:]})
        if "dtype" not in b:
            assert L.tan_cover_topk_e4m3(*e.values(), None) == -1, b
    e = dict(Tq=p, q_scale=p, Vn=p, v_scale=p, **{n: good[n] for n in list(good)[3:]})
    for b in (dict(q_scale=None), dict(v_scale=None)):
        assert L.tan_cover_topk_e4m3(*{**e, **b}.values(), None) == -1, b


def test_ops_cover_topk_checks_its_arguments_before_any_launch():
    tq, vn = torch.zeros(40, 512), torch.zeros(100, 512)
    q_off, v_off = torch.tensor([0, 10, 40], dtype=torch.int32), torch.tensor([0, 20, 50, 100], dtype=torch.int32)
    for bad in (dict(rank="best"), dict(rank=2), dict(k=0), dict(k=4), dict(k=33),
                dict(q_off=torch.arange(42, dtype=torch.int32)),    # 41 sets over 40 rows
                dict(tq=torch.zeros(4097, 512), q_off=torch.tensor([0, 4097], dtype=torch.int32)),       # one set of 4097 rows
                dict(check_offsets=True, q_off=torch.tensor([1, 10, 40], dtype=torch.int32)),
                dict(check_offsets=True, q_off=torch.tensor([0, 10, 39], dtype=torch.int32)),
                dict(check_offsets=True, q_off=torch.tensor([0, 40, 40], dtype=torch.int32)),
                dict(check_offsets=True, tq=torch.zeros(4100, 512), q_off=torch.tensor([0, 4097, 4100], dtype=torch.int32)),
                dict(check_offsets=True, v_off=torch.tensor([0, 50, 50, 100], dtype=torch.int32)),
                dict(check_offsets=True, v_off=torch.tensor([0, 20, 50, 99], dtype=torch.int32))):
        kw = dict(tq=tq, vn=vn, q_off=q_off, v_off=v_off, k=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.cover_topk(**kw)
    with pytest.raises(TypeError):                                  # scales go with e4m3 codes only
        ops.cover_topk(tq, vn, q_off, v_off, 2, q_scale=torch.ones(40), v_scale=torch.ones(100))
    with pytest.raises(_lib.TanHipError):                           # valid arguments on the host: there is no CPU path
        ops.cover_topk(tq, vn, q_off, v_off, 2, check_offsets=True)


# ------------------------------------------------------------------------------------------------------------------ the host logic
def _cpu_index(e4m3=False):
    feat = torch.randn(60, 512, generator=torch.Generator().manual_seed(5))
    vids, v_off = ["a", "b", "c", "b"], [0, 10, 50, 55, 60]         # equal names are distinct videos
    if e4m3:
        return search.VideoIndex(torch.zeros(60, 512, dtype=torch.uint8), v_off, vids, torch.ones(60))
    return search.VideoIndex(feat, v_off, vids)


def test_search_cover_raises_before_anything_touches_a_device():
    idx = _cpu_index()
    sharded = search.ShardedIndex([search.VideoIndex(idx.feat[:50], [0, 10, 50], ["a", "b"]),
                                   search.VideoIndex(idx.feat[50:], [0, 5, 10], ["c", "b"])])
    bad = ["nope", 4, -1, ("nope", 0, 1), ("a", 5, 4), ("a", 0, 10), torch.zeros(4097, 512), torch.zeros(0, 512), torch.zeros(4, 256),
           torch.zeros(4, 512, dtype=torch.int32), ("a", 1), 1.5]
    for index in (idx, sharded, _cpu_index(e4m3=True)):
        for query in bad:
            with pytest.raises(ValueError):
                search.search_cover(index, [("a", 0, 3), query])
        for kw in (dict(rank="best"), dict(k=0), dict(k=-1), dict(k=0, exclude_source=True)):
            with pytest.raises(ValueError):
                search.search_cover(index, ["a"], **kw)
        assert search.search_cover(index, []) == []
        with pytest.raises(ValueError):
            search.search_cover(index, [], rank="best")
    big = search.VideoIndex(torch.zeros(40, 512), np.arange(41), [f"v{i}" for i in range(40)])
    for k, kw in ((33, {}), (32, dict(exclude_source=True))):
        with pytest.raises(ValueError):
            search.search_cover(big, ["v0"], k=k, **kw)
    long = search.VideoIndex(torch.zeros(4097, 512), [0, 4097], ["v"])
    with pytest.raises(ValueError):                                 # a whole video of 4097 seconds
        search.search_cover(long, ["v"])
    with pytest.raises(_lib.TanHipError):                           # 4096 of them pass every check: no CPU path
        search.search_cover(long, [("v", 1, 4096)])
    assert search.CoverHit("v", 0.5, 0.75, 0.25)._fields == ("vid", "score", "forward", "backward")


def test_similar_cover_command_line():
    argv = ["similar", "--index", "i.npz", "--clip", "vid:0-4095"]
    a = search.parse_args(argv + ["--cover"])
    assert a.cover and a.rank is None and a.clip == [("vid", 0, 4095)] and a.k == 10 and not a.keep_source and not a.align
    a = search.parse_args(argv + ["--cover", "--rank", "video", "-k", "32", "--keep-source", "--shard", "j.npz", "--host-resident"])
    assert a.cover and a.rank == "video" and a.k == 32 and a.keep_source and a.shard == ["j.npz"] and a.host_resident
    for rank in ("both", "query", "video"):
        assert search.parse_args(argv + ["--cover", "--rank", rank]).rank == rank
    for bad in (["--cover", "--align", "--threshold", "0.1"],      # one question at a time
                ["--rank", "query"],                                # --rank needs --cover
                ["--cover", "--rank", "best"],
                ["--cover", "--clip", "vid:0-4096"],                # 4097 seconds
                ["--cover", "-k", "32"], ["--cover", "-k", "0"], ["--cover", "-k", "33", "--keep-source"],
                ["--cover", "--threshold", "0.1"], ["--cover", "--pool", "4"], ["--cover", "--map", "m.csv"]):
        with pytest.raises(SystemExit):
            search.parse_args(argv + bad)
    with pytest.raises(SystemExit):                                 # without --cover a clip still holds at most 32 seconds
        search.parse_args(argv)


def test_existing_similar_invocations_parse_as_before():
    argv = ["similar", "--index", "i.npz", "--clip", "vid:10-29"]
    a = search.parse_args(argv)
    assert (a.cmd, a.clip, a.k, a.keep_source, a.align, a.threshold, a.skew, a.pool, a.piece, a.map, a.shard, a.host_resident) == \
        ("similar", [("vid", 10, 29)], 10, False, False, None, None, None, None, None, None, False)
    assert not a.cover and a.rank is None
    a = search.parse_args(["similar", "--index", "i.npz", "--clip", "vid:0-599", "--align", "--threshold", "0.2", "--skew", "0.01",
                           "--pool", "8", "--piece", "12", "-k", "50", "--map", "m.csv"])
    assert (a.align, a.threshold, a.skew, a.pool, a.piece, a.k, a.map, a.clip) == (True, 0.2, 0.01, 8, 12, 50, "m.csv", [("vid", 0, 599)])
    assert not a.cover
    for bad in (["--clip", "vid:0-32"], ["-k", "32"], ["--threshold", "0.1"], ["--map", "m.csv"]):
        with pytest.raises(SystemExit):
            search.parse_args(argv + bad)
