"""Compound search on the host: compound_ref.py (the numpy restatement of tan_compound_topk's definition that test_compound_gpu.py
compares the kernel with) pinned against a brute force over Python numbers, the host tables of `search.search_compound`, its
refusals, the parsing of `query --all`, and the C entry points' argument checks.  No device is used."""
import ctypes as C
import math
import struct

import numpy as np
import pytest
import torch

import compound_ref as ref
from temporalalignnet_amd import _lib, ops, search


# ----------------------------------------------------------------------------------------------------------------- the reference
def _bits(x):
    return struct.pack("<d", float(x))                              # distinguishes the two zeros


def _brute(x, roles, veto):
    """x: one video's rows as a list per term of Python numbers -> (score, weakest clause, vetoed, peaks [(value, second)]), every
    step of the definition spelled out without numpy"""
    pk = []
    for row in x:
        best = None
        for t, s in enumerate(row):
            if best is None or s > best[0]:
                best = (s, t)
        pk.append(best)
    vetoed = any(r < 0 and p[0] >= veto for p, r in zip(pk, roles))
    score = weakest = None
    for j in range(32):
        mine = [p[0] for p, r in zip(pk, roles) if r == j]
        if not mine:
            continue
        g = mine[0]
        for s in mine[1:]:
            if s > g:
                g = s
        if score is None or g < score:
            score, weakest = g, j
    return score, weakest, vetoed, pk


def _random_case(rng, zeros):
    nq, nv = int(rng.integers(1, 4)), int(rng.integers(1, 7))
    ms = rng.integers(1, 7, nq)
    lens = rng.integers(0 if nv > 1 else 1, 6, nv)
    if lens.sum() == 0:
        lens[0] = 2
    t_off, v_off = np.concatenate([[0], np.cumsum(ms)]), np.concatenate([[0], np.cumsum(lens)])
    role = np.concatenate([np.concatenate([[int(rng.integers(0, 3))], rng.integers(-1, 3, m - 1)]) for m in ms]).astype(np.int32)
    X = rng.integers(-2, 3, (int(ms.sum()), int(lens.sum())))      # a small range: ties everywhere
    if zeros:
        X = X.astype(np.float32)
        X[(X == 0) & (rng.random(X.shape) < 0.5)] = -0.0
    return X, t_off, role, v_off


@pytest.mark.parametrize("zeros", (False, True))
def test_the_reference_equals_a_brute_force(zeros):
    rng = np.random.default_rng(11 + zeros)
    seen_veto = seen_short = seen_sign = 0
    for _ in range(300):
        X, t_off, role, v_off = _random_case(rng, zeros)
        veto = [math.inf, 1, 0, 2][int(rng.integers(0, 4))]
        k = int(rng.integers(1, len(v_off)))
        top_s, top_v, p, r, score, cand, weakest = ref.compound(X, t_off, role, v_off, veto, k)
        assert p.dtype == X.dtype and score.dtype == X.dtype
        for q in range(len(t_off) - 1):
            a, b = int(t_off[q]), int(t_off[q + 1])
            want = []
            for v in range(len(v_off) - 1):
                lo, hi = int(v_off[v]), int(v_off[v + 1])
                if hi == lo:
                    assert not cand[q, v] and (r[a:b, v] == ref.SENT).all()
                    continue
                s, w, vetoed, pk = _brute([[X[t, n].item() for n in range(lo, hi)] for t in range(a, b)], role[a:b].tolist(), veto)
                assert [(_bits(p[t, v]), int(r[t, v]) - lo) for t in range(a, b)] == [(_bits(x), t) for x, t in pk], (q, v)
                assert _bits(score[q, v]) == _bits(s) and weakest[q, v] == w and cand[q, v] == (not vetoed), (q, v)
                assert search.compound_weakest(p[a:b, v], role[a:b]) == (score[q, v], w)
                seen_veto += vetoed
                seen_sign += zeros and s == 0 and math.copysign(1, s) < 0
                if not vetoed:
                    want.append((s, v))
            want.sort(key=lambda c: (-c[0], c[1]))                  # stable, and -(+-0) compare equal: equal scores by video
            seen_short += len(want) < k
            got = [(top_s[q, i], int(top_v[q, i])) for i in range(k)]
            assert [(_bits(s), v) for s, v in got[:len(want[:k])]] == [(_bits(s), v) for s, v in want[:k]], q
            assert all(s == -math.inf and v == ref.SENT for s, v in got[len(want):]), q
    assert seen_veto > 20 and seen_short > 5 and (seen_sign > 5 or not zeros)


def test_the_first_of_equal_rows_terms_and_clauses_wins():
    X = np.array([[1, 3, 3, 0, 5],
                  [3, 0, 1, 5, 5],
                  [0, 2, 2, 9, 9]])
    t_off, v_off = np.array([0, 3]), np.array([0, 3, 3, 5])
    p, r = ref.peaks(X, t_off, v_off)
    assert p.tolist() == [[3, 0, 5], [3, 0, 5], [2, 0, 9]] and r.tolist() == [[1, ref.SENT, 4], [0, ref.SENT, 3], [1, ref.SENT, 3]]
    score, cand, weakest = ref.scores(p, r, t_off, np.array([1, 0, -1]), 9)
    assert score.tolist() == [[3, 0, 5]] and weakest.tolist() == [[0, -1, 0]] and cand.tolist() == [[True, False, False]]
    score, cand, weakest = ref.scores(p, r, t_off, np.array([4, 4, 7]), math.inf)
    assert score.tolist() == [[2, 0, 5]] and weakest.tolist() == [[7, -1, 4]] and cand.tolist() == [[True, False, True]]
    top_s, top_v = ref.topk(score, cand, 3)
    assert top_v.tolist() == [[2, 0, ref.SENT]] and top_s.tolist() == [[5, 2, -math.inf]]


# ------------------------------------------------------------------------------------------------------------------ the host tables
def test_compound_tables_for_mixed_clauses():
    Cq = search.Compound
    qs = [Cq(["a", ["b1", "b2", "b3"], "c"], ["x", "y"]), Cq([["d"]]), Cq(["e", ("f1", "f2")], "z"), Cq(all=["g"], none=[])]
    sentences, t_off, role = search.compound_tables(qs)
    assert sentences == ["a", "b1", "b2", "b3", "c", "x", "y", "d", "e", "f1", "f2", "z", "g"]
    assert t_off.tolist() == [0, 7, 8, 12, 13] and t_off.dtype == np.int64
    assert role.tolist() == [0, 1, 1, 1, 2, -1, -1, 0, 0, 1, 1, -1, 0] and role.dtype == np.int32
    assert Cq(["a"]).none == ()
    # 32 terms fit, in any mix
    s, t, r = search.compound_tables([Cq([["p"] * 10] + ["q"] * 12, ["n"] * 10)])
    assert len(s) == 32 and t.tolist() == [0, 32] and r.tolist() == [0] * 10 + list(range(1, 13)) + [-1] * 10
    assert search.compound_weakest(np.float32([0.5, 0.25, 0.75, 0.25, 9.0]), np.int32([2, 0, 0, 1, -1])) == (np.float32(0.25), 1)
    assert search.compound_weakest(np.float32([0.5, 0.5]), np.int32([3, 1])) == (np.float32(0.5), 1)


def _cpu_index():
    return search.VideoIndex(torch.zeros(60, 512), [0, 10, 50, 55, 60], ["a", "b", "c", "d"])


def test_search_compound_raises_before_anything_touches_a_device():
    Cq, idx = search.Compound, _cpu_index()
    sharded = search.ShardedIndex([search.VideoIndex(idx.feat[:50], [0, 10, 50], ["a", "b"]),
                                   search.VideoIndex(idx.feat[50:], [0, 5, 10], ["c", "d"])])
    for index in (idx, sharded):
        assert search.search_compound(index, None, None, []) == []
        for bad, kw in (([Cq(["a", []])], {}),                      # an empty clause
                        ([Cq([], ["x"])], dict(veto=0.5)),          # no clause at all
                        ([Cq([])], {}),
                        ([Cq(["s"] * 33)], {}),                     # more than 32 terms
                        ([Cq([["s"] * 20], ["n"] * 13)], dict(veto=0.5)),
                        ([Cq(["a"], ["x"])], {}),                   # none without veto
                        ([Cq(["a"]), Cq(["b"], ["x"])], {}),
                        ([Cq(["a"])], dict(veto=0.5)),              # veto without any none
                        ([Cq(["a"], ["x"])], dict(veto=float("nan"))),
                        ([Cq(["a"])], dict(k=0)),                   # k outside [1, 32] after clamping to the four videos
                        ([Cq(["a"])], dict(k=-3))):
            with pytest.raises(ValueError):
                search.search_compound(index, None, None, bad, **kw)


# ---------------------------------------------------------------------------------------------------------------- the command line
QUERY = ["query", "--checkpoint", "c", "--vocab", "v", "--index", "i"]


def test_query_all_parses_clauses_and_alternatives():
    a = search.parse_args(QUERY + ["--all", "whisk eggs", "fry bacon | cook bacon|bacon", "--none", "microwave", "oven", "--veto", "0.3",
                                   "-k", "5"])
    assert a.all_ and a.clauses == [["whisk eggs"], ["fry bacon", "cook bacon", "bacon"]] and a.none == ["microwave", "oven"]
    assert a.veto == 0.3 and a.k == 5
    a = search.parse_args(QUERY + ["--all", "one"])
    assert a.clauses == [["one"]] and a.none is None and a.veto is None
    a = search.parse_args(QUERY + ["--all", "--none", "x", "--none", "y", "--veto", "-1", "a|b"])
    assert a.clauses == [["a", "b"]] and a.none == ["x", "y"] and a.veto == -1.0
    assert not search.parse_args(QUERY + ["a|b"]).all_             # without --all a `|` is part of the sentence
    assert search.parse_args(QUERY + ["a|b"]).sentences == ["a|b"]
    thirty_two = ["|".join(["s"] * 10)] + ["t"] * 12 + ["--none"] + ["n"] * 10 + ["--veto", "1"]
    assert sum(len(c) for c in search.parse_args(QUERY + ["--all"] + thirty_two).clauses) == 22


@pytest.mark.parametrize("bad", (
    ["--all", "--moments", "a"], ["--all", "--sequence", "a"], ["--all", "--rerank", "a"], ["--all", "--coarse", "f.npz", "a"],
    ["--all", "--width", "0.1", "a"], ["--all", "--pool", "8", "a"],
    ["--all", "--only", "v", "a"], ["--all", "--only-file", "f", "a"], ["--all", "--exclude", "v", "a"], ["--all", "--exclude-file", "f", "a"],
    ["--all", "--within", "v:1-2", "a"],
    ["--all", "a", "--none", "x"],                                  # --none without --veto
    ["--all", "a", "--veto", "0.5"],                                # --veto without --none
    ["--all", "a", "--none", "x", "--veto", "nan"],
    ["a", "--none", "x", "--veto", "0.5"], ["a", "--veto", "0.5"],  # both need --all
    ["--all", "a|", "b"], ["--all", "a||b"], ["--all", " "],        # an empty alternative
    ["--all"] + ["s"] * 33,                                         # more than 32 terms
    ["--all", "|".join(["s"] * 20)] + ["t"] * 3 + ["--none"] + ["n"] * 10 + ["--veto", "1"]))
def test_query_all_refusals(bad, capsys):
    with pytest.raises(SystemExit) as e:
        search.parse_args(QUERY + bad)
    assert e.value.code == 2
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------- the C entry points
def test_the_header_declares_what_the_library_exports():
    i, l, p, f = C.c_int, C.c_long, C.c_void_p, C.c_float
    names, protos, L = _lib.declared_symbols(), _lib.declared_prototypes(), _lib.lib()
    topk = [l, l, i, p, p, l, p, l, f, i, i, p, p, p, p]            # Qt N C t_off role n_query v_off n_videos veto k splits top_* ws stream
    peak = [l, l, i, p, l, p, l, p, l, p, p, p]                     # Qt N C t_off n_query v_off n_videos hits n_hits peak_* stream
    want = {"tan_compound_topk_ws_bytes": (l, [l, l, i]),
            "tan_compound_topk": (i, [p, p, i] + topk), "tan_compound_topk_e4m3": (i, [p, p, p, p] + topk),
            "tan_compound_peaks": (i, [p, p, i] + peak), "tan_compound_peaks_e4m3": (i, [p, p, p, p] + peak)}
    for n, proto in want.items():
        assert n in names and protos[n] == proto, n
        assert getattr(L, n).argtypes == proto[1] and getattr(L, n).restype == proto[0], n
    assert L.tan_version() >= 110


def test_the_scratch_size():
    ws = ops.compound_topk_ws_bytes
    assert ws(3, 40, 3) == 1 * 3 * 3 * 8 and ws(5, 2742, 32) == 43 * 5 * 32 * 8 and ws(1, 64 * 300, 1) == 256 * 8
    assert ws(3, 40, 3) == ops.sequence_topk_ws_bytes(3, 40, 3)
    for bad in ((0, 40, 3), (3, 0, 3), (3, 1 << 31, 3), (3, 40, 0), (3, 40, 33), (1 << 29, 40, 3)):
        assert _lib.lib().tan_compound_topk_ws_bytes(*bad) == -1, bad
        with pytest.raises(_lib.TanHipError):
            ws(*bad)


def test_entry_points_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    p = 4096                                                        # a non-NULL, aligned address: every call is refused before use
    sizes = [dict(C=256), dict(dtype=2), dict(dtype=-1),            # another width, an unknown dtype (-1: the e4m3 twin's, no scales)
             dict(n_query=0), dict(Qt=1), dict(Qt=2 * 32 + 1), dict(N=0), dict(N=1 << 31), dict(n_videos=0), dict(n_videos=101),
             dict(Tq=None), dict(Vn=None), dict(t_off=None), dict(v_off=None), dict(Tq=p + 8), dict(Vn=p + 4)]
    good = dict(Tq=p, Vn=p, dtype=1, Qt=40, N=100, C=512, t_off=p, role=p, n_query=2, v_off=p, n_videos=5, veto=0.5, k=3, splits=0,
                top_score=p, top_video=p, ws=p)
    bad = sizes + [dict(role=None), dict(top_score=None), dict(top_video=None), dict(ws=None), dict(ws=p + 8),
                   dict(k=0), dict(k=33), dict(k=6), dict(splits=-1), dict(veto=float("nan"))]
    for b in bad:
        a = {**good, **b}
        assert L.tan_compound_topk(*a.values(), None) == -1, b
        if "dtype" not in b:
            e = dict(Tq=a["Tq"], q_scale=p, Vn=a["Vn"], v_scale=p, **{n: a[n] for n in list(a)[3:]})
            assert L.tan_compound_topk_e4m3(*e.values(), None) == -1, b
    good_p = dict(Tq=p, Vn=p, dtype=1, Qt=40, N=100, C=512, t_off=p, n_query=2, v_off=p, n_videos=5, hits=p, n_hits=4, peak_score=p,
                  peak_row=p)
    for b in sizes + [dict(hits=None), dict(peak_score=None), dict(peak_row=None), dict(n_hits=0), dict(n_hits=-1), dict(n_hits=1 << 26)]:
        a = {**good_p, **b}
        assert L.tan_compound_peaks(*a.values(), None) == -1, b
        if "dtype" not in b:
            e = dict(Tq=a["Tq"], q_scale=p, Vn=a["Vn"], v_scale=p, **{n: a[n] for n in list(a)[3:]})
            assert L.tan_compound_peaks_e4m3(*e.values(), None) == -1, b
    for b in (dict(q_scale=None), dict(v_scale=None)):
        e = dict(Tq=p, q_scale=p, Vn=p, v_scale=p)
        e.update(b)
        assert L.tan_compound_topk_e4m3(*e.values(), *list(good.values())[3:], None) == -1, b
        assert L.tan_compound_peaks_e4m3(*e.values(), *list(good_p.values())[3:], None) == -1, b


def test_ops_check_their_arguments_before_any_launch():
    tq, vn = torch.zeros(8, 512), torch.zeros(40, 512)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)              # noqa: E731
    t_off, v_off, role = i32([0, 3, 4, 8]), i32([0, 10, 11, 25, 40]), i32([0, 0, -1, 5, 31, -1, -1, 2])
    for bad in (dict(t_off=i32([0, 3, 3, 8])), dict(t_off=i32([1, 3, 4, 8])), dict(t_off=i32([0, 3, 4, 7])),
                dict(v_off=i32([0, 10, 10, 25, 40])), dict(v_off=i32([0, 10, 11, 25, 39])),
                dict(role=i32([0, 0, -1, 5, 32, -1, -1, 2])),       # a role above 31
                dict(role=i32([0, 0, -2, 5, 31, -1, -1, 2])),       # a role below -1
                dict(role=i32([0, 0, -1, -1, 31, -1, -1, 2])),      # the second query has no clause term
                dict(role=i32([0, 0, -1, 5, -1, -1, -1, -1])),      # nor has the third
                dict(tq=torch.zeros(40, 512), t_off=i32([0, 33, 40]), role=torch.zeros(40, dtype=torch.int32))):    # 33 terms
        kw = dict(tq=tq, vn=vn, t_off=t_off, role=role, v_off=v_off, k=3, check_offsets=True)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.compound_topk(**kw)
    with pytest.raises(ValueError):
        ops.compound_topk(tq, vn, t_off, role, v_off, 3, veto=float("nan"))
    with pytest.raises(AssertionError):
        ops.compound_topk(tq, vn, t_off, role[:7], v_off, 3)
    with pytest.raises(ValueError):
        ops.compound_peaks(tq, vn, i32([0, 3, 3, 8]), v_off, torch.zeros(2, 2, dtype=torch.int32), check_offsets=True)
    with pytest.raises(TypeError):                                  # scales go with e4m3 codes only
        ops.compound_topk(tq, vn, t_off, role, v_off, 3, q_scale=torch.ones(8), v_scale=torch.ones(40))
    with pytest.raises(_lib.TanHipError):                           # valid arguments on the host: there is no CPU path
        ops.compound_topk(tq, vn, t_off, role, v_off, 3, check_offsets=True)
    with pytest.raises(_lib.TanHipError):
        ops.compound_peaks(tq, vn, t_off, v_off, torch.zeros(2, 2, dtype=torch.int32), check_offsets=True)
