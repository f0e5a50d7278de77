"""Chapters without a device: the numpy reference of tan_chapter_costs / tan_chapter_decode (chapter_ref.py) against a plain-Python
brute force over Python ints, the 'six scenes' and 'A B A' inputs of the GPU test shown to satisfy the reference alone (in f32, and
with the rows rounded to bf16 and to e4m3 codes with row scales), every argument the entry points and the wrappers refuse, the
parsed prototypes, the pass planning of `search.chapters`, `Chapters.spans` through `transfer_segments`, and the command line
with its CSV writer."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import chapter_ref as ref
import storyboard_ref
from temporalalignnet_amd import _lib, ops, search
from test_retrieve_fp8_gpu import _host_quant


# ------------------------------------------------------------------------------------------------------------------- the reference
def _small_block(V, trial, rng):
    """few distinct values (ties everywhere), not symmetric; trial 1 all negative; trial 2 halves of the fixed-point unit; trial 3
    strongly asymmetric (the upper triangle dwarfs the lower)"""
    x = rng.integers(-3, 4, (V, V)).astype(np.float32) / np.float32(4)
    if trial == 1:
        x = -np.abs(x) - np.float32(0.25)
    if trial == 2:
        x = (rng.integers(-5, 6, (V, V)) * 0.5).astype(np.float32) * np.float32(2.0 ** -30)
    if trial == 3:
        x = np.triu(x * np.float32(2), 1) + np.tril(x / np.float32(64))
    return x


def test_reference_against_brute_force_for_every_small_block_shape():
    rng = np.random.default_rng(12)
    for V in range(1, 9):
        for trial in range(4):
            x = _small_block(V, trial, rng)
            F = [[int(v) for v in row] for row in ref.fix(x)]
            J = ref.costs(x)
            for s in range(V):                                      # the costs: direct double sums with Python's //
                for e in range(s + 1, V + 1):
                    D = sum(F[t][t] for t in range(s, e))
                    Q = sum(F[i][t] for i in range(s, e) for t in range(s, e))
                    assert int(J[s, e]) == D - Q // (e - s), (V, trial, s, e)
            block, mask = ref.cost_block(x)
            assert all(int(block[e - 1, s]) == int(J[s, e]) for s in range(V) for e in range(s + 1, V + 1)) and mask.sum() == V * (V + 1) // 2
            for min_len in (1, 2, 3):
                _, levels = ref.brute(F, V + 1, min_len, 0)
                drops = sorted({levels[j] - levels[j + 1] for j in levels if j + 1 in levels})
                between = [(drops[0] + drops[-1]) / 2.0 ** 31] if drops and drops[-1] > 0 else []
                for penalty in [0.0, 1e30] + [p for p in between if p > 0]:
                    G = ref.g_of(penalty)
                    for k in range(1, V + 2):
                        want_count, want_levels = ref.brute(F, k, min_len, G)
                        count, start, scatter, chapter = ref.decode(J, k, min_len, penalty)
                        what = (V, trial, min_len, penalty, k)
                        assert count == want_count, what
                        for j in range(1, k + 1):                   # every level's exact minimum, +inf where there is no such cut
                            if j in want_levels:
                                assert scatter[j - 1] == np.int64(want_levels[j]).astype(np.float32) * np.float32(2.0 ** -30), what
                            else:
                                assert np.isposinf(scatter[j - 1]), what
                        starts, total = ref.dp_starts(F, count, min_len)
                        assert start[:count].tolist() == starts and (start[count:] == -1).all() and total == want_levels[count], what
                        edges = starts + [V]
                        assert chapter.tolist() == [c for c in range(count) for _ in range(edges[c + 1] - edges[c])], what
                        assert count == 1 or min(np.diff(edges)) >= min_len, what
                        if penalty == 1e30:
                            assert count == 1, what


def test_reference_properties_on_hand_made_blocks():
    assert ref.g_of(0.0) == 0 and ref.g_of(1.0) == 1 << 30 and ref.g_of(3e38) == ref.MAX_G == ref.g_of(2.0 ** 20) and ref.g_of(1e30) == ref.MAX_G
    J = ref.costs(np.full((5, 5), 0.375, np.float32))               # all equal: no scatter anywhere, one chapter under any penalty > 0
    assert (J == 0).all()
    assert ref.decode(J, 4, 1, 2.0 ** -30)[0] == 1 and ref.decode(J, 4, 1, 0.0)[0] == 1          # equal totals: the lowest j
    # block-diagonal 0/1: two scenes of a and b seconds; one chapter costs (a + b) - (a^2 + b^2) / (a + b) = 2ab / (a + b), two cost 0
    a, b = 3, 6                                                     # 2ab / (a + b) = 4 exactly
    x = np.zeros((a + b, a + b), np.float32)
    x[:a, :a], x[a:, a:] = 1, 1
    J = ref.costs(x)
    assert int(J[0, a + b]) == 4 << 30 and int(J[0, a]) == 0 == int(J[a, a + b])
    drop = np.float32(4)
    for penalty, want in ((0.0, 2), (float(np.nextafter(drop, np.float32(0))), 2), (float(drop), 1), (float(np.nextafter(drop, np.float32(9))), 1)):
        count, start, scatter, chapter = ref.decode(J, 2, 1, penalty)                             # drop == G: equal totals, the lowest j
        assert count == want and scatter.tolist() == [4.0, 0.0], penalty
        assert start.tolist() == ([0, a] if want == 2 else [0, -1]) and chapter.tolist() == ([0] * a + [1] * b if want == 2 else [0] * (a + b))
    # min_len: a video shorter than min_len is one chapter; V // min_len bounds the levels
    count, start, scatter, _ = ref.decode(J, 4, 10, 0.0)
    assert count == 1 and start.tolist() == [0, -1, -1, -1] and scatter[0] == 4.0 and np.isposinf(scatter[1:]).all()
    count, start, scatter, _ = ref.decode(J, 4, 4, 0.0)
    assert count == 2 and np.isfinite(scatter[:2]).all() and np.isposinf(scatter[2:]).all() and 4 <= start[1] <= 5


def _quantised(rows, fmt):
    """the rows as an index of this format holds them, dequantised to f32"""
    t = torch.from_numpy(rows)
    if fmt == "bf16":
        return t.bfloat16().float().numpy()
    if fmt == "e4m3":
        codes, scale, _ = _host_quant(t)
        return (codes.view(torch.float8_e4m3fn).float() * scale[:, None]).numpy()
    return rows


@pytest.mark.parametrize("fmt", ("f32", "bf16", "e4m3"))
def test_six_scenes_satisfy_the_reference_alone(fmt):
    """The GPU test's 'meaning' input: with k = 10 and penalty 1.0 six chapters whose starts are exactly the scene changes, and each of
    the five real boundaries lowers the summed scatter by more than ten times what a sixth boundary does (in f32 at least 6.18
    against at most 0.107)."""
    least, most = np.inf, 0.0
    for seed in range(20):
        rows, scene = storyboard_ref.scenes(seed)
        rows = _quantised(rows, fmt)
        count, start, scatter, chapter = ref.decode(ref.costs(rows @ rows.T), 10, 1, 1.0)
        assert count == 6 and start[:6].tolist() == [0] + (np.flatnonzero(np.diff(scene)) + 1).tolist(), (fmt, seed)
        assert np.array_equal(chapter, scene), (fmt, seed)
        drop = -np.diff(scatter.astype(np.float64))
        assert (drop[:5] > 10 * drop[5]).all(), (fmt, seed, drop)
        least, most = min(least, drop[:5].min()), max(most, drop[5])
        for penalty in (0.25, 0.5, 2.0):
            assert ref.decode(ref.costs(rows @ rows.T), 10, 1, penalty)[0] == 6, (fmt, seed, penalty)
    print(f"chapters scenes {fmt}: the five real drops are at least {least:.3f}, the sixth at most {most:.3f}")
    assert least > 1.0 > most                                       # penalty 1.0 separates them on every format


def test_a_scene_that_comes_back_is_three_chapters_but_one_storyboard_entry():
    for seed in range(5):
        rows, scene = ref.scenes_aba(seed)
        x = rows @ rows.T
        count, start, scatter, chapter = ref.decode(ref.costs(x), 10, 1, 1.0)
        cuts = (np.flatnonzero(np.diff(scene)) + 1).tolist()
        assert count == 3 and start[:3].tolist() == [0] + cuts and chapter.tolist() == [0] * cuts[0] + [1] * (cuts[1] - cuts[0]) + [2] * (len(scene) - cuts[1])
        second, coverage, owner = storyboard_ref.select(x, 10, 0.01)
        assert int((second >= 0).sum()) == 2 and scene[second[0]] == 0 and scene[second[1]] == 1
        assert np.array_equal(owner, scene)                         # the first entry owns both stretches of scene A


# ------------------------------------------------------------------------------------------------------------- the C entry points
def test_the_header_declares_what_the_library_exports():
    i, l, p, f = C.c_int, C.c_long, C.c_void_p, C.c_float
    names, protos, L = _lib.declared_symbols(), _lib.declared_prototypes(), _lib.lib()
    want = {"tan_chapter_max_rows": (i, []),
            "tan_chapter_costs": (i, [p, l, p, p, l, p, p]),
            "tan_chapter_decode_ws_bytes": (l, [l, l, i]),
            "tan_chapter_decode": (i, [p, l, p, p, l, l, i, i, f, p, p, p, p, p, p])}
    for n, proto in want.items():
        assert n in names and protos[n] == proto, n
        assert getattr(L, n).argtypes == proto[1] and getattr(L, n).restype == proto[0], n
    assert L.tan_version() >= 109
    assert L.tan_chapter_max_rows() == 4096 == ops.CHAPTER_MAX_ROWS == search.MAX_CHAPTER_SECONDS == ref.MAX_ROWS
    assert ops.CHAPTER_MAX_K == search.MAX_CHAPTER_K == ref.MAX_K == 256
    assert L.tan_chapter_decode_ws_bytes(3, 100, 12) == 100 * 12 * 2 == ops.chapter_decode_ws_bytes(3, 100, 12)
    for bad in ((0, 100, 12), (1 << 31, (1 << 31) - 1, 1), (3, 2, 12), (3, 1 << 31, 12), (3, 100, 0), (3, 100, 257)):
        assert L.tan_chapter_decode_ws_bytes(*bad) == -1, bad


def test_entry_points_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    p = 4096                                                        # a non-NULL address: every call is refused before use
    good = dict(x=p, n_x=100, x_off=p, table=p, P=2, cost=p)
    for b in (dict(x=None), dict(x_off=None), dict(table=None), dict(cost=None), dict(n_x=0), dict(n_x=-5), dict(P=0), dict(P=-1),
              dict(P=1 << 31)):
        assert L.tan_chapter_costs(*{**good, **b}.values(), None) == -1, b
    good = dict(cost=p, n_x=100, x_off=p, table=p, P=2, sum_V=10, k=8, min_len=1, penalty=0.0, count=p, start=p, scatter=p, chapter=p, ws=p)
    bad = [dict(cost=None), dict(x_off=None), dict(table=None), dict(count=None), dict(start=None), dict(scatter=None), dict(chapter=None),
           dict(ws=None), dict(n_x=0), dict(n_x=-5), dict(P=0), dict(P=-1), dict(P=1 << 31, sum_V=(1 << 31) - 1), dict(sum_V=1), dict(sum_V=0),
           dict(sum_V=1 << 31), dict(k=0), dict(k=-1), dict(k=257), dict(min_len=0), dict(min_len=-2), dict(min_len=4097),
           dict(penalty=-1e-9), dict(penalty=float("inf")), dict(penalty=float("nan")), dict(penalty=-float("inf"))]
    for b in bad:
        assert L.tan_chapter_decode(*{**good, **b}.values(), None) == -1, b


def test_ops_wrappers_check_their_arguments_before_any_launch():
    x, x_off = torch.zeros(13), torch.tensor([0, 4], dtype=torch.int64)
    table = torch.tensor([[2, 0], [3, 2]], dtype=torch.int32)
    cost = torch.zeros(13, dtype=torch.int64)
    for bad in (dict(x=torch.zeros(13, dtype=torch.float64)), dict(x=torch.zeros(0)), dict(x=torch.zeros(13, 1)), dict(x=torch.zeros(26)[::2]),
                dict(x_off=x_off.int()), dict(x_off=torch.zeros(0, dtype=torch.int64)), dict(x_off=x_off[None]),
                dict(table=table.long()), dict(table=table[:1]), dict(table=torch.zeros(2, 3, dtype=torch.int32)),
                dict(out=cost.int()), dict(out=cost[:12]), dict(out=torch.zeros(26, dtype=torch.int64)[::2])):
        kw = dict(x=x, x_off=x_off, table=table, out=cost)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.chapter_costs(**kw)
    for kw in (dict(out=cost), {}):                                 # valid arguments on the host: there is no CPU path
        with pytest.raises(_lib.TanHipError):
            ops.chapter_costs(x, x_off, table, **kw)
    out = (torch.zeros(2, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4), torch.zeros(5, dtype=torch.int32))
    ws = torch.zeros(5 * 4 * 2, dtype=torch.uint8)
    for bad in (dict(cost=cost.int()), dict(cost=torch.zeros(0, dtype=torch.int64)), dict(cost=cost[:, None]),
                dict(x_off=x_off.int()), dict(x_off=x_off[None]), dict(table=table.long()), dict(table=table[:1]),
                dict(k=0), dict(k=257), dict(k=-3), dict(min_len=0), dict(min_len=4097),
                dict(penalty=-0.1), dict(penalty=float("inf")), dict(penalty=float("nan")),
                dict(sum_V=1), dict(sum_V=2 ** 31), dict(sum_V=4),              # below P; too large; not chapter's size
                dict(out=(out[0], out[1], out[2], torch.zeros(6, dtype=torch.int32))),        # (sum_V read from the table: 5)
                dict(out=(out[0].long(), out[1], out[2], out[3])), dict(out=(out[0], out[1], out[2].double(), out[3])),
                dict(out=(out[0], out[1][:, :3], out[2], out[3])), dict(out=(out[0][:1], out[1], out[2], out[3])),
                dict(out=out[:3]), dict(k=5),                                   # out holds k = 4 entries
                dict(ws=ws[:-1]), dict(ws=ws.int()), dict(ws=ws[:-1], sum_V=5)):
        kw = dict(cost=cost, x_off=x_off, table=table, k=4, penalty=1.0, out=out, ws=ws)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.chapter_decode(**kw)
    with pytest.raises(TypeError):                                  # penalty has no default
        ops.chapter_decode(cost, x_off, table, 4)
    for kw in (dict(out=out, ws=ws), dict(sum_V=5), {}):
        with pytest.raises(_lib.TanHipError):
            ops.chapter_decode(cost, x_off, table, 4, penalty=1.0, **kw)


# ------------------------------------------------------------------------------------------------------------------ the host logic
def _cpu_index(e4m3=False, long=False):
    vids, v_off = ["a", "b", "c", "b"], [0, 10, 50, 55, 60]         # equal names are distinct videos
    if long:
        vids, v_off = vids + ["long", "edge"], v_off + [60 + 4097, 60 + 4097 + 4096]
    n = v_off[-1]
    if e4m3:
        return search.VideoIndex(torch.zeros(n, 512, dtype=torch.uint8), v_off, vids, torch.ones(n))
    return search.VideoIndex(torch.zeros(n, 512), v_off, vids)


def test_chapters_raises_before_anything_touches_a_device():
    idx = _cpu_index()
    sharded = search.ShardedIndex([search.VideoIndex(idx.feat[:50], [0, 10, 50], ["a", "b"]),
                                   search.VideoIndex(idx.feat[50:], [0, 5, 10], ["c", "b"])])
    for index in (idx, sharded, _cpu_index(e4m3=True)):
        for kw in (dict(k=0), dict(k=257), dict(penalty=-1.0), dict(penalty=float("nan")), dict(penalty=float("inf")),
                   dict(min_len=0), dict(min_len=4097), dict(budget=0), dict(budget=2 ** 31)):
            with pytest.raises(ValueError, match="^chapters: "):
                search.chapters(index, **{"k": 8, "penalty": 1.0, **kw})
        with pytest.raises(TypeError):                              # penalty has no default
            search.chapters(index)
        for videos in (["nope"], [4], [-1], [1.5]):
            with pytest.raises(KeyError, match="chapters"):
                search.chapters(index, penalty=1.0, videos=videos)
        with pytest.raises(_lib.TanHipError):                       # everything checks out: there is no CPU path
            search.chapters(index, penalty=1.0, videos=["b"])
        got = search.chapters(index, penalty=1.0, videos=[])        # nothing wanted: nothing launched
        assert len(got) == 0 and got.start.shape == (0, 12) and got.count.shape == (0,) and got.skipped == []


def test_pass_planning_under_the_chapter_budget_and_over_long_videos():
    assert search.plan_passes([3, 4, 5, 100, 2], 30, "chapters") == search.plan_passes([3, 4, 5, 100, 2], 30) == [(0, 2), (2, 3), (3, 4), (4, 5)]
    assert search.plan_passes([4096] * 9, 2 ** 27, "chapters") == [(0, 8), (8, 9)]             # the default budget: eight videos of 4096 seconds
    with pytest.raises(ValueError, match=r"^chapters: budget \(score elements per pass\) must lie in \[1, 2\^31\)$"):
        search.plan_passes([1], 0, "chapters")
    with pytest.raises(ValueError, match=r"^storyboard: budget \(score elements per pass\) must lie in \[1, 2\^31\)$"):
        search.plan_passes([1], 0)                                  # storyboard's own message, byte for byte
    idx = _cpu_index(long=True)
    with pytest.raises(ValueError, match="^chapters: video 'long' .number 4. holds 4097 seconds; a chapter cut takes at most 4096"):
        search.chapters(idx, penalty=1.0)
    with pytest.raises(ValueError, match="^storyboard: video 'long' .number 4. holds 4097 seconds; a storyboard takes at most 4096 "
                                         r"\(skip_long=True leaves such videos out\)$"):
        search.storyboard(idx)
    got = search.chapters(idx, penalty=1.0, videos=["long"], skip_long=True)                   # all that was wanted is left out
    assert got.skipped == ["long"] and len(got) == 0
    with pytest.raises(_lib.TanHipError):                           # 4096 seconds pass
        search.chapters(idx, penalty=1.0, videos=["edge"])


def _chapters():
    return search.Chapters(["a", "b,c", "a"], [0, 2, 5], [2, 1, 3], [[0, 2, -1], [0, -1, -1], [0, 1, 3]],
                           np.array([[2.5, 0.5, np.inf], [0, np.inf, np.inf], [3, 1, 0.25]], np.float32), [0, 3, 4, 8],
                           [0, 0, 1, 0, 0, 1, 1, 2], skipped=["far too long"])


def test_chapters_accessors_files_and_the_round_trip_through_transfer_segments(tmp_path):
    chaps = _chapters()
    assert len(chaps) == 3
    assert chaps.spans("a") == chaps.spans(0) == [(0, 1, 0), (2, 2, 1)]             # a name: the first video that carries it
    assert chaps.spans("b,c") == [(0, 0, 0)] and chaps.spans(5) == [(0, 0, 0), (1, 2, 1), (3, 3, 2)]
    assert chaps.of(5).tolist() == [0, 1, 1, 2] and chaps.of("a").dtype == np.int32
    for v in (0, 2, 5):                                             # spans and the per-second numbers say the same
        assert [c for s, e, c in chaps.spans(v) for _ in range(s, e + 1)] == chaps.of(v).tolist()
    for missing in ("z", 1):
        with pytest.raises(KeyError):
            chaps.spans(missing)
    path = str(tmp_path / "chapters.npz")
    chaps.save(path)
    again = search.Chapters.load(path)
    assert again == chaps and again.skipped == ["far too long"] and again.spans(5) == chaps.spans(5)
    other = _chapters()
    other.scatter[0, 0] = np.float32(2.5000002)
    assert other != chaps
    f = io.StringIO()
    search.write_chapters_csv(f, chaps)
    assert f.getvalue().splitlines() == ["vid,chapter,start,end,seconds", "a,0,0,1,2", "a,1,2,2,1", '"b,c",0,0,0,1', "a,0,0,0,1", "a,1,1,2,2",
                                         "a,2,3,3,1"]
    # a re-timed copy of video 5: its seconds 0..3 are shown at the copy's seconds 10, 11-12, 13, 14 (second 1 held twice as long)
    hit = search.CopyHit("copy", 10, 14, 0, 3, 4.0, 5)
    path = search.CopyPath(hit, np.array([[10, 10], [11, 12], [13, 13], [14, 14]], dtype=np.int32))
    moved = search.transfer_segments(path, chaps.spans(5))
    assert moved == [(10, 10, 0), (11, 13, 1), (14, 14, 2)]


def test_chapters_command_line(capsys):
    argv = ["chapters", "--index", "i.npz", "--out", "c.csv", "--penalty", "1.5"]
    a = search.parse_args(argv)
    assert (a.cmd, a.index, a.out, a.k, a.penalty, a.min_len, a.only, a.only_file, a.skip_long, a.npz, a.shard, a.host_resident) == \
        ("chapters", "i.npz", "c.csv", 12, 1.5, None, None, None, False, None, None, False)
    a = search.parse_args(argv + ["-k", "256", "--min-len", "5", "--only", "v1", "--only", "v2", "--skip-long", "--npz", "c.npz",
                                  "--shard", "j.npz", "--host-resident"])
    assert (a.k, a.min_len, a.only, a.skip_long, a.npz, a.shard, a.host_resident) == (256, 5, ["v1", "v2"], True, "c.npz", ["j.npz"], True)
    assert search.parse_args(argv + ["--only-file", "vids.txt"]).only_file == "vids.txt"
    for bad in (["-k", "0"], ["-k", "257"], ["--penalty", "-0.5"], ["--penalty", "nan"], ["--penalty", "inf"], ["--min-len", "0"],
                ["--min-len", "4097"], ["--only", "v", "--only-file", "f.txt"], ["--checkpoint", "c.pth"], ["--min-gain", "0.1"]):
        with pytest.raises(SystemExit) as e:
            search.parse_args(argv + bad)
        assert e.value.code == 2, bad
    for missing in (["chapters", "--index", "i.npz", "--penalty", "1"], ["chapters", "--out", "c.csv", "--penalty", "1"],
                    ["chapters", "--index", "i.npz", "--out", "c.csv"]):                     # --penalty has no default
        with pytest.raises(SystemExit):
            search.parse_args(missing)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        search.parse_args(argv + ["-k", "0"])
    err = capsys.readouterr().err
    assert err.startswith("usage: search.py") and "search.py: error: -k must lie in [1, 256]" in err
