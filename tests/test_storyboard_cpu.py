"""Storyboards without a device: the numpy reference of tan_storyboard_select (storyboard_ref.py) against a plain-Python brute force
over Python ints, the 'six scenes' input of the GPU test shown to satisfy the reference alone, the pass planning of
`search.storyboard`, every argument the entry point and the wrappers refuse, and the command line with its CSV writer."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import storyboard_ref as ref
from temporalalignnet_amd import _lib, ops, search


# ------------------------------------------------------------------------------------------------------------------- the reference
def _against_brute(x, k, min_gain=0.0):
    """ref.select on the float32 block x == ref.brute on its fixed image, entry for entry"""
    V = x.shape[0]
    F = ref.fix(x)
    seconds, sums, owner = ref.brute([[int(v) for v in row] for row in F], k, ref.g_min(min_gain))
    second, coverage, own = ref.select(x, k, min_gain)
    n = len(seconds)
    assert second[:n].tolist() == seconds and (second[n:] == -1).all() and (coverage[n:] == 0).all()
    assert own.tolist() == owner
    for j, total in enumerate(sums):
        assert coverage[j] == ref.mean_of_sum(total, V)
    return seconds, sums, owner


def test_reference_against_brute_force_for_every_small_block_shape():
    rng = np.random.default_rng(11)
    for V in range(1, 8):
        for trial in range(6):
            # few distinct values: ties everywhere, so the lowest s must win; not symmetric; trial 1 all negative; trial 2 halves of
            # the fixed-point unit (2.5 ulp -> 2: rounding to even)
            x = rng.integers(-3, 4, (V, V)).astype(np.float32) / np.float32(4)
            if trial == 1:
                x = -np.abs(x) - np.float32(0.25)
            if trial == 2:
                x = (rng.integers(-5, 6, (V, V)) * 0.5).astype(np.float32) * np.float32(2.0 ** -30)
            if trial == 3:
                x = (x + x.T) / np.float32(2)
            for k in range(1, V + 3):
                seconds, sums, owner = _against_brute(x, k)
                assert 1 <= len(seconds) <= min(k, V) and len(set(seconds)) == len(seconds)          # no second twice
                assert all(b > a for a, b in zip(sums, sums[1:]))                                     # every entry gained
                assert set(owner) <= set(range(len(seconds)))


def test_reference_properties_on_hand_made_blocks():
    V = 5
    second, coverage, owner = ref.select(np.full((V, V), 0.5, np.float32), 4)       # all equal: one entry, the lowest s
    assert second.tolist() == [0, -1, -1, -1] and coverage.tolist() == [0.5, 0, 0, 0] and owner.tolist() == [0] * V
    second, coverage, owner = ref.select(np.eye(V, dtype=np.float32), V + 3)         # identity: V entries, coverage j / V
    assert second.tolist() == [0, 1, 2, 3, 4, -1, -1, -1] and owner.tolist() == [0, 1, 2, 3, 4]
    assert coverage[:V].tolist() == [np.float32(j + 1) / np.float32(V) for j in range(V)]
    x = np.array([[1, 0, 0], [1, 0, 0], [0, 1, 1]], dtype=np.float32)                # a duplicated row is never chosen
    second, _, owner = ref.select(x, 3)
    assert second.tolist() == [2, 0, -1] and owner.tolist() == [1, 0, 0]
    # min_gain just below, at and just above the second entry's gain per second: 2^30 / 4 per second of a 4-second video
    x = np.zeros((4, 4), np.float32)
    x[0, :2], x[1, 2] = 1, 1                                                         # entry 0: row 0 (sum 2); entry 1: row 1 gains 1
    assert ref.select(x, 2)[0].tolist() == [0, 1]
    g = np.float32(0.25)
    assert ref.select(x, 2, float(np.nextafter(g, np.float32(0))))[0].tolist() == [0, 1]
    assert ref.select(x, 2, float(g))[0].tolist() == [0, 1]                          # gain == G_min * V: not below it
    assert ref.select(x, 2, float(np.nextafter(g, np.float32(1))))[0].tolist() == [0, -1]
    assert ref.g_min(0.0) == 0 and ref.g_min(1.0) == 1 << 30 and ref.g_min(3e38) == ref.MAX_GMIN == ref.g_min(1024.0)
    # the exact-integer form gives what the float form gives
    xi = np.array([[3, -1], [2, 4]], dtype=np.int64)
    a, b = ref.select(xi, 2, mult=256), ref.select((xi / 256).astype(np.float32), 2)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_six_scenes_satisfy_the_reference_alone():
    """The GPU test's 'meaning' input, in f32 numpy: with k = 6 one second of every scene, every second owned by the entry of its own
    scene; entries seven and eight gain less than a tenth of what the sixth gains.  The sixth entry brings the last scene's seconds
    from a cross-scene cosine (below 0.2 in absolute value for random directions in 512 dimensions) to a within-scene one (about
    1 / 1.09), so it gains at least 0.7 x the shortest scene's share of the video; on these 20 seeds that is 0.04 to 0.1, against
    about 0.001 for the entries after it."""
    for seed in range(20):
        rows, scene = ref.scenes(seed)
        x = rows @ rows.T
        second, coverage, owner = ref.select(x, 8)
        assert (second >= 0).all()
        assert sorted(scene[second[:6]].tolist()) == list(range(6)), seed
        _, _, owner6 = ref.select(x, 6)
        assert np.array_equal(scene[second[:6]][owner6], scene), seed
        gain = np.diff(coverage.astype(np.float64))
        assert gain[4] >= 0.7 * np.bincount(scene).min() / len(scene), (seed, gain)
        assert gain[5] < gain[4] / 10 and gain[6] < gain[4] / 10, (seed, gain)


# ------------------------------------------------------------------------------------------------------------------- pass planning
def test_passes_never_split_a_video_and_stay_in_order():
    rng = np.random.default_rng(3)
    for budget in (1, 50, 999, 10 ** 4, 10 ** 6):
        Vs = rng.integers(1, 120, 40)
        passes = search.plan_passes(Vs, budget)
        assert [a for a, _ in passes] == [0] + [b for _, b in passes[:-1]] and passes[-1][1] == len(Vs)       # consecutive, complete
        for a, b in passes:
            assert b > a and (int((Vs[a:b] ** 2).sum()) <= budget or b - a == 1)                             # within budget, or alone
        for (a, b), (_, d) in zip(passes, passes[1:]):                                                        # greedy: the next video did not fit
            assert int((Vs[a:b + 1] ** 2).sum()) > budget
    assert search.plan_passes([3, 4, 5, 100, 2], 30) == [(0, 2), (2, 3), (3, 4), (4, 5)]       # 100^2 alone exceeds the budget
    assert search.plan_passes([], 30) == [] and search.plan_passes([4096], 2 ** 31 - 1) == [(0, 1)]
    for bad in (0, -1, 2 ** 31, 2 ** 40):
        with pytest.raises(ValueError):
            search.plan_passes([1, 2], bad)


# ------------------------------------------------------------------------------------------------------------- the C entry point
def test_the_header_declares_what_the_library_exports():
    i, l, p, f = C.c_int, C.c_long, C.c_void_p, C.c_float
    names, protos, L = _lib.declared_symbols(), _lib.declared_prototypes(), _lib.lib()
    want = {"tan_storyboard_max_rows": (i, []), "tan_storyboard_select": (i, [p, l, p, p, l, l, i, f, p, p, p, p])}
    for n, proto in want.items():
        assert n in names and protos[n] == proto, n
        assert getattr(L, n).argtypes == proto[1] and getattr(L, n).restype == proto[0], n
    assert L.tan_version() >= 108
    assert L.tan_storyboard_max_rows() == 4096 == ops.STORYBOARD_MAX_ROWS == search.MAX_STORYBOARD_SECONDS == ref.MAX_ROWS
    assert ops.STORYBOARD_MAX_K == search.MAX_STORYBOARD_K == ref.MAX_K == 4096


def test_entry_point_rejects_bad_arguments_without_a_device():
    L = _lib.lib()
    p = 4096                                                        # a non-NULL address: every call is refused before use
    good = dict(x=p, n_x=100, x_off=p, table=p, P=2, sum_V=10, k=8, min_gain=0.0, second=p, coverage=p, owner=p)
    bad = [dict(x=None), dict(x_off=None), dict(table=None), dict(second=None), dict(coverage=None), dict(owner=None),
           dict(n_x=0), dict(n_x=-5), dict(P=0), dict(P=-1), dict(P=1 << 31, sum_V=(1 << 31) - 1), dict(sum_V=1), dict(sum_V=0),
           dict(sum_V=1 << 31), dict(k=0), dict(k=-1), dict(k=4097),
           dict(min_gain=-1e-9), dict(min_gain=float("inf")), dict(min_gain=float("nan")), dict(min_gain=-float("inf"))]
    for b in bad:
        assert L.tan_storyboard_select(*{**good, **b}.values(), None) == -1, b


def test_ops_storyboard_select_checks_its_arguments_before_any_launch():
    x, x_off = torch.zeros(13), torch.tensor([0, 4], dtype=torch.int64)
    table = torch.tensor([[2, 0], [3, 2]], dtype=torch.int32)
    out = (torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4), torch.zeros(5, dtype=torch.int32))
    for bad in (dict(x=torch.zeros(13, dtype=torch.float64)), dict(x=torch.zeros(0)), dict(x=torch.zeros(13, 1)), dict(x=torch.zeros(26)[::2]),
                dict(x_off=x_off.int()), dict(x_off=torch.zeros(0, dtype=torch.int64)), dict(x_off=x_off[None]),
                dict(table=table.long()), dict(table=table[:1]), dict(table=torch.zeros(2, 3, dtype=torch.int32)),
                dict(k=0), dict(k=4097), dict(k=-3),
                dict(min_gain=-0.1), dict(min_gain=float("inf")), dict(min_gain=float("nan")),
                dict(sum_V=1), dict(sum_V=2 ** 31), dict(sum_V=4),              # below P; too large; not the owner's size
                dict(out=(out[0], out[1], torch.zeros(6, dtype=torch.int32))),  # (sum_V read from the table's last entry: 5)
                dict(out=(out[0].long(), out[1], out[2])), dict(out=(out[0], out[1].double(), out[2])),
                dict(out=(out[0][:, :3], out[1], out[2])), dict(out=(out[0], out[1], out[2].float())),
                dict(k=5)):                                                     # out holds k = 4 entries
        kw = dict(x=x, x_off=x_off, table=table, k=4, out=out)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.storyboard_select(**kw)
    for kw in (dict(out=out), dict(sum_V=5), {}):                   # valid arguments on the host: there is no CPU path
        with pytest.raises(_lib.TanHipError):
            ops.storyboard_select(x, x_off, table, 4, **kw)


# ------------------------------------------------------------------------------------------------------------------ the host logic
def _cpu_index(e4m3=False, long=False):
    vids, v_off = ["a", "b", "c", "b"], [0, 10, 50, 55, 60]         # equal names are distinct videos
    if long:
        vids, v_off = vids + ["long", "edge"], v_off + [60 + 4097, 60 + 4097 + 4096]
    n = v_off[-1]
    if e4m3:
        return search.VideoIndex(torch.zeros(n, 512, dtype=torch.uint8), v_off, vids, torch.ones(n))
    return search.VideoIndex(torch.zeros(n, 512), v_off, vids)


def test_storyboard_raises_before_anything_touches_a_device():
    idx = _cpu_index()
    sharded = search.ShardedIndex([search.VideoIndex(idx.feat[:50], [0, 10, 50], ["a", "b"]),
                                   search.VideoIndex(idx.feat[50:], [0, 5, 10], ["c", "b"])])
    for index in (idx, sharded, _cpu_index(e4m3=True)):
        for kw in (dict(k=0), dict(k=4097), dict(min_gain=-1.0), dict(min_gain=float("nan")), dict(min_gain=float("inf")),
                   dict(budget=0), dict(budget=2 ** 31)):
            with pytest.raises(ValueError):
                search.storyboard(index, **{"k": 8, **kw})
        for videos in (["nope"], [4], [-1], [1.5]):
            with pytest.raises(KeyError):
                search.storyboard(index, videos=videos)
        with pytest.raises(_lib.TanHipError):                       # everything checks out: there is no CPU path
            search.storyboard(index, videos=["b"])
        board = search.storyboard(index, videos=[])                 # nothing wanted: nothing launched
        assert len(board) == 0 and board.second.shape == (0, 8) and board.skipped == []


def test_an_over_long_video_is_named_or_skipped():
    idx = _cpu_index(long=True)
    with pytest.raises(ValueError, match="'long'.*4097"):
        search.storyboard(idx)
    with pytest.raises(ValueError, match="'long'"):
        search.storyboard(idx, videos=["a", "long"])
    board = search.storyboard(idx, videos=["long"], skip_long=True)                 # all that was wanted is left out
    assert board.skipped == ["long"] and len(board) == 0
    with pytest.raises(_lib.TanHipError):                           # 4096 seconds pass, and so do the others without the long one
        search.storyboard(idx, skip_long=True)
    with pytest.raises(_lib.TanHipError):
        search.storyboard(idx, videos=["edge"])


def _board():
    return search.Storyboard(["a", "b,c", "a"], [0, 2, 5], [[1, 0, -1], [0, -1, -1], [2, 0, 1]],
                             np.array([[0.5, 0.75, 0], [1, 0, 0], [0.25, 0.5, 0.625]], np.float32), [0, 3, 4, 8],
                             [1, 0, 0, 0, 1, 2, 0, 0], skipped=["far too long"])


def test_storyboard_accessors_and_files(tmp_path):
    board = _board()
    assert len(board) == 3
    assert board.frames("a") == board.frames(0) == [(1, 0.5, 2), (0, 0.75, 1)]      # a name: the first video that carries it
    assert board.frames("b,c") == [(0, 1.0, 1)] and board.frames(5) == [(2, 0.25, 2), (0, 0.5, 1), (1, 0.625, 1)]
    assert board.owners(5).tolist() == [1, 2, 0, 0] and board.owners("a").dtype == np.int32
    for missing in ("z", 1):
        with pytest.raises(KeyError):
            board.frames(missing)
    path = str(tmp_path / "story.npz")
    board.save(path)
    again = search.Storyboard.load(path)
    assert again == board and again.skipped == ["far too long"] and again.frames(5) == board.frames(5)
    other = _board()
    other.coverage[0, 0] = np.float32(0.5000001)
    assert other != board
    f = io.StringIO()
    search.write_storyboard_csv(f, board)
    assert f.getvalue().splitlines() == ["vid,rank,second,coverage,share", "a,0,1,0.500000,2", "a,1,0,0.750000,1", '"b,c",0,0,1.000000,1',
                                         "a,0,2,0.250000,2", "a,1,0,0.500000,1", "a,2,1,0.625000,1"]


def test_storyboard_command_line():
    argv = ["storyboard", "--index", "i.npz", "--out", "s.csv"]
    a = search.parse_args(argv)
    assert (a.cmd, a.index, a.out, a.k, a.min_gain, a.only, a.only_file, a.skip_long, a.npz, a.shard, a.host_resident) == \
        ("storyboard", "i.npz", "s.csv", 8, None, None, None, False, None, None, False)
    a = search.parse_args(argv + ["-k", "4096", "--min-gain", "0.01", "--only", "v1", "--only", "v2", "--skip-long", "--npz", "s.npz",
                                  "--shard", "j.npz", "--host-resident"])
    assert (a.k, a.min_gain, a.only, a.skip_long, a.npz, a.shard, a.host_resident) == (4096, 0.01, ["v1", "v2"], True, "s.npz", ["j.npz"], True)
    assert search.parse_args(argv + ["--only-file", "vids.txt", "--min-gain", "0"]).only_file == "vids.txt"
    for bad, text in ((["-k", "0"], "-k must lie"), (["-k", "4097"], "-k must lie"), (["--min-gain", "-0.5"], "--min-gain"),
                      (["--min-gain", "nan"], "--min-gain"), (["--min-gain", "inf"], "--min-gain"),
                      (["--only", "v", "--only-file", "f.txt"], "--only-file"), (["--checkpoint", "c.pth"], "unrecognized"),
                      (["--threshold", "0.1"], "unrecognized")):
        with pytest.raises(SystemExit) as e:
            search.parse_args(argv + bad)
        assert e.value.code == 2, bad
    for missing in (["storyboard", "--index", "i.npz"], ["storyboard", "--out", "s.csv"]):
        with pytest.raises(SystemExit):
            search.parse_args(missing)


def test_argument_errors_read_like_the_other_subcommands(capsys):
    with pytest.raises(SystemExit):
        search.parse_args(["storyboard", "--index", "i.npz", "--out", "s.csv", "-k", "0"])
    err = capsys.readouterr().err
    assert err.startswith("usage: search.py") and "search.py: error: -k must lie in [1, 4096]" in err
    with pytest.raises(SystemExit):                                 # the same channel as, say, `similar`'s
        search.parse_args(["similar", "--index", "i.npz", "--clip", "v:0-3", "-k", "0"])
    assert capsys.readouterr().err.startswith("usage: search.py")
