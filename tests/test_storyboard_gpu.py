"""Storyboards on the GPU: tan_storyboard_select (greedy facility location over a video's own [V, V] score block, in 64-bit fixed
point), `ops.storyboard_select`, `search.storyboard`, `storyboard --out`.  The definition is restated in numpy in storyboard_ref.py
(pinned against a brute force over Python ints by test_storyboard_cpu.py); every sum is an integer, so everything is compared with ==.

  1. the kernel alone on hand-made blocks (x built here, not by a sweep): V = 1 ... 257 in ONE call for every k, on tie-rich,
     asymmetric, all-negative, +-2 / -0.0 / denormal, all-equal, identity and duplicated-row blocks, and min_gain around a gain;
  2. limits and hardening: V = 4096, entries that break the limits among valid ones, dirty outputs between guard words, two runs;
  3. `search.storyboard` end to end on f32 / bf16 / e4m3 indices against the reference over tan_sequence_scores' device bits, with
     several passes, `videos=`, three shards (device- and host-resident), and every coverage against the fp64 mean of maxima of the
     stored operands within test_cover_gpu.py's bound: a max of scores inherits the per-score bound EPS (e4m3: the block's largest
     ACC_EPS * sum |a b|), fix() adds at most 2^-31 per term, and the int64 -> f32 conversion and the division are two roundings of
     at most 2^-24 relative at |value| <= 2 -- less than 2^-21 in all;
  4. meaning: a video of six scenes gets one second per scene, and its storyboard finds a shuffled copy through `search_cover`."""
import io

import numpy as np
import pytest
import torch

import storyboard_ref as ref
from test_moments_gpu import FORMATS
from test_retrieve_fp8_gpu import ACC_EPS, _deq
from test_retrieve_gpu import EPS, _unit_rows
from test_shards_gpu import _pinned

pytestmark = pytest.mark.gpu

VS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 257)
KS = (1, 2, 8, 32, max(VS) + 3)                                     # the last one is V + 3 or more for every V: entries beyond V


def _ops():
    from temporalalignnet_amd import ops
    return ops


def _srch():
    from temporalalignnet_amd import search
    return search


def _cuda(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _layout(blocks):
    """blocks [V, V] one after the other, as `align_tables` lays them out with ms = Vs: (x f32 device, x_off, table [P, 2], sum_V)"""
    Vs = np.array([b.shape[0] for b in blocks], dtype=np.int64)
    x_off = np.concatenate([[0], np.cumsum(Vs * Vs)])
    slot = np.concatenate([[0], np.cumsum(Vs)])
    x = np.concatenate([np.asarray(b, dtype=np.float32).reshape(-1) for b in blocks])
    return _cuda(x, np.float32), x_off[:-1], np.stack((Vs, slot[:-1]), 1), int(slot[-1])


def _select(blocks, k, min_gain=0.0):
    x, x_off, table, sum_V = _layout(blocks)
    second, coverage, owner = _ops().storyboard_select(x, _cuda(x_off, np.int64), _cuda(table, np.int32), k, min_gain=min_gain, sum_V=sum_V)
    return second.cpu().numpy(), coverage.cpu().numpy(), owner.cpu().numpy()


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("second", "coverage", "owner")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), (what, name)


# ------------------------------------------------------------------------------------------------- 1. the kernel on hand-made blocks
def _block(kind, V, rng):
    if kind == "ties":                                              # small integers / 256, not symmetric: many equal sums
        return rng.integers(-3, 4, (V, V)).astype(np.float32) / np.float32(256)
    if kind == "negative":
        return -rng.integers(1, 9, (V, V)).astype(np.float32) / np.float32(256)
    if kind == "special":                                           # +-2, -0.0, denormals, halves of the fixed-point unit
        values = np.array([2.0, -2.0, -0.0, 0.0, 1e-40, -1e-40, 1.5 * 2.0 ** -30, 2.5 * 2.0 ** -30, -0.5 * 2.0 ** -30, 0.75], dtype=np.float32)
        return values[rng.integers(0, len(values), (V, V))]
    if kind == "equal":
        return np.full((V, V), 0.375, dtype=np.float32)
    if kind == "identity":
        return np.eye(V, dtype=np.float32)
    if kind == "duplicates":                                        # every odd row repeats the row before it
        x = rng.integers(0, 64, (V, V)).astype(np.float32) / np.float32(256)
        x[1::2] = x[0:V - 1:2]
        return x
    raise AssertionError(kind)


@pytest.fixture(scope="module")
def hand_made():
    """kind -> (blocks, {k: the reference's result}): computed once, shared, never changed"""
    out = {}
    for n, kind in enumerate(("ties", "negative", "special", "equal", "identity", "duplicates")):
        rng = np.random.default_rng(100 + n)
        blocks = [_block(kind, V, rng) for V in VS]
        out[kind] = (blocks, {k: ref.select_many(blocks, k) for k in KS})
    return out


@pytest.mark.parametrize("kind", ("ties", "negative", "special", "equal", "identity", "duplicates"))
def test_hand_made_blocks_of_every_size_in_one_call(kind, hand_made):
    blocks, want = hand_made[kind]
    if kind == "ties":
        sym = [bool((b == b.T).all()) for b in blocks]
        print(f"storyboard ties: x == x.T holds for V = {[V for V, s in zip(VS, sym) if s]} only")
        assert not all(sym)
    for k in KS:
        got = _select(blocks, k)
        _same(got, want[k], (kind, k))
        second, coverage, owner = got
        slot = np.concatenate([[0], np.cumsum(VS)])
        for p, V in enumerate(VS):
            n = int((second[p] >= 0).sum())
            own = owner[slot[p]:slot[p + 1]]
            assert 1 <= n <= min(k, V) and (second[p, n:] == -1).all() and (coverage[p, n:] == 0).all()
            assert len(set(second[p, :n].tolist())) == n and own.min() >= 0 and own.max() < n
            assert (np.diff(coverage[p, :n]) >= 0).all()
            if kind == "equal":                                     # exactly one entry: the lowest second, which owns everything
                assert n == 1 and second[p, 0] == 0 and coverage[p, 0] == np.float32(0.375) and (own == 0).all()
            if kind == "identity":                                  # V entries in order, coverage j / V
                assert n == min(k, V) and second[p, :n].tolist() == list(range(n))
                assert coverage[p, :n].tolist() == [np.float32(j + 1) / np.float32(V) for j in range(n)]
            if kind == "duplicates":                                # the repeat of a row is never chosen
                assert all(s % 2 == 0 for s in second[p, :n].tolist())
            if kind == "negative":
                assert (coverage[p, :n] < 0).all()


@pytest.mark.parametrize("V", (4, 128))
def test_min_gain_just_below_at_and_just_above_a_gain(V):
    """Row 0 shows the first half of the video, row 1 a further quarter: the second entry gains 2^30 * V / 4, a quarter per second"""
    x = np.zeros((V, V), np.float32)
    x[0, :V // 2], x[1, V // 2:3 * V // 4] = 1, 1
    g = np.float32(0.25)
    below, above = float(np.nextafter(g, np.float32(0))), float(np.nextafter(g, np.float32(1)))
    for min_gain, want in ((0.0, [0, 1, -1]), (below, [0, 1, -1]), (float(g), [0, 1, -1]), (above, [0, -1, -1]), (1e30, [0, -1, -1])):
        got = _select([x, x], 3, min_gain)
        _same(got, ref.select_many([x, x], 3, min_gain), (V, min_gain))
        assert got[0].tolist() == [want, want], (V, min_gain)
        assert got[2].tolist() == ([0] * (V // 2) + [int(want[1] == 1)] * (V // 4) + [0] * (V // 4)) * 2


# --------------------------------------------------------------------------------------------------------- 2. limits and hardening
def test_a_video_of_4096_seconds():
    rng = np.random.default_rng(7)
    x = rng.integers(-64, 65, (4096, 4096)).astype(np.float32) / np.float32(256)
    _same(_select([x], 3), ref.select_many([x], 3), "V = 4096")


def test_entries_that_break_the_limits_among_valid_ones():
    ops = _ops()
    rng = np.random.default_rng(8)
    valid = [_block("ties", V, rng) for V in (5, 70, 33, 129)]
    x, x_off, table, sum_V = _layout(valid)
    n_x, k, G, dirty = x.numel(), 6, 64, 0x7fc00001
    want = _select(valid, k)
    # entries 0, 2, 4, 7 are the valid ones; each bad one claims owner slots of its own beyond the valid ones', which stay untouched
    spare = sum_V
    bad = {1: (0, 4097, spare),                                     # V = 4097
           3: (n_x - 99, 10, spare),                                # a [10, 10] block that leaves x by one element
           5: (0, 8, spare + 100 - 7),                              # owner slots that leave [0, sum_V) by one
           6: (-1, 4, spare), 8: (0, 0, spare), 9: (0, -3, spare), 10: (0, 4, -1), 11: (n_x, 1, spare)}
    sum_all = sum_V + 100
    offs, tab, at = [], [], iter(range(4))
    for e in range(12):
        if e in bad:
            offs.append(bad[e][0])
            tab.append(bad[e][1:])
        else:
            i = next(at)
            offs.append(int(x_off[i]))
            tab.append(tuple(table[i]))
    P = len(offs)
    bufs = [torch.full((G + n + G,), dirty, dtype=torch.int32, device="cuda") for n in (P * k, P * k, sum_all)]
    out = (bufs[0][G:-G].view(P, k), bufs[1][G:-G].view(torch.float32).view(P, k), bufs[2][G:-G])
    got = ops.storyboard_select(x, _cuda(offs, np.int64), _cuda(tab, np.int32), k, sum_V=sum_all, out=out)
    assert all(g is o for g, o in zip(got, out))
    torch.cuda.synchronize()
    for buf in bufs:                                                # nothing outside the outputs
        assert bool((buf[:G] == dirty).all()) and bool((buf[-G:] == dirty).all())
    second, coverage, owner = (t.cpu().numpy() for t in out)
    good = [e for e in range(P) if e not in bad]
    _same((second[good], coverage[good], owner[:sum_V]), want, "the valid entries")
    for e in bad:                                                   # the empty result ...
        assert (second[e] == -1).all() and (coverage[e].view(np.int32) == 0).all(), e
    assert (owner[sum_V:] == dirty).all()                           # ... and their owner slots untouched


def test_the_same_call_twice_gives_identical_bits_on_dirty_outputs():
    ops = _ops()
    rng = np.random.default_rng(9)
    blocks = [rng.standard_normal((V, V)).astype(np.float32) / np.float32(4) for V in (300, 1, 65, 2, 511)]
    x, x_off, table, sum_V = _layout(blocks)
    x_off, table, k, P, G = _cuda(x_off, np.int64), _cuda(table, np.int32), 9, len(blocks), 32
    runs = []
    for dirty in (0x7fc00001, -559038737):
        bufs = [torch.full((G + n + G,), dirty, dtype=torch.int32, device="cuda") for n in (P * k, P * k, sum_V)]
        out = (bufs[0][G:-G].view(P, k), bufs[1][G:-G].view(torch.float32).view(P, k), bufs[2][G:-G])
        ops.storyboard_select(x, x_off, table, k, sum_V=sum_V, out=out)
        torch.cuda.synchronize()
        for buf in bufs:
            assert bool((buf[:G] == dirty).all()) and bool((buf[-G:] == dirty).all())
        runs.append([buf[G:-G].cpu().numpy() for buf in bufs])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    want = ref.select_many(blocks, k)
    _same((runs[0][0].reshape(P, k), runs[0][1].view(np.float32).reshape(P, k), runs[0][2]), want, "random blocks")
    # without sum_V the wrapper reads it from the table's last entry
    _same(tuple(t.cpu().numpy() for t in ops.storyboard_select(x, x_off, table, k)), want, "sum_V from the table")


# ------------------------------------------------------------------------------------------------------------------ 3. end to end
LENS = (1, 300, 2, 31, 32, 33, 64, 65, 100, 7, 129, 200)            # videos of 1 .. 300 rows: one piece, piece edges, many pieces
CUTS = ((0, 4), (4, 9), (9, 12))                                    # three shards


def _parts(fmt, lens=LENS, cuts=CUTS, seed=81, rows=None):
    srch, ops = _srch(), _ops()
    v_off = np.concatenate([[0], np.cumsum(lens)])
    feat = _unit_rows(int(v_off[-1]), seed, torch.float32) if rows is None else rows
    scale = None
    if fmt == "e4m3":
        feat, scale = ops.quantize_rows_e4m3(feat.contiguous())
    elif fmt == "bf16":
        feat = feat.bfloat16()
    parts = []
    for a, b in cuts:
        r0, r1 = int(v_off[a]), int(v_off[b])
        parts.append(srch.VideoIndex(feat[r0:r1].contiguous(), v_off[a:b + 1] - r0, [f"v{i:03d}" for i in range(a, b)],
                                     None if scale is None else scale[r0:r1].contiguous()))
    return parts


def _device_blocks(idx):
    """every video's own [V, V] block with tan_sequence_scores' bits: the index's rows as queries in 32-row pieces, per video"""
    srch, ops = _srch(), _ops()
    lens = idx.v_off[1:] - idx.v_off[:-1]
    s_off, first = srch.piece_offsets(lens)
    videos = np.arange(len(lens))
    hits, hit_off, x_off, _, n_x, _ = srch.align_tables(lens, lens, first[:-1], videos)
    kw = dict(q_scale=idx.scale, v_scale=idx.scale) if idx.e4m3 else {}
    x = ops.sequence_scores(idx.feat, idx.feat, _cuda(s_off, np.int32), idx.v_off_device, _cuda(hits, np.int32), _cuda(hit_off, np.int64),
                            torch.empty(n_x, dtype=torch.float32, device="cuda"), **kw).cpu().numpy()
    return [x[o:o + V * V].reshape(V, V) for o, V in zip(x_off, lens)]


@pytest.fixture(scope="module")
def corpus():
    """fmt -> (parts, the concatenated index, its device blocks, the reference's result for k = 8, the full Storyboard): made once"""
    made = {}

    def get(fmt):
        if fmt not in made:
            srch = _srch()
            parts = _parts(fmt)
            idx = srch.VideoIndex.concat(parts)
            blocks = _device_blocks(idx)
            made[fmt] = (parts, idx, blocks, ref.select_many(blocks, 8), srch.storyboard(idx, 8))
        return made[fmt]
    return get


@pytest.mark.parametrize("fmt", FORMATS)
def test_storyboard_reproduces_the_reference_over_the_device_scores(fmt, corpus):
    srch = _srch()
    parts, idx, blocks, want, board = corpus(fmt)
    sym = sum(bool((b == b.T).all()) for b in blocks)
    print(f"storyboard {fmt}: x == x.T bit for bit in {sym} of {len(blocks)} blocks")
    assert isinstance(board, srch.Storyboard) and board.vids == idx.vids and board.numbers.tolist() == list(range(len(LENS)))
    assert board.owner_off.tolist() == idx.v_off.tolist() and board.skipped == []
    _same((board.second, board.coverage, board.owner), want, fmt)
    for v, V in enumerate(LENS):
        frames = board.frames(v)
        assert 1 <= len(frames) <= min(8, V)
        assert [f[0] for f in frames] == board.second[v, :len(frames)].tolist() and sum(f[2] for f in frames) == V
        assert np.array_equal(board.owners(v), want[2][idx.v_off[v]:idx.v_off[v + 1]])
    # min_gain and another k, against the reference again
    for k, min_gain in ((3, 0.0), (8, 0.02), (40, 0.005)):
        got = srch.storyboard(idx, k, min_gain=min_gain)
        _same((got.second, got.coverage, got.owner), ref.select_many(blocks, k, min_gain), (fmt, k, min_gain))


@pytest.mark.parametrize("fmt", FORMATS)
def test_passes_videos_and_shards_give_the_same_storyboard(fmt, corpus):
    srch = _srch()
    parts, idx, blocks, want, board = corpus(fmt)
    for budget in (1, 70 * 70, 300 * 300, 2 ** 31 - 1):             # a pass per video; the longer ones alone; ...; all in one
        assert srch.storyboard(idx, 8, budget=budget) == board, budget
    assert 4 < len(srch.plan_passes(LENS, 70 * 70)) < len(LENS) and len(srch.plan_passes(LENS, 300 * 300)) == 3
    some = srch.storyboard(idx, 8, videos=["v010", 3, "v001", 3])    # in index order, each once
    assert some.vids == ["v001", "v003", "v010"] and some.numbers.tolist() == [1, 3, 10]
    for v in (1, 3, 10):
        assert some.frames(v) == board.frames(v) and np.array_equal(some.owners(v), board.owners(v))
    assert np.array_equal(some.second, board.second[[1, 3, 10]]) and np.array_equal(some.coverage, board.coverage[[1, 3, 10]])
    for resident in ("device", "host"):
        sharded = srch.ShardedIndex(parts, resident="device") if resident == "device" else srch.ShardedIndex(_pinned(parts), resident="host")
        assert srch.storyboard(sharded, 8) == board, resident
        assert srch.storyboard(sharded, 8, budget=70 * 70) == board, resident
        only = srch.storyboard(sharded, 8, videos=[10, 11])         # the first two shards hold none of them: not visited
        assert only.numbers.tolist() == [10, 11] and only.frames(11) == board.frames(11)
    torch.cuda.synchronize()


@pytest.mark.parametrize("fmt", FORMATS)
def test_coverage_against_the_fp64_mean_of_maxima(fmt, corpus):
    parts, idx, blocks, want, board = corpus(fmt)
    a = _deq(idx.feat, idx.scale) if fmt == "e4m3" else idx.feat.double()
    worst = 0.0
    for v, V in enumerate(LENS):
        rows = a[idx.v_off[v]:idx.v_off[v + 1]]
        S = (rows @ rows.T).cpu().numpy()
        eps = float((ACC_EPS * (rows.abs() @ rows.abs().T)).max()) if fmt == "e4m3" else EPS
        assert np.abs(blocks[v] - S).max() <= eps
        best = np.full(V, -np.inf)
        for j, s in enumerate(board.second[v]):
            if s < 0:
                break
            best = np.maximum(best, S[s])                           # given the device's chosen seconds
            err = abs(float(board.coverage[v, j]) - best.mean())
            worst = max(worst, err)
            assert err <= eps + 2.0 ** -21, (v, j, err, eps)
    print(f"storyboard {fmt}: largest |coverage - fp64 mean of maxima| = {worst:.3e}")


# ----------------------------------------------------------------------------------------------------------------------- 4. meaning
@pytest.mark.parametrize("fmt", ("bf16", "e4m3"))
def test_six_scenes_one_second_each_and_the_storyboard_finds_a_shuffled_copy(fmt, tmp_path):
    srch = _srch()
    rows, scene = ref.scenes(4)
    V = len(scene)
    own = _parts(fmt, lens=[40, V, 25], cuts=((0, 3),), rows=torch.cat((_unit_rows(40, 91, torch.float32), torch.from_numpy(rows).cuda(),
                                                                         _unit_rows(25, 92, torch.float32))))[0]
    board6, board8 = srch.storyboard(own, 6, videos=[1]), srch.storyboard(own, 8, videos=[1])
    second = board6.second[0]
    assert sorted(scene[second].tolist()) == list(range(6))         # one second of every scene
    assert np.array_equal(scene[second][board6.owners(1)], scene)   # every second belongs to the entry of its own scene
    assert [f[2] for f in board6.frames(1)] == np.bincount(scene)[scene[second]].tolist()
    gain = np.diff(board8.coverage[0].astype(np.float64))
    print(f"storyboard scenes {fmt}: coverage {board8.coverage[0].tolist()}")
    assert np.array_equal(board8.second[0, :6], second) and gain[5] < gain[4] / 10 and gain[6] < gain[4] / 10
    # the six rows as a cover query: a shuffled, noisy copy of the video comes first in a corpus of unrelated videos
    perm = np.random.default_rng(5).permutation(V)
    copy = torch.nn.functional.normalize(torch.from_numpy(rows[perm]).cuda() + 0.1 * _unit_rows(V, 93, torch.float32), dim=1)
    lens = [60, 90, V, 30]
    corpus = _parts(fmt, lens=lens, cuts=((0, 4),), rows=torch.cat((_unit_rows(150, 94, torch.float32), copy, _unit_rows(30, 95, torch.float32))))[0]
    query = board6.rows(own, 1)
    assert query.shape == (6, 512) and query.dtype == torch.float32
    hits = srch.search_cover(corpus, [query], k=2, rank="query")[0]
    assert hits[0].vid == "v002" and hits[0].forward > 0.8 > hits[1].forward
    # the command line writes the same numbers
    path, out, npz = str(tmp_path / "own.npz"), str(tmp_path / "story.csv"), str(tmp_path / "story.npz")
    own.save(path)
    assert srch.main(["storyboard", "--index", path, "-k", "6", "--only", "v001", "--out", out, "--npz", npz]) == 0
    f = io.StringIO()
    srch.write_storyboard_csv(f, board6)
    assert open(out, newline="").read() == f.getvalue() and len(f.getvalue().splitlines()) == 7
    assert srch.Storyboard.load(npz) == board6
    assert srch.main(["storyboard", "--index", path, "--only", "nobody", "--out", out]) == 2
    torch.cuda.synchronize()
