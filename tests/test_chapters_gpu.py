"""Chapters on the GPU: tan_chapter_costs and tan_chapter_decode (kernel temporal segmentation over a video's own [V, V] score block,
in 64-bit fixed point), `ops.chapter_costs` / `ops.chapter_decode`, `search.chapters`, `chapters --out`.  The definition is restated
in numpy in chapter_ref.py (pinned against a brute force over Python ints by test_chapters_cpu.py); everything is an integer, so
everything is compared with ==.

  1. the costs alone on hand-made blocks: V = 1 ... 257 in ONE call, with holes between the blocks whose guard words must survive;
  2. the decode on those costs for every k and min_len, penalties around an exact drop, all-equal blocks;
  3. limits and hardening: V = 4096, entries that break the limits among valid ones, dirty outputs between guard words, two runs;
  4. `search.chapters` end to end on f32 / bf16 / e4m3 indices against the reference over tan_sequence_scores' device bits, with
     several passes, `videos=`, three shards (device- and host-resident), and every scatter[count - 1] against the fp64 scatter of
     the returned boundaries over the stored operands.  The bound is derived: a score is within E of the fp64 product (E = EPS, or
     for e4m3 the block's largest ACC_EPS * sum |a b|) and fix() adds at most 2^-31, so D is within V (E + 2^-31), and so is every
     chapter's Q / n (n^2 terms over n), which sum to at most V (E + 2^-31) over the chapters; every floor loses at most 2^-30; the
     int64 -> f32 conversion at most 2^-24 relative, and the reader's own fp64 -> f32 comparison the same:
     2 V (E + 2^-31) + count * 2^-30 + 2^-23 |value|;
  5. meaning: a video of six scenes is cut at its five scene changes, an A B A video into three chapters."""
import io

import numpy as np
import pytest
import torch

import chapter_ref as ref
import storyboard_ref
from test_moments_gpu import FORMATS
from test_retrieve_fp8_gpu import ACC_EPS, _deq
from test_retrieve_gpu import EPS, _unit_rows
from test_shards_gpu import _pinned
from test_storyboard_gpu import CUTS, LENS, _cuda, _device_blocks, _parts

pytestmark = pytest.mark.gpu

VS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 257)
KINDS = ("ties", "negative", "special", "equal", "identity", "asymmetric")
GAP = 37                                                            # elements between two blocks: odd, so 16-byte alignment varies
DIRTY = -0x0123456789abcdef


def _ops():
    from temporalalignnet_amd import ops
    return ops


def _srch():
    from temporalalignnet_amd import search
    return search


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
    if kind == "asymmetric":                                        # the upper triangle dwarfs the lower one
        x = rng.integers(-64, 65, (V, V)).astype(np.float32) / np.float32(64)
        return np.triu(x * np.float32(2), 1) + np.tril(x / np.float32(1024))
    raise AssertionError(kind)


def _layout(blocks, gap=0):
    """blocks [V, V] one after the other with `gap` elements before each: (x f32 host, x_off, table [P, 2], sum_V)"""
    Vs = np.array([b.shape[0] for b in blocks], dtype=np.int64)
    x_off = np.cumsum(Vs * Vs + gap) - Vs * Vs
    slot = np.concatenate([[0], np.cumsum(Vs)])
    x = np.zeros(int(x_off[-1] + Vs[-1] ** 2 + gap), dtype=np.float32)
    for b, o in zip(blocks, x_off):
        x[o:o + b.size] = np.asarray(b, dtype=np.float32).reshape(-1)
    return x, x_off, np.stack((Vs, slot[:-1]), 1), int(slot[-1])


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("count", "start", "scatter", "chapter")):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), (what, name)


@pytest.fixture(scope="module")
def hand_made():
    """kind -> (blocks, their J, device (cost, x_off, table, sum_V)): made once, shared, never changed"""
    made = {}

    def get(kind):
        if kind not in made:
            rng = np.random.default_rng(200 + KINDS.index(kind))
            blocks = [_block(kind, V, rng) for V in VS]
            x, x_off, table, sum_V = _layout(blocks, GAP)
            cost = torch.full((len(x),), DIRTY, dtype=torch.int64, device="cuda")
            x_off_dev, table_dev = _cuda(x_off, np.int64), _cuda(table, np.int32)
            assert _ops().chapter_costs(_cuda(x, np.float32), x_off_dev, table_dev, out=cost) is cost
            made[kind] = (blocks, [ref.costs(b) for b in blocks], (cost, x_off_dev, table_dev, sum_V), x_off)
        return made[kind]
    return get


# ------------------------------------------------------------------------------------------------------------------- 1. the costs
@pytest.mark.parametrize("kind", KINDS)
def test_costs_of_every_size_in_one_call_with_holes_between_the_blocks(kind, hand_made):
    blocks, Js, (cost, _, _, _), x_off = hand_made(kind)
    got = cost.cpu().numpy()
    inside = np.zeros(len(got), dtype=bool)
    for b, o in zip(blocks, x_off):
        V = b.shape[0]
        want, mask = ref.cost_block(b)
        assert np.array_equal(got[o:o + V * V].reshape(V, V)[mask], want[mask]), (kind, V)
        inside[o:o + V * V] = True
    assert (got[~inside] == DIRTY).all() and (~inside).sum() == GAP * (len(VS) + 1)              # the guard words in the holes
    if kind == "ties":
        assert not all(bool((b == b.T).all()) for b in blocks)
    if kind == "equal":
        assert all((J == 0).all() for J in Js)


# ------------------------------------------------------------------------------------------------------------------- 2. the decode
def _decode(dev, k, min_len=1, penalty=0.0):
    cost, x_off, table, sum_V = dev
    return _ops().chapter_decode(cost, x_off, table, k, penalty=penalty, min_len=min_len, sum_V=sum_V)


@pytest.mark.parametrize("kind", KINDS)
def test_decode_for_every_k_and_min_len(kind, hand_made):
    blocks, Js, dev, _ = hand_made(kind)
    # 64 is V for one block and V + 1 for another; 257 and 258 are V and V + 1 of the longest
    cases = [(k, 1, 0.0) for k in (1, 2, 8, 32, 256)] + [(k, m, 0.0) for k in (8, 256) for m in (2, 7, 64, 257, 258)] + \
            [(8, 1, 1e30), (256, 2, 1e30), (32, 7, 2.0 ** -12)]
    for k, min_len, penalty in cases:
        got = _decode(dev, k, min_len, penalty)
        want = ref.decode_many(Js, k, min_len, penalty)
        _same(got, want, (kind, k, min_len, penalty))
        count, start, scatter, chapter = (t.cpu().numpy() for t in got)
        slot = np.concatenate([[0], np.cumsum(VS)])
        for p, V in enumerate(VS):
            n, levels = int(count[p]), min(k, max(1, V // min_len))
            assert 1 <= n <= levels and start[p, 0] == 0 and (start[p, n:] == -1).all() and (np.diff(start[p, :n]) >= min_len).all()
            assert np.isfinite(scatter[p, :levels]).all() and (scatter[p, levels:].view(np.int32) == 0x7f800000).all()
            assert np.array_equal(np.flatnonzero(np.diff(chapter[slot[p]:slot[p + 1]])) + 1, start[p, 1:n])
            if penalty == 1e30 or kind == "equal":                  # `equal`: every cost is 0, equal totals go to the lowest j
                assert n == 1
        if kind == "identity" and min_len == 1 and penalty == 0.0:  # J = (n - 1) 2^30: as many chapters as allowed
            assert count.tolist() == [min(k, V) for V in VS]


@pytest.mark.parametrize("a,b", ((3, 6), (40, 120)))
def test_penalties_just_below_at_and_just_above_an_exact_drop(a, b):
    """Block-diagonal 0/1, two scenes of a and b seconds: one chapter costs 2ab / (a + b), an integer here; two cost nothing"""
    ops = _ops()
    x = np.zeros((a + b, a + b), np.float32)
    x[:a, :a], x[a:, a:] = 1, 1
    drop = np.float32(2 * a * b / (a + b))
    assert float(drop) * (a + b) == 2 * a * b
    flat, x_off, table, sum_V = _layout([x, x])
    x_off, table = _cuda(x_off, np.int64), _cuda(table, np.int32)
    cost = ops.chapter_costs(_cuda(flat, np.float32), x_off, table)
    J = ref.costs(x)
    for penalty, want in ((0.0, 2), (float(np.nextafter(drop, np.float32(0))), 2), (float(drop), 1),
                          (float(np.nextafter(drop, np.float32(1e9))), 1), (1e30, 1)):
        got = ops.chapter_decode(cost, x_off, table, 2, penalty=penalty, sum_V=sum_V)
        _same(got, ref.decode_many([J, J], 2, 1, penalty), (a, b, penalty))
        assert got[0].tolist() == [want, want] and got[2].tolist() == [[float(drop), 0.0]] * 2
        assert got[1].tolist() == [[0, a] if want == 2 else [0, -1]] * 2
    for penalty in (2.0 ** -30, 1e-3, 1.0):                         # an all-equal block: one chapter under any positive penalty
        flat, xo, tb, sv = _layout([np.full((a + b, a + b), -0.625, np.float32)])
        xo, tb = _cuda(xo, np.int64), _cuda(tb, np.int32)
        got = ops.chapter_decode(ops.chapter_costs(_cuda(flat, np.float32), xo, tb), xo, tb, 9, penalty=penalty, sum_V=sv)
        assert got[0].tolist() == [1] and got[1].tolist() == [[0] + [-1] * 8]


# --------------------------------------------------------------------------------------------------------- 3. limits and hardening
@pytest.fixture(scope="module")
def longest():
    """V = 4096, block-diagonal in three scenes with small integer noise: (J, device costs and tables)"""
    rng = np.random.default_rng(17)
    V = 4096
    scene = np.repeat(np.arange(3), (1000, 2000, 1096))
    x = ((scene[:, None] == scene[None, :]) * 64 + rng.integers(-8, 9, (V, V))).astype(np.float32) / np.float32(128)
    flat, x_off, table, sum_V = _layout([x])
    x_off, table = _cuda(x_off, np.int64), _cuda(table, np.int32)
    cost = _ops().chapter_costs(_cuda(flat, np.float32), x_off, table)
    return x, ref.costs(x), (cost, x_off, table, sum_V)


def test_a_video_of_4096_seconds(longest):
    x, J, dev = longest
    want, mask = ref.cost_block(x)
    assert np.array_equal(dev[0].cpu().numpy().reshape(4096, 4096)[mask], want[mask])
    got = _decode(dev, 3, 1, 1.0)
    _same(got, ref.decode_many([J], 3, 1, 1.0), "V = 4096")
    assert got[0].tolist() == [3] and got[1].tolist() == [[0, 1000, 3000]]


def test_4096_seconds_with_min_len_2048_have_exactly_two_feasible_levels(longest):
    x, J, dev = longest
    got = _decode(dev, 4, 2048, 0.0)
    _same(got, ref.decode_many([J], 4, 2048, 0.0), "V = 4096, min_len = 2048")
    assert got[0].tolist() == [2] and got[1].tolist() == [[0, 2048, -1, -1]]
    scatter = got[2].cpu().numpy()[0]
    assert np.isfinite(scatter[:2]).all() and (scatter[2:].view(np.int32) == 0x7f800000).all()


def test_entries_that_break_the_limits_among_valid_ones():
    ops = _ops()
    rng = np.random.default_rng(8)
    valid = [_block("ties", V, rng) for V in (5, 70, 33, 129)]
    spare_blocks = [_block("ties", V, rng) for V in (4, 8)]          # real blocks for the two entries whose SLOTS are broken
    flat, x_off, table, sum_V = _layout(valid + spare_blocks)
    n_x, k, G, dirty = len(flat), 6, 64, 0x7fc00001
    # entries 0, 2, 4, 7 are the valid ones; a broken entry claims chapter slots beyond the valid ones', which stay untouched
    spare = sum_V
    bad = {1: (0, 4097, spare),                                     # V = 4097
           3: (n_x - 99, 10, spare),                                # a [10, 10] block that leaves x by one element
           5: (int(x_off[5]), 8, spare + 100 - 7),                  # chapter slots that leave [0, sum_V) by one
           6: (-1, 4, spare), 8: (0, 0, spare), 9: (0, -3, spare), 10: (int(x_off[4]), 4, -1), 11: (n_x, 1, spare)}
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
    offs_dev, tab_dev = _cuda(offs, np.int64), _cuda(tab, np.int32)
    x = _cuda(flat, np.float32)
    cost = torch.full((n_x,), DIRTY, dtype=torch.int64, device="cuda")
    ops.chapter_costs(x, offs_dev, tab_dev, out=cost)
    got_cost = cost.cpu().numpy()
    Js = [ref.costs(b) for b in valid]
    for b, o in zip(valid + spare_blocks, x_off):                   # the valid blocks, and the two whose blocks are sound, are computed
        V = b.shape[0]
        want, mask = ref.cost_block(b)
        assert np.array_equal(got_cost[o:o + V * V].reshape(V, V)[mask], want[mask])
    assert (got_cost[int(x_off[-1]) + 64:] == DIRTY).all()          # nothing behind the last block
    bufs = [torch.full((G + n + G,), dirty, dtype=torch.int32, device="cuda") for n in (P, P * k, P * k, sum_all)]
    out = (bufs[0][G:-G], bufs[1][G:-G].view(P, k), bufs[2][G:-G].view(torch.float32).view(P, k), bufs[3][G:-G])
    ws = torch.full((ops.chapter_decode_ws_bytes(P, sum_all, k) + 2 * G,), 0x5a, dtype=torch.uint8, device="cuda")
    got = ops.chapter_decode(cost, offs_dev, tab_dev, k, penalty=0.001, sum_V=sum_all, out=out, ws=ws[G:-G])
    assert all(g is o for g, o in zip(got, out))
    torch.cuda.synchronize()
    for buf in bufs + [ws]:                                         # nothing outside the outputs and the scratch
        fill = 0x5a if buf is ws else dirty
        assert bool((buf[:G] == fill).all()) and bool((buf[-G:] == fill).all())
    assert np.array_equal(cost.cpu().numpy(), got_cost)             # the decode writes no cost
    count, start, scatter, chapter = (t.cpu().numpy() for t in out)
    good = [e for e in range(P) if e not in bad]
    _same((count[good], start[good], scatter[good], chapter[:sum_V - 12]), ref.decode_many(Js, k, 1, 0.001), "the valid entries")
    for e in bad:                                                   # the empty result ...
        assert count[e] == 0 and (start[e] == -1).all() and (scatter[e].view(np.int32) == 0x7f800000).all(), e
    assert (chapter[sum_V - 12:] == dirty).all()                    # ... and their chapter slots untouched (the spare blocks' too)


def test_the_same_calls_twice_give_identical_bits_on_dirty_outputs():
    ops = _ops()
    rng = np.random.default_rng(9)
    blocks = [rng.standard_normal((V, V)).astype(np.float32) / np.float32(4) for V in (300, 1, 65, 2, 511)]
    flat, x_off, table, sum_V = _layout(blocks, 5)
    x, x_off_dev, table_dev, k, P, G = _cuda(flat, np.float32), _cuda(x_off, np.int64), _cuda(table, np.int32), 9, len(blocks), 32
    inside = np.zeros(len(flat), dtype=bool)
    lower = np.zeros(len(flat), dtype=bool)
    for b, o in zip(blocks, x_off):
        V = b.shape[0]
        inside[o:o + V * V] = True
        lower[o:o + V * V] = np.tril(np.ones((V, V), dtype=bool)).reshape(-1)
    runs = []
    for dirty in (0x7fc00001, -559038737):
        cost = torch.full((len(flat),), dirty, dtype=torch.int64, device="cuda")
        ops.chapter_costs(x, x_off_dev, table_dev, out=cost)
        bufs = [torch.full((G + n + G,), dirty, dtype=torch.int32, device="cuda") for n in (P, P * k, P * k, sum_V)]
        out = (bufs[0][G:-G], bufs[1][G:-G].view(P, k), bufs[2][G:-G].view(torch.float32).view(P, k), bufs[3][G:-G])
        ops.chapter_decode(cost, x_off_dev, table_dev, k, penalty=0.05, min_len=2, sum_V=sum_V, out=out)
        torch.cuda.synchronize()
        for buf in bufs:
            assert bool((buf[:G] == dirty).all()) and bool((buf[-G:] == dirty).all())
        c = cost.cpu().numpy()
        assert (c[~inside] == dirty).all()
        runs.append([c[lower]] + [buf[G:-G].cpu().numpy() for buf in bufs])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    want = ref.decode_many([ref.costs(b) for b in blocks], k, 2, 0.05)
    _same((runs[0][1], runs[0][2].reshape(P, k), runs[0][3].view(np.float32).reshape(P, k), runs[0][4]), want, "random blocks")
    # without sum_V the wrapper reads it from the table's last entry
    _same(ops.chapter_decode(cost, x_off_dev, table_dev, k, penalty=0.05, min_len=2), want, "sum_V from the table")


# ------------------------------------------------------------------------------------------------------------------ 4. end to end
K, PENALTY = 8, 0.05


@pytest.fixture(scope="module")
def corpus():
    """fmt -> (parts, the concatenated index, its device blocks, their J, the full Chapters): made once"""
    made = {}

    def get(fmt):
        if fmt not in made:
            srch = _srch()
            parts = _parts(fmt)
            idx = srch.VideoIndex.concat(parts)
            blocks = _device_blocks(idx)
            made[fmt] = (parts, idx, blocks, [ref.costs(b) for b in blocks], srch.chapters(idx, K, penalty=PENALTY))
        return made[fmt]
    return get


def _fields(c):
    return c.count, c.start, c.scatter, c.chapter


@pytest.mark.parametrize("fmt", FORMATS)
def test_chapters_reproduce_the_reference_over_the_device_scores(fmt, corpus):
    srch = _srch()
    parts, idx, blocks, Js, chaps = corpus(fmt)
    assert isinstance(chaps, srch.Chapters) and chaps.vids == idx.vids and chaps.numbers.tolist() == list(range(len(LENS)))
    assert chaps.chapter_off.tolist() == idx.v_off.tolist() and chaps.skipped == []
    _same(_fields(chaps), ref.decode_many(Js, K, 1, PENALTY), fmt)
    for v, V in enumerate(LENS):
        spans = chaps.spans(v)
        assert len(spans) == chaps.count[v] and spans[0][0] == 0 and spans[-1][1] == V - 1
        assert [c for s, e, c in spans for _ in range(s, e + 1)] == chaps.of(v).tolist()
    for k, min_len, penalty in ((3, 1, 0.0), (12, 5, 0.01), (40, 2, 0.2)):
        got = srch.chapters(idx, k, penalty=penalty, min_len=min_len)
        _same(_fields(got), ref.decode_many(Js, k, min_len, penalty), (fmt, k, min_len, penalty))


@pytest.mark.parametrize("fmt", FORMATS)
def test_passes_videos_and_shards_give_the_same_chapters(fmt, corpus):
    srch = _srch()
    parts, idx, blocks, Js, chaps = corpus(fmt)
    for budget in (1, 70 * 70, 300 * 300, 2 ** 31 - 1):             # a pass per video; the longer ones alone; ...; all in one
        assert srch.chapters(idx, K, penalty=PENALTY, budget=budget) == chaps, budget
    assert 4 < len(srch.plan_passes(LENS, 70 * 70, "chapters")) < len(LENS)
    some = srch.chapters(idx, K, penalty=PENALTY, videos=["v010", 3, "v001", 3])                   # in index order, each once
    assert some.vids == ["v001", "v003", "v010"] and some.numbers.tolist() == [1, 3, 10]
    for v in (1, 3, 10):
        assert some.spans(v) == chaps.spans(v) and np.array_equal(some.of(v), chaps.of(v))
    assert np.array_equal(some.start, chaps.start[[1, 3, 10]]) and np.array_equal(some.scatter.view(np.int32), chaps.scatter[[1, 3, 10]].view(np.int32))
    for resident in ("device", "host"):
        sharded = srch.ShardedIndex(parts, resident="device") if resident == "device" else srch.ShardedIndex(_pinned(parts), resident="host")
        assert srch.chapters(sharded, K, penalty=PENALTY) == chaps, resident
        assert srch.chapters(sharded, K, penalty=PENALTY, budget=70 * 70) == chaps, resident
        only = srch.chapters(sharded, K, penalty=PENALTY, videos=[10, 11])                         # the first two shards hold none of them
        assert only.numbers.tolist() == [10, 11] and only.spans(11) == chaps.spans(11)
    torch.cuda.synchronize()


@pytest.mark.parametrize("fmt", FORMATS)
def test_scatter_against_the_fp64_scatter_of_the_returned_boundaries(fmt, corpus):
    parts, idx, blocks, Js, chaps = corpus(fmt)
    a = _deq(idx.feat, idx.scale) if fmt == "e4m3" else idx.feat.double()
    worst = 0.0
    for v, V in enumerate(LENS):
        rows = a[idx.v_off[v]:idx.v_off[v + 1]]
        S = (rows @ rows.T).cpu().numpy()
        eps = float((ACC_EPS * (rows.abs() @ rows.abs().T)).max()) if fmt == "e4m3" else EPS
        assert np.abs(blocks[v] - S).max() <= eps
        n = int(chaps.count[v])
        value = sum(np.trace(S[s:e + 1, s:e + 1]) - S[s:e + 1, s:e + 1].sum() / (e + 1 - s) for s, e, _ in chaps.spans(v))
        err = abs(float(chaps.scatter[v, n - 1]) - value)
        worst = max(worst, err)
        assert err <= 2 * V * (eps + 2.0 ** -31) + n * 2.0 ** -30 + 2.0 ** -23 * abs(value), (v, err, eps)
    print(f"chapters {fmt}: largest |scatter[count - 1] - fp64 scatter of the returned boundaries| = {worst:.3e}")


# ----------------------------------------------------------------------------------------------------------------------- 5. meaning
@pytest.mark.parametrize("fmt", FORMATS)
def test_six_scenes_are_cut_at_the_scene_changes_and_a_b_a_gives_three_chapters(fmt, tmp_path):
    srch = _srch()
    rows, scene = storyboard_ref.scenes(4)
    aba, aba_scene = ref.scenes_aba(2)
    V, W = len(scene), len(aba_scene)
    own = _parts(fmt, lens=[40, V, W], cuts=((0, 3),), rows=torch.cat((_unit_rows(40, 91, torch.float32), torch.from_numpy(rows).cuda(),
                                                                         torch.from_numpy(aba).cuda())))[0]
    chaps = srch.chapters(own, 10, penalty=1.0, videos=[1, 2])
    print(f"chapters scenes {fmt}: scatter {chaps.scatter[0].tolist()}")
    assert chaps.count.tolist() == [6, 3]
    assert chaps.start[0, :6].tolist() == [0] + (np.flatnonzero(np.diff(scene)) + 1).tolist() and np.array_equal(chaps.of(1), scene)
    drop = -np.diff(chaps.scatter[0].astype(np.float64))
    assert (drop[:5] > 10 * drop[5]).all()
    cuts = (np.flatnonzero(np.diff(aba_scene)) + 1).tolist()
    assert chaps.start[1, :3].tolist() == [0] + cuts and chaps.spans(2) == [(0, cuts[0] - 1, 0), (cuts[0], cuts[1] - 1, 1), (cuts[1], W - 1, 2)]
    board = srch.storyboard(own, 10, videos=[2], min_gain=0.01)     # the storyboard of the same video: two entries, the first owns both A's
    assert int((board.second[0] >= 0).sum()) == 2 and np.array_equal(board.owners(2), aba_scene)
    # the command line writes the same numbers
    path, out, npz = str(tmp_path / "own.npz"), str(tmp_path / "chapters.csv"), str(tmp_path / "chapters.npz")
    own.save(path)
    assert srch.main(["chapters", "--index", path, "-k", "10", "--penalty", "1.0", "--only", "v001", "--only", "v002", "--out", out,
                      "--npz", npz]) == 0
    f = io.StringIO()
    srch.write_chapters_csv(f, chaps)
    assert open(out, newline="").read() == f.getvalue() and len(f.getvalue().splitlines()) == 1 + 6 + 3
    assert srch.Chapters.load(npz) == chaps
    assert srch.main(["chapters", "--index", path, "--penalty", "1.0", "--only", "nobody", "--out", out]) == 2
    torch.cuda.synchronize()
