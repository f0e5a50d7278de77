"""Filtered search on the GPU: the filter image (tan_row_filter_build) against its numpy statement (filter_ref.py), the filtered row and
video sweeps against the plain sweeps over the GATHERED admitted rows and against exact integer arithmetic, and `search` /
`search_moments` / `search_rerank` / `ShardedIndex` under a `RowFilter`.  Every comparison is `==` (scores by value or as bit
patterns): a filtered sweep returns the plain sweep's scores, not scores close to them.

N = 64 * 300 + 17 rows: 301 tiles (more than the 256 splits a sweep launches at most) and a tail tile of 17 rows.  The row filter
STD holds a span over the tile edge 63 | 64, one inside a tile, three in one tile, one over 100 tiles, a one-row span in the tail
tile and 60 random ones; inputs are those of test_retrieve_gpu.py / test_moments_gpu.py (exact multiples of 1/16, small-integer e4m3
codes; random unit rows)."""
import functools

import numpy as np
import pytest
import torch

import filter_ref as ref
from test_moments_gpu import DT, FORMATS, _dev, _exact_case, _expected, _from_bounds, _layout_d, _row_sweep, _unit_case

pytestmark = pytest.mark.gpu

N0 = 64 * 300 + 17
KS = (1, 10, 32)
SPLITS = (0, 1, 3, 256)
QS = (1, 130)


def _ops():
    from temporalalignnet_amd import ops
    return ops


def _srch():
    from temporalalignnet_amd import search
    return search


def _spans_dev(spans):
    return torch.from_numpy(np.ascontiguousarray(spans, dtype=np.int32).reshape(-1, 2)).cuda()


def _image(spans, N):
    return _ops().row_filter_build(_spans_dev(spans), N)


@functools.lru_cache(maxsize=None)
def _std():
    """(spans int64 [n, 2], rows: the admitted rows) of the standard filter over N0 rows"""
    cuts = np.unique(np.random.default_rng(7).integers(8000, N0 - 64, size=600))
    cuts = cuts[:len(cuts) // 2 * 2].reshape(-1, 2)
    fixed = [[0, 1], [63, 65], [130, 140], [200, 203], [210, 211], [250, 256], [1000, 7405], [N0 - 1, N0]]
    spans = np.array(fixed[:-1] + cuts.tolist() + fixed[-1:], dtype=np.int64)
    assert (spans[1:, 0] > spans[:-1, 1]).all() and (spans[:, 1] > spans[:, 0]).all()
    return spans, ref.admitted_rows(spans)


# ------------------------------------------------------------------------------------------------------------ 1. the image
IMAGE_CASES = {
    "edge 63": [[63, 64]], "edge 64": [[64, 65]], "edge 63-64": [[63, 65]], "edge adjacent spans": [[63, 64], [64, 65]],
    "tile 0 less one": [[0, 63]], "tile 0": [[0, 64]], "inside one tile": [[130, 140]],
    "three in one tile": [[200, 203], [210, 211], [250, 256]], "one row in the tail tile": [[N0 - 1, N0]],
    "the tail tile": [[N0 - 17, N0]], "over 100 tiles": [[1000, 7405]], "everything": [[0, N0]],
    "every other row of two tiles": [[r, r + 1] for r in range(128, 256, 2)],
}


def _check_image(img, spans, N):
    n, T, tiles, masks = ref.parse_image(img.cpu().numpy(), N)
    want_t, want_m = ref.tile_image(np.asarray(spans), N)
    assert T == (N + 63) // 64 and n == len(want_t)
    assert np.array_equal(tiles, want_t) and np.array_equal(masks, want_m)
    return n


@pytest.mark.parametrize("name", sorted(IMAGE_CASES) + ["std"])
def test_image_equals_the_numpy_tile_list_and_masks(name):
    ops = _ops()
    spans = _std()[0] if name == "std" else np.array(IMAGE_CASES[name])
    assert ops.row_filter_bytes(N0) == ref.image_bytes(N0)
    img = _image(spans, N0)
    n = _check_image(img, spans, N0)
    if name in ("std", "everything"):
        assert n > 256                                                  # more listed tiles than a sweep has splits
    poisoned = torch.full((ref.image_bytes(N0) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    again = ops.row_filter_build(_spans_dev(spans), N0, out=poisoned)   # caller-owned, dirty memory: the same documented part
    assert again is poisoned and (poisoned[ref.image_bytes(N0):] == 0xA5).all()
    assert ref.parse_image(again.cpu().numpy(), N0)[0] == n and _check_image(again[:ref.image_bytes(N0)], spans, N0) == n
    T2 = (((N0 + 63) // 64) + 1) // 2 * 2
    documented = lambda t: (t[:4 * (4 + n)].tolist(), t[4 * (4 + T2):4 * (4 + T2) + 8 * n].tolist())      # noqa: E731
    assert documented(img.cpu()) == documented(poisoned.cpu())          # run-to-run identical


@pytest.mark.parametrize("N", (1, 64, 65, 64 * 256 * 257 + 5))
def test_image_at_other_sizes(N):
    """One tile; one tile exactly; a one-row tail tile; and more than 256 * 256 tiles, where the scan launch takes a second round."""
    rng = np.random.default_rng(N % 1000)
    if N <= 65:
        cases = [[[0, N]], [[N - 1, N]], [[0, 1]]]
    else:
        cuts = np.unique(rng.integers(0, N, size=4000))
        cuts = cuts[:len(cuts) // 2 * 2].reshape(-1, 2)
        cases = [cuts, [[0, N]], [[N - 1, N]]]
    for spans in cases:
        _check_image(_image(spans, N), spans, N)


# ---------------------------------------------------------------------------------------------------------- 2. the row sweep
def _gather_kw(kw, rows_t):
    return dict(q_scale=kw["q_scale"], v_scale=kw["v_scale"][rows_t].contiguous()) if kw else {}


def _plant(vn, kw, src, dst):
    vn[dst] = vn[src]
    if kw:
        kw["v_scale"][dst] = kw["v_scale"][src]


R_IN2, R_OUT = 7404, 7415                                               # admitted (the long span's last row) / not admitted


@functools.lru_cache(maxsize=None)
def _exact(fmt, Q):
    """exact inputs with query 0's best admitted row planted again inside (R_IN2) and outside (R_OUT) the filter"""
    spans, rows = _std()
    tq, vn, kw, S, mult = _exact_case(fmt, Q, N0)
    rows_t = torch.from_numpy(rows).cuda()
    r1 = int(rows_t[S[0, rows_t].argmax()])
    assert r1 not in (R_IN2, R_OUT) and R_IN2 in rows and R_OUT not in rows
    for dst in (R_IN2, R_OUT):
        _plant(vn, kw, r1, dst)
        S[:, dst] = S[:, r1]
    return tq, vn, kw, S, mult, r1


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("Q", QS)
def test_filtered_row_sweep_exact_arithmetic(Q, fmt):
    ops = _ops()
    spans, rows = _std()
    tq, vn, kw, S, mult, r1 = _exact(fmt, Q)
    rows_t = torch.from_numpy(rows).cuda()
    filt = _image(spans, N0)
    Sg = S[:, rows_t]
    order = torch.sort(Sg, dim=1, descending=True, stable=True).indices  # equal scores by ascending gathered row = ascending row
    for k in KS:
        for splits in SPLITS:
            top_s, top_r = ops.rank_topk_filtered(tq, vn, filt, k, splits=splits, **kw)
            assert torch.equal(top_r.long(), rows_t[order[:, :k]]), (k, splits)
            assert torch.equal(top_s.double() * mult, Sg.gather(1, order[:, :k])), (k, splits)
    top_s, top_r = ops.rank_topk_filtered(tq, vn, filt, 10, **kw)
    at = [top_r[0].tolist().index(r) for r in sorted((r1, R_IN2))]                   # the planted tie: both there, by ascending row
    assert at[0] < at[1] and top_s[0, at[0]] == top_s[0, at[1]] == top_s[0, 0]
    assert not (top_r == R_OUT).any()
    assert float(S[0, R_OUT]) == float(S[0, r1])                                      # ... which the plain sweep would have returned


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("Q", QS)
def test_filtered_row_sweep_has_the_gathered_sweeps_bits(Q, fmt):
    ops = _ops()
    spans, rows = _std()
    tq, vn, kw, _, _ = _unit_case(fmt, Q, N0)
    rows_t = torch.from_numpy(rows).cuda()
    best = int(_row_sweep(tq, vn[rows_t].contiguous(), _gather_kw(kw, rows_t), 1)[1][0, 0])
    assert int(rows[best]) != R_IN2
    for dst in (R_IN2, R_OUT):
        _plant(vn, kw, int(rows[best]), dst)
    filt = _image(spans, N0)
    vg, kwg = vn[rows_t].contiguous(), _gather_kw(kw, rows_t)
    for k in KS:
        want_s, want_r = _row_sweep(tq, vg, kwg, k)
        for splits in SPLITS:
            top_s, top_r = ops.rank_topk_filtered(tq, vn, filt, k, splits=splits, **kw)
            assert torch.equal(top_s.view(torch.int32), want_s.view(torch.int32)), (k, splits)
            assert torch.equal(top_r.long(), rows_t[want_r.long()]), (k, splits)
    assert sorted(top_r[0, :2].tolist()) == sorted((int(rows[best]), R_IN2)) and not (top_r == R_OUT).any()


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_filter_that_admits_everything_is_the_plain_sweep(fmt):
    ops = _ops()
    for case in (_exact_case, _unit_case):
        tq, vn, kw, *_ = case(fmt, 130, N0)
        filt = _image([[0, N0]], N0)
        for k in KS:
            want_s, want_r = _row_sweep(tq, vn, kw, k)
            for splits in (0, 3):
                top_s, top_r = ops.rank_topk_filtered(tq, vn, filt, k, splits=splits, **kw)
                assert torch.equal(top_s.view(torch.int32), want_s.view(torch.int32)) and torch.equal(top_r, want_r), (k, splits)


@pytest.mark.parametrize("fmt", FORMATS)
def test_fewer_admitted_rows_than_k_leaves_the_defined_empty_tail(fmt):
    ops = _ops()
    tq, vn, kw, S, mult = _exact_case(fmt, 130, N0)
    spans = np.array([[62, 64], [N0 - 1, N0]])                           # three rows, in the first and in the tail tile
    rows_t = torch.from_numpy(ref.admitted_rows(spans)).cuda()
    order = torch.sort(S[:, rows_t], dim=1, descending=True, stable=True).indices
    for splits in SPLITS:
        top_s = torch.full((130, 10), 7.0, device="cuda")                # dirty outputs: every slot is written
        top_r = torch.full((130, 10), -7, dtype=torch.int32, device="cuda")
        ops.rank_topk_filtered(tq, vn, _image(spans, N0), 10, splits=splits, out=(top_s, top_r), **kw)
        assert torch.equal(top_r[:, :3].long(), rows_t[order]) and torch.equal(top_s[:, :3].double() * mult, S[:, rows_t].gather(1, order))
        assert torch.isneginf(top_s[:, 3:]).all() and (top_r[:, 3:] == ref.SENT).all(), splits


# -------------------------------------------------------------------------------------------------------- 3. the video sweep
@functools.lru_cache(maxsize=None)
def _video_layout():
    """v_off over N0 rows and the spans of a filter made for it.  Below row 2000 by hand:
      video [100, 150)    straddles tiles 1 | 2; only its rows of tile 2 are admitted
      video [300, 420)    cut by two windows
      video [420, 1000)   not admitted
      video [1000, 1400)  tiles 16 .. 20 lie inside it (the one-video path): admitted in parts of tiles 16, 17 and 18 only
    from row 2000 on layout (d) of test_moments_gpu.py, every third video admitted whole; BEST (>= 3 rows, admitted) is where the
    tests plant query 0's best row in the MIDDLE and the filter leaves exactly that row out."""
    tail = [int(b) for b in _layout_d(N0) if b > 2000]
    v_off = _from_bounds(N0, [100, 150, 300, 420, 1000, 1400, 2000] + tail)
    spans = [[128, 150], [310, 330], [400, 415], [1030, 1100], [1200, 1210]]
    first = int(np.searchsorted(v_off, 2000))
    whole = list(range(first, len(v_off) - 1, 3))
    best = next(v for v in whole if v_off[v + 1] - v_off[v] >= 3 and v_off[v] > 9000)
    x = int(v_off[best] + (v_off[best + 1] - v_off[best]) // 2)
    for v in whole:
        spans += [[int(v_off[v]), x], [x + 1, int(v_off[v + 1])]] if v == best else [[int(v_off[v]), int(v_off[v + 1])]]
    return v_off, np.array(spans, dtype=np.int64), best, x


def _video_case(case, fmt, Q):
    """inputs with query 0's best row of all planted at the excluded row x of video BEST"""
    v_off, spans, best, x = _video_layout()
    tq, vn, kw, S, mult = case(fmt, Q, N0)[:5]
    top = int(_row_sweep(tq, vn, kw, 1)[1][0, 0])
    if fmt != "e4m3":                                                     # a row that beats every row for query 0: +-1 along the query
        vn[x] = torch.where(tq[0].float() >= 0, 1.0, -1.0).to(vn.dtype)
    else:
        _plant(vn, kw, top, x)
        kw["v_scale"][x] = kw["v_scale"][top] * 2                         # the best row's codes at twice its scale
    return tq, vn, kw


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("Q", QS)
def test_filtered_video_sweep_equals_the_plain_one_over_the_gathered_index(Q, fmt):
    ops = _ops()
    v_off, spans, best, x = _video_layout()
    rows = ref.admitted_rows(spans)
    g_off, kept = ref.gathered_videos(rows, v_off)
    assert best in kept and not {1, 3, 5} - set(kept.tolist()) and 4 not in kept        # the hand-made videos: in, in, in, out
    rows_t, kept_t = torch.from_numpy(rows).cuda(), torch.from_numpy(kept).cuda()
    filt = _image(spans, N0)
    for case in (_exact_case, _unit_case):
        tq, vn, kw = _video_case(case, fmt, Q)
        assert int(_row_sweep(tq, vn, kw, 1)[1][0, 0]) == x                             # the global best row of query 0 is excluded
        vg, kwg = vn[rows_t].contiguous(), _gather_kw(kw, rows_t)
        for k in KS:
            want_s, want_r, want_v = ops.rank_topk_video(tq, vg, _dev(g_off), k, check_v_off=True, **kwg)
            for splits in SPLITS:
                top_s, top_r, top_v = ops.rank_topk_video_filtered(tq, vn, _dev(v_off), filt, k, splits=splits, **kw)
                assert torch.equal(top_s.view(torch.int32), want_s.view(torch.int32)), (case.__name__, k, splits)
                assert torch.equal(top_r.long(), rows_t[want_r.long()]) and torch.equal(top_v.long(), kept_t[want_v.long()])
        assert not (top_r == x).any()
        # a video's entry is its best ADMITTED row: the row sweep over that video's admitted rows alone
        for v in (1, 3, 5, best):
            mine = rows_t[(rows_t >= int(v_off[v])) & (rows_t < int(v_off[v + 1]))]
            s1, r1 = _row_sweep(tq, vn[mine].contiguous(), _gather_kw(kw, mine), 1)
            one = _image(np.stack((mine.cpu().numpy(), mine.cpu().numpy() + 1), 1), N0)
            o_s, o_r, o_v = ops.rank_topk_video_filtered(tq, vn, _dev(v_off), one, 1, **kw)
            assert (o_v == v).all() and torch.equal(o_r.long(), mine[r1.long()]) and torch.equal(o_s.view(torch.int32), s1.view(torch.int32))


@pytest.mark.parametrize("fmt", FORMATS)
def test_filtered_video_sweep_exact_arithmetic(fmt):
    ops = _ops()
    v_off, spans, best, x = _video_layout()
    rows = ref.admitted_rows(spans)
    g_off, kept = ref.gathered_videos(rows, v_off)
    rows_t, kept_t = torch.from_numpy(rows).cuda(), torch.from_numpy(kept).cuda()
    tq, vn, kw, S, mult = _exact_case(fmt, 130, N0)
    vmax, vrow, order = _expected(S[:, rows_t], g_off, 32)
    top_s, top_r, top_v = ops.rank_topk_video_filtered(tq, vn, _dev(v_off), _image(spans, N0), 32, **kw)
    assert torch.equal(top_v.long(), kept_t[order]) and torch.equal(top_r.long(), rows_t[vrow]) and torch.equal(top_s.double() * mult, vmax)


@pytest.mark.parametrize("fmt", FORMATS)
def test_fewer_admitted_videos_than_k_leaves_the_defined_empty_tail(fmt):
    ops = _ops()
    v_off = _video_layout()[0]
    tq, vn, kw, S, mult = _exact_case(fmt, 130, N0)
    spans = np.array([[140, 150], [310, 312], [400, 401], [N0 - 1, N0]])  # videos 1, 3 and the last one
    rows_t = torch.from_numpy(ref.admitted_rows(spans)).cuda()
    g_off, kept = ref.gathered_videos(rows_t.cpu().numpy(), v_off)
    assert kept.tolist() == [1, 3, len(v_off) - 2]
    vmax, vrow, order = _expected(S[:, rows_t], g_off, 3)
    for splits in SPLITS:
        out = (torch.full((130, 10), 7.0, device="cuda"), torch.full((130, 10), -7, dtype=torch.int32, device="cuda"),
               torch.full((130, 10), -7, dtype=torch.int32, device="cuda"))
        top_s, top_r, top_v = ops.rank_topk_video_filtered(tq, vn, _dev(v_off), _image(spans, N0), 10, splits=splits, out=out, **kw)
        assert torch.equal(top_v[:, :3].long(), torch.from_numpy(kept).cuda()[order]) and torch.equal(top_r[:, :3].long(), rows_t[vrow])
        assert torch.equal(top_s[:, :3].double() * mult, vmax)
        assert torch.isneginf(top_s[:, 3:]).all() and (top_r[:, 3:] == ref.SENT).all() and (top_v[:, 3:] == -1).all(), splits


# ------------------------------------------------------------------------------- 4. search / search_moments / search_rerank
def _gathered_index(idx, f):
    """The index rebuilt from the admitted rows of filter f, and (vid, second there) -> second in idx"""
    srch = _srch()
    rows = ref.admitted_rows(f.spans)
    g_off, kept = ref.gathered_videos(rows, idx.v_off)
    rows_t = torch.from_numpy(rows).to(idx.feat.device)
    small = srch.VideoIndex(idx.feat[rows_t].contiguous(), g_off, [idx.vids[v] for v in kept],
                            idx.scale[rows_t].contiguous() if idx.e4m3 else None, idx.stem[rows_t].contiguous() if idx.stem is not None else None)
    second = {(idx.vids[v], int(j)): int(rows[g_off[n] + j] - idx.v_off[v]) for n, v in enumerate(kept) for j in range(g_off[n + 1] - g_off[n])}
    return small, second


SEARCH_FILTERS = {
    "whole videos": dict(videos=["v1", "v3", "v4", "v6", 0], exclude=["v3"]),
    "windows": dict(exclude=["v5"], windows=[("v6", 10, 40), ("v6", 100, 150), ("v6", 190, 500), ("v4", 60, 64), ("v2", 5, 5)]),
}


@pytest.mark.parametrize("e4m3", (False, True), ids=("f32", "e4m3"))
@pytest.mark.parametrize("name", sorted(SEARCH_FILTERS))
def test_search_and_moments_under_a_filter_equal_the_gathered_index(name, e4m3):
    from test_rerank_gpu import QUERIES, _embed, _index, _model
    srch, m = _srch(), _model("fp32")
    idx = _index("fp32", "e4m3") if e4m3 else _index("fp32")
    f = idx.restrict(**SEARCH_FILTERS[name])
    small, second = _gathered_index(idx, f)
    assert f.n_rows == len(small) and f.n_videos == len(small.vids) < len(idx.vids)
    for k in (1, 10, 32):
        got = srch.search(idx, m, _embed, QUERIES, k=k, restrict=f)
        want = srch.search(small, m, _embed, QUERIES, k=k)
        assert got == [[(vid, second[vid, sec], score) for vid, sec, score in hs] for hs in want], k
        assert all(len(hs) == min(k, f.n_rows) for hs in got)
    for k in (1, 10):
        got = srch.search_moments(idx, m, _embed, QUERIES, k=k, restrict=f)
        want = srch.search_moments(small, m, _embed, QUERIES, k=k)
        assert all(len(hs) == min(k, f.n_videos) for hs in got)
        assert [[(h.vid, h.second, h.score) for h in hs] for hs in got] == [[(h.vid, second[h.vid, h.second], h.score) for h in hs] for hs in want]
        if name == "whole videos":                                        # nothing is cut: the extents are the gathered index's too
            assert got == want
        wide = srch.search_moments(idx, m, _embed, QUERIES, k=k, width=100.0, restrict=f)   # everything passes: the admitted span itself
        for hs in wide:
            for h in hs:
                v = idx.vids.index(h.vid)
                row = idx.v_off[v] + h.second
                lo, hi = f.spans[np.searchsorted(f.spans[:, 0], row, side="right") - 1]
                assert h.start == max(lo, idx.v_off[v]) - idx.v_off[v] and h.end == min(hi, idx.v_off[v + 1]) - 1 - idx.v_off[v]
        for hs, ws in zip(got, wide):                                     # and the default width lies inside it, around the peak
            assert all(w.start <= h.start <= h.second <= h.end <= w.end for h, w in zip(hs, ws))


def test_search_rerank_under_a_filter_equals_the_gathered_index():
    from test_rerank_gpu import QUERIES, _embed, _index, _model
    srch, m = _srch(), _model("fp32")
    idx = _index("fp32")
    f = idx.restrict(**SEARCH_FILTERS["whole videos"])
    small, second = _gathered_index(idx, f)
    got = srch.search_rerank(idx, m, _embed, QUERIES, k=3, pool=32, restrict=f)
    assert got == srch.search_rerank(small, m, _embed, QUERIES, k=3, pool=32) and all(len(hs) == 3 for hs in got)
    assert {h.vid for hs in got for h in hs} <= set(small.vids)
    with pytest.raises(ValueError, match="windows"):
        srch.search_rerank(idx, m, _embed, QUERIES, restrict=idx.restrict(**SEARCH_FILTERS["windows"]))


# ---------------------------------------------------------------------------------------------------------------- 5. shards
@pytest.mark.parametrize("fmt", FORMATS)
def test_sharded_search_under_a_filter_equals_concat_and_skips_empty_shards(fmt):
    from test_shards_gpu import QUERIES, _embed, _pinned, _shards, _the_model
    srch, m = _srch(), _the_model()
    parts = _shards(fmt)                                                  # 1, 63, 64, 65 and 4097 rows
    whole = srch.VideoIndex.concat(parts)
    nv = np.concatenate([[0], np.cumsum([len(p.vids) for p in parts])])
    videos = [int(nv[1])] + list(range(int(nv[2]), int(nv[3]))) + list(range(int(nv[4]), int(nv[5]), 2))     # none of shards 0 and 3
    last = int(nv[5]) - 1 if (int(nv[5]) - 1 - int(nv[4])) % 2 == 0 else int(nv[5]) - 2
    kw = dict(videos=videos, windows=[(last, 0, 0), (int(nv[4]), 1, 10 ** 6)])
    want_f = whole.restrict(**kw)
    poisoned = _pinned(parts)
    for s in (0, 3):                                                      # rows that cannot surface: these shards are never copied
        poisoned[s].feat.fill_(0x7F if fmt == "e4m3" else float("nan"))
    for sharded in (srch.ShardedIndex(parts), srch.ShardedIndex(poisoned, resident="host")):
        f = sharded.restrict(**kw)
        assert f.shards() == [1, 2, 4] and f.spans.tolist() == want_f.spans.tolist()
        seen, views = [], sharded.shard_views
        sharded.shard_views = lambda order=None: seen.append(None if order is None else list(order)) or views(order)
        for k in (1, 10, 32):
            assert srch.search(sharded, m, _embed, QUERIES, k=k, restrict=f) == srch.search(whole, m, _embed, QUERIES, k=k, restrict=want_f)
            assert srch.search_moments(sharded, m, _embed, QUERIES, k=k, restrict=f) == \
                srch.search_moments(whole, m, _embed, QUERIES, k=k, restrict=want_f), k
        assert seen == [[1, 2, 4]] * 6                                    # every call asked for the admitted shards only
        if sharded.resident == "host":
            assert sharded._slots[0][0].shape[0] == 4097
    torch.cuda.synchronize()
