"""Moment search on the GPU: tan_rank_topk_video (the k best DISTINCT videos per query), tan_moment_extent (how far the moment
extends around a video's best second), `ops.rank_topk_video` / `ops.moment_extent`, `search.search_moments`.

Inputs and references are those of test_retrieve_gpu.py / test_retrieve_fp8_gpu.py:
  * exact arithmetic (multiples of 1/16 for f32 / bf16 with an integer dot product as reference, small-integer codes for e4m3):
    scores, rows, videos and order are compared with `==`;
  * random unit rows: against the fp64 scores of the stored (bf16-rounded / dequantised) rows with the per-score bound EPS = 2e-5
    for f32 / bf16 and 512 * 2^-23 * sum |a_i b_i| for e4m3 (bound (a) of DESIGN 3.12).
Extents on random rows: with W(d) the maximal run around the peak p of rows whose fp64 score is >= fp64(p) - width + d, the
returned [start, end] contains W(+3 EPS) and lies inside W(-3 EPS): the sweep's error on the peak, the extent kernel's on the row,
and the f32 subtraction.  The extent kernel sums 8 products per lane and 6 levels of a tree: well inside either bound.
`v_off` layouts: (a) one row per video, (b) one video, (c) 64-row videos on tile boundaries, (d) random lengths 1..300 (shorter in an index
too small to hold ten such videos), (e) = (d) with boundaries forced at rows 64 and 65, at the first row of each split of `splits = 3`, and a one-row video at the end."""
import ctypes as C

import numpy as np
import pytest
import torch

from temporalalignnet_amd import _lib
from test_retrieve_fp8_gpu import ACC_EPS, _deq, _int_codes
from test_retrieve_gpu import EPS, _embed, _exact_rows, _gen, _model, _unit_rows, _videos

pytestmark = pytest.mark.gpu

QS, NS, KS = (1, 33, 130), (1, 64, 65, 4097, 200003), (1, 10, 32)
FORMATS = ("f32", "bf16", "e4m3")
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _ops():
    from temporalalignnet_amd import ops
    return ops


# --------------------------------------------------------------------------------------------------------------------- layouts
def _split_starts(N, splits=3):
    """The first rows of the splits a sweep with `splits` makes (the launch's own arithmetic)."""
    n_tiles = (N + 63) // 64
    want = min(splits, n_tiles)
    tps = (n_tiles + want - 1) // want
    return [s * tps * 64 for s in range(1, (n_tiles + tps - 1) // tps)]


def _from_bounds(N, bounds):
    return np.array(sorted({0, N} | {int(b) for b in bounds if 0 < b < N}), dtype=np.int64)


def _layout_d(N):
    """Random lengths 1..300; an index of fewer than 7200 rows draws from 1..N // 24 instead, so that it still holds k = 32 videos
    (k = 10 at N = 63)."""
    top = min(300, max(2, N // 24))
    cuts = np.cumsum(np.random.default_rng(1234).integers(1, top + 1, size=2 * N // top + 8))
    return _from_bounds(N, cuts)


def _layouts(N):
    """name -> v_off (int64, host); only the layouts N allows"""
    out = {"a": np.arange(N + 1, dtype=np.int64), "b": np.array([0, N], dtype=np.int64)}
    if N % 64 == 0:
        out["c"] = np.arange(0, N + 1, 64, dtype=np.int64)
    if N > 1:
        out["d"] = _layout_d(N)
        out["e"] = _from_bounds(N, list(_layout_d(N)) + [64, 65, N - 1] + _split_starts(N))
    return out


def _dev(v_off):
    return torch.from_numpy(np.asarray(v_off).astype(np.int32)).cuda()


def _video_of_row(v_off):
    v_off = torch.as_tensor(v_off)
    return torch.repeat_interleave(torch.arange(len(v_off) - 1), v_off[1:] - v_off[:-1]).cuda()


def _video_ref(S, v_off):
    """S [Q, N] fp64 (device) -> per video (maximum [Q, n_videos] fp64, its first arg-max row [Q, n_videos] int64)"""
    Q, N = S.shape
    nv = len(v_off) - 1
    vid = _video_of_row(v_off)[None].expand(Q, N).contiguous()
    vmax = torch.full((Q, nv), -float("inf"), dtype=torch.float64, device="cuda").scatter_reduce(1, vid, S, "amax")
    rows = torch.where(S == vmax.gather(1, vid), torch.arange(N, device="cuda", dtype=torch.float64)[None], float(N))
    vrow = torch.full((Q, nv), float(N), dtype=torch.float64, device="cuda").scatter_reduce(1, vid, rows, "amin")
    return vmax, vrow.long()


def _expected(S, v_off, k):
    vmax, vrow = _video_ref(S, v_off)
    order = torch.sort(vmax, dim=1, descending=True, stable=True).indices[:, :k]       # equal maxima: ascending video = ascending row
    return vmax.gather(1, order), vrow.gather(1, order), order


# ----------------------------------------------------------------------------------------------------------------------- inputs
def _exact_case(fmt, Q, N, seed=0):
    """tq, vn, scale keywords, S (fp64, integer valued), mult with top_score * mult == S"""
    if fmt != "e4m3":
        tq, vn = _exact_rows(Q, 100 + Q + seed, DT[fmt]), _exact_rows(N, 200 + N % 1000 + seed, DT[fmt])
        vn[N // 2] = vn[0]
        return tq, vn, {}, ((tq.double() * 16) @ (vn.double() * 16).T).round(), 256.0
    xq = torch.randint(-16, 17, (Q, 512), generator=_gen(100 + Q + seed), device="cuda")
    xv = torch.randint(-16, 9, (N, 512), generator=_gen(200 + N % 1000 + seed), device="cuda")
    xv[:, 0] = 16
    xv[N // 2] = xv[0]
    eq = torch.randint(-6, 4, (Q,), generator=_gen(7), device="cuda")
    ev = torch.randint(-6, 4, (N,), generator=_gen(8), device="cuda")
    ev[N // 2] = ev[0]
    acc = ((xq.double() * 16) @ (xv.double() * 16).T).round()
    assert float(acc.abs().max()) <= 2 ** 25
    S = acc * (2.0 ** (ev + 6))[None, :] * (2.0 ** (eq + 6))[:, None]
    kw = dict(q_scale=torch.ldexp(torch.ones(Q, device="cuda"), eq), v_scale=torch.ldexp(torch.ones(N, device="cuda"), ev))
    return _int_codes(xq), _int_codes(xv), kw, S, 4096.0


def _stored(fmt, fq, fv):
    """f32 rows -> (tq, vn, scale keywords) in the format, S fp64 of the stored rows, eps [Q, 1]: the bound on a score's error"""
    if fmt != "e4m3":
        tq, vn = fq.to(DT[fmt]), fv.to(DT[fmt])
        return tq, vn, {}, tq.double() @ vn.double().T, torch.full((fq.shape[0], 1), EPS, dtype=torch.float64, device="cuda")
    ops = _ops()
    (tq, qs), (vn, vs) = ops.quantize_rows_e4m3(fq.contiguous()), ops.quantize_rows_e4m3(fv.contiguous())
    a, b = _deq(tq, qs), _deq(vn, vs)
    return tq, vn, dict(q_scale=qs, v_scale=vs), a @ b.T, (ACC_EPS * (a.abs() @ b.abs().T)).amax(1, keepdim=True)


def _unit_case(fmt, Q, N, seed=0):
    return _stored(fmt, _unit_rows(Q, 300 + Q + seed, torch.float32), _unit_rows(N, 400 + N % 1000 + seed, torch.float32))


def _row_sweep(tq, vn, kw, k, **more):
    ops = _ops()
    if kw:
        return ops.rank_topk_e4m3(tq, kw["q_scale"], vn, kw["v_scale"], None, k, **more)[2:]
    return ops.rank_topk(tq, vn, None, k, **more)[2:]


# ------------------------------------------------------------------------------------------------------------- 1. exact arithmetic
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("Q", QS)
def test_rank_topk_video_exact_arithmetic(Q, N, fmt):
    ops = _ops()
    tq, vn, kw, S, mult = _exact_case(fmt, Q, N)
    for name, v_off in _layouts(N).items():
        nv = len(v_off) - 1
        want_s, want_r, want_v = _expected(S, v_off, min(32, nv))
        for k in ((1,) if name == "b" else KS):
            if k > nv:
                continue
            top_s, top_r, top_v = ops.rank_topk_video(tq, vn, _dev(v_off), k, check_v_off=True, **kw)
            assert torch.equal(top_v.long(), want_v[:, :k]), (name, k)
            assert torch.equal(top_r.long(), want_r[:, :k]), (name, k)
            assert torch.equal(top_s.double() * mult, want_s[:, :k]), (name, k)


# -------------------------------------------------------------------------------------------------- 2. the row sweep's own bits
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("Q", QS)
def test_rank_topk_video_has_the_row_sweeps_bits(Q, N, fmt):
    ops = _ops()
    tq, vn, kw, _, _ = _unit_case(fmt, Q, N)
    lay = _layouts(N)
    for k in KS:
        if k > N:
            continue
        row_s, row_r = _row_sweep(tq, vn, kw, k)
        top_s, top_r, top_v = ops.rank_topk_video(tq, vn, _dev(lay["a"]), k, **kw)
        assert torch.equal(top_s, row_s) and torch.equal(top_r, row_r) and torch.equal(top_v, top_r), k
    row_s, row_r = _row_sweep(tq, vn, kw, 1)
    top_s, top_r, top_v = ops.rank_topk_video(tq, vn, _dev(lay["b"]), 1, **kw)
    assert torch.equal(top_s, row_s) and torch.equal(top_r, row_r) and int(top_v.abs().max()) == 0


# ------------------------------------------------------------------------------------------------- 3. random unit rows, bounded
def _bounded_video_checks(S, eps, v_off, k, top_s, top_r, top_v):
    """Returns the largest |returned score - fp64 score of the returned row|."""
    vmax, _ = _video_ref(S, v_off)
    best = torch.topk(vmax, k, dim=1).values
    assert ((top_s.double() - best).abs() <= eps).all()
    assert (vmax.gather(1, top_v.long()) >= best[:, -1:] - 2 * eps).all()
    assert all(len(set(v)) == k for v in top_v.tolist())
    off = torch.from_numpy(np.asarray(v_off)).cuda()
    assert ((off[top_v.long()] <= top_r) & (top_r < off[top_v.long() + 1])).all()
    got = S.gather(1, top_r.long())
    assert (got >= vmax.gather(1, top_v.long()) - 2 * eps).all()
    return float((top_s.double() - got).abs().max())


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("Q", QS)
def test_rank_topk_video_random_unit_rows(Q, N, fmt):
    ops = _ops()
    tq, vn, kw, S, eps = _unit_case(fmt, Q, N)
    worst = 0.0
    for name, v_off in _layouts(N).items():
        for k in ((1,) if name == "b" else KS):
            if k <= len(v_off) - 1:
                out = ops.rank_topk_video(tq, vn, _dev(v_off), k, **kw)
                worst = max(worst, _bounded_video_checks(S, eps, v_off, k, *out))
    print(f"rank_topk_video max |score - fp64| Q={Q} N={N} {fmt}: {worst:.3e} (bound {float(eps.max()):.3e})")
    assert worst <= float(eps.max())


# --------------------------------------------------------------------------------------------------------------------- 4. ties
@pytest.mark.parametrize("fmt", FORMATS)
def test_ties_between_and_inside_videos_across_tiles_and_splits(fmt):
    ops = _ops()
    Q, N = 7, 200003
    tq, vn, kw, _, _ = _stored(fmt, _unit_rows(Q, 1, torch.float32), _unit_rows(N, 2, torch.float32))
    t_edge, s_edge = 64 * 500, _split_starts(N)[0]                  # a tile boundary inside split 0; the first row of split 1
    a, c = 64 * 700 + 33, N - 4                                     # query 0: two videos, different tiles and (splits = 3) splits
    keep = [b for b in _layout_d(N) if min(abs(b - t_edge), abs(b - s_edge)) > 10]
    v_off = _from_bounds(N, keep + [t_edge - 5, t_edge + 5, s_edge - 5, s_edge + 5, a, a + 1])
    plant = {0: (a, c), 1: (t_edge - 2, t_edge + 1), 2: (s_edge - 2, s_edge + 1)}      # queries 1, 2: twice inside ONE video
    for q, rows in plant.items():
        for r in rows:
            vn[r] = tq[q]                                           # the query's own row: its best match by far
            if kw:
                kw["v_scale"][r] = kw["q_scale"][q]
    vid = np.searchsorted(v_off, [r for rows in plant.values() for r in rows], side="right") - 1
    assert vid[0] != vid[1] and vid[2] == vid[3] and vid[4] == vid[5]
    assert t_edge < a < s_edge < _split_starts(N)[1] < c
    for splits in (0, 1, 3, 200):
        top_s, top_r, top_v = ops.rank_topk_video(tq, vn, _dev(v_off), 10, splits=splits, check_v_off=True, **kw)
        assert top_r[0, :2].tolist() == [a, c] and top_v[0, :2].tolist() == [vid[0], vid[1]], splits
        assert top_s[0, 0].item() == top_s[0, 1].item() > top_s[0, 2].item()
        for q in (1, 2):
            assert top_r[q, 0].item() == plant[q][0] and top_v[q, 0].item() == vid[2 * q], (q, splits)
            assert top_s[q, 0].item() > top_s[q, 1].item() and top_v[q, 1].item() != top_v[q, 0].item()


# ----------------------------------------------------------------------------------------------------------------- 5. flooding
def _count_rows(counts, val16, fmt):
    """Rows with `val16 / 16` in their first counts[i] columns and 0 elsewhere -> (rows in the format, v_scale or None)"""
    on = (torch.arange(512, device="cuda")[None, :] < torch.as_tensor(np.asarray(counts), device="cuda")[:, None])
    val16 = torch.as_tensor(np.broadcast_to(np.asarray(val16, dtype=np.float32), (len(counts),)).copy(), device="cuda")
    if fmt != "e4m3":
        return (on.float() * (val16 / 16)[:, None]).to(DT[fmt]), None
    return _int_codes(on.long()), val16 / 256                                          # code 16 x scale val16 / 256


@pytest.mark.parametrize("rising", (True, False), ids=("rising", "falling"))
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_long_video_does_not_flood_the_candidate_buffers(fmt, rising):
    """One 512-row video whose score (i + 1 for query 0, the all-ones row) rises -- or falls -- with the row: every row of it passes
    the threshold its own earlier rows set.  Many low-scoring videos follow."""
    ops = _ops()
    lens = [37, 512] + list(np.random.default_rng(5).integers(1, 41, size=300))
    v_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(v_off[-1])
    tq, vn, kw, S, mult = _exact_case(fmt, 3, N, seed=50)
    if kw:                                                          # every element in [-1, 0.5], as the other formats' rows
        kw["q_scale"].fill_(2.0 ** -8)
        kw["v_scale"].fill_(2.0 ** -8)
    ramp = np.arange(1, 513) if rising else np.arange(512, 0, -1)
    rows, rs = _count_rows(ramp, 16, fmt)
    ones, qs = _count_rows([512], 16, fmt)
    vn[37:37 + 512], tq[0] = rows, ones[0]
    if kw:
        kw["v_scale"][37:37 + 512], kw["q_scale"][0] = rs, qs[0]
        S = (_deq(tq, kw["q_scale"]) @ _deq(vn, kw["v_scale"]).T * mult).round()
    else:
        S = ((tq.double() * 16) @ (vn.double() * 16).T).round()
    assert S[0, 37:37 + 512].tolist() == [float(r * mult) for r in ramp]
    want_s, want_r, want_v = _expected(S, v_off, 32)
    assert want_v[0, 0].item() == 1 and want_r[0, 0].item() == (37 + 511 if rising else 37)
    for splits in (1, 7):
        top_s, top_r, top_v = ops.rank_topk_video(tq, vn, _dev(v_off), 32, splits=splits, **kw)
        assert torch.equal(top_v.long(), want_v) and torch.equal(top_r.long(), want_r), splits
        assert torch.equal(top_s.double() * mult, want_s), splits


# ---------------------------------------------------------------------------------------- 6. determinism and split invariance
@pytest.mark.parametrize("fmt", FORMATS)
def test_rank_topk_video_is_deterministic_and_split_invariant(fmt):
    ops = _ops()
    for Q, N, k in ((130, 4097, 32), (64, 200003, 10), (7, 63, 10)):
        tq, vn, kw, _, _ = _unit_case(fmt, Q, N, seed=20)
        v_off = _dev(_layouts(N)["e"])
        ref = ops.rank_topk_video(tq, vn, v_off, k, check_v_off=True, **kw)
        for splits in (0, 1, 2, 5, 64, 256, 1000):
            got = ops.rank_topk_video(tq, vn, v_off, k, splits=splits, **kw)
            assert all(torch.equal(x, y) for x, y in zip(ref, got)), (Q, N, k, splits)


# ------------------------------------------------------------------------------- 7. writes every output and nothing else
@pytest.mark.parametrize("fmt", FORMATS)
def test_rank_topk_video_writes_every_output_and_nothing_else(fmt):
    ops = _ops()
    G = 64
    for Q, N, k in ((7, 63, 10), (130, 4097, 32), (1, 1, 1), (33, 200003, 10)):
        tq, vn, kw, S, eps = _unit_case(fmt, Q, N, seed=30)
        v_off = _layouts(N)["e" if N > 1 else "a"]
        v_dev = _dev(v_off)
        top_s = torch.full((Q * k + G,), float("nan"), device="cuda")
        top_r = torch.full((Q * k + G,), -777, dtype=torch.int32, device="cuda")
        top_v = torch.full((Q * k + G,), -777, dtype=torch.int32, device="cuda")
        start = torch.full((Q * k + G,), -777, dtype=torch.int32, device="cuda")
        end = torch.full((Q * k + G,), -777, dtype=torch.int32, device="cuda")
        nws = ops.rank_topk_video_ws_bytes(Q, N, len(v_off) - 1, k)
        ws = torch.full((nws + G,), 0xFF, dtype=torch.uint8, device="cuda")
        out = tuple(t[:Q * k].view(Q, k) for t in (top_s, top_r, top_v))
        ext = tuple(t[:Q * k].view(Q, k) for t in (start, end))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ops.rank_topk_video(tq, vn, v_dev, k, out=out, ws=ws[:nws], **kw)
        ops.moment_extent(tq, vn, v_dev, *out, 0.07, out=ext, **kw)
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() == base, (Q, N, k)
        assert (ws[nws:] == 0xFF).all() and torch.isnan(top_s[Q * k:]).all()
        assert all((t[Q * k:] == -777).all() for t in (top_r, top_v, start, end))
        assert torch.isfinite(out[0]).all() and ((out[1] >= 0) & (out[1] < N)).all()
        _bounded_video_checks(S, eps, v_off, k, *out)
        off = v_dev.long()
        assert ((off[out[2].long()] <= ext[0]) & (ext[0] <= out[1]) & (out[1] <= ext[1]) & (ext[1] < off[out[2].long() + 1])).all()


# ------------------------------------------------------------------------------------------------------------- 8. extents, exact
@pytest.mark.parametrize("fmt", FORMATS)
def test_moment_extent_exact(fmt):
    """Query = the all-ones row, so a row's score is (its number of set columns) x (its value).  Videos: 0 = three rows of score 40;
    1 = the rising ramp (i + 1) / 16; 2 = ONE row of score 100; 3 = the falling ramp (512 - i) / 16; 4 = a plateau 1 5 5 5 5 5 2;
    then one-row fillers.  Both ramps' peaks (32) touch a neighbour that scores higher."""
    ops = _ops()
    lens = [3, 512, 1, 512, 7] + [1] * 8
    v_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(v_off[-1])
    counts = [40] * 3 + list(range(1, 513)) + [100] + list(range(512, 0, -1)) + [1, 5, 5, 5, 5, 5, 2] + [3] * 8
    val16 = [16] * 3 + [1] * 512 + [16] + [1] * 512 + [16] * 7 + [16] * 8
    vn, vs = _count_rows(counts, val16, fmt)
    tq, qs = _count_rows([512, 512], 16, fmt)
    kw = dict(q_scale=qs, v_scale=vs) if fmt == "e4m3" else {}
    o = [int(x) for x in v_off]
    # (video, peak row, peak score): the ramps' ends, the one-row video, the plateau from its first row and from its middle
    hits = [(1, o[2] - 1, 32.0), (3, o[3], 32.0), (2, o[2], 100.0), (4, o[4] + 1, 5.0), (4, o[4] + 3, 5.0)]
    order = (hits, hits[::-1])                                      # query 1: the same hits in another order
    top_v = torch.tensor([[h[0] for h in hs] for hs in order], dtype=torch.int32, device="cuda")
    top_r = torch.tensor([[h[1] for h in hs] for hs in order], dtype=torch.int32, device="cuda")
    top_s = torch.tensor([[h[2] for h in hs] for hs in order], dtype=torch.float32, device="cuda")
    sweep = ops.rank_topk_video(tq, vn, _dev(v_off), 4, **kw)       # the lists the sweep itself makes agree with the hand-made hits
    assert sweep[2][0].tolist() == [2, 0, 1, 3] and sweep[1][0].tolist() == [o[2], 0, o[2] - 1, o[3]]
    assert sweep[0][0].tolist() == [100.0, 40.0, 32.0, 32.0]
    for j in (0, 1, 16, 24, 32, 256, 768, 1024, 8191, 8192, 100000):
        w = j / 256
        lo = max(0, -(-(512 * 16 - j) // 16) - 1)                   # rising: (i + 1) / 16 >= 32 - j / 256  <=>  i + 1 >= 512 - j / 16
        hi = min(511, j // 16)                                      # falling: (512 - i) / 16 >= 32 - j / 256  <=>  i <= j / 16
        plateau = (o[4] + 1, o[4] + 5) if w < 3 else ((o[4] + 1, o[4] + 6) if w < 4 else (o[4], o[4] + 6))
        want = [(o[1] + lo, o[2] - 1), (o[3], o[3] + hi), (o[2], o[2]), plateau, plateau]
        start, end = ops.moment_extent(tq, vn, _dev(v_off), top_s, top_r, top_v, w, **kw)
        got = [list(zip(start[q].tolist(), end[q].tolist())) for q in range(2)]
        assert got[0] == want and got[1] == want[::-1], (j, got, want)


# ------------------------------------------------------------------------------------------- 9. extents, bounded on random rows
def _runs(s, p, lo, hi, thr):
    """The maximal run [a, b] around p inside [lo, hi) of rows n != p with s[n] >= thr."""
    a = b = p
    while a > lo and s[a - 1] >= thr:
        a -= 1
    while b + 1 < hi and s[b + 1] >= thr:
        b += 1
    return a, b


def _check_extents(S, eps, v_off, width, top_r, top_v, start, end):
    S, eps = S.cpu().numpy(), eps.cpu().numpy().reshape(-1)
    top_r, top_v, start, end = (t.cpu().numpy() for t in (top_r, top_v, start, end))
    longest = 0
    for q in range(S.shape[0]):
        for i in range(top_r.shape[1]):
            p, v = int(top_r[q, i]), int(top_v[q, i])
            lo, hi = int(v_off[v]), int(v_off[v + 1])
            thr = S[q, p] - width
            in_a, in_b = _runs(S[q], p, lo, hi, thr + 3 * eps[q])
            out_a, out_b = _runs(S[q], p, lo, hi, thr - 3 * eps[q])
            assert out_a <= start[q, i] <= in_a and in_b <= end[q, i] <= out_b, (q, i, width, (start[q, i], end[q, i]),
                                                                                 (in_a, in_b), (out_a, out_b))
            longest = max(longest, int(end[q, i] - start[q, i]) + 1)
    return longest


def _smooth_case(fmt, Q, N):
    """Index rows that change slowly (a moving sum of 32 random rows: neighbours' cosine is about 31 / 32) and queries near some of
    them: moments longer than one row."""
    c = torch.randn(N + 32, 512, generator=_gen(61), device="cuda").cumsum(0)
    fv = c[32:] - c[:-32]
    fv = fv / fv.norm(dim=-1, keepdim=True)
    pick = torch.randint(0, N, (Q,), generator=_gen(62), device="cuda")
    fq = fv[pick] + 0.02 * torch.randn(Q, 512, generator=_gen(63), device="cuda")
    return _stored(fmt, fq / fq.norm(dim=-1, keepdim=True), fv)


@pytest.mark.parametrize("fmt", FORMATS)
def test_moment_extent_bounded_on_random_rows(fmt):
    ops = _ops()
    Q, N, k = 33, 4097, 10
    tq, vn, kw, S, eps = _smooth_case(fmt, Q, N)
    v_off = _layouts(N)["d"]
    v_dev = _dev(v_off)
    top_s, top_r, top_v = ops.rank_topk_video(tq, vn, v_dev, k, **kw)
    _bounded_video_checks(S, eps, v_off, k, top_s, top_r, top_v)
    lens = {}
    for width in (0.0, 0.01, 0.07, 2.0):
        start, end = ops.moment_extent(tq, vn, v_dev, top_s, top_r, top_v, width, **kw)
        again = ops.moment_extent(tq, vn, v_dev, top_s, top_r, top_v, width, **kw)
        assert torch.equal(start, again[0]) and torch.equal(end, again[1])
        lens[width] = _check_extents(S, eps, v_off, width, top_r, top_v, start, end)
    off = v_dev.long()
    assert torch.equal(start.long(), off[top_v.long()]) and torch.equal(end.long(), off[top_v.long() + 1] - 1)     # width 2: the video
    print(f"moment_extent {fmt}: longest moment per width {lens}")
    assert lens[0.07] > 1


# --------------------------------------------------------------------------------------------------------- 10. invalid arguments
def test_moment_entry_points_reject_invalid_arguments():
    ops = _ops()
    L = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                     # noqa: E731
    Q, N, k = 4, 40, 3
    v_off = _dev([0, 10, 11, 25, 40])
    ws = torch.empty(ops.rank_topk_video_ws_bytes(Q, N, 4, k), dtype=torch.uint8, device="cuda")
    ts, tr, tv = torch.empty(Q, k, device="cuda"), torch.empty(Q, k, dtype=torch.int32, device="cuda"), torch.empty(Q, k, dtype=torch.int32, device="cuda")
    st, en = torch.empty_like(tr), torch.empty_like(tr)
    f32 = (_unit_rows(Q, 1, torch.float32), _unit_rows(N, 2, torch.float32))
    (q8, qs), (v8, vs) = ops.quantize_rows_e4m3(f32[0]), ops.quantize_rows_e4m3(f32[1])

    def sweep(e4m3=False, dtype=0, Q=Q, N=N, Cc=512, vo=v_off, nv=4, k=k, splits=0, s=ts, r=tr, v=tv, w=ws, a=None, b=None, sa=qs, sb=vs):
        a, b = (q8 if e4m3 else f32[0]) if a is None else a, (v8 if e4m3 else f32[1]) if b is None else b
        if e4m3:
            return L.tan_rank_topk_video_e4m3(p(a), p(sa), p(b), p(sb), Q, N, Cc, p(vo), nv, k, splits, p(s), p(r), p(v), p(w), None)
        return L.tan_rank_topk_video(p(a), p(b), dtype, Q, N, Cc, p(vo), nv, k, splits, p(s), p(r), p(v), p(w), None)

    def extent(e4m3=False, dtype=0, Q=Q, N=N, Cc=512, vo=v_off, nv=4, k=k, s=ts, r=tr, v=tv, width=0.07, st=st, en=en, a=None, b=None,
               sa=qs, sb=vs):
        a, b = (q8 if e4m3 else f32[0]) if a is None else a, (v8 if e4m3 else f32[1]) if b is None else b
        if e4m3:
            return L.tan_moment_extent_e4m3(p(a), p(sa), p(b), p(sb), Q, N, Cc, p(vo), nv, k, p(s), p(r), p(v), width, p(st), p(en), None)
        return L.tan_moment_extent(p(a), p(b), dtype, Q, N, Cc, p(vo), nv, k, p(s), p(r), p(v), width, p(st), p(en), None)

    class Null:                                                                       # a NULL pointer for one argument
        @staticmethod
        def data_ptr():
            return None
    null = Null()
    sizes = (dict(Cc=256), dict(Cc=1024), dict(k=0), dict(k=33), dict(k=5), dict(k=-1), dict(Q=0), dict(N=0), dict(N=1 << 31),
             dict(nv=0), dict(nv=41), dict(nv=-1))
    for e4m3 in (False, True):
        assert sweep(e4m3) == 0 and extent(e4m3) == 0
        torch.cuda.synchronize()
        for kw in sizes + (dict(splits=-1), dict(vo=null), dict(s=null), dict(r=null), dict(v=null), dict(w=null), dict(a=null), dict(b=null)):
            assert sweep(e4m3, **kw) == -1, (e4m3, kw)
        for kw in sizes + (dict(width=-0.5), dict(width=float("nan")), dict(vo=null), dict(s=null), dict(r=null), dict(v=null),
                           dict(st=null), dict(en=null), dict(a=null), dict(b=null)):
            assert extent(e4m3, **kw) == -1, (e4m3, kw)
    assert sweep(dtype=2) == -1 and extent(dtype=2) == -1
    for kw in (dict(sa=null), dict(sb=null)):
        assert sweep(True, **kw) == -1 and extent(True, **kw) == -1
    # hits that point outside the index: memory-safe, extents unspecified
    tr.fill_(1 << 30)
    tv.fill_(-5)
    assert extent() == 0 and extent(True) == 0
    torch.cuda.synchronize()

    with pytest.raises(_lib.TanHipError):
        ops.rank_topk_video(f32[0].cpu(), f32[1].cpu(), v_off.cpu(), k)
    with pytest.raises(_lib.TanHipError):
        ops.moment_extent(f32[0].cpu(), f32[1].cpu(), v_off.cpu(), ts.cpu(), tr.cpu(), tv.cpu(), 0.07)
    with pytest.raises(_lib.TanHipError):
        ops.rank_topk_video(*f32, v_off, 5)                                          # k > n_videos
    for bad in ([0, 10, 10, 25, 40], [0, 10, 9, 25, 40], [0, 10, 11, 25, 39], [1, 10, 11, 25, 40]):
        with pytest.raises(ValueError):
            ops.rank_topk_video(*f32, _dev(bad), k, check_v_off=True)
        ops.rank_topk_video(*f32, _dev(bad), k)                                      # unchecked: the caller's error, but memory-safe
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- 11. end to end
@pytest.mark.parametrize("fmt", FORMATS)
def test_search_moments_end_to_end(fmt, tmp_path):
    from temporalalignnet_amd import search as srch
    m = _model()
    vids = _videos([70, 33, 150, 64, 20], seed=9)
    f32 = srch.build_index(m, vids, dtype=torch.float32)
    queries = [f"query {i}" for i in range(9)]
    fq = srch.query_features(f32, m, _embed, queries)
    off = [int(x) for x in f32.v_off]
    # query 0: the FIRST second of video 2; query 1: the LAST second of video 1; query 2: the middle of video 0
    planted = {0: (2, 0), 1: (1, 32), 2: (0, 40)}
    for q, (v, sec) in planted.items():
        for d, g in ((0, 1.0), (-1, 0.99), (1, 0.99), (-2, 0.98), (2, 0.98)):
            if 0 <= sec + d < off[v + 1] - off[v]:
                f32.feat[off[v] + sec + d] = fq[q] * g
    idx = f32 if fmt == "f32" else (f32.quantize() if fmt == "e4m3" else srch.VideoIndex(f32.feat.bfloat16(), f32.v_off, f32.vids))
    tq = srch.query_features(idx, m, _embed, queries)
    if fmt == "e4m3":
        a, b = _deq(*tq), _deq(idx.feat, idx.scale)
        S, eps = a @ b.T, (ACC_EPS * (a.abs() @ b.abs().T)).amax(1, keepdim=True)
        S0, A0 = fq.double() @ f32.feat.double().T, fq.double().abs() @ f32.feat.double().abs().T
        bound = (2.0 ** -3 + 2.0 ** -8) * A0 + 512 * 2.0 ** -10 * (idx.scale.double()[None, :] * fq.double().abs().amax(1)[:, None]
                                                                    + tq[1].double()[:, None] * f32.feat.double().abs().amax(1)[None, :])
        score_ref, score_eps = _video_ref(S0, f32.v_off)[0], bound.amax(1, keepdim=True)       # bound (b): against the unquantised rows
    else:
        S = tq.double() @ idx.feat.double().T
        eps = torch.full((9, 1), EPS, dtype=torch.float64, device="cuda")
        score_ref, score_eps = _video_ref(S, idx.v_off)[0], eps
    before = srch.search(idx, m, _embed, queries, k=10)
    res = srch.search_moments(idx, m, _embed, queries, k=5)
    assert srch.search(idx, m, _embed, queries, k=10) == before
    assert len(res) == 9 and all(len(h) == 5 and all(isinstance(x, srch.Moment) for x in h) for h in res)
    best = torch.sort(score_ref, dim=1, descending=True).values.cpu()
    rows, vnum = [], []
    for q, hits in enumerate(res):
        assert len({h.vid for h in hits}) == 5
        for i, h in enumerate(hits):
            v = idx.vids.index(h.vid)
            assert 0 <= h.start <= h.second <= h.end < off[v + 1] - off[v]
            assert abs(h.score - best[q, i].item()) <= score_eps[q].item(), (q, i, h)
        rows.append([off[idx.vids.index(h.vid)] + h.second for h in hits])
        vnum.append([idx.vids.index(h.vid) for h in hits])
    for q, (v, sec) in planted.items():
        assert res[q][0].vid == idx.vids[v] and res[q][0].second == sec, (q, res[q][0])
        assert res[q][0].start <= max(sec - 1, 0) and res[q][0].end >= min(sec + 1, off[v + 1] - off[v] - 1)    # 0.99 is within 0.07
    start = torch.tensor([[off[v] + h.start for v, h in zip(vs, hits)] for vs, hits in zip(vnum, res)])
    end = torch.tensor([[off[v] + h.end for v, h in zip(vs, hits)] for vs, hits in zip(vnum, res)])
    _check_extents(S, eps, idx.v_off, srch.TEMPERATURE, torch.tensor(rows), torch.tensor(vnum), start, end)
    p = str(tmp_path / "index.npz")
    idx.save(p)
    assert srch.search_moments(srch.VideoIndex.load(p), m, _embed, queries, k=5) == res
    assert len(srch.search_moments(idx, m, _embed, queries, k=50)[0]) == 5            # k is clamped to the number of videos
