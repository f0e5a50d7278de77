"""Clip search on the GPU: tan_clip_topk (per clip of up to 32 query rows the k videos that hold it best SECOND FOR SECOND, and
where), `ops.clip_topk`, `search.clip_features` / `search_clips` / the `similar` command.  The match is restated in numpy in
clip_ref.py (pinned against a loop over Python ints by test_clips_cpu.py).

  * exact arithmetic: test_sequences_gpu._exact_case's inputs (multiples of 1/16; e4m3 integer codes with power-of-two scales): every
    score and every sum of 32 of them is exact in f32, and (top_score * mult, top_row, top_video) equal the int64 reference's lists
    with `==`, empty slots included, for every `splits`.
  * random unit rows: x for ALL (clip, video) pairs from the existing `ops.sequence_scores` (c_off as its s_off); clip_ref in float32
    over THOSE device bits reproduces the three output arrays with `==`.  Every listed score is also held against the fp64 diagonal
    sum of the stored rows: m scores, each within the project's bound (EPS = 2e-5 for f32 / bf16, ACC_EPS * sum |a b| for e4m3),
    plus m - 1 adds of partial sums of at most m, each rounded once: m * EPS + m * m * 2^-24.
The layout is test_sequences_gpu.py's (2742 rows, 168 videos): videos of 1, 2, 63, 64, 65, 128, 129 and 3 rows, 150 videos of
1 .. 5 rows, nine of 200 rows and a last one of 37.  Largest observed errors are recorded in DESIGN.md 3.19."""
import ctypes as C

import numpy as np
import pytest
import torch

import clip_ref as ref
from temporalalignnet_amd import _lib
from test_moments_gpu import FORMATS, _dev, _ops, _stored
from test_retrieve_fp8_gpu import ACC_EPS, _deq
from test_retrieve_gpu import EPS, _unit_rows
from test_sequences_gpu import LENS, N, NV, SPLITS, STEPS, V_OFF, _all_pairs, _exact_case, _s_off, _scores, _seq_split_starts, _unit_case
from test_shards_gpu import _pinned

pytestmark = pytest.mark.gpu

CLIPS = STEPS                                                       # n_clip -> m per clip; five clips cross a workgroup
KS = (1, 10, 20)


def _srch():
    from temporalalignnet_amd import search
    return search


def test_the_layout_has_the_edges_it_claims():
    assert N == 2742 and NV == 168 and CLIPS == {1: [31], 4: [1, 2, 31, 32], 5: [32, 1, 2, 31, 7]}
    assert {1, 2, 3} <= set(LENS)                                   # m = 2: a video shorter than, equal to and one longer than the clip
    assert {64, 65} <= set(LENS)                                    # the last start on and across a tile edge
    assert {129, 200} <= set(LENS)                                  # diagonals carried across two successive edges
    assert sum(V >= 2 for V in LENS) > 2 * 64                       # splits = 1: the candidate registers are compacted more than once
    for splits in (2, 7):
        inside = [b for b in _seq_split_starts(N, splits)
                  if any(lo < b < hi and hi - lo > 128 for lo, hi in zip(V_OFF[:-1], V_OFF[1:]))]
        assert inside, splits                                       # a video of more than two tiles straddles a split boundary
    assert sum(V >= 32 for V in LENS) == 15 and max(KS) == 20       # m = 32, k = 20: five empty slots


def _lists(out):
    return tuple(t.cpu().numpy() for t in out)


# ------------------------------------------------------------------------------------------------------------- 1. exact arithmetic
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n_clip", sorted(CLIPS))
def test_clip_topk_exact_arithmetic(n_clip, fmt):
    ops = _ops()
    ms = CLIPS[n_clip]
    c_off = _s_off(ms)
    tq, vn, kw, X, mult = _exact_case(fmt, ms)
    match, start = ref.matches(X, c_off, V_OFF)                     # int64
    assert (start < 0).any() and (start >= 0).any()                 # videos shorter than a clip, and videos that hold it
    for k in KS:
        want_s, want_r, want_v = ref.topk(match, start, V_OFF, k)
        if 32 in ms and k == 20:
            assert (want_v[ms.index(32)] == -1).sum() == 5
        for splits in SPLITS:
            top_s, top_r, top_v = _lists(ops.clip_topk(tq, vn, _dev(c_off), _dev(V_OFF), k, splits=splits, check_offsets=True, **kw))
            assert np.array_equal(top_v, want_v), (k, splits)
            assert np.array_equal(top_r, want_r), (k, splits)
            assert np.array_equal(top_s.astype(np.float64) * mult, want_s), (k, splits)


# --------------------------------------------------------------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("fmt", FORMATS)
def test_identical_videos_rank_by_row_and_equal_starts_go_to_the_first(fmt):
    """An index of one 200-row video twice: both are listed with the same score, the lower row first, each at the same second.
    A video that holds the same run twice (from second 40 on, across a tile edge, and from 130 on, inside a tile) reports the first."""
    ops = _ops()
    ms = [7, 32, 1]
    fq, fv = _unit_rows(int(sum(ms)), 41, torch.float32), _unit_rows(400, 42, torch.float32)
    fv[200:] = fv[:200]
    tq, vn, kw, _, _ = _stored(fmt, fq, fv)
    for splits in SPLITS:
        top_s, top_r, top_v = ops.clip_topk(tq, vn, _dev(_s_off(ms)), _dev([0, 200, 400]), 2, splits=splits, **kw)
        assert top_v.tolist() == [[0, 1]] * 3 and torch.equal(top_s[:, 0], top_s[:, 1]), splits
        assert torch.equal(top_r[:, 1], top_r[:, 0] + 200), splits
    twice = _unit_rows(300, 43, torch.float32)
    twice[40:72] = fq[7:39] * 0.5 + twice[40:72] * 0.5           # the 32-row clip: about 16 against sums of about 0.25 elsewhere
    twice[130:162] = twice[40:72]
    tq, vn, kw, _, _ = _stored(fmt, fq, twice)
    for splits in (0, 1):
        top_s, top_r, top_v = ops.clip_topk(tq, vn, _dev(_s_off(ms)), _dev([0, 300]), 1, splits=splits, **kw)
        assert top_r[1].item() == 40 and top_v[1].item() == 0, splits


# ------------------------------------------------------------------------------------------------------- 3. random unit rows
@pytest.mark.parametrize("fmt", FORMATS)
def test_clip_topk_random_unit_rows(fmt):
    ops = _ops()
    ms = CLIPS[5]
    c_off = _s_off(ms)
    tq, vn, kw, S, _ = _unit_case(fmt, ms)
    hits = _all_pairs(len(ms), NV)
    x, hm, hv, x_off = _scores(tq, vn, kw, c_off, V_OFF, hits)     # the sweep's own bits, for every (clip, video)
    xs = x.cpu().numpy()
    match = np.zeros((len(ms), NV), dtype=np.float32)
    start = np.full((len(ms), NV), -1, dtype=np.int64)
    for h, (p, v) in enumerate(hits):
        got = ref.match_and_start(xs[x_off[h]:x_off[h] + hm[h] * hv[h]].reshape(hm[h], hv[h]))
        if got is not None:
            match[p, v], start[p, v] = got
    S_h = S.cpu().numpy()
    if fmt == "e4m3":
        A_h = (_deq(tq, kw["q_scale"]).abs() @ _deq(vn, kw["v_scale"]).abs().T).cpu().numpy()
    worst, worst_bound = 0.0, 0.0
    for k in KS:
        want_s, want_r, want_v = ref.topk(match, start, V_OFF, k)
        for splits in SPLITS:
            top_s, top_r, top_v = _lists(ops.clip_topk(tq, vn, _dev(c_off), _dev(V_OFF), k, splits=splits, **kw))
            assert np.array_equal(top_v, want_v), (k, splits)
            assert np.array_equal(top_r, want_r), (k, splits)
            assert np.array_equal(top_s.view(np.int32), want_s.astype(np.float32).view(np.int32)), (k, splits)
        # the listed scores against the fp64 diagonal sums of the stored rows
        for p, m in enumerate(ms):
            i = np.arange(m)
            for j in range(k):
                if top_v[p, j] < 0:
                    continue
                exact = S_h[c_off[p] + i, top_r[p, j] + i].sum()
                terms = ACC_EPS * A_h[c_off[p] + i, top_r[p, j] + i].sum() if fmt == "e4m3" else m * EPS
                bound = terms + m * m * 2.0 ** -24
                err = abs(float(top_s[p, j]) - exact)
                if err > worst:
                    worst, worst_bound = err, bound
                assert err <= bound, (p, j, err, bound)
    print(f"clip_topk max |top_score - fp64 diagonal sum| {fmt}: {worst:.3e} (its bound {worst_bound:.3e})")


# --------------------------------------------------------------------------------------- 4. one row: the existing video sweep
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_row_clips_equal_rank_topk_video(fmt):
    ops = _ops()
    Q = 9
    tq, vn, kw, _, _ = _unit_case(fmt, [1] * Q, seed=3)
    c_off = np.arange(Q + 1, dtype=np.int64)
    for k in KS:
        want = ops.rank_topk_video(tq, vn, _dev(V_OFF), k, **kw)
        for splits in SPLITS:
            got = ops.clip_topk(tq, vn, _dev(c_off), _dev(V_OFF), k, splits=splits, **kw)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (k, splits)


# -------------------------------------------------------------------- 5. determinism, split invariance, nothing else is written
@pytest.mark.parametrize("fmt", FORMATS)
def test_clip_topk_is_deterministic_and_writes_nothing_else(fmt):
    ops = _ops()
    G = 64
    for ms, k in ((CLIPS[5], 10), (CLIPS[1], 20), (CLIPS[4], 1)):
        n_clip, c_off = len(ms), _s_off(ms)
        tq, vn, kw, _, _ = _unit_case(fmt, ms, seed=20)
        c_dev, v_dev = _dev(c_off), _dev(V_OFF)
        ref_out = ops.clip_topk(tq, vn, c_dev, v_dev, k, check_offsets=True, **kw)
        top_s = torch.full((n_clip * k + G,), float("nan"), device="cuda")
        top_r = torch.full((n_clip * k + G,), -777, dtype=torch.int32, device="cuda")
        top_v = torch.full((n_clip * k + G,), -777, dtype=torch.int32, device="cuda")
        nws = ops.clip_topk_ws_bytes(n_clip, N, k)
        assert nws == min((N + 63) // 64, 256) * n_clip * k * 12    # the splits' lists of triples only
        ws = torch.full((nws + G,), 0xFF, dtype=torch.uint8, device="cuda")
        out = tuple(t[:n_clip * k].view(n_clip, k) for t in (top_s, top_r, top_v))
        for splits in SPLITS + SPLITS + (5, 43, 256, 1000):
            out[0].fill_(float("nan"))
            out[1].fill_(-777)
            out[2].fill_(-777)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ops.clip_topk(tq, vn, c_dev, v_dev, k, splits=splits, out=out, ws=ws[:nws], **kw)
            torch.cuda.synchronize()
            assert torch.cuda.max_memory_allocated() == base, (ms, k, splits)
            assert all(torch.equal(a, b) for a, b in zip(out, ref_out)), (ms, k, splits)
            assert (ws[nws:] == 0xFF).all() and torch.isnan(top_s[n_clip * k:]).all()
            assert (top_r[n_clip * k:] == -777).all() and (top_v[n_clip * k:] == -777).all()
        s, r, v = _lists(out)
        held = v >= 0
        assert np.isfinite(s[held]).all() and (s[~held] == -np.inf).all() and (r[~held] == ref.EMPTY_ROW).all() and (v[~held] == -1).all()
        m_of = np.asarray(ms)[:, None]
        assert ((r >= V_OFF[np.maximum(v, 0)]) & (r + m_of <= V_OFF[np.maximum(v, 0) + 1]))[held].all()    # the placement lies inside its video
        assert all(len(set(row[row >= 0])) == (row >= 0).sum() for row in v)


# --------------------------------------------------------------------------------------------------------- 6. invalid arguments
def test_clip_topk_rejects_invalid_arguments():
    ops = _ops()
    L = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                     # noqa: E731
    ms, k = [3, 1, 4], 3
    Qt, Nn = 8, 40
    c_off, v_off = _dev(_s_off(ms)), _dev([0, 10, 11, 25, 40])
    f32 = (_unit_rows(Qt, 1, torch.float32), _unit_rows(Nn, 2, torch.float32))
    (q8, qs), (v8, vs) = ops.quantize_rows_e4m3(f32[0]), ops.quantize_rows_e4m3(f32[1])
    ts = torch.empty(3, k, device="cuda")
    tr, tv = (torch.empty(3, k, dtype=torch.int32, device="cuda") for _ in range(2))
    ws = torch.empty(ops.clip_topk_ws_bytes(3, Nn, k), dtype=torch.uint8, device="cuda")

    def topk(e4m3=False, dtype=0, Qt=Qt, N=Nn, Cc=512, co=c_off, n_clip=3, vo=v_off, nv=4, k=k, splits=0, s=ts, r=tr, v=tv, w=ws,
             sa=qs, sb=vs):
        a, b = (q8, v8) if e4m3 else f32
        if e4m3:
            return L.tan_clip_topk_e4m3(p(a), p(sa), p(b), p(sb), Qt, N, Cc, p(co), n_clip, p(vo), nv, k, splits, p(s), p(r), p(v), p(w), None)
        return L.tan_clip_topk(p(a), p(b), dtype, Qt, N, Cc, p(co), n_clip, p(vo), nv, k, splits, p(s), p(r), p(v), p(w), None)

    class Null:                                                                       # a NULL pointer for one argument
        @staticmethod
        def data_ptr():
            return None
    null = Null()
    for e4m3 in (False, True):
        assert topk(e4m3) == 0
        torch.cuda.synchronize()
        for kw in (dict(Cc=256), dict(Cc=1024), dict(n_clip=0), dict(Qt=2), dict(Qt=97), dict(nv=0), dict(nv=41), dict(nv=-1), dict(N=0),
                   dict(N=1 << 31), dict(k=0), dict(k=33), dict(k=5), dict(k=-1), dict(splits=-1), dict(co=null), dict(vo=null),
                   dict(s=null), dict(r=null), dict(v=null), dict(w=null)):
            assert topk(e4m3, **kw) == -1, (e4m3, kw)
    assert topk(dtype=2) == -1
    for kw in (dict(sa=null), dict(sb=null)):
        assert topk(True, **kw) == -1
    assert L.tan_clip_topk_ws_bytes(3, Nn, k) == 1 * 3 * k * 12
    for bad in ((0, Nn, k), (1 << 29, Nn, k), (3, 0, k), (3, 1 << 31, k), (3, Nn, 0), (3, Nn, 33)):
        assert L.tan_clip_topk_ws_bytes(*bad) == -1, bad
        with pytest.raises(_lib.TanHipError):
            ops.clip_topk_ws_bytes(*bad)

    with pytest.raises(_lib.TanHipError):
        ops.clip_topk(f32[0].cpu(), f32[1].cpu(), c_off.cpu(), v_off.cpu(), k)
    with pytest.raises(_lib.TanHipError):
        ops.clip_topk(*f32, c_off, v_off, 5)                                         # k > n_videos
    with pytest.raises(TypeError):
        ops.clip_topk(*f32, c_off, v_off, k, q_scale=qs, v_scale=vs)
    for bad in ([0, 10, 10, 25, 40], [0, 10, 9, 25, 40], [0, 10, 11, 25, 39], [1, 10, 11, 25, 40]):
        with pytest.raises(ValueError):
            ops.clip_topk(*f32, c_off, _dev(bad), k, check_offsets=True)
        ops.clip_topk(*f32, c_off, _dev(bad), k)                                     # unchecked: the caller's error, but memory-safe
    for bad in ([0, 3, 3, 8], [0, 5, 4, 8], [0, 3, 4, 7], [1, 3, 4, 8]):
        with pytest.raises(ValueError):
            ops.clip_topk(*f32, _dev(bad), v_off, k, check_offsets=True)
        ops.clip_topk(*f32, _dev(bad), v_off, k)
    # a clip of 33 rows: refused on request; unchecked it is cut to 32 rows -- only the return and a clean synchronisation are asserted
    wide = _unit_rows(40, 5, torch.float32)
    with pytest.raises(ValueError):
        ops.clip_topk(wide, f32[1], _dev([0, 33, 40]), v_off, 2, check_offsets=True)
    ops.clip_topk(wide, f32[1], _dev([0, 33, 40]), v_off, 2)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 7. planted copies through search_clips
def _planted(fmt):
    """An index made from tensors: six videos of random unit rows; seconds 10..29 of video A = 2 reappear, with noise, in video B = 5
    from second 55 on (across a tile edge).  Video 4 is shorter than the clip."""
    srch = _srch()
    lens = [70, 33, 150, 64, 12, 90]
    v_off = np.concatenate([[0], np.cumsum(lens)])
    feat = _unit_rows(int(v_off[-1]), 51, torch.float32)
    A, B, a0, b0, m = 2, 5, 10, 55, 20
    run = feat[v_off[A] + a0:v_off[A] + a0 + m]
    noisy = run + 0.1 * _unit_rows(m, 52, torch.float32)
    feat[v_off[B] + b0:v_off[B] + b0 + m] = noisy / noisy.norm(dim=1, keepdim=True)
    f32 = srch.VideoIndex(feat, v_off, [f"v{i:03d}" for i in range(len(lens))])
    idx = f32.quantize() if fmt == "e4m3" else srch.VideoIndex(feat.to(torch.bfloat16 if fmt == "bf16" else torch.float32), v_off, f32.vids)
    return idx, (A, a0), (B, b0), m


def _fp64(idx, tq):
    """the stored rows of the index and of `clip_features`' query side in fp64"""
    if idx.e4m3:
        return _deq(*tq), _deq(idx.feat, idx.scale)
    return tq.double(), idx.feat.double()


@pytest.mark.parametrize("fmt", ("bf16", "e4m3"))
def test_search_clips_finds_the_planted_copy(fmt, tmp_path, capsys):
    srch, ops = _srch(), _ops()
    idx, (A, a0), (B, b0), m = _planted(fmt)
    clip = (idx.vids[A], a0, a0 + m - 1)
    tq, c_off = srch.clip_features(idx, [clip])
    assert c_off.tolist() == [0, m] and c_off.dtype == torch.int32
    q64, v64 = _fp64(idx, tq)
    assert torch.allclose(q64.norm(dim=1), torch.ones(m, dtype=torch.float64, device="cuda"), atol=2.0 ** -4 if fmt == "e4m3" else 2.0 ** -8)
    # the margins in fp64: every diagonal of every video, and the format's bound on a diagonal sum
    S, Ab = (q64 @ v64.T).cpu().numpy(), (q64.abs() @ v64.abs().T).cpu().numpy()
    nv, off = len(idx.vids), idx.v_off
    sums = [ref.diag_sums(S[:, off[v]:off[v + 1]]) for v in range(nv)]
    per_term = [ACC_EPS * ref.diag_sums(Ab[:, off[v]:off[v + 1]]) if fmt == "e4m3" else np.full(len(sums[v]), m * EPS) for v in range(nv)]
    bound = [b + m * m * 2.0 ** -24 for b in per_term]
    assert len(sums[4]) == 0 and all(len(sums[v]) for v in range(nv) if v != 4)
    lo = lambda v, t: sums[v][t] - bound[v][t]                                       # noqa: E731
    hi_but = lambda v, t: max((sums[v][u] + bound[v][u] for u in range(len(sums[v])) if u != t), default=-np.inf)   # noqa: E731
    assert lo(A, a0) > hi_but(A, a0) and lo(B, b0) > hi_but(B, b0)                    # the planted starts stand clear inside their videos
    assert lo(A, a0) > sums[B][b0] + bound[B][b0]                                     # the source beats its noisy copy
    rest = max(hi_but(v, -1) for v in range(nv) if v not in (A, B, 4))
    assert lo(B, b0) > rest                                                           # and the copy every other diagonal of the corpus
    print(f"search_clips {fmt}: fp64 sums source {sums[A][a0]:.4f}, copy {sums[B][b0]:.4f}, best other {rest:.4f}; "
          f"bounds {bound[A][a0]:.2e} / {bound[B][b0]:.2e}")
    k = 5
    hits = srch.search_clips(idx, [clip], k=k)[0]
    assert len(hits) == k and all(isinstance(h, srch.ClipHit) for h in hits)
    assert tuple(hits[0])[:3] == (idx.vids[A], a0, a0 + m - 1) and tuple(hits[1])[:3] == (idx.vids[B], b0, b0 + m - 1)
    assert all(h.end - h.start + 1 == m for h in hits) and len({h.vid for h in hits}) == k
    assert [h.score for h in hits] == sorted((h.score for h in hits), reverse=True)
    sweep = dict(q_scale=tq[1], v_scale=idx.scale) if idx.e4m3 else {}
    top_s, top_r, top_v = ops.clip_topk(tq[0] if idx.e4m3 else tq, idx.feat, c_off, idx.v_off_device, k, **sweep)
    assert [h.score for h in hits] == [float(s) / m for s in top_s[0].tolist()]
    assert [idx.vids.index(h.vid) for h in hits] == top_v[0].tolist()
    assert abs(hits[0].score * m - sums[A][a0]) <= bound[A][a0] and abs(hits[1].score * m - sums[B][b0]) <= bound[B][b0]
    # without the source: the same list without A; k is clamped and a list is shorter than k when fewer videos are long enough
    assert srch.search_clips(idx, [clip], k=k - 1, exclude_source=True)[0] == [h for h in hits if h.vid != idx.vids[A]]
    assert srch.search_clips(idx, [clip], k=50)[0] == hits
    assert srch.search_clips(idx, [clip], k=50, exclude_source=True)[0] == hits[1:]
    for splits in (1, 2, 7):
        assert srch.search_clips(idx, [clip], k=k, splits=splits)[0] == hits
    # the same rows handed over as a tensor: the same hits; a tensor has no source to leave out
    rows = v64[off[A] + a0:off[A] + a0 + m].float()                                  # exact: bf16 values, or code x power of two
    assert srch.search_clips(idx, [rows], k=k)[0] == hits
    assert srch.search_clips(idx, [rows], k=k - 1, exclude_source=True)[0] == hits[:k - 1]
    # several clips in one call, among them one second and 32 seconds
    many = srch.search_clips(idx, [clip, (idx.vids[A], a0, a0), (B, b0 - 6, b0 + 25), rows], k=k)
    assert many[0] == hits == many[3] and len(many[1]) == k and all(h.start == h.end for h in many[1])
    assert many[2][0][:3] == (idx.vids[B], b0 - 6, b0 + 25) and len(many[2]) == 5                        # 12 rows are too short
    # the command line: no checkpoint, no model; the source is left out unless --keep-source
    path = str(tmp_path / "index.npz")
    idx.save(path)
    capsys.readouterr()
    assert srch.main(["similar", "--index", path, "--clip", f"{idx.vids[A]}:{a0}-{a0 + m - 1}", "-k", "3"]) == 0
    out = [line.split("\t") for line in capsys.readouterr().out.splitlines()]
    assert [(o[0], int(o[1]), int(o[2])) for o in out] == [tuple(h)[:3] for h in hits[1:4]]
    assert [o[3] for o in out] == [f"{h.score:.6f}" for h in hits[1:4]]
    assert srch.main(["similar", "--index", path, "--clip", f"{idx.vids[A]}:{a0}-{a0 + m - 1}", "-k", "3", "--keep-source"]) == 0
    out = [line.split("\t") for line in capsys.readouterr().out.splitlines()]
    assert [(o[0], int(o[1]), int(o[2])) for o in out] == [tuple(h)[:3] for h in hits[:3]]
    assert srch.main(["similar", "--index", path, "--clip", "nobody:0-3"]) == 2 and "nobody" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------------------- 8. sharded
@pytest.mark.parametrize("fmt", FORMATS)
def test_sharded_search_clips_equal_the_concatenated_index(fmt):
    """The layout cut into three shards: videos 0..7, the 150 videos of 1..5 rows -- every one shorter than all clips but the
    one-second one, so for those the shard contributes only empty slots --, and the long ones."""
    srch, ops = _srch(), _ops()
    feat = _unit_rows(N, 61, torch.float32)
    feat[V_OFF[163] + 40:V_OFF[163] + 70] = feat[V_OFF[160] + 10:V_OFF[160] + 40]   # a re-upload among the 200-row videos
    scale = None
    if fmt == "e4m3":
        feat, scale = ops.quantize_rows_e4m3(feat)
    elif fmt == "bf16":
        feat = feat.bfloat16()
    cuts = (0, 8, 158, NV)
    assert max(LENS[8:158]) == 5
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        r0, r1 = int(V_OFF[a]), int(V_OFF[b])
        parts.append(srch.VideoIndex(feat[r0:r1].contiguous(), V_OFF[a:b + 1] - r0, [f"v{i:03d}" for i in range(a, b)],
                                     None if scale is None else scale[r0:r1].contiguous()))
    whole = srch.VideoIndex.concat(parts)
    clips = [("v160", 10, 39), ("v005", 100, 106), _unit_rows(32, 62, torch.float32), ("v100", 0, 0), (163, 150, 181), ("v002", 0, 5)]
    for resident in ("device", "host"):
        sharded = srch.ShardedIndex(parts, resident="device") if resident == "device" else srch.ShardedIndex(_pinned(parts), resident="host")
        for k, kw in ((20, {}), (1, {}), (10, dict(exclude_source=True)), (20, dict(splits=7))):
            want = srch.search_clips(whole, clips, k=k, **kw)
            got = srch.search_clips(sharded, clips, k=k, **kw)
            assert got == want, (resident, k, kw)
        assert [len(h) for h in want] == [15, 15, 15, 20, 15, 15]                  # 15 videos hold 6 rows or more
    want = srch.search_clips(whole, clips, k=20)
    assert want[0][0][:3] == ("v160", 10, 39) and want[0][1][:3] == ("v163", 40, 69)
    assert want[3][0][:3] == ("v100", 0, 0)                                         # the one-second clip finds itself in the middle shard
    assert all(h.vid not in ("v160",) for h in srch.search_clips(sharded, clips[:1], k=5, exclude_source=True)[0])
    torch.cuda.synchronize()
