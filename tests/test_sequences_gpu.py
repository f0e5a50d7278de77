"""Ordered-sequence search on the GPU: tan_sequence_topk (the k videos with the best order-preserving path per sequence of steps),
tan_sequence_scores (the winners' step x second scores, the sweep's own bits), `ops.sequence_topk` / `ops.sequence_scores`,
`search.search_sequences`.  The path and its tie rule are restated in numpy in sequence_ref.py (pinned against exhaustive
enumeration by test_sequences_cpu.py).

  * exact arithmetic: f32 / bf16 rows are multiples of 1/16 in [-1, 1], so 256 x score is an integer of at most 2^17 and a path of
    32 steps stays below 2^22 < 2^24: every score and every partial sum is exact in f32.  e4m3: codes 16 x with x in [-16, 16]
    (queries) and [-8, 8] (index), scales 2^-9 / 2^-8 (queries) and 2^-8 / 2^-7 (index): 512 x score is an integer of at most 2^18,
    a path stays below 2^23.  Lists are compared with `==` against an int64 dynamic programme.
  * random unit rows: tan_sequence_scores for ALL (sequence, video) pairs against the fp64 product of the stored rows, with
    test_moments_gpu.py's bounds (EPS = 2e-5 for f32 / bf16, ACC_EPS * sum |a b| for e4m3); the numpy recurrence over THOSE device
    bits gives every video's path, whose top k equal the lists with `==`; tan_monotonic_decode over the same blocks returns the same
    paths bit for bit and the numpy backtrack's seconds.
The layout (2742 rows, 168 videos): videos of 1, 2, 63, 64, 65, 128, 129 and 3 rows (tile edges; V < m), 150 videos of 1 .. 5 rows
(more than 64 finished videos per split: the candidate registers are compacted), nine of 200 rows (more than two tiles each) and a
last one of 37 rows that ends off-tile.  The boundaries of splits = 2 and 7 fall inside videos of more than two tiles."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import sequence_ref as ref
from temporalalignnet_amd import _lib
from test_moments_gpu import DT, FORMATS, _dev, _ops, _stored
from test_retrieve_fp8_gpu import ACC_EPS, _deq, _int_codes
from test_retrieve_gpu import EPS, _embed, _exact_rows, _gen, _model, _unit_rows, _videos

pytestmark = pytest.mark.gpu

LENS = [1, 2, 63, 64, 65, 128, 129, 3] + [1 + j % 5 for j in range(150)] + [200] * 9 + [37]
V_OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
N, NV = int(V_OFF[-1]), len(LENS)
STEPS = {1: [31], 4: [1, 2, 31, 32], 5: [32, 1, 2, 31, 7]}         # n_seq -> m per sequence; five sequences cross a workgroup
SPLITS = (0, 1, 2, 7)


def _s_off(ms):
    return np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)


def _seq_split_starts(n_rows, splits):
    """The first rows of the splits the sequence sweep makes (the launch's own arithmetic); a video belongs to the split that
    holds its first row."""
    want = min(splits, (n_rows + 63) // 64)
    rps = (n_rows + want - 1) // want
    return list(range(rps, n_rows, rps))


def test_the_layout_has_the_edges_it_claims():
    assert N == 2742 and NV == 168 and N % 64 != 0 and N <= 3000
    for splits in (2, 7):
        inside = [b for b in _seq_split_starts(N, splits)
                  if any(lo < b < hi and hi - lo > 128 for lo, hi in zip(V_OFF[:-1], V_OFF[1:]))]
        assert inside, splits                                      # a video of more than two tiles straddles a split boundary
    assert NV > 2 * 64                                             # splits = 1: the 64 candidates are compacted more than once


# ----------------------------------------------------------------------------------------------------------------------- inputs
def _exact_case(fmt, ms, seed=0):
    """tq, vn, scale keywords, X int64 [Qt, N] (host) with score * mult == X"""
    Qt = int(sum(ms))
    if fmt != "e4m3":
        tq, vn = _exact_rows(Qt, 500 + Qt + seed, DT[fmt]), _exact_rows(N, 600 + seed, DT[fmt])
        X = ((tq.double() * 16) @ (vn.double() * 16).T).round().long().cpu().numpy()
        assert 32 * int(np.abs(X).max()) < 2 ** 24
        return tq, vn, {}, X, 256.0
    xq = torch.randint(-16, 17, (Qt, 512), generator=_gen(500 + Qt + seed), device="cuda")
    xv = torch.randint(-8, 9, (N, 512), generator=_gen(600 + seed), device="cuda")
    eq = torch.randint(-9, -7, (Qt,), generator=_gen(7), device="cuda")
    ev = torch.randint(-8, -6, (N,), generator=_gen(8), device="cuda")
    I = (xq.double() @ xv.double().T).round().long()               # score = 256 I 2^(ev + eq); x 512 = I 2^(17 + ev + eq)
    X = (I * (torch.ones_like(I) << (17 + ev[None, :] + eq[:, None]))).cpu().numpy()
    assert 32 * int(np.abs(X).max()) < 2 ** 24
    kw = dict(q_scale=torch.ldexp(torch.ones(Qt, device="cuda"), eq), v_scale=torch.ldexp(torch.ones(N, device="cuda"), ev))
    return _int_codes(xq), _int_codes(xv), kw, X, 512.0


def _unit_case(fmt, ms, seed=0):
    return _stored(fmt, _unit_rows(int(sum(ms)), 700 + seed, torch.float32), _unit_rows(N, 800 + seed, torch.float32))


def _all_pairs(n_seq, n_videos):
    return np.stack((np.repeat(np.arange(n_seq), n_videos), np.tile(np.arange(n_videos), n_seq)), 1)


def _blocks(hits, s_off, v_off, guard=0):
    """hits [P, 2] (host) -> m [P], V [P], x_off [P + 1]: the [m, V] blocks one after the other, `guard` elements before each"""
    hm = (s_off[hits[:, 0] + 1] - s_off[hits[:, 0]]).astype(np.int64)
    hv = (v_off[hits[:, 1] + 1] - v_off[hits[:, 1]]).astype(np.int64)
    x_off = np.concatenate([[0], np.cumsum(hm * hv + guard)]) + guard
    return hm, hv, x_off


def _scores(tq, vn, kw, s_off, v_off, hits, guard=0, fill=float("nan")):
    """x (device, one buffer) and the blocks' geometry for `hits`"""
    hm, hv, x_off = _blocks(hits, s_off, v_off, guard)
    x = torch.full((int(x_off[-1]),), fill, device="cuda")
    _ops().sequence_scores(tq, vn, _dev(s_off), _dev(v_off), _dev(hits), torch.from_numpy(x_off[:-1].copy()).cuda(), x,
                           check_offsets=True, **kw)
    return x, hm, hv, x_off


def _decode(x, hm, hv, x_off):
    """tan_monotonic_decode over the blocks: one "video" of its tables per hit, the hit's m rows in step order ->
    (seconds: a list of tuples, path [P] f32 device)"""
    P = len(hm)
    first = np.concatenate([[0], np.cumsum(hm)])
    hit_of_row = np.repeat(np.arange(P), hm)
    step = np.arange(first[-1]) - first[hit_of_row]
    rows = np.stack((x_off[hit_of_row] + step * hv[hit_of_row], hv[hit_of_row]), 1)
    vtab = np.stack((first[:-1], hm, np.concatenate([[0], np.cumsum(hv)])[:-1]), 1)
    ts = torch.full((int(first[-1]),), -7, dtype=torch.int32, device="cuda")
    path = torch.empty(P, device="cuda")
    _ops().monotonic_decode(x, _dev(rows), torch.arange(int(first[-1]), dtype=torch.int32, device="cuda"), _dev(vtab), None,
                            torch.empty(x.numel(), dtype=torch.int32, device="cuda"), torch.empty(int(hv.sum()), device="cuda"), ts, path)
    ts = ts.cpu().numpy()
    return [tuple(int(t) for t in ts[first[h]:first[h + 1]]) for h in range(P)], path


# ------------------------------------------------------------------------------------------------------------- 1. exact arithmetic
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n_seq", sorted(STEPS))
def test_sequence_topk_exact_arithmetic(n_seq, fmt):
    ops = _ops()
    ms = STEPS[n_seq]
    s_off = _s_off(ms)
    tq, vn, kw, X, mult = _exact_case(fmt, ms)
    want = ref.paths(X, s_off, V_OFF)                               # int64
    assert any(V < m for V in LENS for m in ms)
    for k in (1, 10, 32):
        want_s, want_v = ref.topk(want, k)
        for splits in SPLITS:
            top_s, top_v = ops.sequence_topk(tq, vn, _dev(s_off), _dev(V_OFF), k, splits=splits, check_offsets=True, **kw)
            assert np.array_equal(top_v.cpu().numpy(), want_v), (k, splits)
            assert np.array_equal((top_s.double() * mult).cpu().numpy(), want_s.astype(np.float64)), (k, splits)
    # the score blocks of the winners hold the integer scores themselves
    hits = np.stack((np.repeat(np.arange(n_seq), 10), ref.topk(want, 10)[1].reshape(-1)), 1)
    x, hm, hv, x_off = _scores(tq, vn, kw, s_off, V_OFF, hits)
    x = (x.double() * mult).cpu().numpy()
    for h, (p, v) in enumerate(hits):
        assert np.array_equal(x[x_off[h]:x_off[h] + hm[h] * hv[h]].reshape(hm[h], hv[h]),
                              X[s_off[p]:s_off[p + 1], V_OFF[v]:V_OFF[v + 1]].astype(np.float64)), (p, v)


# --------------------------------------------------------------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("fmt", FORMATS)
def test_ties_between_videos_and_between_seconds(fmt):
    """Two bit-identical videos rank by their number.  A video whose two steps tie at seconds 3 and 7 -- (3, 3), (3, 7) and (7, 7)
    all reach the same sum -- gets the decode's seconds: the smallest last second, then the smallest second to last, (3, 3)."""
    ops = _ops()
    ms = [2, 1, 5]
    s_off = _s_off(ms)
    fq, fv = _unit_rows(int(sum(ms)), 31, torch.float32), _unit_rows(N, 32, torch.float32)
    a, b = 159, 165                                                 # two of the 200-row videos (four tiles each), in different splits of 2 and 7
    assert LENS[a] == LENS[b] == 200
    fv[V_OFF[b]:V_OFF[b + 1]] = fv[V_OFF[a]:V_OFF[a + 1]]
    c = 6                                                           # the 129-row video: both steps of sequence 0 fit seconds 3 and 7 best
    strong = (fq[0] + fq[1]) / (fq[0] + fq[1]).norm()
    fv[V_OFF[c] + 3] = strong
    fv[V_OFF[c] + 7] = strong
    tq, vn, kw, S, _ = _stored(fmt, fq, fv)
    for splits in SPLITS:
        top_s, top_v = ops.sequence_topk(tq, vn, _dev(s_off), _dev(V_OFF), 32, splits=splits, **kw)
        full_s, full_v = top_s.cpu().numpy(), top_v.cpu().numpy()
        assert full_v[0, 0] == c, splits
    # an index of the identical pair alone: both are in the lists, the lower number first
    pair_off = np.array([0, 200, 400], dtype=np.int64)
    pair_rows = torch.cat((torch.arange(V_OFF[b], V_OFF[b + 1]), torch.arange(V_OFF[a], V_OFF[a + 1]))).cuda()
    pv = vn[pair_rows].contiguous()
    pkw = dict(q_scale=kw["q_scale"], v_scale=kw["v_scale"][pair_rows].contiguous()) if kw else {}
    for splits in SPLITS:
        top_s, top_v = ops.sequence_topk(tq, pv, _dev(s_off), _dev(pair_off), 2, splits=splits, **pkw)
        assert top_v.tolist() == [[0, 1]] * 3 and torch.equal(top_s[:, 0], top_s[:, 1]), splits
    # inside the full index: ranked over every video the pair is adjacent and in order, and so it is in the lists where it made them
    hits = _all_pairs(3, NV)
    x, hm, hv, x_off = _scores(tq, vn, kw, s_off, V_OFF, hits)
    xs = x.cpu().numpy()
    path = np.array([ref.path_and_seconds(xs[x_off[h]:x_off[h] + hm[h] * hv[h]].reshape(hm[h], hv[h]))[0] for h in range(len(hits))],
                    dtype=np.float32).reshape(3, NV)
    assert (path[:, a] == path[:, b]).all()
    order = ref.topk(path, NV)[1]
    for p in range(3):
        ia, ib = list(order[p]).index(a), list(order[p]).index(b)
        assert ib == ia + 1, p
        if ib < 32:
            assert full_v[p, ia] == a and full_v[p, ib] == b and full_s[p, ia] == full_s[p, ib]
    seconds, dpath = _decode(x, hm, hv, x_off)
    h = 0 * NV + c
    blk = xs[x_off[h]:x_off[h] + 2 * 129].reshape(2, 129)
    assert blk[0, 3] == blk[0, 7] and blk[1, 3] == blk[1, 7]
    assert seconds[h] == (3, 3) == ref.path_and_seconds(blk)[1]
    assert dpath[h].item() == full_s[0, 0] == np.float32(blk[0, 3] + blk[1, 3])


# --------------------------------------------------------------------------------------- 3. one step: the existing video sweep
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_step_sequences_equal_rank_topk_video(fmt):
    ops = _ops()
    Q = 9
    tq, vn, kw, _, _ = _unit_case(fmt, [1] * Q, seed=3)
    s_off = np.arange(Q + 1, dtype=np.int64)
    for k in (1, 10, 32):
        row_s, _, row_v = ops.rank_topk_video(tq, vn, _dev(V_OFF), k, **kw)
        for splits in SPLITS:
            top_s, top_v = ops.sequence_topk(tq, vn, _dev(s_off), _dev(V_OFF), k, splits=splits, **kw)
            assert torch.equal(top_s, row_s) and torch.equal(top_v, row_v), (k, splits)


# ------------------------------------------------------------------------------------------------------- 4. random unit rows
@pytest.mark.parametrize("fmt", FORMATS)
def test_sequence_topk_random_unit_rows(fmt):
    ops = _ops()
    ms = STEPS[5]
    s_off = _s_off(ms)
    tq, vn, kw, S, _ = _unit_case(fmt, ms)
    if fmt == "e4m3":
        a, b = _deq(tq, kw["q_scale"]), _deq(vn, kw["v_scale"])
        eps = ACC_EPS * (a.abs() @ b.abs().T)                       # per score
    else:
        eps = torch.full_like(S, EPS)
    hits = _all_pairs(len(ms), NV)
    x, hm, hv, x_off = _scores(tq, vn, kw, s_off, V_OFF, hits)
    xs = x.cpu().numpy()
    S_h, eps_h = S.cpu().numpy(), eps.cpu().numpy()
    path = np.empty((len(ms), NV), dtype=np.float32)
    want_sec, worst = [], 0.0
    for h, (p, v) in enumerate(hits):
        blk = xs[x_off[h]:x_off[h] + hm[h] * hv[h]].reshape(hm[h], hv[h])
        err = np.abs(blk.astype(np.float64) - S_h[s_off[p]:s_off[p + 1], V_OFF[v]:V_OFF[v + 1]])
        worst = max(worst, float(err.max()))
        assert (err <= eps_h[s_off[p]:s_off[p + 1], V_OFF[v]:V_OFF[v + 1]]).all(), (p, v, float(err.max()))
        path[p, v], sec = ref.path_and_seconds(blk)
        want_sec.append(sec)
    print(f"sequence_scores max |x - fp64| {fmt}: {worst:.3e} (bound {float(eps.max()):.3e})")
    assert np.isfinite(path).all()
    for k in (1, 10, 32):
        want_s, want_v = ref.topk(path, k)
        for splits in SPLITS:
            top_s, top_v = ops.sequence_topk(tq, vn, _dev(s_off), _dev(V_OFF), k, splits=splits, **kw)
            assert np.array_equal(top_v.cpu().numpy(), want_v), (k, splits)
            assert np.array_equal(top_s.cpu().numpy().view(np.int32), want_s.view(np.int32)), (k, splits)
    # the decode over the same blocks: the paths bit for bit (hence top_score for the winners), and the backtrack's seconds
    seconds, dpath = _decode(x, hm, hv, x_off)
    assert np.array_equal(dpath.cpu().numpy().view(np.int32).reshape(len(ms), NV), path.view(np.int32))
    assert seconds == want_sec
    top_s, top_v = ops.sequence_topk(tq, vn, _dev(s_off), _dev(V_OFF), 10, **kw)
    assert torch.equal(top_s, dpath.view(len(ms), NV).gather(1, top_v.long()))


# -------------------------------------------------------------------- 5. determinism, split invariance, nothing else is written
@pytest.mark.parametrize("fmt", FORMATS)
def test_sequence_entry_points_are_deterministic_and_write_nothing_else(fmt):
    ops = _ops()
    G = 64
    for ms, k in ((STEPS[5], 10), (STEPS[1], 32), (STEPS[4], 1)):
        n_seq, s_off = len(ms), _s_off(ms)
        tq, vn, kw, _, _ = _unit_case(fmt, ms, seed=20)
        s_dev, v_dev = _dev(s_off), _dev(V_OFF)
        ref_out = ops.sequence_topk(tq, vn, s_dev, v_dev, k, check_offsets=True, **kw)
        top_s = torch.full((n_seq * k + G,), float("nan"), device="cuda")
        top_v = torch.full((n_seq * k + G,), -777, dtype=torch.int32, device="cuda")
        nws = ops.sequence_topk_ws_bytes(n_seq, N, k)
        ws = torch.full((nws + G,), 0xFF, dtype=torch.uint8, device="cuda")
        out = (top_s[:n_seq * k].view(n_seq, k), top_v[:n_seq * k].view(n_seq, k))
        for splits in SPLITS + SPLITS + (5, 43, 256, 1000):
            out[0].fill_(float("nan"))
            out[1].fill_(-777)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ops.sequence_topk(tq, vn, s_dev, v_dev, k, splits=splits, out=out, ws=ws[:nws], **kw)
            torch.cuda.synchronize()
            assert torch.cuda.max_memory_allocated() == base, (ms, k, splits)
            assert torch.equal(out[0], ref_out[0]) and torch.equal(out[1], ref_out[1]), (ms, k, splits)
            assert (ws[nws:] == 0xFF).all() and torch.isnan(top_s[n_seq * k:]).all() and (top_v[n_seq * k:] == -777).all()
        assert torch.isfinite(out[0]).all() and ((out[1] >= 0) & (out[1] < NV)).all()
        assert all(len(set(v)) == k for v in out[1].tolist())
        # the winners' score blocks, with a guard band before, between and after them
        hits = np.stack((np.repeat(np.arange(n_seq), k), out[1].cpu().numpy().reshape(-1)), 1)
        x, hm, hv, x_off = _scores(tq, vn, kw, s_off, V_OFF, hits, guard=G, fill=-123.0)
        again = _scores(tq, vn, kw, s_off, V_OFF, hits, guard=G, fill=-123.0)[0]
        assert torch.equal(x, again)
        inside = torch.zeros(x.numel(), dtype=torch.bool, device="cuda")
        for h in range(len(hits)):
            inside[x_off[h]:x_off[h] + hm[h] * hv[h]] = True
        assert (x[~inside] == -123.0).all() and int((~inside).sum()) == G * (len(hits) + 1)
        assert (x[inside] != -123.0).all() and torch.isfinite(x[inside]).all()
        seconds, dpath = _decode(x, hm, hv, x_off)
        assert torch.equal(dpath.view(n_seq, k), out[0])
        assert all(len(s) == m and all(0 <= a <= b for a, b in zip(s, s[1:])) and s[-1] < V for s, m, V in zip(seconds, hm, hv))


# --------------------------------------------------------------------------------------------------------- 6. invalid arguments
def test_sequence_entry_points_reject_invalid_arguments():
    ops = _ops()
    L = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                     # noqa: E731
    ms, k = [3, 1, 4], 3
    Qt, Nn = 8, 40
    s_off, v_off = _dev(_s_off(ms)), _dev([0, 10, 11, 25, 40])
    f32 = (_unit_rows(Qt, 1, torch.float32), _unit_rows(Nn, 2, torch.float32))
    (q8, qs), (v8, vs) = ops.quantize_rows_e4m3(f32[0]), ops.quantize_rows_e4m3(f32[1])
    ts, tv = torch.empty(3, k, device="cuda"), torch.empty(3, k, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.sequence_topk_ws_bytes(3, Nn, k), dtype=torch.uint8, device="cuda")
    hits = _dev([[0, 0], [1, 3], [2, 2]])
    x_off = torch.tensor([0, 30, 45], dtype=torch.int64, device="cuda")
    x = torch.empty(45 + 4 * 14, device="cuda")

    def topk(e4m3=False, dtype=0, Qt=Qt, N=Nn, Cc=512, so=s_off, n_seq=3, vo=v_off, nv=4, k=k, splits=0, s=ts, v=tv, w=ws, sa=qs, sb=vs):
        a, b = (q8, v8) if e4m3 else f32
        if e4m3:
            return L.tan_sequence_topk_e4m3(p(a), p(sa), p(b), p(sb), Qt, N, Cc, p(so), n_seq, p(vo), nv, k, splits, p(s), p(v), p(w), None)
        return L.tan_sequence_topk(p(a), p(b), dtype, Qt, N, Cc, p(so), n_seq, p(vo), nv, k, splits, p(s), p(v), p(w), None)

    def scores(e4m3=False, dtype=0, Qt=Qt, N=Nn, Cc=512, so=s_off, n_seq=3, vo=v_off, nv=4, h=hits, xo=x_off, P=3, x=x, n_x=None,
               sa=qs, sb=vs):
        a, b = (q8, v8) if e4m3 else f32
        n_x = x.numel() if n_x is None else n_x
        if e4m3:
            return L.tan_sequence_scores_e4m3(p(a), p(sa), p(b), p(sb), Qt, N, Cc, p(so), n_seq, p(vo), nv, p(h), p(xo), P, p(x), n_x, None)
        return L.tan_sequence_scores(p(a), p(b), dtype, Qt, N, Cc, p(so), n_seq, p(vo), nv, p(h), p(xo), P, p(x), n_x, None)

    class Null:                                                                       # a NULL pointer for one argument
        @staticmethod
        def data_ptr():
            return None

        @staticmethod
        def numel():
            return 100
    null = Null()
    sizes = (dict(Cc=256), dict(Cc=1024), dict(n_seq=0), dict(Qt=2), dict(Qt=97), dict(nv=0), dict(nv=41), dict(nv=-1), dict(N=0),
             dict(N=1 << 31))
    for e4m3 in (False, True):
        assert topk(e4m3) == 0 and scores(e4m3) == 0
        torch.cuda.synchronize()
        for kw in sizes + (dict(k=0), dict(k=33), dict(k=5), dict(k=-1), dict(splits=-1), dict(so=null), dict(vo=null), dict(s=null),
                           dict(v=null), dict(w=null)):
            assert topk(e4m3, **kw) == -1, (e4m3, kw)
        for kw in sizes + (dict(P=0), dict(n_x=0), dict(so=null), dict(vo=null), dict(h=null), dict(xo=null), dict(x=null)):
            assert scores(e4m3, **kw) == -1, (e4m3, kw)
    assert topk(dtype=2) == -1 and scores(dtype=2) == -1
    for kw in (dict(sa=null), dict(sb=null)):
        assert topk(True, **kw) == -1 and scores(True, **kw) == -1
    # hits and offsets that point outside the tables or outside x: skipped, nothing is written
    x.fill_(-5.0)
    bad_hits = _dev([[-1, 0], [3, 1], [0, 1 << 30]])
    assert scores(h=bad_hits, xo=torch.tensor([0, 0, x.numel() - 1], dtype=torch.int64, device="cuda")) == 0
    assert scores(xo=torch.tensor([-1, x.numel(), 1 << 40], dtype=torch.int64, device="cuda")) == 0
    assert scores(n_x=29) == 0                                                        # every block would end past n_x
    torch.cuda.synchronize()
    assert (x == -5.0).all()

    with pytest.raises(_lib.TanHipError):
        ops.sequence_topk(f32[0].cpu(), f32[1].cpu(), s_off.cpu(), v_off.cpu(), k)
    with pytest.raises(_lib.TanHipError):
        ops.sequence_topk(*f32, s_off, v_off, 5)                                     # k > n_videos
    with pytest.raises(TypeError):
        ops.sequence_topk(*f32, s_off, v_off, k, q_scale=qs, v_scale=vs)
    for bad in ([0, 10, 10, 25, 40], [0, 10, 9, 25, 40], [0, 10, 11, 25, 39], [1, 10, 11, 25, 40]):
        with pytest.raises(ValueError):
            ops.sequence_topk(*f32, s_off, _dev(bad), k, check_offsets=True)
        ops.sequence_topk(*f32, s_off, _dev(bad), k)                                 # unchecked: the caller's error, but memory-safe
    for bad in ([0, 3, 3, 8], [0, 5, 4, 8], [0, 3, 4, 7], [1, 3, 4, 8]):
        with pytest.raises(ValueError):
            ops.sequence_topk(*f32, _dev(bad), v_off, k, check_offsets=True)
        ops.sequence_topk(*f32, _dev(bad), v_off, k)
    wide = _unit_rows(40, 5, torch.float32)
    with pytest.raises(ValueError):
        ops.sequence_topk(wide, f32[1], _dev([0, 33, 40]), v_off, k, check_offsets=True)        # 33 steps
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- 7. end to end
def _dual_basis(F):
    """rows u_i with <F[j], u_i> = 1 if i == j else 0 (fp64)"""
    return torch.linalg.pinv(F.double()).T.contiguous()


@pytest.mark.parametrize("fmt", FORMATS)
def test_search_sequences_end_to_end(fmt, tmp_path):
    """Video A (number 2) holds six steps' rows in order, video B (0) the same rows in reverse order, video C (3) only the first
    step's, half again as strong.  The planted rows are G times the steps' dual basis: step i scores G on its own row and 0 on the
    others' (before the format's rounding), and at most 1 in absolute value on any unplanted row (an index row is a mean of unit
    vectors).  So A's path is at least 6 G, B's at most G + 5 and C's at most 1.5 G + 5."""
    from temporalalignnet_amd import search as srch
    m = _model()
    vids = _videos([70, 33, 150, 64, 20], seed=9)
    f32 = srch.build_index(m, vids, dtype=torch.float32)
    M = 6
    pool = [f"step {i}" for i in range(10)]
    fpool = srch.query_features(f32, m, _embed, pool)
    # the six least alike sentences of the pool: the smallest dual basis
    pick = min(itertools.combinations(range(10), M), key=lambda c: float(_dual_basis(fpool[list(c)]).norm(dim=1).max()))
    steps = [pool[i] for i in pick]
    U = _dual_basis(fpool[list(pick)]).float()
    G = 8.0
    off = [int(x) for x in f32.v_off]
    assert (f32.feat.norm(dim=1) <= 1 + 1e-5).all()
    A, B, Cv = 2, 0, 3
    sec_a, sec_b = (10, 40, 63, 64, 104, 149), (5, 30, 31, 50, 64, 69)
    for i in range(M):
        f32.feat[off[A] + sec_a[i]] = G * U[i]
        f32.feat[off[B] + sec_b[i]] = G * U[M - 1 - i]
    f32.feat[off[Cv] + 5] = 1.5 * G * U[0]
    idx = f32 if fmt == "f32" else (f32.quantize() if fmt == "e4m3" else srch.VideoIndex(f32.feat.bfloat16(), f32.v_off, f32.vids))
    # fp64 paths of the unquantised rows, and per (step, row) the format's bound on a score: (b) of DESIGN 3.12 for e4m3, the
    # operand rounding (2^-8 relative on each side) plus EPS for bf16, EPS scaled by the planted rows' size for f32
    fq = fpool[list(pick)]
    S0, A0 = (fq.double() @ f32.feat.double().T).cpu().numpy(), (fq.double().abs() @ f32.feat.double().abs().T).cpu().numpy()
    if fmt == "e4m3":
        tq = srch.query_features(idx, m, _embed, steps)
        bound = (2.0 ** -3 + 2.0 ** -8) * A0 + 512 * 2.0 ** -10 * (
            idx.scale.double()[None, :] * fq.double().abs().amax(1)[:, None]
            + tq[1].double()[:, None] * f32.feat.double().abs().amax(1)[None, :]).cpu().numpy()
    elif fmt == "bf16":
        bound = (2.0 ** -7 + 2.0 ** -16) * A0 + EPS * np.maximum(A0, 1.0)
    else:
        bound = EPS * np.maximum(A0, 1.0)
    ref_path = ref.paths(S0, np.array([0, M]), f32.v_off)[0]
    slack = np.array([sum(bound[i, off[v]:off[v + 1]].max() for i in range(M)) for v in range(5)])
    print(f"search_sequences {fmt}: fp64 paths {ref_path}, path bounds {slack}, dual basis norms {U.norm(dim=1).tolist()}")
    assert ref_path[A] >= M * G - 1e-3 and ref_path[B] <= G + M - 1 + 1e-3 and ref_path[Cv] <= 1.5 * G + M - 1 + 1e-3
    others = [v for v in range(5) if v != A]
    assert ref_path[A] - slack[A] > max(ref_path[v] + slack[v] for v in others)       # the planted margin exceeds the format's bound
    for i in range(M):                                              # and every step's planted second stands clear of A's other seconds
        row = S0[i, off[A]:off[A + 1]].copy()
        b = bound[i, off[A]:off[A + 1]]
        own = row[sec_a[i]] - b[sec_a[i]]
        row[sec_a[i]] = -np.inf
        assert own > (row + b).max() + 1e-3
    before = srch.search_moments(idx, m, _embed, steps[:1], k=3)
    res = srch.search_sequences(idx, m, _embed, [steps, steps[:1], steps[::-1]], k=5)
    assert srch.search_moments(idx, m, _embed, steps[:1], k=3) == before
    assert len(res) == 3 and all(len(h) == 5 and all(isinstance(x, srch.SequenceHit) for x in h) for h in res)
    for p, hits in enumerate(res):
        mm = (M, 1, M)[p]
        assert len({h.vid for h in hits}) == 5 and [h.score for h in hits] == sorted((h.score for h in hits), reverse=True)
        for h in hits:
            v = idx.vids.index(h.vid)
            assert len(h.seconds) == mm and all(a <= b for a, b in zip(h.seconds, h.seconds[1:]))
            assert 0 <= h.seconds[0] and h.seconds[-1] < off[v + 1] - off[v]
    top = res[0][0]
    assert top.vid == idx.vids[A] and top.seconds == sec_a, top
    assert abs(top.score - ref_path[A]) <= slack[A]
    by_vid = {h.vid: h for h in res[0]}
    assert by_vid[idx.vids[B]].score < top.score and by_vid[idx.vids[Cv]].score < top.score
    for v in range(5):
        assert abs(by_vid[idx.vids[v]].score - ref_path[v]) <= slack[v], v
    # C wins step one alone, in the moment search and as a one-step sequence; the reversed steps find B in B's order
    assert before[0][0].vid == idx.vids[Cv] and before[0][0].second == 5
    assert res[1][0].vid == idx.vids[Cv] and res[1][0].seconds == (5,) and res[1][0].score == before[0][0].score
    assert [h.vid for h in res[1][:3]] == [mo.vid for mo in before[0]]
    assert res[2][0].vid == idx.vids[B] and res[2][0].seconds == sec_b
    path = str(tmp_path / "index.npz")
    idx.save(path)
    assert srch.search_sequences(srch.VideoIndex.load(path), m, _embed, [steps, steps[:1], steps[::-1]], k=5) == res
    assert len(srch.search_sequences(idx, m, _embed, [steps], k=50)[0]) == 5          # k is clamped to the number of videos
    for splits in (1, 2, 7):
        assert srch.search_sequences(idx, m, _embed, [steps, steps[:1], steps[::-1]], k=5, splits=splits) == res
    with pytest.raises(ValueError):
        srch.search_sequences(idx, m, _embed, [steps, []])
    with pytest.raises(ValueError):
        srch.search_sequences(idx, m, _embed, [["s"] * 33])
