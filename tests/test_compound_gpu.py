"""Compound search on the GPU: tan_compound_topk (per compound query the k videos whose WEAKEST clause peaks highest, a clause being
worth its best term, minus the videos a banned term matches), tan_compound_peaks (the winners' per-term peaks and rows, the sweep's
own bits), `ops.compound_topk` / `ops.compound_peaks`, `search.search_compound`, `query --all`.  The definition is restated in
numpy in compound_ref.py (pinned against a brute force by test_compound_cpu.py).  Every comparison is `==` on bit patterns.

  * exact arithmetic: test_sequences_gpu.py's inputs -- 256 x score (f32 / bf16) or 512 x score (e4m3) is an integer below 2^24 --
    against the reference over the int64 matrix; the veto is one of the banned peaks, so the `>=` is met with equality.
  * random unit rows: x for ALL (query, video) pairs from tan_sequence_scores (existing code); the reference in float32 over those
    device bits reproduces lists and peaks, and every score lies within the per-score bound of the fp64 min-of-max over the stored
    operands (max and min are 1-Lipschitz: they inherit the bound of a single score and nothing more).
The layout is test_sequences_gpu.py's (2742 rows, 168 videos: one tile, tile edges, several tiles with a tail, 150 videos of 1 .. 5
rows so that a query's candidates overflow the 64 candidate registers, splits whose boundaries fall inside long videos)."""
import ctypes as C

import numpy as np
import pytest
import torch

import compound_ref as ref
from temporalalignnet_amd import _lib
from test_cover_gpu import _exact
from test_moments_gpu import FORMATS, _dev, _ops, _stored
from test_retrieve_fp8_gpu import ACC_EPS, _deq
from test_retrieve_gpu import EPS, _embed, _model, _unit_rows, _videos
from test_sequences_gpu import LENS, N, NV, SPLITS, V_OFF, _all_pairs, _exact_case, _s_off, _scores, _unit_case
from test_shards_gpu import _pinned

pytestmark = pytest.mark.gpu

INF = float("inf")
ONE, C32, O32, MIX = [0], list(range(32)), [7] * 32, [0, 0, 1, -1, 2, 2, 2, -1]
T31 = [-1 if j % 6 == 0 else (5 * j) % 11 for j in range(31)]      # 31 terms: six banned, clauses 1 .. 10 out of order
ROLES = {1: [MIX], 4: [ONE, C32, O32, T31], 5: [C32, ONE, MIX, T31, O32]}     # n_query -> roles per query; the fifth query: a second workgroup


def _tables(roles):
    return _s_off([len(r) for r in roles]), np.concatenate(roles).astype(np.int32)


def _i32(t):
    return t.cpu().numpy().view(np.int32)


def _peaks_all(tq, vn, kw, t_off, v_off):
    """tan_compound_peaks for ALL (query, video) pairs: (peak_s f32 [nq, nv, 32], peak_r int32 [nq, nv, 32]) on the host"""
    nq, nv = len(t_off) - 1, len(v_off) - 1
    ps, pr = _ops().compound_peaks(tq, vn, _dev(t_off), _dev(v_off), _dev(_all_pairs(nq, nv)), check_offsets=True, **kw)
    return ps.cpu().numpy().reshape(nq, nv, 32), pr.cpu().numpy().reshape(nq, nv, 32)


def _check_peaks(got_s, got_r, p, r, t_off, scale=None):
    """the kernel's [nq, nv, 32] peaks against the reference's [Qt, nv]: columns < m the peaks (scale: x mult as float64, else bits),
    columns >= m the filler"""
    for q in range(len(t_off) - 1):
        a, m = int(t_off[q]), int(t_off[q + 1] - t_off[q])
        if scale is None:
            assert np.array_equal(got_s[q, :, :m].view(np.int32), p[a:a + m].T.view(np.int32)), q
        else:
            assert np.array_equal(got_s[q, :, :m].astype(np.float64) * scale, p[a:a + m].T.astype(np.float64)), q
        assert np.array_equal(got_r[q, :, :m], r[a:a + m].T), q
        assert np.isneginf(got_s[q, :, m:]).all() and (got_r[q, :, m:] == ref.SENT).all(), q


def _median_veto(p, role):
    """one of the banned terms' peaks, near their median: some videos are banned by it (one with equality) and some are not"""
    banned = np.sort(p[role < 0].reshape(-1))
    return banned[len(banned) // 2]


# ------------------------------------------------------------------------------------------------------------- 1. exact arithmetic
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n_query", sorted(ROLES))
def test_compound_topk_exact_arithmetic(n_query, fmt):
    ops = _ops()
    t_off, role = _tables(ROLES[n_query])
    tq, vn, kw, X, mult = _exact_case(fmt, np.diff(t_off))
    p, r = ref.peaks(X, t_off, V_OFF)
    veto = int(_median_veto(p, role))
    score, cand, _ = ref.scores(p, r, t_off, role, veto)
    with_ban = [q for q in range(n_query) if (role[t_off[q]:t_off[q + 1]] < 0).any()]
    assert with_ban and all(cand[q].any() and not cand[q].all() for q in with_ban)
    t_dev, r_dev, v_dev = _dev(t_off), _dev(role), _dev(V_OFF)
    for k in (1, 10, 32):
        want_s, want_v = ref.topk(score, cand, k)
        for splits in SPLITS:
            top_s, top_v = ops.compound_topk(tq, vn, t_dev, r_dev, v_dev, k, veto=veto / mult, splits=splits, check_offsets=True, **kw)
            assert np.array_equal(top_v.cpu().numpy(), want_v), (k, splits)
            assert np.array_equal((top_s.double() * mult).cpu().numpy(), want_s), (k, splits)
    got_s, got_r = _peaks_all(tq, vn, kw, t_off, V_OFF)
    _check_peaks(got_s, got_r, p, r, t_off, scale=mult)


# ---------------------------------------------------------------------------------------------------------- 2. all-negative scores
@pytest.mark.parametrize("fmt", FORMATS)
def test_all_negative_scores(fmt):
    """Every video's last tile ends in zero-filled rows (1, 63, 65 and 129 rows), and 0 beats every real score: a tail row must be
    neither a peak nor a peak's row."""
    ops = _ops()
    lens = [1, 63, 65, 129]
    t_off, role = _tables([ONE, MIX, [0, 1, 1, -1, -1]])
    v_off = _s_off(lens)
    tq, vn, kw, X, mult = _exact(fmt, int(t_off[-1]), int(v_off[-1]), 1, negative=True)
    p, r = ref.peaks(X, t_off, v_off)
    assert (p < 0).all()
    got_s, got_r = _peaks_all(tq, vn, kw, t_off, v_off)
    _check_peaks(got_s, got_r, p, r, t_off, scale=mult)
    for veto in (INF, int(_median_veto(p, role))):
        score, cand, _ = ref.scores(p, r, t_off, role, veto)
        assert (score < 0).all() and (veto == INF or (cand.any() and not cand.all()))
        for k in (1, 4):
            want_s, want_v = ref.topk(score, cand, k)
            for splits in (0, 1, 2):
                top_s, top_v = ops.compound_topk(tq, vn, _dev(t_off), _dev(role), _dev(v_off), k, veto=veto / mult, splits=splits, **kw)
                assert np.array_equal(top_v.cpu().numpy(), want_v), (veto, k, splits)
                assert np.array_equal((top_s.double() * mult).cpu().numpy(), want_s), (veto, k, splits)


# --------------------------------------------------------------------------------------------------------------------- 3. ties
@pytest.mark.parametrize("fmt", FORMATS)
def test_ties_between_videos_rows_and_terms(fmt):
    """Two bit-identical videos rank by their number.  A video whose best row for a term stands at seconds 3 and 70 (its second
    tile) reports 3.  Two bit-identical terms in one clause peak alike, and the clause is worth what the first alone is worth."""
    ops = _ops()
    roles = [[0, 1, 1], [0], [2, 2, 0, 1, 1]]
    t_off, role = _tables(roles)
    fq, fv = _unit_rows(int(t_off[-1]), 31, torch.float32), _unit_rows(N, 32, torch.float32)
    fq[2] = fq[1]                                                   # query 0: the two terms of clause 1 are one row
    a, b = 159, 165                                                 # two of the 200-row videos, in different splits of 2 and 7
    assert LENS[a] == LENS[b] == 200
    fv[V_OFF[b]:V_OFF[b + 1]] = fv[V_OFF[a]:V_OFF[a + 1]]
    c = 6                                                           # the 129-row video
    assert LENS[c] == 129
    fv[V_OFF[c] + 3] = fq[3]
    fv[V_OFF[c] + 70] = fq[3]                                       # query 1's only term: its own row, twice
    tq, vn, kw, _, _ = _stored(fmt, fq, fv)
    t_dev, r_dev, v_dev = _dev(t_off), _dev(role), _dev(V_OFF)
    got_s, got_r = _peaks_all(tq, vn, kw, t_off, V_OFF)
    assert got_r[1, c, 0] == V_OFF[c] + 3 and got_s[1, c, 0] > 0.9
    assert np.array_equal(got_s[0, :, 1].view(np.int32), got_s[0, :, 2].view(np.int32)) and np.array_equal(got_r[0, :, 1], got_r[0, :, 2])
    assert np.array_equal(got_s[:, a].view(np.int32), got_s[:, b].view(np.int32))
    real = got_r[:, a] != ref.SENT                                  # the terms' columns; the filler is no row
    assert np.array_equal(real, got_r[:, b] != ref.SENT) and real.sum() == t_off[-1]
    assert np.array_equal(got_r[:, a][real] - V_OFF[a], got_r[:, b][real] - V_OFF[b])
    # the reference over the kernel's own peaks: the whole ranking, the identical pair adjacent and in order
    p = np.concatenate([got_s[q, :, :len(rl)].T for q, rl in enumerate(roles)])
    r = np.concatenate([got_r[q, :, :len(rl)].T for q, rl in enumerate(roles)]).astype(np.int64)
    score, cand, _ = ref.scores(p, r, t_off, role, INF)
    order = ref.topk(score, cand, NV)[1]
    for q in range(3):
        ia, ib = list(order[q]).index(a), list(order[q]).index(b)
        assert ib == ia + 1 and score[q, a].view(np.int32) == score[q, b].view(np.int32), q
    want_s, want_v = ref.topk(score, cand, 32)
    for splits in SPLITS:
        top_s, top_v = ops.compound_topk(tq, vn, t_dev, r_dev, v_dev, 32, splits=splits, **kw)
        assert np.array_equal(top_v.cpu().numpy(), want_v) and np.array_equal(_i32(top_s), want_s.view(np.int32)), splits
        assert top_v[1, 0].item() == c, splits
    # query 0 without its duplicated term gives query 0's list
    keep = torch.tensor([0, 1], device="cuda")
    one_kw = dict(q_scale=kw["q_scale"][keep].contiguous(), v_scale=kw["v_scale"]) if kw else {}
    one_s, one_v = ops.compound_topk(tq[keep].contiguous(), vn, _dev([0, 2]), _dev([0, 1]), v_dev, 32, **one_kw)
    assert torch.equal(one_s[0], top_s[0]) and torch.equal(one_v[0], top_v[0])
    # an index of the identical pair alone: both are in the lists, the lower number first
    pair_rows = torch.cat((torch.arange(V_OFF[b], V_OFF[b + 1]), torch.arange(V_OFF[a], V_OFF[a + 1]))).cuda()
    pkw = dict(q_scale=kw["q_scale"], v_scale=kw["v_scale"][pair_rows].contiguous()) if kw else {}
    for splits in SPLITS:
        top_s, top_v = ops.compound_topk(tq, vn[pair_rows].contiguous(), t_dev, r_dev, _dev([0, 200, 400]), 2, splits=splits, **pkw)
        assert top_v.tolist() == [[0, 1]] * 3 and torch.equal(top_s[:, 0], top_s[:, 1]), splits


# --------------------------------------------------------------------------------------------------------------------- 4. veto
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_veto_is_met_with_equality_and_leaves_short_and_empty_lists(fmt):
    ops = _ops()
    roles = [[0, 1, -1], [-1, 3]]
    t_off, role = _tables(roles)
    tq, vn, kw, _, _ = _unit_case(fmt, np.diff(t_off), seed=11)
    t_dev, r_dev, v_dev = _dev(t_off), _dev(role), _dev(V_OFF)
    got_s, got_r = _peaks_all(tq, vn, kw, t_off, V_OFF)
    p = np.concatenate([got_s[q, :, :len(rl)].T for q, rl in enumerate(roles)])
    r = np.concatenate([got_r[q, :, :len(rl)].T for q, rl in enumerate(roles)]).astype(np.int64)
    # v0: query 0's best video among those whose banned peak is at most the median one; its banned peak is the veto.  With the veto
    # one ulp higher v0 is a candidate again, and the best of them
    free = ref.scores(p, r, t_off, role, INF)[0]
    v0 = int(ref.topk(free[:1], (p[2] <= np.median(p[2]))[None], 1)[1][0, 0])
    at = p[2, v0]
    above = np.nextafter(at, np.float32(INF))
    for veto, inside in ((at, False), (above, True)):
        score, cand, _ = ref.scores(p, r, t_off, role, veto)
        assert cand[0, v0] == inside and cand[0].any() and not cand[0].all()           # some videos are out, some are in, either way
        want_s, want_v = ref.topk(score, cand, 10)
        assert (want_v[0, 0] == v0) == inside
        for splits in SPLITS:
            top_s, top_v = ops.compound_topk(tq, vn, t_dev, r_dev, v_dev, 10, veto=float(veto), splits=splits, **kw)
            assert np.array_equal(top_v.cpu().numpy(), want_v) and np.array_equal(_i32(top_s), want_s.view(np.int32)), (inside, splits)
    # fewer than k candidates: short lists with the defined tail
    low = np.sort(np.minimum(p[2], p[3]))[19]                       # at most 19 videos stay below it for either query
    score, cand, _ = ref.scores(p, r, t_off, role, low)
    assert (cand.sum(1) < 32).all() and cand.any()
    want_s, want_v = ref.topk(score, cand, 32)
    assert (want_v == ref.SENT).any() and (want_v != ref.SENT).any()
    for splits in SPLITS:
        top_s, top_v = ops.compound_topk(tq, vn, t_dev, r_dev, v_dev, 32, veto=float(low), splits=splits, **kw)
        assert np.array_equal(top_v.cpu().numpy(), want_v) and np.array_equal(_i32(top_s), want_s.view(np.int32)), splits
    # every video vetoed: all-empty lists
    floor = float(min(p[2].min(), p[3].min()))
    assert not ref.scores(p, r, t_off, role, floor)[1].any()
    for veto in (floor, -INF):
        for splits in SPLITS:
            top_s, top_v = ops.compound_topk(tq, vn, t_dev, r_dev, v_dev, 5, veto=veto, splits=splits, **kw)
            assert bool(torch.isneginf(top_s).all()) and bool((top_v == ref.SENT).all()), (veto, splits)


# --------------------------------------------------------------------------------- 5. one term, one clause: the existing video sweep
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_term_queries_equal_rank_topk_video(fmt):
    ops = _ops()
    Q = 9
    tq, vn, kw, _, _ = _unit_case(fmt, [1] * Q, seed=3)
    t_off = np.arange(Q + 1, dtype=np.int64)
    role = _dev(np.array([0, 31, 5, 0, 1, 2, 3, 4, 30]))
    for k in (1, 10, 32):
        row_s, row_r, row_v = ops.rank_topk_video(tq, vn, _dev(V_OFF), k, **kw)
        for splits in SPLITS:
            top_s, top_v = ops.compound_topk(tq, vn, _dev(t_off), role, _dev(V_OFF), k, splits=splits, **kw)
            assert torch.equal(top_s, row_s) and torch.equal(top_v, row_v), (k, splits)
        hits = torch.stack((torch.arange(Q, device="cuda", dtype=torch.int32).repeat_interleave(k), row_v.reshape(-1)), 1).contiguous()
        ps, pr = ops.compound_peaks(tq, vn, _dev(t_off), _dev(V_OFF), hits, **kw)
        assert torch.equal(ps[:, 0].view(Q, k), row_s) and torch.equal(pr[:, 0].view(Q, k), row_r), k


# ------------------------------------------------------------------------------------------------------- 6. random unit rows
@pytest.mark.parametrize("fmt", FORMATS)
def test_compound_topk_random_unit_rows(fmt):
    ops = _ops()
    roles = ROLES[5]
    t_off, role = _tables(roles)
    ms = np.diff(t_off)
    tq, vn, kw, S, _ = _unit_case(fmt, ms)
    if fmt == "e4m3":
        a, b = _deq(tq, kw["q_scale"]), _deq(vn, kw["v_scale"])
        eps = (ACC_EPS * (a.abs() @ b.abs().T)).cpu().numpy()       # per score
    else:
        eps = np.full(tuple(S.shape), EPS)
    S = S.cpu().numpy()
    hits = _all_pairs(len(ms), NV)
    x, hm, hv, x_off = _scores(tq, vn, kw, t_off, V_OFF, hits)      # existing code: the device's own scores for all pairs
    xs = x.cpu().numpy()
    X = np.empty((int(t_off[-1]), N), dtype=np.float32)
    for h, (q, v) in enumerate(hits):
        X[t_off[q]:t_off[q + 1], V_OFF[v]:V_OFF[v + 1]] = xs[x_off[h]:x_off[h] + hm[h] * hv[h]].reshape(hm[h], hv[h])
    assert (np.abs(X - S) <= eps).all()
    p, r = ref.peaks(X, t_off, V_OFF)
    got_s, got_r = _peaks_all(tq, vn, kw, t_off, V_OFF)
    _check_peaks(got_s, got_r, p, r, t_off)
    t_dev, r_dev, v_dev = _dev(t_off), _dev(role), _dev(V_OFF)
    for veto in (INF, float(_median_veto(p, role))):
        score, cand, _ = ref.scores(p, r, t_off, role, veto)
        assert veto == INF or (cand.any() and not cand.all())
        for k in (1, 10, 32):
            want_s, want_v = ref.topk(score, cand, k)
            for splits in SPLITS:
                top_s, top_v = ops.compound_topk(tq, vn, t_dev, r_dev, v_dev, k, veto=veto, splits=splits, **kw)
                assert np.array_equal(top_v.cpu().numpy(), want_v), (veto, k, splits)
                assert np.array_equal(_i32(top_s), want_s.view(np.int32)), (veto, k, splits)
    # against fp64 over the stored operands: min over clauses of max over the clause's terms and the video's rows
    worst = 0.0
    for q, rl in enumerate(roles):
        rl = np.asarray(rl)
        for v in range(NV):
            blk = S[t_off[q]:t_off[q + 1], V_OFF[v]:V_OFF[v + 1]]
            want = min(blk[rl == j].max() for j in set(rl[rl >= 0].tolist()))
            err = abs(float(score[q, v]) - want)
            worst = max(worst, err)
            assert err <= eps[t_off[q]:t_off[q + 1], V_OFF[v]:V_OFF[v + 1]].max(), (q, v, err)
    print(f"compound_topk {fmt}: largest |score - fp64 min of max| = {worst:.3e} (bound {float(eps.max()):.3e})")


# ------------------------------------------------------------------------------------------- 7. determinism and write discipline
@pytest.mark.parametrize("fmt", FORMATS)
def test_compound_entry_points_are_deterministic_and_write_nothing_else(fmt):
    ops = _ops()
    G = 64
    for roles, k in ((ROLES[5], 10), (ROLES[1], 32), (ROLES[4], 1)):
        t_off, role = _tables(roles)
        nq = len(roles)
        tq, vn, kw, _, _ = _unit_case(fmt, np.diff(t_off), seed=20)
        t_dev, r_dev, v_dev = _dev(t_off), _dev(role), _dev(V_OFF)
        veto = 0.08                                                 # random unit rows in 512 dimensions: a peak over a video's rows is near it
        ref_out = ops.compound_topk(tq, vn, t_dev, r_dev, v_dev, k, veto=veto, check_offsets=True, **kw)
        top_s = torch.full((nq * k + G,), float("nan"), device="cuda")
        top_v = torch.full((nq * k + G,), -777, dtype=torch.int32, device="cuda")
        nws = ops.compound_topk_ws_bytes(nq, N, k)
        ws = torch.full((nws + G,), 0xFF, dtype=torch.uint8, device="cuda")
        out = (top_s[:nq * k].view(nq, k), top_v[:nq * k].view(nq, k))
        for splits in SPLITS + SPLITS + (5, 43, 256, 1000):
            out[0].fill_(float("nan"))
            out[1].fill_(-777)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ops.compound_topk(tq, vn, t_dev, r_dev, v_dev, k, veto=veto, splits=splits, out=out, ws=ws[:nws], **kw)
            torch.cuda.synchronize()
            assert torch.cuda.max_memory_allocated() == base, (k, splits)
            assert torch.equal(out[0], ref_out[0]) and torch.equal(out[1], ref_out[1]), (k, splits)
            assert (ws[nws:] == 0xFF).all() and torch.isnan(top_s[nq * k:]).all() and (top_v[nq * k:] == -777).all()
        real = out[1] != ref.SENT
        assert bool(real.any()) and torch.isfinite(out[0][real]).all() and ((out[1][real] >= 0) & (out[1][real] < NV)).all()
        assert bool(torch.isneginf(out[0][~real]).all())
        assert all(len(set(v)) == len(v) for v in ([x for x in row if x != ref.SENT] for row in out[1].tolist()))
        # the peaks of every listed (query, video), guard elements around both outputs
        qs, slot = torch.nonzero(real, as_tuple=True)
        hits = torch.stack((qs.int(), out[1][qs, slot]), 1).contiguous()
        P = hits.shape[0]
        runs = []
        for dirty in (0x7fc00001, -559038737):                      # a NaN pattern, then another: the outputs start dirty
            bufs = [torch.full((G + P * 32 + G,), dirty, dtype=torch.int32, device="cuda") for _ in range(2)]
            po = (bufs[0][G:-G].view(torch.float32).view(P, 32), bufs[1][G:-G].view(P, 32))
            got = ops.compound_peaks(tq, vn, t_dev, v_dev, hits, out=po, **kw)
            assert got[0] is po[0] and got[1] is po[1]
            torch.cuda.synchronize()
            assert all(bool((buf[:G] == dirty).all()) and bool((buf[-G:] == dirty).all()) for buf in bufs)
            runs.append([buf[G:-G].clone() for buf in bufs])
        assert all(torch.equal(x, y) for x, y in zip(*runs))
        ps, pr = runs[0][0].view(torch.float32).view(P, 32).cpu().numpy(), runs[0][1].view(P, 32).cpu().numpy()
        first, last = V_OFF[hits[:, 1].cpu().numpy()], V_OFF[hits[:, 1].cpu().numpy() + 1]
        for h, q in enumerate(qs.tolist()):
            m, rl = len(roles[q]), np.asarray(roles[q])
            assert np.isneginf(ps[h, m:]).all() and (pr[h, m:] == ref.SENT).all()             # columns >= m: the defined filler
            assert np.isfinite(ps[h, :m]).all() and ((pr[h, :m] >= first[h]) & (pr[h, :m] < last[h])).all()
            # the listed score is the weakest clause of exactly these peaks, and no banned peak reaches the veto
            want = min(max(ps[h, :m][rl == j]) for j in set(rl[rl >= 0].tolist()))
            assert np.float32(want).view(np.int32) == out[0][q, slot[h]].cpu().numpy().view(np.int32)
            assert (ps[h, :m][rl < 0] < veto).all()


# --------------------------------------------------------------------------------------------------------- 8. invalid arguments
def test_compound_entry_points_reject_invalid_arguments():
    ops = _ops()
    L = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                     # noqa: E731
    roles, k = [[0, 1, -1], [4], [0, 0, -1, 2]], 3
    Qt, Nn = 8, 40
    t_off, role = (_dev(x) for x in _tables(roles))
    v_off = _dev([0, 10, 11, 25, 40])
    f32 = (_unit_rows(Qt, 1, torch.float32), _unit_rows(Nn, 2, torch.float32))
    (q8, qs), (v8, vs) = ops.quantize_rows_e4m3(f32[0]), ops.quantize_rows_e4m3(f32[1])
    ts, tv = torch.empty(3, k, device="cuda"), torch.empty(3, k, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.compound_topk_ws_bytes(3, Nn, k), dtype=torch.uint8, device="cuda")
    hits = _dev([[0, 0], [1, 3], [2, 2]])
    ps, pr = torch.empty(3, 32, device="cuda"), torch.empty(3, 32, dtype=torch.int32, device="cuda")

    def topk(e4m3=False, dtype=0, Qt=Qt, N=Nn, Cc=512, to=t_off, ro=role, nq=3, vo=v_off, nv=4, veto=0.5, k=k, splits=0, s=ts, v=tv,
             w=ws, sa=qs, sb=vs):
        a, b = (q8, v8) if e4m3 else f32
        tail = (Qt, N, Cc, p(to), p(ro), nq, p(vo), nv, veto, k, splits, p(s), p(v), p(w), None)
        if e4m3:
            return L.tan_compound_topk_e4m3(p(a), p(sa), p(b), p(sb), *tail)
        return L.tan_compound_topk(p(a), p(b), dtype, *tail)

    def peaks(e4m3=False, dtype=0, Qt=Qt, N=Nn, Cc=512, to=t_off, nq=3, vo=v_off, nv=4, h=hits, P=3, s=ps, r=pr, sa=qs, sb=vs):
        a, b = (q8, v8) if e4m3 else f32
        tail = (Qt, N, Cc, p(to), nq, p(vo), nv, p(h), P, p(s), p(r), None)
        if e4m3:
            return L.tan_compound_peaks_e4m3(p(a), p(sa), p(b), p(sb), *tail)
        return L.tan_compound_peaks(p(a), p(b), dtype, *tail)

    class Null:                                                                       # a NULL pointer for one argument
        @staticmethod
        def data_ptr():
            return None
    null = Null()
    sizes = (dict(Cc=256), dict(Cc=1024), dict(nq=0), dict(Qt=2), dict(Qt=97), dict(nv=0), dict(nv=41), dict(nv=-1), dict(N=0),
             dict(N=1 << 31), dict(to=null), dict(vo=null))
    for e4m3 in (False, True):
        assert topk(e4m3) == 0 and peaks(e4m3) == 0
        torch.cuda.synchronize()
        for kw in sizes + (dict(k=0), dict(k=33), dict(k=5), dict(k=-1), dict(splits=-1), dict(veto=float("nan")), dict(ro=null),
                           dict(s=null), dict(v=null), dict(w=null)):
            assert topk(e4m3, **kw) == -1, (e4m3, kw)
        for kw in sizes + (dict(P=0), dict(P=-1), dict(h=null), dict(s=null), dict(r=null)):
            assert peaks(e4m3, **kw) == -1, (e4m3, kw)
    assert topk(dtype=2) == -1 and peaks(dtype=2) == -1
    for kw in (dict(sa=null), dict(sb=null)):
        assert topk(True, **kw) == -1 and peaks(True, **kw) == -1
    # hits outside the tables: their 32 columns hold the filler, nothing else is written
    ps.fill_(-5.0)
    pr.fill_(-5)
    assert peaks(h=_dev([[-1, 0], [3, 1], [0, 1 << 30]])) == 0
    torch.cuda.synchronize()
    assert bool(torch.isneginf(ps).all()) and bool((pr == ref.SENT).all())

    with pytest.raises(_lib.TanHipError):
        ops.compound_topk(f32[0].cpu(), f32[1].cpu(), t_off.cpu(), role.cpu(), v_off.cpu(), k)
    with pytest.raises(_lib.TanHipError):
        ops.compound_topk(*f32, t_off, role, v_off, 5)                                # k > n_videos
    with pytest.raises(TypeError):
        ops.compound_topk(*f32, t_off, role, v_off, k, q_scale=qs, v_scale=vs)
    with pytest.raises(ValueError):
        ops.compound_topk(*f32, t_off, role, v_off, k, veto=float("nan"))
    for bad in ([0, 10, 10, 25, 40], [0, 10, 9, 25, 40], [0, 10, 11, 25, 39], [1, 10, 11, 25, 40]):
        with pytest.raises(ValueError):
            ops.compound_topk(*f32, t_off, role, _dev(bad), k, check_offsets=True)
        ops.compound_topk(*f32, t_off, role, _dev(bad), k)                            # unchecked: the caller's error, but memory-safe
        ops.compound_peaks(*f32, t_off, _dev(bad), hits)
    for bad in ([0, 3, 3, 8], [0, 5, 4, 8], [0, 3, 4, 7], [1, 3, 4, 8]):
        with pytest.raises(ValueError):
            ops.compound_topk(*f32, _dev(bad), role, v_off, k, check_offsets=True)
        with pytest.raises(ValueError):
            ops.compound_peaks(*f32, _dev(bad), v_off, hits, check_offsets=True)
        ops.compound_topk(*f32, _dev(bad), role, v_off, k)
        ops.compound_peaks(*f32, _dev(bad), v_off, hits)
    for bad in ([0, 1, -1, 4, 0, 0, -1, 32], [0, 1, -2, 4, 0, 0, -1, 2], [0, 1, -1, -1, 0, 0, -1, 2], [-1, -1, -1, 4, 0, 0, -1, 2]):
        with pytest.raises(ValueError):
            ops.compound_topk(*f32, t_off, _dev(bad), v_off, k, check_offsets=True)   # a role out of range; a query without a clause
        ops.compound_topk(*f32, t_off, _dev(bad), v_off, k)
    # a query without a clause term has no candidate
    top_s, top_v = ops.compound_topk(*f32, t_off, _dev([-1, -1, -1, 4, 0, 0, -1, 2]), v_off, k)
    assert bool(torch.isneginf(top_s[0]).all()) and bool((top_v[0] == ref.SENT).all()) and bool((top_v[1] != ref.SENT).all())
    wide = _unit_rows(40, 5, torch.float32)
    with pytest.raises(ValueError):
        ops.compound_topk(wide, f32[1], _dev([0, 33, 40]), _dev([0] * 40), v_off, k, check_offsets=True)        # 33 terms
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- 9. end to end
def _dual_basis(F):
    """rows u_i with <F[j], u_i> = 1 if i == j else 0 (fp64)"""
    return torch.linalg.pinv(F.double()).T.contiguous()


@pytest.mark.parametrize("fmt", FORMATS)
def test_search_compound_end_to_end(fmt, tmp_path, capsys, monkeypatch):
    """Sentences 0 and 1 are the steps, sentence 2 the banned one, sentence 3 a paraphrase that no video shows.  Video A (number 2) shows step 1 and later step 0 -- the reverse
    order -- with strengths 12 and 8; video B (0) shows step 0 alone at 16; video C (3) shows steps 0 and 1 at 24 and 20, and the
    banned sentence at 8.  The planted rows are multiples of the sentences' dual basis: a sentence scores the strength on its own row
    and 0 on the others' (before the format's rounding), and at most 1 in absolute value on any unplanted row (an index row is a
    mean of unit vectors).  So A scores about 8 by clause 0, B at most 1 by clause 1 (the missing step), C about 20 by clause 1,
    and with a veto of 4 C is out: every other video's banned peak is at most 1."""
    import itertools
    from temporalalignnet_amd import search as srch
    from temporalalignnet_amd.search import cli
    m = _model()
    vids = _videos([70, 33, 150, 64, 20], seed=9)
    f32 = srch.build_index(m, vids, dtype=torch.float32)
    pool = [f"step {i}" for i in range(10)]
    fpool = srch.query_features(f32, m, _embed, pool)
    pick = min(itertools.combinations(range(10), 4), key=lambda c: float(_dual_basis(fpool[list(c)]).norm(dim=1).max()))
    s0, s1, ban, alt = (pool[i] for i in pick)
    U = _dual_basis(fpool[list(pick)]).float()
    off = [int(x) for x in f32.v_off]
    assert (f32.feat.norm(dim=1) <= 1 + 1e-5).all()
    A, B, Cv = 2, 0, 3
    f32.feat[off[A] + 10] = 12.0 * U[1]
    f32.feat[off[A] + 100] = 8.0 * U[0]                             # in A's second tile, after step 1
    f32.feat[off[B] + 5] = 16.0 * U[0]
    f32.feat[off[Cv] + 7] = 24.0 * U[0]
    f32.feat[off[Cv] + 50] = 20.0 * U[1]
    f32.feat[off[Cv] + 20] = 8.0 * U[2]
    idx = f32 if fmt == "f32" else (f32.quantize() if fmt == "e4m3" else srch.VideoIndex(f32.feat.bfloat16(), f32.v_off, f32.vids))
    Cq = srch.Compound
    queries = [Cq([s0, s1], [ban]), Cq([s1, [s0, alt]], [ban]), Cq([[s0, s1]], [ban])]
    before = srch.search_moments(idx, m, _embed, [s0], k=3)
    res = srch.search_compound(idx, m, _embed, queries, k=5, veto=4.0)
    assert srch.search_moments(idx, m, _embed, [s0], k=3) == before
    assert all(isinstance(h, srch.CompoundHit) for hits in res for h in hits)
    vid = idx.vids
    for hits, mm in zip(res, (3, 4, 3)):
        assert [h.vid for h in hits].count(vid[Cv]) == 0 and len(hits) == 4 and len({h.vid for h in hits}) == 4      # C is vetoed
        assert [h.score for h in hits] == sorted((h.score for h in hits), reverse=True)
        for h in hits:
            v = vid.index(h.vid)
            assert len(h.seconds) == len(h.scores) == mm and all(0 <= t < off[v + 1] - off[v] for t in h.seconds)
            assert h.scores[-1] < 4.0                               # the banned sentence's peak: below the veto
    top, by_vid = res[0][0], {h.vid: h for h in res[0]}
    assert top.vid == vid[A] and top.seconds[:2] == (100, 10) and top.weakest == 0 and top.score == top.scores[0]
    assert abs(top.score - 8.0) <= 0.4 and abs(top.scores[1] - 12.0) <= 0.6
    hb = by_vid[vid[B]]
    assert hb.score < 1.01 < top.score and hb.weakest == 1 and hb.seconds[0] == 5 and abs(hb.scores[0] - 16.0) <= 0.8
    assert hb.score == hb.scores[1]
    # the clauses swapped, step 0 with the paraphrase as its alternative: the same videos, weakest by position in `all`
    top = res[1][0]
    assert top.vid == vid[A] and top.seconds[:2] == (10, 100) and top.weakest == 1 and top.score == res[0][0].score
    assert top.score == max(top.scores[1], top.scores[2])
    # one clause of both steps (OR): B's single step is enough, and it is the strongest of the videos left
    assert res[2][0].vid == vid[B] and res[2][0].weakest == 0 and res[2][0].score == res[2][0].scores[0]
    assert res[2][1].vid == vid[A] and res[2][1].score == res[2][1].scores[1]
    # without the veto C is first, by its weaker step
    free = srch.search_compound(idx, m, _embed, [Cq([s0, s1])], k=5)
    assert [h.vid for h in free[0][:2]] == [vid[Cv], vid[A]] and len(free[0]) == 5
    assert free[0][0].seconds == (7, 50) and free[0][0].weakest == 1 and abs(free[0][0].score - 20.0) <= 1.0
    assert [(h.vid, h.score, h.seconds, h.scores) for h in free[0] if h.vid != vid[Cv]] == \
        [(h.vid, h.score, h.seconds[:2], h.scores[:2]) for h in res[0]]
    loose = srch.search_compound(idx, m, _embed, queries[:1], k=5, veto=1000.0)
    assert loose[0][0].vid == vid[Cv] and loose[0][0].seconds == (7, 50, 20) and abs(loose[0][0].scores[2] - 8.0) <= 0.4
    # saved and loaded, k clamped, every split count
    path = str(tmp_path / "index.npz")
    idx.save(path)
    assert srch.search_compound(srch.VideoIndex.load(path), m, _embed, queries, k=5, veto=4.0) == res
    assert srch.search_compound(idx, m, _embed, queries, k=50, veto=4.0) == res
    assert [hits[:2] for hits in res] == srch.search_compound(idx, m, _embed, queries, k=2, veto=4.0)
    for splits in (1, 2, 7):
        assert srch.search_compound(idx, m, _embed, queries, k=5, veto=4.0, splits=splits) == res
    # three shards, device- and host-resident: the concatenated index's answer
    parts = []
    for a, b in ((0, 2), (2, 4), (4, 5)):
        r0, r1 = off[a], off[b]
        parts.append(srch.VideoIndex(idx.feat[r0:r1].contiguous(), idx.v_off[a:b + 1] - r0, idx.vids[a:b],
                                     None if idx.scale is None else idx.scale[r0:r1].contiguous()))
    for sharded in (srch.ShardedIndex(parts, resident="device"), srch.ShardedIndex(_pinned(parts), resident="host")):
        assert srch.search_compound(sharded, m, _embed, queries, k=5, veto=4.0) == res
        assert srch.search_compound(sharded, m, _embed, [Cq([s0, s1])], k=5) == free
        assert srch.search_compound(sharded, m, _embed, queries, k=2, veto=4.0) == [hits[:2] for hits in res]
    # the command line prints the same hits
    monkeypatch.setattr(cli, "_load_searcher", lambda a: (m, _embed, idx))
    capsys.readouterr()
    argv = ["query", "--checkpoint", "c", "--vocab", "v", "--index", path, "-k", "5", "--all", s1, f"{s0}|{alt}", "--none", ban,
            "--veto", "4"]
    assert srch.main(argv) == 0
    lines = [ln.split("\t") for ln in capsys.readouterr().out.splitlines()]
    assert len(lines) == 4
    for ln, h in zip(lines, res[1]):
        assert ln[0] == h.vid and float(ln[1]) == round(h.score, 6)
        assert ln[2:] == [f"{t}:{s:.6f}" for t, s in zip(h.seconds, h.scores)]
    with pytest.raises(ValueError):
        srch.search_compound(idx, m, _embed, queries, k=5)          # `none` without veto
    with pytest.raises(ValueError):
        srch.search_compound(idx, m, _embed, [Cq([s0, []])], k=5)
