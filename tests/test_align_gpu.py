"""Copy alignment on the GPU: tan_local_align (the best local alignment of every [m, V] block of scores, with its extent in both
videos), `ops.local_align`, `search.align_spans` / `search_copies` / the `similar --align` command.  The recurrence and its tie rules
are restated in numpy in align_ref.py (pinned against a loop over Python ints by test_align_cpu.py).

  * shapes: the kernel walks strips of S = 64 query seconds and stages the scores in slabs of W = 64 video seconds, four blocks per
    workgroup: m in 1, 2, S - 1, S, S + 1, 2 S + 1 times V in 1, 2, W - 1, W, W + 1, 2 W + 1, 200, in launches of 1, 4, 5 and all 42.
  * exact arithmetic: blocks of multiples of 1/16 in [-1/2, 1], theta and skew multiples of 1/16: every H is a multiple of 1/16 of at
    most m + V < 2^9, exact in f32, and (score * 16, span) equal the int64 reference with `==`.
  * random unit rows: x from `ops.sequence_scores`, the queries cut into 32-row pieces; align_ref in float32 over THOSE device bits
    reproduces score (as int32 bits) and span with `==`.  The score is also held against the fp64 recurrence over the fp64 scores of
    the stored rows: a path has at most m + V - 1 cells, each one score within the project's bound (EPS = 2e-5 for f32 / bf16,
    ACC_EPS * max sum |a b| for e4m3) plus three roundings of values of at most 2 (m + V), and a maximum over paths is 1-Lipschitz:
    (m + V) * (EPS + 2^-24 * (2 + 4 (m + V))).  Spans are not compared against fp64 (an argmax may flip).
Largest observed errors are recorded in DESIGN.md 3.21."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import align_ref as ref
import clip_ref
from temporalalignnet_amd import _lib
from test_moments_gpu import FORMATS, _dev, _ops, _stored
from test_retrieve_fp8_gpu import ACC_EPS, _deq
from test_retrieve_gpu import EPS, _unit_rows
from test_shards_gpu import _pinned

pytestmark = pytest.mark.gpu

S, W, WAVES = 64, 64, 4                                             # strip height, slab width, blocks per workgroup (csrc/tan_align.hip)
MS = (1, 2, S - 1, S, S + 1, 2 * S + 1)
VS = (1, 2, W - 1, W, W + 1, 2 * W + 1, 200)
ALL = tuple(itertools.product(MS, VS))
LAUNCHES = {1: ((129, 200),), 4: ((129, 200), (1, 1), (65, 129), (64, 64)), 5: ((2, 200), (129, 1), (63, 65), (65, 63), (129, 129)), 42: ALL}
PRICES = ((0.25, 0.0), (0.5, 0.125), (0.4375, 0.5))                 # (theta, skew), multiples of 1/16; skew = 0 included
EMPTY = (0.0,) + ref.EMPTY


def _srch():
    from temporalalignnet_amd import search
    return search


def test_the_shapes_hold_the_edges_they_claim():
    assert (S, W) == (64, 64) and set(MS) == {1, 2, 63, 64, 65, 129} and set(VS) == {1, 2, 63, 64, 65, 129, 200}
    assert len(ALL) == 42 and all(set(blocks) <= set(ALL) for blocks in LAUNCHES.values())
    assert sorted(LAUNCHES) == [1, 4, 5, 42] and all(len(b) == P for P, b in LAUNCHES.items())
    assert 1 < WAVES == 4 and 5 % WAVES == 1 and 42 % WAVES == 2     # a workgroup is partly filled, and one is crossed
    assert any(m > 2 * S for m, _ in ALL) and any(V > 3 * W for _, V in ALL)      # three strips; a fourth, partial slab
    assert any(0.0 == skew for _, skew in PRICES)


# ----------------------------------------------------------------------------------------------------------------------- launching
def _tables(shapes):
    ms, vs = np.array([m for m, _ in shapes], dtype=np.int64), np.array([V for _, V in shapes], dtype=np.int64)
    x_off = np.concatenate([[0], np.cumsum(ms * vs)])
    slot = np.concatenate([[0], np.cumsum(vs)])
    return x_off, np.stack((ms, vs, slot[:-1]), 1), int(slot[-1])


def _align(blocks, theta, skew):
    """blocks: f32 arrays [m, V] (host) -> [(score, a_first, a_last, b_first, b_last, cells)] from one launch"""
    x_off, table, sum_V = _tables([b.shape for b in blocks])
    x = torch.from_numpy(np.concatenate([b.reshape(-1) for b in blocks]).astype(np.float32)).cuda()
    score, span = _ops().local_align(x, torch.from_numpy(x_off[:-1].copy()).cuda(), _dev(table), theta, skew, sum_V=sum_V)
    return [(float(s),) + tuple(int(v) for v in sp) for s, sp in zip(score.cpu().numpy(), span.cpu().numpy())]


@functools.lru_cache(maxsize=None)
def _exact_blocks():
    rng = np.random.default_rng(11)
    return {mv: rng.integers(-8, 17, mv) for mv in ALL}             # sixteenths, int64


@functools.lru_cache(maxsize=None)
def _exact_want(theta16, skew16):
    out = {}
    for mv, xi in _exact_blocks().items():
        score, span = ref.align(xi, theta16, skew16)
        out[mv] = (float(score),) + span
    return out


# ------------------------------------------------------------------------------------------------------------- 1. exact arithmetic
@pytest.mark.parametrize("prices", PRICES)
@pytest.mark.parametrize("P", sorted(LAUNCHES))
def test_local_align_exact_arithmetic(P, prices):
    theta, skew = prices
    want = _exact_want(int(theta * 16), int(skew * 16))
    shapes = LAUNCHES[P]
    got = _align([(_exact_blocks()[mv] / 16.0).astype(np.float32) for mv in shapes], theta, skew)
    assert any(w[0] > 0 and w[5] > max(w[2] - w[1], w[4] - w[3]) + 1 for w in want.values())      # paths with steps along one axis
    for mv, g in zip(shapes, got):
        assert (g[0] * 16,) + g[1:] == want[mv], (mv, prices, g, want[mv])


# --------------------------------------------------------------------------------------------------------------------- 2. ties
def test_a_constant_block_is_a_diagonal_from_the_corner():
    """gain 1/2 per cell, skew 1/2: diag >= up, left everywhere, so diag always wins; H[i][j] = (min(i, j) + 1) / 2 and the first
    cell attaining the maximum is (n - 1, n - 1), n = min(m, V)."""
    shapes = ((70, 130), (130, 70), (64, 64), (1, 5), (129, 129))
    got = _align([np.ones(mv, dtype=np.float32) for mv in shapes], 0.5, 0.5)
    for (m, V), g in zip(shapes, got):
        n = min(m, V)
        assert g == (n / 2.0, 0, n - 1, 0, n - 1, n), ((m, V), g)


def _runs(m, V, runs, length=10):
    x = np.full((m, V), -1.0, dtype=np.float32)
    for a, b in runs:
        for t in range(length):
            x[a + t, b + t] = 1.0
    return x


def test_of_two_equal_runs_the_first_end_wins():
    """The same diagonal run of 10 cells twice in one block: equal scores, and the end with the smallest i, then the smallest j,
    is reported -- across a slab edge and inside a slab, across a strip edge, in the same rows, and found by a later lane."""
    cases = [((100, 200), ((5, 60), (20, 80)), (5, 14, 60, 69)),     # across the slab edge at 64 first, inside a slab second
             ((100, 200), ((5, 80), (20, 60)), (5, 14, 80, 89)),     # the smaller i wins although its columns come later
             ((100, 200), ((60, 10), (70, 30)), (60, 69, 10, 19)),   # across the strip edge at 64
             ((100, 200), ((70, 10), (60, 30)), (60, 69, 30, 39)),
             ((100, 200), ((5, 10), (5, 120)), (5, 14, 10, 19)),     # the same rows: the smaller j
             ((140, 70), ((3, 3), (67, 5)), (3, 12, 3, 12)),         # the same lanes, one strip apart: the earlier strip
             ((140, 70), ((70, 3), (3, 50)), (3, 12, 50, 59))]
    got = _align([_runs(m, V, runs) for (m, V), runs, _ in cases], 0.5, 0.25)
    for (mv, runs, want), g in zip(cases, got):
        assert g == (5.0,) + want + (10,), (mv, runs, g)
        xi = (_runs(*mv, runs) * 16).astype(np.int64)
        assert ref.align(xi, 8, 4) == (80, want + (10,))


def test_nothing_above_the_threshold_gives_the_empty_result():
    blocks = [np.full(mv, 0.25, dtype=np.float32) for mv in ((1, 1), (65, 129), (129, 3))] + [_runs(70, 70, ((0, 0),))]
    got = _align(blocks, 0.25, 0.0)                                 # a gain of exactly 0 is not positive
    assert got[:3] == [EMPTY] * 3 and got[3] == (7.5, 0, 9, 0, 9, 10)
    assert _align(blocks[:3], 1.0, 0.125) == [EMPTY] * 3


# ------------------------------------------------------------------------------------------------------- 3. random unit rows
THETA, SKEW = 0.02, 0.01                                            # random unit rows score about +-0.044: many positive cells, long paths


@pytest.mark.parametrize("fmt", FORMATS)
def test_local_align_random_unit_rows(fmt):
    ops, srch = _ops(), _srch()
    v_off = np.concatenate([[0], np.cumsum(VS)]).astype(np.int64)
    tq, vn, kw, S64, _ = _stored(fmt, _unit_rows(int(sum(MS)), 901, torch.float32), _unit_rows(int(v_off[-1]), 902, torch.float32))
    s_off, first = srch.piece_offsets(MS)
    assert (np.diff(s_off) <= 32).all() and len(s_off) - 1 == sum((m + 31) // 32 for m in MS)
    pairs = [(q, v) for q in range(len(MS)) for v in range(len(VS))]
    hits, hit_off, x_off, table, n_x, sum_V = srch.align_tables([MS[q] for q, _ in pairs], [VS[v] for _, v in pairs],
                                                                first[[q for q, _ in pairs]], [v for _, v in pairs])
    x = torch.full((n_x,), float("nan"), device="cuda")
    ops.sequence_scores(tq, vn, _dev(s_off), _dev(v_off), _dev(hits), torch.from_numpy(hit_off.copy()).cuda(), x, check_offsets=True, **kw)
    assert not torch.isnan(x).any()                                 # the pieces' blocks tile every pair's [m, V] block
    score, span = ops.local_align(x, torch.from_numpy(x_off.copy()).cuda(), _dev(table), THETA, SKEW, sum_V=sum_V)
    score, span, xs = score.cpu().numpy(), span.cpu().numpy(), x.cpu().numpy()
    S_h = S64.cpu().numpy()
    q_row = np.concatenate([[0], np.cumsum(MS)])
    if fmt == "e4m3":
        A_h = (_deq(tq, kw["q_scale"]).abs() @ _deq(vn, kw["v_scale"]).abs().T).cpu().numpy()
    worst, worst_bound = 0.0, 0.0
    for h, (q, v) in enumerate(pairs):
        m, V = MS[q], VS[v]
        block = xs[x_off[h]:x_off[h] + m * V].reshape(m, V)
        rows, cols = slice(q_row[q], q_row[q + 1]), slice(v_off[v], v_off[v + 1])
        assert np.abs(block - S_h[rows, cols]).max() <= (ACC_EPS * A_h[rows, cols].max() if fmt == "e4m3" else EPS)
        want_s, want_span = ref.align(block, THETA, SKEW)           # float32, over the device's own bits
        assert want_s.dtype == np.float32
        assert score[h:h + 1].view(np.int32)[0] == np.array([want_s]).view(np.int32)[0], (fmt, m, V, score[h], want_s)
        assert tuple(span[h].tolist()) == want_span, (fmt, m, V)
        exact, _ = ref.align(S_h[rows, cols], THETA, SKEW)          # fp64 recurrence over the fp64 scores of the stored rows
        eps = ACC_EPS * A_h[rows, cols].max() if fmt == "e4m3" else EPS
        bound = (m + V) * (eps + 2.0 ** -24 * (2 + 4 * (m + V)))
        err = abs(float(score[h]) - float(exact))
        if err > worst:
            worst, worst_bound = err, bound
        assert err <= bound, (fmt, m, V, err, bound)
    assert (score > 0).sum() >= 36 and (span[:, 4] > span[:, 1] - span[:, 0] + 1).any()
    print(f"local_align max |score - fp64 recurrence| {fmt}: {worst:.3e} (its bound {worst_bound:.3e})")


# -------------------------------------------------------------------------------- 4. bad arguments, skipped entries, guard bands
def test_local_align_rejects_bad_arguments_and_skips_bad_entries():
    ops = _ops()
    L = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                     # noqa: E731
    G = 64
    shapes = [(65, 70), (3, 5), (129, 40), (2, 2), (64, 129)]
    blocks = [(_exact_blocks()[(129, 200)][:m, :V] / 16.0).astype(np.float32) for m, V in shapes]
    want = _align(blocks, 0.25, 0.125)
    assert all(w[0] > 0 for w in want)
    x_off, table, sum_V = _tables(shapes)
    P, n_x = len(shapes), int(x_off[-1])
    x = torch.from_numpy(np.concatenate([b.reshape(-1) for b in blocks])).cuda()
    xo, tb = torch.from_numpy(x_off[:-1].copy()).cuda(), _dev(table)
    sc_all = torch.full((P + 2 * G,), float("nan"), device="cuda")
    sp_all = torch.full((5 * P + 2 * G,), -777, dtype=torch.int32, device="cuda")
    nws = ops.local_align_ws_bytes(P, sum_V)
    assert nws == 32 * sum_V + 16
    ws_all = torch.full((nws + 2 * G,), 0xEE, dtype=torch.uint8, device="cuda")
    sc, sp, ws = sc_all[G:G + P], sp_all[G:G + 5 * P].view(P, 5), ws_all[G:G + nws]

    def clean():
        torch.cuda.synchronize()
        return (torch.isnan(sc_all[:G]).all() and torch.isnan(sc_all[G + P:]).all() and (sp_all[:G] == -777).all()
                and (sp_all[G + 5 * P:] == -777).all() and (ws_all[:G] == 0xEE).all() and (ws_all[G + nws:] == 0xEE).all())

    def call(x=x, n_x=n_x, xo=xo, tb=tb, P=P, sum_V=sum_V, theta=0.25, skew=0.125, sc=sc, sp=sp, ws=ws):
        return L.tan_local_align(p(x), n_x, p(xo), p(tb), P, sum_V, theta, skew, p(sc), p(sp), p(ws), None)

    class Null:                                                                       # a NULL pointer for one argument
        @staticmethod
        def data_ptr():
            return None
    null = Null()
    for kw in (dict(x=null), dict(xo=null), dict(tb=null), dict(sc=null), dict(sp=null), dict(ws=null), dict(n_x=0), dict(P=0), dict(P=-1),
               dict(P=1 << 31), dict(sum_V=P - 1), dict(sum_V=1 << 31), dict(theta=float("nan")), dict(theta=float("inf")),
               dict(theta=float("-inf")), dict(skew=-0.125), dict(skew=float("inf")), dict(skew=float("nan"))):
        assert call(**kw) == -1, kw
    assert clean() and torch.isnan(sc).all() and (sp == -777).all() and (ws == 0xEE).all()       # refused: nothing was written
    for bad in ((0, 5), (3, 2), (3, 1 << 31), (1 << 31, 1 << 31)):
        assert L.tan_local_align_ws_bytes(*bad) == -1, bad
        with pytest.raises(_lib.TanHipError):
            ops.local_align_ws_bytes(*bad)
    # the launch itself, into caller-owned outputs and scratch between guard bands
    got = ops.local_align(x, xo, tb, 0.25, 0.125, sum_V=sum_V, out=(sc, sp), ws=ws)
    assert got[0].data_ptr() == sc.data_ptr() and clean()
    assert [(float(s),) + tuple(r) for s, r in zip(sc.tolist(), sp.tolist())] == want
    # table entries outside the limits are skipped with the empty result; their neighbours are not disturbed
    for h, entry, off in ((0, (0, 70, 0), None), (1, (4097, 5, 70), None), (2, (129, 0, 75), None), (3, (2, 1 << 20, 115), None),
                          (4, (4096, 1 << 19, 117), None),                       # m * V = 2^31
                          (0, None, -1), (4, None, n_x - 64 * 129 + 1), (2, None, n_x),          # the block leaves [0, n_x)
                          (1, (3, 5, -1), None), (4, (64, 129, sum_V - 128), None), (3, (2, 2, sum_V), None)):        # its slots leave ws
        t2, o2 = table.copy(), x_off[:-1].copy()
        if entry is not None:
            t2[h] = entry
        if off is not None:
            o2[h] = off
        sc.fill_(float("nan"))
        sp.fill_(-777)
        ops.local_align(x, torch.from_numpy(o2).cuda(), _dev(t2), 0.25, 0.125, sum_V=sum_V, out=(sc, sp), ws=ws)
        assert clean(), (h, entry, off)
        got = [(float(s),) + tuple(r) for s, r in zip(sc.tolist(), sp.tolist())]
        assert got == [EMPTY if i == h else w for i, w in enumerate(want)], (h, entry, off)
    # the wrapper's own checks
    for kw in (dict(theta=float("nan")), dict(skew=-1.0), dict(skew=float("inf"))):
        with pytest.raises(ValueError):
            ops.local_align(x, xo, tb, kw.get("theta", 0.25), kw.get("skew", 0.0))
    for args in ((x.double(), xo, tb), (x.view(1, -1), xo, tb), (x, xo.int(), tb), (x, xo, tb.long()), (x, xo, tb[:, :2].contiguous()),
                 (x, xo[:2], tb)):
        with pytest.raises(ValueError):
            ops.local_align(*args, 0.25, 0.0)
    with pytest.raises(ValueError):
        ops.local_align(x, xo, tb, 0.25, 0.0, sum_V=sum_V, ws=ws[:nws - 1])
    with pytest.raises(ValueError):
        ops.local_align(x, xo, tb, 0.25, 0.0, out=(sc, sp.view(-1)))
    with pytest.raises(_lib.TanHipError):
        ops.local_align(x.cpu(), xo.cpu(), tb.cpu(), 0.25, 0.0, sum_V=sum_V, ws=ws)
    got = ops.local_align(x, xo, tb, 0.25, 0.125, check_table=True)  # sum_V read from the table, fresh scratch and outputs
    assert [(float(s),) + tuple(r) for s, r in zip(got[0].tolist(), got[1].tolist())] == want
    for col2 in ([0, 70, 70, 115, 117], [1, 71, 76, 116, 118], [0, 70, 75, 115, 116]):      # shared slots, a shifted start, an overlap
        t2 = table.copy()
        t2[:, 2] = col2
        with pytest.raises(ValueError, match="running sum"):
            ops.local_align(x, xo, _dev(t2), 0.25, 0.125, check_table=True)


# ------------------------------------------------------------------------------------------- 5. a planted, re-timed copy through search
LENS = [70, 90, 33, 200, 120, 64]
SRC, COPY, DECOY, Q0, QM = 1, 3, 4, 20, 40
CUTS = (0, 2, 4, 6)                                                 # three shards of two videos


@functools.lru_cache(maxsize=None)
def _planted(fmt):
    """Six videos of random unit rows.  The query is seconds 20..59 of video 1.  Video 3 holds a copy from second 50 on: the query's
    first 20 seconds at half speed (50..89), 6 unrelated seconds, the other 20 seconds at normal speed (96..115).  Video 4, the
    decoy, holds the query's seconds 4..11 once (30..37).  Every copied row is mixed with 0.6 of a random unit row."""
    srch = _srch()
    v_off = np.concatenate([[0], np.cumsum(LENS)])
    feat = _unit_rows(int(v_off[-1]), 71, torch.float32)
    q = feat[v_off[SRC] + Q0:v_off[SRC] + Q0 + QM].clone()
    noise = _unit_rows(68, 72, torch.float32)

    def mixed(rows, nz):
        r = rows + 0.6 * nz
        return r / r.norm(dim=1, keepdim=True)
    feat[v_off[COPY] + 50:v_off[COPY] + 90] = mixed(q[:20].repeat_interleave(2, 0), noise[:40])
    feat[v_off[COPY] + 96:v_off[COPY] + 116] = mixed(q[20:], noise[40:60])
    feat[v_off[DECOY] + 30:v_off[DECOY] + 38] = mixed(q[4:12], noise[60:68])
    vids = [f"v{i:03d}" for i in range(len(LENS))]
    f32 = srch.VideoIndex(feat, v_off, vids)
    return f32.quantize() if fmt == "e4m3" else srch.VideoIndex(feat.to(torch.bfloat16 if fmt == "bf16" else torch.float32), v_off, vids)


def _shards(idx):
    srch = _srch()
    parts = []
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        r0, r1 = int(idx.v_off[a]), int(idx.v_off[b])
        parts.append(srch.VideoIndex(idx.feat[r0:r1].contiguous(), idx.v_off[a:b + 1] - r0, idx.vids[a:b],
                                     None if idx.scale is None else idx.scale[r0:r1].contiguous()))
    return parts


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_planted_retimed_copy_is_found_where_clip_search_prefers_the_decoy(fmt, tmp_path, capsys):
    srch = _srch()
    idx = _planted(fmt)
    theta, skew = 0.4, 0.1
    query = (idx.vids[SRC], Q0, Q0 + QM - 1)
    nv, off = len(LENS), idx.v_off
    # ---- the margins in fp64, from the stored rows
    tq, _ = srch.clip_features(idx, [query], srch.MAX_ALIGN_SECONDS)
    q64, v64 = (_deq(*tq), _deq(idx.feat, idx.scale)) if idx.e4m3 else (tq.double(), idx.feat.double())
    S_h, A_h = (q64 @ v64.T).cpu().numpy(), (q64.abs() @ v64.abs().T).cpu().numpy()
    exact, bound = [], []
    for v in range(nv):
        cols = slice(off[v], off[v + 1])
        exact.append(ref.align(S_h[:, cols], theta, skew))
        eps = ACC_EPS * A_h[:, cols].max() if fmt == "e4m3" else EPS
        bound.append((QM + LENS[v]) * (eps + 2.0 ** -24 * (2 + 4 * (QM + LENS[v]))))
    others = [v for v in range(nv) if v not in (SRC, COPY, DECOY)]
    assert exact[COPY][1] == (0, 39, 50, 115, 66) and exact[DECOY][1] == (4, 11, 30, 37, 8) and exact[SRC][1] == (0, 39, Q0, Q0 + QM - 1, QM)
    assert exact[SRC][0] - bound[SRC] > exact[COPY][0] + bound[COPY] and exact[COPY][0] - bound[COPY] > exact[DECOY][0] + bound[DECOY]
    assert exact[DECOY][0] > bound[DECOY]
    for v in others:                                                # no second of the other videos comes near the threshold
        assert S_h[:, off[v]:off[v + 1]].max() + (ACC_EPS * A_h[:, off[v]:off[v + 1]].max() if fmt == "e4m3" else EPS) < theta
    # the best 16-second diagonal of the query's first piece: the decoy's stands clear ABOVE the copy's
    dbound = lambda v: (ACC_EPS * clip_ref.diag_sums(A_h[:16, off[v]:off[v + 1]]).max() if fmt == "e4m3" else 16 * EPS) + 256 * 2.0 ** -24   # noqa: E731
    diag = [clip_ref.diag_sums(S_h[:16, off[v]:off[v + 1]]).max() for v in range(nv)]
    assert diag[DECOY] - dbound(DECOY) > diag[COPY] + dbound(COPY) and diag[COPY] - dbound(COPY) > max(diag[v] + dbound(v) for v in others)
    print(f"search_copies {fmt}: fp64 alignment copy {exact[COPY][0]:.4f} / decoy {exact[DECOY][0]:.4f} (bounds {bound[COPY]:.2e} / "
          f"{bound[DECOY]:.2e}); fp64 best 16 s diagonal copy {diag[COPY]:.4f} / decoy {diag[DECOY]:.4f}")
    # ---- align_spans
    got = srch.align_spans(idx, [(query, v) for v in range(nv)], theta, skew)
    assert [g is None for g in got] == [v in others for v in range(nv)]
    assert tuple(got[COPY])[:5] == (idx.vids[COPY], 50, 115, 0, 39) and got[COPY].cells == 66 and isinstance(got[COPY], srch.CopyHit)
    assert tuple(got[DECOY])[:5] == (idx.vids[DECOY], 30, 37, 4, 11) and got[DECOY].cells == 8
    assert tuple(got[SRC])[:5] == (idx.vids[SRC], Q0, Q0 + QM - 1, 0, 39) and got[SRC].cells == QM
    for v in (SRC, COPY, DECOY):
        assert abs(got[v].score - exact[v][0]) <= bound[v], (v, got[v].score, exact[v][0])
    # a vid by name, the query as a tensor of the stored rows, several queries and repeated pairs in one call
    rows = v64[off[SRC] + Q0:off[SRC] + Q0 + QM].float()            # exact: bf16 values, or code x power of two
    again = srch.align_spans(idx, [(rows, idx.vids[COPY]), (query, idx.vids[DECOY]), ((SRC, Q0, Q0), COPY), (rows, COPY), (rows[:1], 2)], theta, skew)
    assert again[0] == got[COPY] == again[3] and again[1] == got[DECOY] and again[4] is None
    assert again[2][1:5] == (50, 51, 0, 0) and again[2].cells == 2   # one second shown for two: a path of two cells along the video
    # ---- search_copies: the copy first and the decoy second, nothing else; the source ahead of both unless it is left out
    hits = srch.search_copies(idx, [query], threshold=theta, skew=skew, exclude_source=True)[0]
    assert hits == [got[COPY], got[DECOY]]
    assert srch.search_copies(idx, [query], threshold=theta, skew=skew)[0] == [got[SRC], got[COPY], got[DECOY]]
    assert srch.search_copies(idx, [rows], threshold=theta, skew=skew, exclude_source=True)[0] == [got[SRC], got[COPY], got[DECOY]]
    assert srch.search_copies(idx, [query], k=1, threshold=theta, skew=skew, exclude_source=True)[0] == hits[:1]
    two = srch.search_copies(idx, [query, (COPY, 96, 115)], pool=3, piece=32, threshold=theta, skew=skew, exclude_source=True)
    assert two[0] == hits and two[1][0][:5] == (idx.vids[SRC], Q0 + 20, Q0 + 39, 0, 19)
    # ---- the gap this closes: clip search on the query's first 16 seconds ranks the decoy above the copy
    clips = srch.search_clips(idx, [(idx.vids[SRC], Q0, Q0 + 15)], k=5, exclude_source=True)[0]
    assert [h.vid for h in clips[:2]] == [idx.vids[DECOY], idx.vids[COPY]]
    # ---- three shards, device- and host-resident: the same hits bit for bit
    parts = _shards(idx)
    pairs = [(query, v) for v in range(nv)] + [(rows, COPY), ((4, 30, 37), SRC)]
    want = srch.align_spans(idx, pairs, theta, skew)
    for sharded in (srch.ShardedIndex(parts, resident="device"), srch.ShardedIndex(_pinned(parts), resident="host")):
        assert srch.align_spans(sharded, pairs, theta, skew) == want
        assert srch.align_spans(sharded, pairs[COPY:COPY + 1], theta, skew) == [got[COPY]]      # one shard visited
        assert srch.search_copies(sharded, [query], threshold=theta, skew=skew, exclude_source=True)[0] == hits
        assert srch.search_copies(sharded, [query, rows], pool=2, piece=8, threshold=theta, skew=skew)[1][:2] == [got[SRC], got[COPY]]
    # ---- the command line: no checkpoint, no model
    path = str(tmp_path / "index.npz")
    idx.save(path)
    capsys.readouterr()
    argv = ["similar", "--index", path, "--clip", f"{idx.vids[SRC]}:{Q0}-{Q0 + QM - 1}", "--align", "--threshold", "0.4", "--skew", "0.1"]
    assert srch.main(argv) == 0
    out = [line.split("\t") for line in capsys.readouterr().out.splitlines()]
    assert [(o[0],) + tuple(int(t) for t in o[1:3] + o[4:]) for o in out] == [(h.vid, h.start, h.end, h.q_start, h.q_end, h.cells) for h in hits]
    assert [o[3] for o in out] == [f"{h.score:.6f}" for h in hits]
    assert srch.main(argv + ["--keep-source", "-k", "2", "--pool", "4", "--piece", "20"]) == 0
    out = [line.split("\t") for line in capsys.readouterr().out.splitlines()]
    assert [o[0] for o in out] == [idx.vids[SRC], idx.vids[COPY]]
    assert srch.main(["similar", "--index", path, "--clip", "nobody:0-99", "--align", "--threshold", "0.4"]) == 2
    assert "nobody" in capsys.readouterr().err
    torch.cuda.synchronize()
