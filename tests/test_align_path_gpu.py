"""The time map of copy alignment on the GPU: tan_local_align_path (tan_local_align with the best path's second-to-second map),
`ops.local_align_path`, `search.align_paths` / `search_copies(paths=True)` / the `similar --align --map` command.  The codes and the
walk back are restated as a plain loop in path_ref.py (pinned against align_ref.align by test_align_path_cpu.py).

  * shapes, launches and prices are test_align_gpu.py's: m in 1, 2, 63, 64, 65, 129 times V in 1, 2, 63, 64, 65, 129, 200, in launches of
    1, 4, 5 and all 42 blocks.
  * exact arithmetic: on blocks of sixteenths every H is exact in f32, so (score * 16, span, qmap) equal the int64 reference with `==`,
    and (score, span) equal `ops.local_align`'s bits.
  * staircases: planted paths whose cells are known (path_ref.staircase), crossing the strip edges at rows 64 and 128 and the slab
    edges at columns 64 and 128 by every kind of step.
  * random unit rows: path_ref in float32 over the device's own score bits reproduces score (as bits), span and qmap with `==`.  Maps are
    not compared against fp64 (an argmax may flip); the planted copy's robust rows are."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import path_ref as ref
from temporalalignnet_amd import _lib
from test_align_gpu import (ALL, COPY, DECOY, LAUNCHES, LENS, MS, PRICES, Q0, QM, SKEW, SRC, THETA, VS, _exact_blocks, _planted, _shards, _srch,
                            _tables)
from test_moments_gpu import FORMATS, _dev, _ops, _stored
from test_retrieve_fp8_gpu import _deq
from test_retrieve_gpu import _unit_rows
from test_shards_gpu import _pinned

pytestmark = pytest.mark.gpu

FILL = -777                                                         # what the tests put into qmap before a launch


def _launch(blocks, theta, skew):
    """blocks: f32 arrays [m, V] (host) -> the device arguments of one launch"""
    srch = _srch()
    shapes = [b.shape for b in blocks]
    x_off, table, sum_V = _tables(shapes)
    path_off, n_map, n_trace = srch.path_tables(table[:, 0], table[:, 1])
    x = torch.from_numpy(np.concatenate([b.reshape(-1) for b in blocks]).astype(np.float32)).cuda()
    return dict(x=x, x_off=torch.from_numpy(x_off[:-1].copy()).cuda(), table=_dev(table), theta=theta, skew=skew,
                path_off=torch.from_numpy(path_off.copy()).cuda(), sum_V=sum_V, n_map=n_map, n_trace=n_trace), path_off, shapes


def _align_path(blocks, theta, skew, raw=False):
    """-> [(score, span tuple, qmap [m, 2] list)] from one launch over a FILL-filled map"""
    ops = _ops()
    kw, path_off, shapes = _launch(blocks, theta, skew)
    P = len(blocks)
    out = (torch.full((P,), float("nan"), device="cuda"), torch.full((P, 5), FILL, dtype=torch.int32, device="cuda"),
           torch.full((kw["n_map"], 2), FILL, dtype=torch.int32, device="cuda"))
    score, span, qmap = ops.local_align_path(kw.pop("x"), kw.pop("x_off"), kw.pop("table"), kw.pop("theta"), kw.pop("skew"), kw.pop("path_off"),
                                             out=out, **kw)
    if raw:
        return score, span, qmap
    s, sp, q = score.cpu().numpy(), span.cpu().numpy(), qmap.cpu().numpy()
    return [(float(s[h]), tuple(int(v) for v in sp[h]), q[path_off[h, 0]:path_off[h, 0] + m].tolist()) for h, (m, _) in enumerate(shapes)]


def _well_formed(got, m):
    """what holds for every valid entry whatever the scores: all m rows written, -1 outside [a_first, a_last], the four identities"""
    score, (a0, a1, b0, b1, cells), qmap = got
    q = np.array(qmap).reshape(m, 2)
    assert (q != FILL).all()
    if not score > 0:
        assert (a0, a1, b0, b1, cells) == ref.EMPTY and (q == -1).all()
        return
    assert (q[:a0] == -1).all() and (q[a1 + 1:] == -1).all() and (q[a0:a1 + 1] >= 0).all()
    assert q[a0, 0] == b0 and q[a1, 1] == b1 and int((q[a0:a1 + 1, 1] - q[a0:a1 + 1, 0] + 1).sum()) == cells
    step = q[a0 + 1:a1 + 1, 0] - q[a0:a1, 1]
    assert ((step == 0) | (step == 1)).all()


@functools.lru_cache(maxsize=None)
def _exact_want(theta16, skew16):
    out = {}
    for mv, xi in _exact_blocks().items():
        score, span, qmap = ref.align_path(xi, theta16, skew16)
        out[mv] = (float(score), span, qmap.tolist())
    return out


# ------------------------------------------------------------------------------------------------------------- 1. exact arithmetic
@pytest.mark.parametrize("prices", PRICES)
@pytest.mark.parametrize("P", sorted(LAUNCHES))
def test_local_align_path_exact_arithmetic(P, prices):
    theta, skew = prices
    want = _exact_want(int(theta * 16), int(skew * 16))
    shapes = LAUNCHES[P]
    blocks = [(_exact_blocks()[mv] / 16.0).astype(np.float32) for mv in shapes]
    got = _align_path(blocks, theta, skew)
    assert any(w[0] > 0 and w[1][4] > max(w[1][1] - w[1][0], w[1][3] - w[1][2]) + 1 for w in want.values())      # steps along one axis
    for mv, g in zip(shapes, got):
        _well_formed(g, mv[0])
        assert (g[0] * 16, g[1], g[2]) == want[mv], (mv, prices, g[:2], want[mv][:2])
    # score and span are tan_local_align's, bit for bit
    kw, _, _ = _launch(blocks, theta, skew)
    score, span, _ = _align_path(blocks, theta, skew, raw=True)
    s0, sp0 = _ops().local_align(kw["x"], kw["x_off"], kw["table"], theta, skew, sum_V=kw["sum_V"])
    assert torch.equal(score.view(torch.int32), s0.view(torch.int32)) and torch.equal(span, sp0)


def test_the_shapes_are_the_alignments():
    assert set(MS) == {1, 2, 63, 64, 65, 129} and set(VS) == {1, 2, 63, 64, 65, 129, 200} and len(ALL) == 42
    assert sorted(LAUNCHES) == [1, 4, 5, 42] and len(PRICES) == 3


# ------------------------------------------------------------------------------------------------------------------ 2. staircases
@functools.lru_cache(maxsize=None)
def _stairs():
    out = []
    for (m, V), start in ref.STAIR_CASES:
        x, cells = ref.staircase(m, V, start)
        out.append(((x / 16.0).astype(np.float32), cells, ref.map_of(cells, m).tolist()))
    return out


def _stair_want(cells, theta16, skew16, qmap):
    n_axis = sum(1 for (i, j), (i2, j2) in ref.steps(cells) if (i2 - i) + (j2 - j) == 1)
    return ((len(cells) * (24 - theta16) - n_axis * skew16) / 16.0, (cells[0][0], cells[-1][0], cells[0][1], cells[-1][1], len(cells)), qmap)


@pytest.mark.parametrize("prices", ref.STAIR_PRICES)
def test_planted_staircases_come_back_cell_for_cell(prices):
    theta16, skew16 = prices
    stairs = _stairs()
    got = _align_path([x for x, _, _ in stairs], theta16 / 16.0, skew16 / 16.0)      # 25 blocks: the last alone in its workgroup
    assert len(stairs) % 4 == 1
    for (x, cells, qmap), g in zip(stairs, got):
        assert g == _stair_want(cells, theta16, skew16, qmap), (x.shape, cells[0], prices, g[:2])


def test_a_staircase_is_found_first_last_and_in_a_partly_filled_workgroup():
    """launches of 5 consecutive cases: every case is the first block of one launch and the last of another, where it sits alone in
    the second workgroup; the prices rotate"""
    stairs = _stairs()
    n = len(stairs)
    for k in range(n):
        theta16, skew16 = ref.STAIR_PRICES[k % len(ref.STAIR_PRICES)]
        pick = [stairs[(k + t) % n] for t in range(5)]
        got = _align_path([x for x, _, _ in pick], theta16 / 16.0, skew16 / 16.0)
        for (x, cells, qmap), g in zip(pick, got):
            assert g == _stair_want(cells, theta16, skew16, qmap), (k, x.shape, cells[0], g[:2])


# ------------------------------------------------------------------------------------------------------------------ 3. run to run
def test_two_runs_are_bit_identical_and_every_row_is_written():
    rng = np.random.default_rng(12)
    shapes = LAUNCHES[42]
    blocks = [rng.normal(0.0, 0.05, mv).astype(np.float32) for mv in shapes]
    blocks[3] = np.full(shapes[3], -1.0, dtype=np.float32)          # nothing positive: all rows -1
    a = _align_path(blocks, 0.02, 0.01, raw=True)
    b = _align_path(blocks, 0.02, 0.01, raw=True)
    for s, t in zip(a, b):
        assert torch.equal(s.view(torch.int32), t.view(torch.int32))                 # the scores as bits
    got = _align_path(blocks, 0.02, 0.01)
    assert got[3] == (0.0, ref.EMPTY, [[-1, -1]] * shapes[3][0])
    for (m, _), g in zip(shapes, got):
        _well_formed(g, m)
    assert sum(g[0] > 0 for g in got) >= 36 and any(g[1][4] > g[1][1] - g[1][0] + 1 for g in got)


# ------------------------------------------------------------------------------------------------------- 4. random unit rows
@pytest.mark.parametrize("fmt", FORMATS)
def test_local_align_path_random_unit_rows(fmt):
    ops, srch = _ops(), _srch()
    v_off = np.concatenate([[0], np.cumsum(VS)]).astype(np.int64)
    tq, vn, kw, _, _ = _stored(fmt, _unit_rows(int(sum(MS)), 901, torch.float32), _unit_rows(int(v_off[-1]), 902, torch.float32))
    s_off, first = srch.piece_offsets(MS)
    pairs = [(q, v) for q in range(len(MS)) for v in range(len(VS))]
    hits, hit_off, x_off, table, n_x, sum_V = srch.align_tables([MS[q] for q, _ in pairs], [VS[v] for _, v in pairs],
                                                                first[[q for q, _ in pairs]], [v for _, v in pairs])
    path_off, n_map, n_trace = srch.path_tables(table[:, 0], table[:, 1])
    x = torch.full((n_x,), float("nan"), device="cuda")
    ops.sequence_scores(tq, vn, _dev(s_off), _dev(v_off), _dev(hits), torch.from_numpy(hit_off.copy()).cuda(), x, check_offsets=True, **kw)
    assert not torch.isnan(x).any()
    xo, tb = torch.from_numpy(x_off.copy()).cuda(), _dev(table)
    score, span, qmap = ops.local_align_path(x, xo, tb, THETA, SKEW, torch.from_numpy(path_off.copy()).cuda(), sum_V=sum_V, n_map=n_map,
                                             n_trace=n_trace)
    s0, sp0 = ops.local_align(x, xo, tb, THETA, SKEW, sum_V=sum_V)
    assert torch.equal(score.view(torch.int32), s0.view(torch.int32)) and torch.equal(span, sp0)
    score, span, qmap, xs = score.cpu().numpy(), span.cpu().numpy(), qmap.cpu().numpy(), x.cpu().numpy()
    for h, (q, v) in enumerate(pairs):
        m, V = MS[q], VS[v]
        want_s, want_span, want_map = ref.align_path(xs[x_off[h]:x_off[h] + m * V].reshape(m, V), THETA, SKEW)       # float32, the device's bits
        assert want_s.dtype == np.float32
        assert score[h:h + 1].view(np.int32)[0] == np.array([want_s]).view(np.int32)[0], (fmt, m, V, score[h], want_s)
        assert tuple(span[h].tolist()) == want_span, (fmt, m, V)
        assert (qmap[path_off[h, 0]:path_off[h, 0] + m] == want_map).all(), (fmt, m, V)
    assert (score > 0).sum() >= 36 and (span[:, 4] > span[:, 1] - span[:, 0] + 1).any()


# -------------------------------------------------------------------------------- 5. bad arguments, skipped entries, guard bands
def test_local_align_path_rejects_bad_arguments_and_skips_bad_entries():
    ops, srch = _ops(), _srch()
    L = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                     # noqa: E731
    G = 64
    shapes = [(65, 70), (3, 5), (129, 40), (2, 2), (64, 129)]
    blocks = [(_exact_blocks()[(129, 200)][:m, :V] / 16.0).astype(np.float32) for m, V in shapes]
    want = _align_path(blocks, 0.25, 0.125)
    assert all(w[0] > 0 for w in want)
    x_off, table, sum_V = _tables(shapes)
    path_off, n_map, n_trace = srch.path_tables(table[:, 0], table[:, 1])
    assert n_map == sum(m for m, _ in shapes) and n_trace == sum((m + 63) // 64 * (V + 63) for m, V in shapes)
    P, n_x = len(shapes), int(x_off[-1])
    x = torch.from_numpy(np.concatenate([b.reshape(-1) for b in blocks])).cuda()
    xo, tb, po = torch.from_numpy(x_off[:-1].copy()).cuda(), _dev(table), torch.from_numpy(path_off.copy()).cuda()
    sc_all = torch.full((P + 2 * G,), float("nan"), device="cuda")
    sp_all = torch.full((5 * P + 2 * G,), FILL, dtype=torch.int32, device="cuda")
    qm_all = torch.full((2 * n_map + 2 * G,), FILL, dtype=torch.int32, device="cuda")
    nws = ops.local_align_path_ws_bytes(P, sum_V, n_trace)
    assert nws == 32 * sum_V + 16 * n_trace + 16
    ws_all = torch.full((nws + 2 * G,), 0xEE, dtype=torch.uint8, device="cuda")
    sc, sp, qm, ws = sc_all[G:G + P], sp_all[G:G + 5 * P].view(P, 5), qm_all[G:G + 2 * n_map].view(n_map, 2), ws_all[G:G + nws]

    def clean():
        torch.cuda.synchronize()
        return (torch.isnan(sc_all[:G]).all() and torch.isnan(sc_all[G + P:]).all() and (sp_all[:G] == FILL).all()
                and (sp_all[G + 5 * P:] == FILL).all() and (qm_all[:G] == FILL).all() and (qm_all[G + 2 * n_map:] == FILL).all()
                and (ws_all[:G] == 0xEE).all() and (ws_all[G + nws:] == 0xEE).all())

    def call(x=x, n_x=n_x, xo=xo, tb=tb, P=P, sum_V=sum_V, theta=0.25, skew=0.125, po=po, n_map=n_map, n_trace=n_trace, sc=sc, sp=sp, qm=qm, ws=ws):
        return L.tan_local_align_path(p(x), n_x, p(xo), p(tb), P, sum_V, theta, skew, p(po), n_map, n_trace, p(sc), p(sp), p(qm), p(ws), None)

    class Null:                                                                       # a NULL pointer for one argument
        @staticmethod
        def data_ptr():
            return None
    null = Null()
    for kw in (dict(x=null), dict(xo=null), dict(tb=null), dict(po=null), dict(sc=null), dict(sp=null), dict(qm=null), dict(ws=null), dict(n_x=0),
               dict(P=0), dict(P=-1), dict(P=1 << 31), dict(sum_V=P - 1), dict(sum_V=1 << 31), dict(n_map=0), dict(n_map=-5), dict(n_trace=0),
               dict(n_trace=-1), dict(theta=float("nan")), dict(theta=float("inf")), dict(theta=float("-inf")), dict(skew=-0.125),
               dict(skew=float("inf")), dict(skew=float("nan"))):
        assert call(**kw) == -1, kw
    assert clean() and torch.isnan(sc).all() and (sp == FILL).all() and (qm == FILL).all() and (ws == 0xEE).all()      # nothing was written
    for bad in ((0, 5, 64), (3, 2, 64), (3, 1 << 31, 64), (1 << 31, 1 << 31, 64), (3, 5, 0), (3, 5, -1)):
        assert L.tan_local_align_path_ws_bytes(*bad) == -1, bad
        with pytest.raises(_lib.TanHipError):
            ops.local_align_path_ws_bytes(*bad)

    def read():
        return [(float(s), tuple(r), qm[path_off[h, 0]:path_off[h, 0] + shapes[h][0]].tolist()) for h, (s, r) in enumerate(zip(sc.tolist(), sp.tolist()))]

    # the launch itself, into caller-owned outputs and scratch between guard bands
    got = ops.local_align_path(x, xo, tb, 0.25, 0.125, po, sum_V=sum_V, n_map=n_map, n_trace=n_trace, out=(sc, sp, qm), ws=ws)
    assert got[2].data_ptr() == qm.data_ptr() and clean()
    assert read() == want
    # skipped entries: the empty result, their FILL-filled map rows untouched, their neighbours undisturbed
    need4 = (64 + 63) // 64 * (129 + 63)
    for h, entry, off, prow in ((0, (0, 70, 0), None, None), (1, (4097, 5, 70), None, None), (2, (129, 0, 75), None, None),      # a bad m or V
                                (3, (2, 1 << 20, 115), None, None),
                                (0, None, -1, None), (4, None, n_x - 64 * 129 + 1, None), (2, None, n_x, None),                   # the block leaves x
                                (1, (3, 5, -1), None, None), (4, (64, 129, sum_V - 128), None, None), (3, (2, 2, sum_V), None, None),   # its slots
                                (0, None, None, (-1, 0)), (4, None, None, (n_map - 63, int(path_off[4, 1]))),                     # its map rows
                                (2, None, None, (n_map, int(path_off[2, 1]))),
                                (1, None, None, (65, -1)), (4, None, None, (int(path_off[4, 0]), n_trace - need4 + 1)),           # its trace entries
                                (3, None, None, (int(path_off[3, 0]), n_trace))):
        t2, o2, p2 = table.copy(), x_off[:-1].copy(), path_off.copy()
        if entry is not None:
            t2[h] = entry
        if off is not None:
            o2[h] = off
        if prow is not None:
            p2[h] = prow
        sc.fill_(float("nan"))
        sp.fill_(FILL)
        qm.fill_(FILL)
        ops.local_align_path(x, torch.from_numpy(o2).cuda(), _dev(t2), 0.25, 0.125, torch.from_numpy(p2).cuda(), sum_V=sum_V, n_map=n_map,
                             n_trace=n_trace, out=(sc, sp, qm), ws=ws)
        assert clean(), (h, entry, off, prow)
        empty = (0.0, ref.EMPTY, [[FILL, FILL]] * shapes[h][0])
        assert read() == [empty if i == h else w for i, w in enumerate(want)], (h, entry, off, prow)
    # the wrapper's own checks
    kwargs = dict(sum_V=sum_V, n_map=n_map, n_trace=n_trace)
    for kw in (dict(theta=float("nan")), dict(skew=-1.0), dict(skew=float("inf"))):
        with pytest.raises(ValueError):
            ops.local_align_path(x, xo, tb, kw.get("theta", 0.25), kw.get("skew", 0.0), po, **kwargs)
    for args in ((x.double(), xo, tb, po), (x, xo.int(), tb, po), (x, xo, tb.long(), po), (x, xo[:2], tb, po), (x, xo, tb, po.int()),
                 (x, xo, tb, po[:, :1].contiguous()), (x, xo, tb, po[:2])):
        with pytest.raises(ValueError):
            ops.local_align_path(*args[:3], 0.25, 0.0, args[3], **kwargs)
    for kw in (dict(kwargs, n_map=0), dict(kwargs, n_trace=0), dict(kwargs, ws=ws[:nws - 1]), dict(kwargs, out=(sc, sp, qm.view(-1))),
               dict(kwargs, out=(sc, sp.view(-1), qm))):
        with pytest.raises(ValueError):
            ops.local_align_path(x, xo, tb, 0.25, 0.0, po, **kw)
    with pytest.raises(TypeError):
        ops.local_align_path(x, xo, tb, 0.25, 0.0, po, sum_V=sum_V)                   # n_map and n_trace have no default
    got = ops.local_align_path(x, xo, tb, 0.25, 0.125, po, n_map=n_map, n_trace=n_trace)     # sum_V read from the table, fresh outputs
    assert [g for g in zip(got[0].tolist(), map(tuple, got[1].tolist()))] == [(w[0], w[1]) for w in want]
    assert got[2].tolist() == [row for w in want for row in w[2]]


# ------------------------------------------------------------------------------------------- 6. the planted, re-timed copy through search
def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.hit == b.hit and a.seconds.dtype == b.seconds.dtype == np.int32 and np.array_equal(a.seconds, b.seconds)


def _robust_rows(copy_map, decoy_map, src_map):
    """the rows of the three maps (full [QM, 2] arrays, -1 outside the aligned span) that no noise moves"""
    i = np.arange(QM)
    assert (copy_map[:19] == np.stack((50 + 2 * i[:19], 51 + 2 * i[:19]), 1)).all()
    assert (copy_map[21:] == np.stack((76 + i[21:], 76 + i[21:]), 1)).all()
    assert copy_map[19, 0] == 88 and copy_map[20, 1] == 96 and copy_map[20, 0] - copy_map[19, 1] in (0, 1)
    assert (decoy_map[4:12] == np.stack((26 + i[4:12], 26 + i[4:12]), 1)).all() and (decoy_map[:4] == -1).all() and (decoy_map[12:] == -1).all()
    assert (src_map == np.stack((Q0 + i, Q0 + i), 1)).all()


def _full(path):
    q = np.full((QM, 2), -1, dtype=np.int32)
    q[path.hit.q_start:path.hit.q_end + 1] = path.seconds
    return q


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_planted_retimed_copy_maps_second_to_second(fmt, tmp_path, capsys):
    srch = _srch()
    idx = _planted(fmt)
    theta, skew = 0.4, 0.1
    query = (idx.vids[SRC], Q0, Q0 + QM - 1)
    nv, off = len(LENS), idx.v_off
    # ---- the fp64 path from the stored rows has the robust rows itself
    tq, _ = srch.clip_features(idx, [query], srch.MAX_ALIGN_SECONDS)
    q64, v64 = (_deq(*tq), _deq(idx.feat, idx.scale)) if idx.e4m3 else (tq.double(), idx.feat.double())
    S_h = (q64 @ v64.T).cpu().numpy()
    exact = {v: ref.align_path(S_h[:, off[v]:off[v + 1]], theta, skew) for v in (SRC, COPY, DECOY)}
    assert exact[COPY][1] == (0, 39, 50, 115, 66) and exact[DECOY][1] == (4, 11, 30, 37, 8)
    _robust_rows(exact[COPY][2], exact[DECOY][2], exact[SRC][2])
    # ---- align_paths
    pairs = [(query, v) for v in range(nv)]
    spans = srch.align_spans(idx, pairs, theta, skew)
    got = srch.align_paths(idx, pairs, theta, skew)
    assert [g is None for g in got] == [s is None for s in spans] == [v not in (SRC, COPY, DECOY) for v in range(nv)]
    for g, s in zip(got, spans):
        if s is not None:
            assert isinstance(g, srch.CopyPath) and g.hit == s and isinstance(g.hit, srch.CopyHit)
            assert g.seconds.dtype == np.int32 and g.seconds.shape == (s.q_end - s.q_start + 1, 2)
            assert g.seconds[0, 0] == s.start and g.seconds[-1, 1] == s.end and int((g.seconds[:, 1] - g.seconds[:, 0] + 1).sum()) == s.cells
    _robust_rows(_full(got[COPY]), _full(got[DECOY]), _full(got[SRC]))
    # ---- the helpers on the device's map
    assert srch.copy_interval(got[COPY], 5, 9) == (60, 69)
    assert srch.transfer_segments(got[COPY], [(5, 9, "whisk"), (100, 120, "beyond")]) == [(60, 69, "whisk")]
    assert srch.transfer_segments(got[DECOY], [(5, 9, "whisk"), (0, 3, "before")]) == [(31, 35, "whisk")]
    inv = srch.copy_inverse(got[COPY])
    assert inv.shape == (66, 2) and inv[:38].tolist() == [[t // 2, t // 2] for t in range(38)] and inv[47:].tolist() == [[t, t] for t in range(21, 40)]
    # ---- search_copies(paths=True) ranks as search_copies does
    plain = srch.search_copies(idx, [query], threshold=theta, skew=skew, exclude_source=True)[0]
    hits = srch.search_copies(idx, [query], threshold=theta, skew=skew, exclude_source=True, paths=True)[0]
    assert [h.hit for h in hits] == plain == [got[COPY].hit, got[DECOY].hit] and _same(hits[0], got[COPY]) and _same(hits[1], got[DECOY])
    kept = srch.search_copies(idx, [query], k=2, threshold=theta, skew=skew, paths=True)[0]
    assert _same(kept[0], got[SRC]) and _same(kept[1], got[COPY])
    # ---- three shards, device- and host-resident: the same paths
    rows = v64[off[SRC] + Q0:off[SRC] + Q0 + QM].float()
    more = pairs + [(rows, COPY), ((4, 30, 37), SRC), ((SRC, Q0, Q0), COPY)]
    want = srch.align_paths(idx, more, theta, skew)
    assert _same(want[nv], got[COPY]) and want[nv + 2].seconds.tolist() == [[50, 51]]
    parts = _shards(idx)
    for sharded in (srch.ShardedIndex(parts, resident="device"), srch.ShardedIndex(_pinned(parts), resident="host")):
        again = srch.align_paths(sharded, more, theta, skew)
        assert len(again) == len(want) and all(_same(a, w) for a, w in zip(again, want))
        assert _same(srch.align_paths(sharded, more[COPY:COPY + 1], theta, skew)[0], got[COPY])       # one shard visited
        sh = srch.search_copies(sharded, [query], threshold=theta, skew=skew, exclude_source=True, paths=True)[0]
        assert len(sh) == 2 and all(_same(a, w) for a, w in zip(sh, hits))
    # ---- the command line
    path, out_csv = str(tmp_path / "index.npz"), str(tmp_path / "map.csv")
    idx.save(path)
    capsys.readouterr()
    clip = f"{idx.vids[SRC]}:{Q0}-{Q0 + QM - 1}"
    argv = ["similar", "--index", path, "--clip", clip, "--align", "--threshold", "0.4", "--skew", "0.1"]
    assert srch.main(argv) == 0
    plain_out = capsys.readouterr().out
    assert srch.main(argv + ["--map", out_csv]) == 0
    assert capsys.readouterr().out == plain_out                      # the printed hits do not change
    with open(out_csv) as f:
        lines = [line.rstrip("\n").split(",") for line in f]
    assert lines[0] == ["query", "vid", "query_second", "first", "last"]
    want_rows = [[clip, h.hit.vid, str(Q0 + h.hit.q_start + i), str(lo), str(hi)] for h in hits for i, (lo, hi) in enumerate(h.seconds.tolist())]
    assert lines[1:] == want_rows and len(want_rows) == 40 + 8
    torch.cuda.synchronize()
