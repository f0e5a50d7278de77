"""Cover search on the GPU: tan_cover_topk / _e4m3 (per set of query rows and per video the Chamfer similarity -- every row's best
second and every second's best row, each summed in 64-bit fixed point -- and the k best videos), `ops.cover_topk`,
`search.search_cover`, `similar --cover`.  The definition is restated in numpy in cover_ref.py (pinned against a brute force over
Fractions by test_cover_cpu.py).

  * exact arithmetic (test_sequences_gpu.py's inputs: every score is an integer / 256 or / 512): fwd, bwd and the lists are compared
    with `==` against cover_ref over the int64 scores -- on the layout of test_sequences_gpu.py (N = 2742, 168 videos of 1, 2, 63,
    64, 65, 128, 129, 200 ... rows: one slab, a partial slab, two slabs), on all-negative scores (a zero-filled tail row of a query
    tile would beat every real row of b_t), on videos of several slabs with a partial last one (a repeated tail column must stay out
    of B), and at the limit of 4096 rows per set.
  * random unit rows: x for ALL (set, video) pairs from tan_sequence_scores (the sets cut into 32-row pieces); cover_ref in float32
    over those device bits reproduces fwd, bwd and the lists with `==`, and every fwd / bwd lies within EPS + 2^-21 of the fp64
    Chamfer means of the stored operands: a max of scores inherits the per-score bound EPS (e4m3: the block's largest
    ACC_EPS * sum |a b|); fix() adds at most 2^-31 per term, so 2^-31 to a mean; the int64 -> f32 conversion, the division and the
    halving are three roundings of at most 2^-24 relative each at |value| <= 2, below 2^-22 together: less than 2^-21 in all."""
import numpy as np
import pytest
import torch

import cover_ref as ref
from temporalalignnet_amd import _lib
from test_moments_gpu import DT, FORMATS, _dev, _ops, _stored
from test_retrieve_fp8_gpu import ACC_EPS, _deq, _int_codes
from test_retrieve_gpu import EPS, _exact_rows, _gen, _unit_rows
from test_sequences_gpu import N, NV, V_OFF, _all_pairs, _exact_case, _s_off, _scores, _unit_case
from test_shards_gpu import _pinned

pytestmark = pytest.mark.gpu

SETS = {1: [31], 4: [1, 64, 65, 32], 3: [200, 33, 129]}             # n_set -> m per set: one tile, a tile edge, four tiles with a tail
KS = (1, 10, 32)


def _srch():
    from temporalalignnet_amd import search
    return search


def _exact(fmt, Qt, n, seed, negative=False):
    """test_sequences_gpu._exact_case for any number of index rows: tq, vn, scale keywords, X int64 [Qt, n] with score * mult == X.
    negative: queries -|rows|, index |rows|: every score is below zero."""
    if fmt != "e4m3":
        tq, vn = _exact_rows(Qt, 900 + seed, DT[fmt]), _exact_rows(n, 950 + seed, DT[fmt])
        if negative:
            tq, vn = -tq.abs(), vn.abs()
        X = ((tq.double() * 16) @ (vn.double() * 16).T).round().long().cpu().numpy()
        kw, mult = {}, 256
    else:
        xq = torch.randint(-16, 17, (Qt, 512), generator=_gen(900 + seed), device="cuda")
        xv = torch.randint(-8, 9, (n, 512), generator=_gen(950 + seed), device="cuda")
        if negative:
            xq, xv = -xq.abs(), xv.abs()
        eq = torch.randint(-9, -7, (Qt,), generator=_gen(7), device="cuda")
        ev = torch.randint(-8, -6, (n,), generator=_gen(8), device="cuda")
        I = (xq.double() @ xv.double().T).round().long()            # score = 256 I 2^(ev + eq); x 512 = I 2^(17 + ev + eq)
        X = (I * (torch.ones_like(I) << (17 + ev[None, :] + eq[:, None]))).cpu().numpy()
        kw = dict(q_scale=torch.ldexp(torch.ones(Qt, device="cuda"), eq), v_scale=torch.ldexp(torch.ones(n, device="cuda"), ev))
        tq, vn, mult = _int_codes(xq), _int_codes(xv), 512
    assert int(np.abs(X).max()) < 2 ** 24                           # every score is exact in f32
    if negative:
        assert X.max() < 0
    return tq, vn, kw, X, mult


def _check(tq, vn, kw, q_off, v_off, fwd_w, bwd_w, ks=KS, what=""):
    """every rank and k: fwd, bwd and the three lists against the reference's, with =="""
    ops = _ops()
    for rank in ref.RANKS:
        want = ref.score(fwd_w, bwd_w, rank)
        for k in ks:
            k = min(k, len(v_off) - 1)
            top_s, top_r, top_v, fwd, bwd = ops.cover_topk(tq, vn, _dev(q_off), _dev(v_off), k, rank=rank, check_offsets=True, **kw)
            assert np.array_equal(fwd.cpu().numpy().view(np.int32), fwd_w.view(np.int32)), (what, rank, k, "fwd")
            assert np.array_equal(bwd.cpu().numpy().view(np.int32), bwd_w.view(np.int32)), (what, rank, k, "bwd")
            want_s, want_r, want_v = ref.topk(want, v_off, k)
            assert np.array_equal(top_v.cpu().numpy(), want_v), (what, rank, k)
            assert np.array_equal(top_r.cpu().numpy(), want_r), (what, rank, k)
            assert np.array_equal(top_s.cpu().numpy().view(np.int32), want_s.view(np.int32)), (what, rank, k)


# ------------------------------------------------------------------------------------------------------------- 1. exact arithmetic
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n_set", sorted(SETS))
def test_cover_topk_exact_arithmetic(n_set, fmt):
    ms = SETS[n_set]
    tq, vn, kw, X, mult = _exact_case(fmt, ms)
    q_off = _s_off(ms)
    fwd_w, bwd_w = ref.cover(X, q_off, V_OFF, int(mult))
    _check(tq, vn, kw, q_off, V_OFF, fwd_w, bwd_w)


# ---------------------------------------------------------------------------------------------------------- 2. all-negative scores
@pytest.mark.parametrize("fmt", FORMATS)
def test_all_negative_scores(fmt):
    """Every tile of these sets ends in zero-filled rows (m = 1, 63, 65), and 0 beats every real score: it must not enter b_t, and no
    tail row may reach the row maxima.  The videos of 127 and 129 rows end in repeated tail columns."""
    ms, lens = [1, 63, 65], [1, 127, 129]
    q_off, v_off = _s_off(ms), _s_off(lens)
    tq, vn, kw, X, mult = _exact(fmt, sum(ms), sum(lens), 1, negative=True)
    fwd_w, bwd_w = ref.cover(X, q_off, v_off, mult)
    assert (fwd_w < 0).all() and (bwd_w < 0).all()
    _check(tq, vn, kw, q_off, v_off, fwd_w, bwd_w, ks=(1, 3))
    _, _, _, fwd, bwd = _ops().cover_topk(tq, vn, _dev(q_off), _dev(v_off), 3, **kw)
    assert bool((fwd < 0).all()) and bool((bwd < 0).all())


# --------------------------------------------------------------------------------------------------------------------- 3. slabs
@pytest.mark.parametrize("fmt", FORMATS)
def test_videos_of_several_slabs(fmt):
    """401 = 3 x 128 + 17 and 1025 = 8 x 128 + 1 rows next to one-row videos; the second set is shorter than the first, so a row
    maximum left over from it would show."""
    ms, lens = [130, 7], [401, 1, 1025, 1]
    q_off, v_off = _s_off(ms), _s_off(lens)
    tq, vn, kw, X, mult = _exact(fmt, sum(ms), sum(lens), 2)
    fwd_w, bwd_w = ref.cover(X, q_off, v_off, mult)
    _check(tq, vn, kw, q_off, v_off, fwd_w, bwd_w, ks=(1, 4))
    # the second set alone gives its row of the two-set call
    _, _, _, fwd, bwd = _ops().cover_topk(tq[130:].contiguous(), vn, _dev([0, 7]), _dev(v_off), 1,
                                          **({k: (v[130:].contiguous() if k == "q_scale" else v) for k, v in kw.items()}))
    assert np.array_equal(fwd.cpu().numpy(), fwd_w[1:]) and np.array_equal(bwd.cpu().numpy(), bwd_w[1:])


# ------------------------------------------------------------------------------------------------------------ 4. random unit rows
@pytest.mark.parametrize("fmt", FORMATS)
def test_cover_topk_random_unit_rows(fmt):
    srch = _srch()
    ms = SETS[3]
    q_off = _s_off(ms)
    tq, vn, kw, S, _ = _unit_case(fmt, ms)
    if fmt == "e4m3":
        a, b = _deq(tq, kw["q_scale"]), _deq(vn, kw["v_scale"])
        eps = (ACC_EPS * (a.abs() @ b.abs().T)).cpu().numpy()       # per score
    else:
        eps = np.full(tuple(S.shape), EPS)
    S = S.cpu().numpy()
    # the device's own scores for all pairs: the sets as 32-row pieces through tan_sequence_scores
    s_off, first = srch.piece_offsets(ms)
    hits = _all_pairs(len(s_off) - 1, NV)
    x, hm, hv, x_off = _scores(tq, vn, kw, s_off, V_OFF, hits)
    xs = x.cpu().numpy()
    X = np.empty((sum(ms), N), dtype=np.float32)
    for h, (j, v) in enumerate(hits):
        X[s_off[j]:s_off[j + 1], V_OFF[v]:V_OFF[v + 1]] = xs[x_off[h]:x_off[h] + hm[h] * hv[h]].reshape(hm[h], hv[h])
    assert np.abs(X - S).max() <= eps.max()
    fwd_w, bwd_w = ref.cover(X, q_off, V_OFF)
    _check(tq, vn, kw, q_off, V_OFF, fwd_w, bwd_w, what=fmt)
    worst = 0.0
    for p in range(len(ms)):
        for v in range(NV):
            blk = S[q_off[p]:q_off[p + 1], V_OFF[v]:V_OFF[v + 1]]
            bound = eps[q_off[p]:q_off[p + 1], V_OFF[v]:V_OFF[v + 1]].max() + 2.0 ** -21
            ef, eb = abs(float(fwd_w[p, v]) - blk.max(1).mean()), abs(float(bwd_w[p, v]) - blk.max(0).mean())
            worst = max(worst, ef, eb)
            assert ef <= bound and eb <= bound, (p, v, ef, eb, bound)
    print(f"cover_topk {fmt}: largest |fwd or bwd - fp64 Chamfer mean| = {worst:.3e}")


# --------------------------------------------------------------------------------------------------------------------- 5. ties
@pytest.mark.parametrize("fmt", FORMATS)
def test_identical_videos_tie_and_the_lower_row_comes_first(fmt):
    ops = _ops()
    ms = [5, 70]
    rows = _unit_rows(200, 41, torch.float32)
    tq, vn, kw, _, _ = _stored(fmt, _unit_rows(sum(ms), 42, torch.float32), torch.cat((rows, rows)))
    for rank in ref.RANKS:
        top_s, top_r, top_v, fwd, bwd = ops.cover_topk(tq, vn, _dev(_s_off(ms)), _dev([0, 200, 400]), 2, rank=rank, **kw)
        assert top_v.tolist() == [[0, 1]] * 2 and top_r.tolist() == [[0, 200]] * 2 and torch.equal(top_s[:, 0], top_s[:, 1]), rank
        assert torch.equal(fwd[:, 0], fwd[:, 1]) and torch.equal(bwd[:, 0], bwd[:, 1])


# ---------------------------------------------------------------------------------------------------------------- 6. the limit
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_set_of_4096_rows_and_none_of_4097(fmt):
    ops = _ops()
    lens = [1, 129, 401]
    v_off = _s_off(lens)
    tq, vn, kw, X, mult = _exact(fmt, 4097, sum(lens), 3)
    cut = {k: (v[:4096].contiguous() if k == "q_scale" else v) for k, v in kw.items()}
    fwd_w, bwd_w = ref.cover(X[:4096], np.array([0, 4096]), v_off, mult)
    _check(tq[:4096].contiguous(), vn, cut, np.array([0, 4096]), v_off, fwd_w, bwd_w, ks=(3,))
    # 4097: refused by the wrapper and by the entry point, and nothing is written
    out = tuple(torch.full((1, 3), 7, dtype=dt, device="cuda") for dt in (torch.float32, torch.int32, torch.int32, torch.float32, torch.float32))
    with pytest.raises(ValueError):
        ops.cover_topk(tq, vn, _dev([0, 4097]), _dev(v_off), 3, out=out, **kw)
    L, p = _lib.lib(), lambda t: t.data_ptr()                       # noqa: E731
    q_off, v_dev = _dev([0, 4097]), _dev(v_off)
    tail = (4097, sum(lens), 512, p(q_off), 1, p(v_dev), 3, 2, 3, p(out[3]), p(out[4]), p(out[0]), p(out[1]), p(out[2]), None)
    if fmt == "e4m3":
        assert L.tan_cover_topk_e4m3(p(tq), p(kw["q_scale"]), p(vn), p(kw["v_scale"]), *tail) == -1
    else:
        assert L.tan_cover_topk(p(tq), p(vn), 0 if fmt == "f32" else 1, *tail) == -1
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out)


# ------------------------------------------------------------------------------------------------ 7. determinism and footprint
@pytest.mark.parametrize("fmt", FORMATS)
def test_outputs_are_reproducible_and_nothing_else_is_written(fmt):
    ops = _ops()
    ms, k = SETS[4], 10
    tq, vn, kw, _, _ = _unit_case(fmt, ms, seed=5)
    ns, G = len(ms), 64
    shapes = [(ns, k)] * 3 + [(ns, NV)] * 2
    runs = []
    for dirty in (0x7fc00001, -559038737):                          # a NaN pattern, then another: the outputs start dirty
        bufs = [torch.full((G + a * b + G,), dirty, dtype=torch.int32, device="cuda") for a, b in shapes]
        out = tuple(buf[G:-G].view(torch.float32 if i in (0, 3, 4) else torch.int32).view(a, b)
                    for i, (buf, (a, b)) in enumerate(zip(bufs, shapes)))
        got = ops.cover_topk(tq, vn, _dev(_s_off(ms)), _dev(V_OFF), k, out=out, **kw)
        assert all(g is o for g, o in zip(got, out))
        torch.cuda.synchronize()
        for buf in bufs:
            assert bool((buf[:G] == dirty).all()) and bool((buf[-G:] == dirty).all())
        runs.append([buf[G:-G].clone() for buf in bufs])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert bool(torch.isfinite(runs[0][3].view(torch.float32)).all()) and bool(torch.isfinite(runs[0][4].view(torch.float32)).all())


# --------------------------------------------------------------------------------------------------- 8. search_cover end to end
def _corpus(fmt):
    """Three shards of an index made from tensors.  Video 0 (70 s) is the query.  Video 5 (90 s) holds its seconds SHUFFLED, with
    noise, among 20 unrelated ones; video 6 (300 s) is a compilation that contains it whole and in order; video 7 (15 s) is a
    noisy excerpt of its seconds 20..34."""
    srch, ops = _srch(), _ops()
    lens = [70, 40, 150, 64, 12, 90, 300, 15]
    v_off = _s_off(lens)
    feat = _unit_rows(int(v_off[-1]), 71, torch.float32)
    q = feat[:70].clone()
    perm = torch.randperm(70, generator=torch.Generator().manual_seed(3)).cuda()
    assert not bool((perm[:32] == torch.arange(32, device="cuda")).all())
    noisy = lambda r, seed: torch.nn.functional.normalize(r + 0.3 * _unit_rows(r.shape[0], seed, torch.float32), dim=1)   # noqa: E731
    feat[v_off[5] + 10:v_off[5] + 80] = noisy(q[perm], 72)
    feat[v_off[6] + 100:v_off[6] + 170] = q
    feat[v_off[7]:v_off[8]] = noisy(q[20:35], 73)
    scale = None
    if fmt == "e4m3":
        feat, scale = ops.quantize_rows_e4m3(feat)
    elif fmt == "bf16":
        feat = feat.bfloat16()
    parts = []
    for a, b in ((0, 3), (3, 6), (6, 8)):
        r0, r1 = int(v_off[a]), int(v_off[b])
        parts.append(srch.VideoIndex(feat[r0:r1].contiguous(), v_off[a:b + 1] - r0, [f"v{i:03d}" for i in range(a, b)],
                                     None if scale is None else scale[r0:r1].contiguous()))
    return parts


@pytest.mark.parametrize("fmt", ("bf16", "e4m3"))
def test_search_cover_end_to_end(fmt, tmp_path, capsys):
    srch = _srch()
    parts = _corpus(fmt)
    idx = srch.VideoIndex.concat(parts)
    both = srch.search_cover(idx, ["v000"], k=5)[0]
    assert len(both) == 5 and all(isinstance(h, srch.CoverHit) for h in both) and len({h.vid for h in both}) == 5
    assert [h.score for h in both] == sorted((h.score for h in both), reverse=True)
    assert both[0].vid == "v000" and both[0].forward > 0.95 and both[0].backward > 0.95      # the query itself
    assert all(h.score == np.float32(np.float32(h.forward) + np.float32(h.backward)) * np.float32(0.5) for h in both)
    assert both[1].vid == "v005"                                    # the shuffled copy: most of either video is in the other
    # a second-for-second sweep of the query's first 32 seconds prefers the in-order compilation to the shuffled copy
    clips = srch.search_clips(idx, [("v000", 0, 31)], k=3, exclude_source=True)[0]
    assert clips[0].vid == "v006" and clips[0].vid != "v005"
    other = {rank: srch.search_cover(idx, [(0, 0, 69)], k=4, rank=rank, exclude_source=True)[0] for rank in ref.RANKS}
    assert all(h.vid != "v000" for hits in other.values() for h in hits) and all(len(hits) == 4 for hits in other.values())
    assert other["both"] == both[1:]                                # exclude_source: the same list without the source
    assert other["both"][0].vid == "v005"
    assert other["query"][0].vid == "v006" and other["query"][0].forward > 0.99          # all of the query is in the compilation
    assert other["video"][0].vid == "v007" and other["video"][0].backward > 0.9           # all of the excerpt is in the query
    assert [h.score for h in other["query"]] == [h.forward for h in other["query"]]
    assert [h.score for h in other["video"]] == [h.backward for h in other["video"]]
    # the same rows as a tensor: the same hits; a tensor has no source to leave out
    rows = srch.video._index_rows(idx, 0, 70, idx.device)
    assert srch.search_cover(idx, [rows], k=5)[0] == both
    assert srch.search_cover(idx, [rows], k=4, exclude_source=True)[0] == both[:4]
    assert srch.search_cover(idx, ["v000"], k=50)[0][:5] == both and len(srch.search_cover(idx, ["v000"], k=50)[0]) == 8
    # three shards, device- and host-resident: VideoIndex.concat's hits
    queries = ["v000", ("v006", 90, 200), rows[:33], 7, ("v002", 5, 5)]
    for resident in ("device", "host"):
        sharded = srch.ShardedIndex(parts, resident="device") if resident == "device" else srch.ShardedIndex(_pinned(parts), resident="host")
        for k, kw in ((8, {}), (1, {}), (3, dict(exclude_source=True)), (5, dict(rank="query")), (5, dict(rank="video", exclude_source=True))):
            want = srch.search_cover(idx, queries, k=k, **kw)
            assert srch.search_cover(sharded, queries, k=k, **kw) == want, (resident, k, kw)
            assert [len(h) for h in want] == [k] * len(queries)
    # the command line: no checkpoint, no model; the source is left out unless --keep-source
    path = str(tmp_path / "index.npz")
    idx.save(path)
    capsys.readouterr()
    assert srch.main(["similar", "--index", path, "--clip", "v000:0-69", "--cover", "-k", "3"]) == 0
    out = [line.split("\t") for line in capsys.readouterr().out.splitlines()]
    assert out == [[h.vid, f"{h.score:.6f}", f"{h.forward:.6f}", f"{h.backward:.6f}"] for h in both[1:4]]
    assert srch.main(["similar", "--index", path, "--clip", "v000:0-69", "--cover", "--rank", "video", "-k", "2", "--keep-source"]) == 0
    out = [line.split("\t") for line in capsys.readouterr().out.splitlines()]
    assert [o[0] for o in out] == [h.vid for h in srch.search_cover(idx, [("v000", 0, 69)], k=2, rank="video")[0]]
    assert srch.main(["similar", "--index", path, "--clip", "nobody:0-3", "--cover"]) == 2 and "nobody" in capsys.readouterr().err
    torch.cuda.synchronize()
