"""GPU retrieval: tan_rank_topk (matrix-free rank / top-k), tan_segment_pool_*, tan_window_feat_*, `test_retrieval_batched`,
`search.build_index` / `search.search`.

Two kinds of input make the rank tests exact without leaving a case out:
  * exact-arithmetic inputs: entries are multiples of 1/16 in [-1, 1] (exact in bf16 and f32); every product is a multiple of 1/256
    and a sum of 512 of them stays below 2^9: 17 bits, exact in f32 in any summation order.  The reference is the integer dot product
    of the entries x 16 (evaluated in fp64 on the device, where integers below 2^53 are exact, and converted to int64); counts, ties,
    top-k scores, rows and tie order are compared with `==`.
  * random unit rows: errors are bounded.  With EPS the bound on a score's error: the i-th returned score is within EPS of the i-th
    largest fp64 score; every returned row's fp64 score is at least the k-th largest minus 2 EPS; #(s > d + 2 EPS) <= higher and
    higher + ties <= #(s >= d - 2 EPS) with d the pair's fp64 score.  fp64 references use the same (bf16: bf16-rounded) inputs.
EPS = 2e-5 absolute, the bound the project uses for f32 cosines (test_hip_retrieval_matches_reference_golden, atol=2e-5); the
worst case for 512 products of unit vectors accumulated in f32 is about 512 * 2^-24 = 3e-5.  `test_rank_topk_random_unit_rows`
prints the largest |score - fp64| of every shape before it asserts; the maximum has not been recorded on an MI355X yet (no device
was available when this file was written).  If it exceeds 1e-5, EPS becomes twice the measured maximum, written next to the constant."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from temporalalignnet_amd import _lib, synth

pytestmark = pytest.mark.gpu

EPS = 2e-5
QS, NS, KS = (1, 7, 64, 130), (1, 63, 64, 4097, 200003), (0, 1, 10, 32)
DTYPES = (torch.float32, torch.bfloat16)
KEYS = ("R1", "R5", "R10", "MR", "C-R1", "C-R5", "C-R10", "C-MR", "S-R1", "S-R5", "S-R10", "S-MR")


def _ops():
    from temporalalignnet_amd import ops
    return ops


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _exact_rows(n, seed, dtype):
    return (torch.randint(-16, 17, (n, 512), generator=_gen(seed), device="cuda").float() / 16).to(dtype)


def _unit_rows(n, seed, dtype):
    x = torch.randn(n, 512, generator=_gen(seed), device="cuda")
    return (x / x.norm(dim=-1, keepdim=True)).to(dtype)


def _pairs(Q, N, seed):
    p = torch.randint(0, N, (Q,), generator=_gen(seed), device="cuda").int()
    p[0] = N - 1
    p[-1] = 0
    return p


def _cases(Q, N):
    for k, with_pair in itertools.product(KS, (True, False)):
        if k <= N and (k > 0 or with_pair):           # k == 0 without pair asks for nothing: TAN_ERR_BAD_ARG (test below)
            yield k, with_pair


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("Q", QS)
def test_rank_topk_exact_arithmetic(Q, N, dtype):
    ops = _ops()
    tq, vn = _exact_rows(Q, 100 + Q, dtype), _exact_rows(N, 200 + N % 1000, dtype)
    vn[N // 2] = vn[0]                                 # on top of the natural ties
    S = ((tq.double() * 16) @ (vn.double() * 16).T).round().long()          # int64, 256 x the score
    order = torch.sort(S, dim=1, descending=True, stable=True).indices       # equal scores by ascending row
    pair = _pairs(Q, N, 7)
    d = S.gather(1, pair.long()[:, None])
    for k, with_pair in _cases(Q, N):
        higher, ties, top_s, top_r = ops.rank_topk(tq, vn, pair if with_pair else None, k, check_pair=True)
        if with_pair:
            assert torch.equal(higher.long(), (S > d).sum(1)) and torch.equal(ties.long(), (S == d).sum(1)), (k, with_pair)
            assert int(ties.min()) >= 1
        else:
            assert higher is None and ties is None
        if k:
            assert torch.equal(top_r.long(), order[:, :k]), (k, with_pair)
            assert torch.equal(top_s.double() * 256, S.gather(1, order[:, :k]).double()), (k, with_pair)
        else:
            assert top_s is None and top_r is None


def _bounded_checks(S, pair, k, higher, ties, top_s, top_r, eps=EPS):
    """S: fp64 scores [Q, N].  Returns the largest |returned score - fp64 score of the returned row| (for the record)."""
    err = 0.0
    if pair is not None:
        d = S.gather(1, pair.long()[:, None])
        assert ((S > d + 2 * eps).sum(1) <= higher.long()).all()
        assert (higher.long() + ties.long() <= (S >= d - 2 * eps).sum(1)).all()
        assert int(ties.min()) >= 1
    if k:
        best = torch.topk(S, k, dim=1).values
        assert ((top_s.double() - best).abs() <= eps).all()
        got = S.gather(1, top_r.long())
        assert (got >= best[:, -1:] - 2 * eps).all()
        assert all(len(set(r)) == k for r in top_r.tolist())                 # k different rows
        err = float((top_s.double() - got).abs().max())
    return err


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("Q", QS)
def test_rank_topk_random_unit_rows(Q, N, dtype):
    ops = _ops()
    tq, vn = _unit_rows(Q, 300 + Q, dtype), _unit_rows(N, 400 + N % 1000, dtype)
    S = tq.double() @ vn.double().T
    pair = _pairs(Q, N, 9)
    worst = 0.0
    for k, with_pair in _cases(Q, N):
        p = pair if with_pair else None
        higher, ties, top_s, top_r = ops.rank_topk(tq, vn, p, k)
        worst = max(worst, _bounded_checks(S, p, k, higher, ties, top_s, top_r))
    print(f"rank_topk max |score - fp64| Q={Q} N={N} {dtype}: {worst:.3e}")
    assert worst <= EPS


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
def test_constructed_ties_across_tiles_and_splits(dtype):
    ops = _ops()
    Q, N = 7, 200003
    tq, vn = _unit_rows(Q, 1, dtype), _unit_rows(N, 2, dtype)
    a, b, c = 5, 64 * 700 + 33, N - 4                  # different rows of a tile, different tiles, different splits
    vn[a] = tq[0]                                      # query 0's best match by far (cosine 1)
    vn[b] = vn[a]
    vn[c] = vn[a]
    for paired in (a, b, c):
        pair = torch.full((Q,), paired, dtype=torch.int32, device="cuda")
        for splits in (0, 1, 3, 200):
            higher, ties, top_s, top_r = ops.rank_topk(tq, vn, pair, 10, splits=splits)
            assert ties.tolist() == [3] * Q, (paired, splits, ties.tolist())
            assert higher[0].item() == 0
            assert top_r[0, :3].tolist() == [a, b, c]
            assert top_s[0, 0].item() == top_s[0, 1].item() == top_s[0, 2].item()
            for q in range(1, Q):                      # wherever the three land in another query's list they are adjacent, ascending
                rows = top_r[q].tolist()
                hit = [i for i, r in enumerate(rows) if r in (a, b, c)]
                if len(hit) == 3:
                    assert hit[2] - hit[0] == 2 and [rows[i] for i in hit] == [a, b, c]


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
def test_rank_topk_is_deterministic_and_split_invariant(dtype):
    ops = _ops()
    for Q, N, k in ((130, 4097, 32), (64, 200003, 10), (7, 63, 10)):
        tq, vn = _unit_rows(Q, 21, dtype), _unit_rows(N, 22, dtype)
        vn[N // 3] = vn[N // 7]
        pair = _pairs(Q, N, 5)
        ref = ops.rank_topk(tq, vn, pair, k)
        for splits in (0, 1, 2, 5, 64, 256, 1000):
            got = ops.rank_topk(tq, vn, pair, k, splits=splits)
            for x, y in zip(ref, got):
                assert torch.equal(x, y), (Q, N, k, splits)


def test_rank_topk_writes_every_output_and_nothing_else():
    ops = _ops()
    G = 64                                             # guard elements after every buffer
    for dtype in DTYPES:
        for Q, N, k in ((7, 63, 10), (130, 4097, 32), (1, 1, 1), (64, 200003, 0)):
            tq, vn = _unit_rows(Q, 31, dtype), _unit_rows(N, 32, dtype)
            pair = _pairs(Q, N, 3)
            higher = torch.full((Q + G,), -777, dtype=torch.int32, device="cuda")
            ties = torch.full((Q + G,), -777, dtype=torch.int32, device="cuda")
            top_s = torch.full((Q * k + G,), float("nan"), device="cuda")
            top_r = torch.full((Q * k + G,), -777, dtype=torch.int32, device="cuda")
            nws = ops.rank_topk_ws_bytes(Q, N, k)
            ws = torch.full((nws + G,), 0xFF, dtype=torch.uint8, device="cuda")      # NaN / -1 patterns in the scratch
            out = (higher[:Q], ties[:Q], top_s[:Q * k].view(Q, k) if k else None, top_r[:Q * k].view(Q, k) if k else None)
            ops.rank_topk(tq, vn, pair, k, out=out, ws=ws[:nws])
            assert (higher[:Q] >= 0).all() and (ties[:Q] >= 1).all()
            assert (higher[Q:] == -777).all() and (ties[Q:] == -777).all() and (ws[nws:] == 0xFF).all()
            assert (top_r[Q * k:] == -777).all() and torch.isnan(top_s[Q * k:]).all()
            if k:
                assert torch.isfinite(top_s[:Q * k]).all() and ((top_r[:Q * k] >= 0) & (top_r[:Q * k] < N)).all()
                S = tq.double() @ vn.double().T
                _bounded_checks(S, pair, k, *out)


def test_rank_topk_rejects_invalid_arguments():
    ops = _ops()
    L = _lib.lib()
    tq, vn = _unit_rows(4, 1, torch.float32), _unit_rows(40, 2, torch.float32)
    pair = torch.zeros(4, dtype=torch.int32, device="cuda")
    hi, ti = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    ts, tr = torch.zeros(4, 40, device="cuda"), torch.zeros(4, 40, dtype=torch.int32, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                                            # noqa: E731

    def call(dtype=0, Q=4, N=40, Cc=512, pr=pair, k=10, splits=0, h=hi, t=ti, s=ts, r=tr, w=ws, a=tq, b=vn):
        f = lambda x: None if x is None else p(x)                                     # noqa: E731
        return L.tan_rank_topk(f(a), f(b), dtype, Q, N, Cc, f(pr), k, splits, f(h), f(t), f(s), f(r), f(w), None)

    assert call() == 0
    torch.cuda.synchronize()
    for kw in (dict(Cc=256), dict(Cc=1024), dict(k=33), dict(k=41, N=40), dict(k=-1), dict(Q=0), dict(N=0), dict(N=1 << 31), dict(dtype=2),
               dict(k=0, pr=None), dict(splits=-1), dict(h=None), dict(s=None), dict(r=None), dict(w=None), dict(a=None), dict(b=None)):
        assert call(**kw) == -1, kw
    with pytest.raises(_lib.TanHipError):
        ops.rank_topk(tq, vn, None, 0)
    with pytest.raises(ValueError):
        ops.rank_topk(tq, vn, torch.full((4,), 40, dtype=torch.int32, device="cuda"), 1, check_pair=True)
    with pytest.raises(_lib.TanHipError):
        ops.rank_topk(tq.cpu(), vn.cpu(), None, 1)


# ------------------------------------------------------------------------------------------------------------------- clip pooling
def _pool_ref(stage64, table, n_clips, normalize=True):
    """The host expression of test_retrieval (:197-214) in fp64: per frame normalise, mean over windows and frames, normalise."""
    out = torch.zeros(n_clips, 512, dtype=torch.float64)
    for c in range(n_clips):
        rows = [stage64[w, f0:f0 + nf] for w, (cc, f0, nf) in enumerate(table.tolist()) if cc == c]
        v = torch.stack(rows, 0)
        if normalize:
            v = v / v.norm(dim=-1, keepdim=True)
        v = v.mean(0).mean(0)
        out[c] = v / v.norm() if normalize else v
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
def test_segment_pool_matches_the_host_expression(dtype):
    ops = _ops()
    W, T, n_clips = 24, 48, 5
    stack = torch.randn(W, 3, T, 512, generator=_gen(5), device="cuda").to(dtype)      # a [W, S, T, C] stack: the stage is a view
    stage = stack[:, -1]
    # clip 0: whole windows; clip 1: one frame; clip 2: the last frame; clip 3: a middle segment; clip 4: one window only
    spec = {0: (0, T), 1: (17, 1), 2: (T - 1, 1), 3: (5, 30), 4: (2, 9)}
    clip_of = [0] * 6 + [1] * 5 + [2] * 4 + [3] * 8 + [4]
    table = torch.tensor([(c, *spec[c]) for c in clip_of], dtype=torch.int32)
    want = _pool_ref(stage.double().cpu(), table, n_clips)
    for cut in (W, 9, 13):                              # one call; cuts inside clip 1 / clip 3: a clip's windows split across calls
        acc, cnt = torch.zeros(n_clips, 512, device="cuda"), torch.zeros(n_clips, device="cuda")
        for a, b in ((0, cut), (cut, W)):
            if b > a:
                ops.segment_pool_acc(stage[a:b], table[a:b].cuda().contiguous(), acc, cnt)
        got = ops.segment_pool_final(acc, cnt, torch.full((n_clips, 512), float("nan"), device="cuda")).double().cpu()
        assert cnt.tolist() == [6.0 * T, 5.0, 4.0, 8 * 30.0, 9.0]
        if dtype == torch.float32:
            assert (got - want).abs().max().item() <= 1e-5
        else:       # the bf16 stage's own rounding (2^-8 relative per element) is in both; the check is the project's norm-relative one
            assert ((got - want).norm(dim=-1) / want.norm(dim=-1)).max().item() <= 1e-2
    # windows of one clip that are not neighbours in the table, and sim != 'cos' (no normalisation)
    perm = torch.randperm(W, generator=torch.Generator().manual_seed(1))
    acc, cnt = torch.zeros(n_clips, 512, device="cuda"), torch.zeros(n_clips, device="cuda")
    ops.segment_pool_acc(stage[perm.cuda()].contiguous(), table[perm].cuda().contiguous(), acc, cnt, normalize=False)
    got = ops.segment_pool_final(acc, cnt, torch.empty(n_clips, 512, device="cuda"), normalize=False).double().cpu()
    want = _pool_ref(stage.double().cpu(), table, n_clips, normalize=False)
    assert ((got - want).norm(dim=-1) / want.norm(dim=-1)).max().item() <= (1e-5 if dtype == torch.float32 else 1e-2)


# --------------------------------------------------------------------------------------------------------------- batched harness
def _model(E=2, D=1, compute_dtype="fp32", seed=113):
    from temporalalignnet_amd.tan_model import TemporalAligner
    m = TemporalAligner(num_encoder_layers=E, num_decoder_layers=D, use_alignability_head=0, language_model=None, random_pos_start=0,
                        compute_dtype=compute_dtype)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_params(seed, E, D, False).items()})
    return m.cuda().eval()


def _fixture_clips():
    fx = synth.yc2_fixture()
    feats = {vid: synth.yc2_features(vid, vlen) for vid, vlen in fx["videos"].items()}
    return [{"feature": feats[c["vid"]], "start": c["segment"][0], "end": c["segment"][1], "str": c["sentence"]} for c in fx["clips"]]


def _embed(strs):
    return torch.stack([torch.from_numpy(synth.yc2_text_embedding(s)) for s in strs])


def test_batched_retrieval_matches_reference_golden(golden):
    from temporalalignnet_amd import eval_retrieval
    g = golden("g12_retrieval")
    m = _model()
    for mw in (256, 16):
        metrics, sim = eval_retrieval.test_retrieval_batched(_fixture_clips(), m, _embed, seq_len=64, max_windows=mw, return_sim=True)
        np.testing.assert_allclose(sim, g["sim"], rtol=1e-3, atol=2e-5)
        for k in KEYS:
            assert float(metrics[k]) == pytest.approx(float(g[k]), abs=1e-12), k


def _synthetic_clips(n, seed=4):
    rng = np.random.default_rng(seed)
    vids = [np.abs(rng.standard_normal((int(v), 1024)) * 0.4 + rng.standard_normal((1, 1024)) * 0.5).astype(np.float32)
            for v in rng.integers(60, 400, 24)]
    clips = []
    for i in range(n):
        f = vids[i % len(vids)]
        s = int(rng.integers(0, f.shape[0] - 6))
        e = int(min(f.shape[0] - 1, s + rng.integers(3, 150)))
        clips.append({"feature": f, "start": s, "end": max(e, s + 2), "str": f"clip {i}"})
    return clips


def test_batched_retrieval_matches_the_per_clip_harness():
    from temporalalignnet_amd import eval_retrieval
    m = _model()
    clips = _synthetic_clips(300)
    n = len(clips)
    vis, txt = [], []

    # the per-clip harness's features: recomputed here with its own expression, from its own model calls
    for item in clips:
        feat = torch.as_tensor(item["feature"])
        idx, s_idx, e_idx = eval_retrieval.clip_windows(feat.shape[0], item["start"], item["end"], 10, -1)
        video = feat[torch.as_tensor(idx)].cuda()
        v = m.get_visual_feature(video, torch.zeros(video.shape[:2], device="cuda", dtype=torch.bool), interpolate_from=64 if video.shape[1] >= 64 else None)[:, -1]
        v = torch.stack([v[i, int(s_idx[i]):int(e_idx[i])] for i in range(v.shape[0])], 0).double()
        v = (v / v.norm(dim=-1, keepdim=True)).mean(0).mean(0)
        t = m.get_textual_feature(_embed([item["str"]]).cuda()).double().reshape(-1)
        vis.append((v / v.norm()).cpu())
        txt.append((t / t.norm()).cpu())
    V, T = torch.stack(vis), torch.stack(txt)
    ref = eval_retrieval.test_retrieval(clips, m.get_visual_feature, m.get_textual_feature, _embed, seq_len=64)
    metrics, (Vb, Tb) = eval_retrieval.test_retrieval_batched(clips, m, _embed, seq_len=64, return_features=True)
    assert (Vb.double().cpu() - V).abs().max().item() <= 1e-5
    assert (Tb.double().cpu() - T).abs().max().item() <= 1e-5
    # counts under the bounded rule against the fp64 matrix of the per-clip features
    from temporalalignnet_amd.eval_retrieval import metrics_from_counts
    S = T @ V.T
    d = S.diag()[:, None]
    lo, hi = (S > d + 2 * EPS).sum(1), (S >= d - 2 * EPS).sum(1)
    ops = _ops()
    higher, ties, _, _ = ops.rank_topk(Tb.contiguous(), Vb.contiguous(), torch.arange(n, dtype=torch.int32, device="cuda"), 0)
    assert (lo <= higher.cpu().long()).all() and (higher.cpu().long() + ties.cpu().long() <= hi).all()
    got = metrics_from_counts(higher.cpu().numpy(), ties.cpu().numpy())
    for k in ("R1", "R5", "R10", "MR"):
        assert float(got[k]) == float(metrics[k])
    if bool((lo == hi - 1).all()):                     # no score within 2 EPS of a diagonal entry: the ranking is unambiguous
        for k in ("R1", "R5", "R10", "MR"):
            assert float(metrics[k]) == float(ref[k]), k
    assert set(metrics) == set(ref) == set(KEYS)


def test_batched_retrieval_bf16_model():
    from temporalalignnet_amd import eval_retrieval
    clips = _synthetic_clips(120)
    _, (V32, T32) = eval_retrieval.test_retrieval_batched(clips, _model(), _embed, return_features=True)
    metrics, (V16, T16) = eval_retrieval.test_retrieval_batched(clips, _model(compute_dtype="bf16"), _embed, return_features=True)
    assert torch.isfinite(V16).all() and torch.isfinite(T16).all() and all(np.isfinite(float(metrics[k])) for k in KEYS)
    assert ((V16 - V32).norm(dim=-1) / V32.norm(dim=-1)).max().item() <= 2e-2
    assert ((T16 - T32).norm(dim=-1) / T32.norm(dim=-1)).max().item() <= 2e-2


# ---------------------------------------------------------------------------------------------------------------- index and search
def _videos(vlens, seed=8):
    rng = np.random.default_rng(seed)
    return [{"vid": f"v{i:03d}", "video": np.abs(rng.standard_normal((int(v), 1024)) * 0.4 + rng.standard_normal((1, 1024)) * 0.5)
             .astype(np.float32)} for i, v in enumerate(vlens)]


def test_index_is_the_stitched_dual_similarity():
    """<index[t], t_hat> / 0.07 == acc_d / cnt of the evaluation loop with every window holding the sentence.  The index averages
    unit vectors, the loop averages cosines: equal up to summation order -- 1e-5 absolute on the cosine."""
    from temporalalignnet_amd.search import build_index, plan_index_windows
    m = _model()
    vids = _videos([20, 31, 64, 130, 1200, 47, 333, 700, 90])       # shorter than a window; 1200 s alone is 74 windows
    sent = torch.randn(3, 512, generator=_gen(12), device="cuda")
    idx = build_index(m, vids, windows_per_pass=256, dtype=torch.float32)
    idx64 = build_index(m, vids, windows_per_pass=64, dtype=torch.float32)
    assert torch.equal(idx.feat, idx64.feat) and idx.v_off.tolist() == idx64.v_off.tolist()
    b16 = build_index(m, vids, windows_per_pass=256), build_index(m, vids, windows_per_pass=64)
    assert b16[0].feat.dtype == torch.bfloat16 and torch.equal(b16[0].feat, b16[1].feat)
    assert idx.vids == [v["vid"] for v in vids] and idx.v_off.tolist() == np.concatenate([[0], np.cumsum([len(v["video"]) for v in vids])]).tolist()
    t_hat = m.get_textual_feature(sent).double()
    t_hat = t_hat / t_hat.norm(dim=-1, keepdim=True)
    for i, v in enumerate(vids):
        video = torch.from_numpy(v["video"]).cuda()
        vlen = video.shape[0]
        acc, cnt = torch.zeros(3, vlen, dtype=torch.float64, device="cuda"), torch.zeros(vlen, dtype=torch.float64, device="cuda")
        for s0, e0 in plan_index_windows(vlen, 64):
            sim = m.get_text_visual_sim_dual(video[None, s0:e0], sent[None])[0, -1]           # [t, K] cosines, last stage
            acc[:, s0:e0] += sim.double().T / 0.07
            cnt[s0:e0] += 1
        want = acc / cnt
        rows = idx.feat[idx.v_off[i]:idx.v_off[i + 1]].double()
        got = (t_hat @ rows.T) * (1 / 0.07)
        assert (cnt >= 1).all()
        assert ((got - want).abs().max().item()) * 0.07 <= 1e-5, (i, vlen)


def test_search_finds_planted_seconds_at_video_boundaries(tmp_path):
    from temporalalignnet_amd.search import VideoIndex, build_index, query_features, search
    m = _model()
    vids = _videos([70, 33, 150, 64, 20], seed=9)
    for dtype in DTYPES:
        idx = build_index(m, vids, dtype=dtype)
        queries = [f"query {i}" for i in range(9)]
        tq = query_features(idx, m, _embed, queries)
        # plant: query 0's own direction at the LAST second of video 1, query 1's at the FIRST second of video 2, query 2's at
        # the last row of the index, query 3's at row 0
        off = idx.v_off
        planted = {0: (int(off[2]) - 1, "v001", 32), 1: (int(off[2]), "v002", 0), 2: (int(off[-1]) - 1, "v004", 19), 3: (0, "v000", 0)}
        for q, (row, _, _) in planted.items():
            idx.feat[row] = tq[q]
        res = search(idx, m, _embed, queries, k=10)
        S = tq.double() @ idx.feat.double().T
        best = torch.topk(S, 10, dim=1)
        for q, hits in enumerate(res):
            assert len(hits) == 10
            for i, (vid, sec, score) in enumerate(hits):
                assert abs(score - best.values[q, i].item()) <= EPS
                row = int(off[idx.vids.index(vid)]) + sec
                assert 0 <= sec < off[idx.vids.index(vid) + 1] - off[idx.vids.index(vid)]
                assert S[q, row].item() >= best.values[q, -1].item() - 2 * EPS
        for q, (row, vid, sec) in planted.items():
            assert res[q][0][:2] == (vid, sec), (q, res[q][0])
        p = str(tmp_path / "index.npz")
        idx.save(p)
        back = VideoIndex.load(p)
        assert torch.equal(back.feat, idx.feat) and back.vids == idx.vids
        assert search(back, m, _embed, queries, k=10) == res


def test_rank_topk_memory_stays_far_below_the_score_matrix():
    ops = _ops()
    Q, N, k = 2048, 2_000_000, 10
    vn = torch.empty(N, 512, dtype=torch.bfloat16, device="cuda")
    for a in range(0, N, 250_000):                     # random rows, made in slices to keep the generator's temporaries small
        vn[a:a + 250_000] = torch.randn(250_000, 512, generator=_gen(a), device="cuda").mul_(512 ** -0.5).to(torch.bfloat16)
    tq = _unit_rows(Q, 77, torch.bfloat16)
    pair = _pairs(Q, N, 1)
    ws_bytes = ops.rank_topk_ws_bytes(Q, N, k)
    out_bytes = Q * 4 * 2 + Q * k * 8
    # caller-owned scratch and outputs of exactly the documented sizes: the call itself must not allocate a byte
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = (torch.empty(Q, dtype=torch.int32, device="cuda"), torch.empty(Q, dtype=torch.int32, device="cuda"),
           torch.empty(Q, k, device="cuda"), torch.empty(Q, k, dtype=torch.int32, device="cuda"))
    assert ws.numel() + sum(t.numel() * t.element_size() for t in out) == ws_bytes + out_bytes
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ops.rank_topk(tq, vn, pair, k, out=out, ws=ws)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == base
    first = [t.clone() for t in out]
    del ws, out
    # the wrapper's own allocations: scratch + outputs, each rounded up by the caching allocator (512 bytes for a small block; a
    # large block is not split when less than 1 MiB of it would remain)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    higher, ties, top_s, top_r = ops.rank_topk(tq, vn, pair, k)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra <= ws_bytes + out_bytes + 4 * 512 + 2 ** 20, (extra, ws_bytes, out_bytes)
    assert all(torch.equal(x, y) for x, y in zip(first, (higher, ties, top_s, top_r)))
    assert ws_bytes + out_bytes < 64 * 2 ** 20
    assert int(ties.min()) >= 1 and torch.isfinite(top_s).all()
    # spot check a few queries against fp64 (a [8, N] slice, not the matrix)
    S = torch.cat([tq[:8].double() @ vn[a:a + 250_000].double().T for a in range(0, N, 250_000)], 1)
    _bounded_checks(S, pair[:8], k, higher[:8], ties[:8], top_s[:8], top_r[:8])
