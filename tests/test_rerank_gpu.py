"""Two-stage search on the GPU: tan_rerank_tail / tan_rerank_select alone, the stem store of `build_index(keep_stem=True)`,
`TemporalAligner.joint_from_stem`, `search.search_rerank` and the `index --keep-stem` / `query --rerank` command line.

Model: 1 encoder and 3 decoder layers with the alignability head, Dv = 16, random_pos_start off, fp32 and bf16 over the same weights.
Corpus: vlen = [1, 20, 33, 64, 65, 130, 203] (516 rows: videos shorter than, equal to and longer than a window); 5 queries.

Bounds.
  (2) A cosine of tan_rerank_tail against the fp64 cosine of the same stored rows (include/tan_hip.h): three 512-term f32
      accumulations, each within 512 * 2^-23 * sum |a_i b_i| (bound (a) of DESIGN 3.12); two square roots, a product and a division:
          |cos - cos64| <= 2^-23 * (512 * A + 516 * |cos64|),  A = sum_i |v_i q_i| / (|v| |q|) <= 1.
  (confidence) 1 / sum_f exp(x_f - x_max), x = cos / 0.07: every exponent is off by at most 2 e / 0.07 (e the largest bound (2) of the
      window) plus two f32 roundings of values below 16 (2 * 2^-20); expf and the <= 70 additions add 80 * 2^-24.  Relative:
          2 e / 0.07 + 2^-19 + 80 * 2^-24.
  (head) the bound tests/test_row_kernels_fp64_gpu.py uses for tan_head_fwd: (14 + 2) * 2^-24 * (|x| . |w| + |b|) -- the same chain
      length: 8 adds per lane, 6 wave levels, the bias.
  (5) against `eval_windows`, fp32 mode: rtol 1e-4, atol 2e-4 on sim / 0.07 and rtol 1e-4, atol 1e-5 on the head logit, the tolerances
      tests/test_infer_align_gpu.py applies to these quantities.
  (6) bf16 mode: max |rerank(bf16) - rerank(fp32)| <= 2 * max |eval_windows(bf16) - eval_windows(fp32)| on the same windows.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from temporalalignnet_amd import ops, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
T, KP, L = 64, 8, 72
VLENS = [1, 20, 33, 64, 65, 130, 203]
QUERIES = [f"rerank query {i}" for i in range(5)]
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
U23 = 2.0 ** -23


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _table(ts, s0s):
    tab = torch.zeros(len(ts), 8, dtype=torch.int32)
    tab[:, 1], tab[:, 3], tab[:, 4] = torch.tensor(ts), 1, torch.tensor(s0s)
    return tab.cuda()


def _tail(last, head, tab, w=None, b=None, sim=True):
    W = tab.shape[0]
    out = torch.full((W, 4), float("nan"), device="cuda")
    s = torch.full((W, T), float("nan"), device="cuda") if sim else None
    ops.rerank_tail(last.view(W * L, 512), None if head is None else head.view(W * L, 512), tab, T, w, b, out, s)
    return out, s


def _cos64(last, ts):
    """fp64 cosines [W, T] of the stored rows (NaN beyond t), and the per-element bound (2)."""
    x = last.double()
    v, q = x[:, :T], x[:, T:T + 1]
    nrm = v.norm(dim=-1) * q.norm(dim=-1)
    cos = (v * q).sum(-1) / nrm
    bound = U23 * (512 * (v * q).abs().sum(-1) / nrm + 516 * cos.abs())
    valid = torch.arange(T, device="cuda")[None] < torch.as_tensor(ts, device="cuda")[:, None]
    return torch.where(valid, cos, float("nan")), torch.where(valid, bound, 0.0), valid


# ---------------------------------------------------------------------------------------------------- 1. tan_rerank_tail, exact
def _exact_stage(W, seed, dtype):
    """Integer rows: every frame row of a window is a signed permutation of ONE vector, so all squared norms of the window are the
    same integer and the cosines order as the integer dot products do; the arg-max row is copied to a second frame (a tie)."""
    g = torch.Generator().manual_seed(seed)
    ts = [(1, 20, 64)[w % 3] for w in range(W)]
    base = torch.randint(-2, 3, (512,), generator=g).float()
    last = torch.full((W, L, 512), float("nan"))
    for w in range(W):
        for f in range(ts[w]):
            last[w, f] = base[torch.randperm(512, generator=g)] * (torch.randint(0, 2, (512,), generator=g) * 2 - 1)
    last[:, T] = torch.randint(-3, 4, (W, 512), generator=g).float()
    for w in range(W):
        if ts[w] > 1:
            d = last[w, :ts[w]] @ last[w, T]
            a = int(d.argmax())
            last[w, (a + 7) % ts[w]] = last[w, a]
    head = torch.full((W, L, 512), float("nan"))
    head[:, T] = torch.randint(-4, 5, (W, 512), generator=g).float()
    hw, hb = torch.randint(-8, 9, (512,), generator=g).float() / 16, torch.tensor([0.375])
    return last.to(dtype).cuda(), head.to(dtype).cuda(), hw.cuda(), hb.cuda(), ts


@pytest.mark.parametrize("fmt", ("f32", "bf16"))
@pytest.mark.parametrize("W", (1, 5, 67))
def test_rerank_tail_exact(W, fmt):
    last, head, hw, hb, ts = _exact_stage(W, 10 + W, DT[fmt])
    s0s = [3 * w + 1 for w in range(W)]
    tab = _table(ts, s0s)
    out, sim = _tail(last, head, tab, hw, hb)
    dots = (last[:, :T].double() * last[:, T:T + 1].double()).sum(-1).cpu().numpy()              # exact integers
    cos, bound, valid = _cos64(last, ts)
    n_ties = 0
    for w in range(W):
        d = dots[w, :ts[w]]
        first = int(np.argmax(d))                                                                 # numpy's first arg-max
        n_ties += int((d == d.max()).sum() > 1)
        assert out[w, 1:2].view(torch.int32).item() == s0s[w] + first, (w, ts[w])
        assert out[w, 0].item() == sim[w, first].item() == sim[w, :ts[w]].max().item()
        assert (sim[w, ts[w]:] == -float("inf")).all()
    assert n_ties >= (2 * W) // 3
    assert ((sim.double() - cos).abs()[valid] <= bound[valid]).all()
    want_head = (head[:, T].double() @ hw.double() + hb.double()).float()                         # exact: multiples of 1 / 16
    assert torch.equal(out[:, 3], want_head)
    conf = 1.0 / torch.where(valid, ((cos - torch.where(valid, cos, -2.0).amax(1, keepdim=True)) / 0.07).exp(), 0.0).sum(1)
    assert ((out[:, 2].double() - conf).abs() <= conf * (2 * bound.amax(1) / 0.07 + 2.0 ** -19 + 80 * 2.0 ** -24)).all()
    # no head: the fourth slot is 0, the rest unchanged; no sim: the same out
    out2, _ = _tail(last, None, tab, sim=False)
    assert torch.equal(out2[:, :3].view(torch.int32), out[:, :3].view(torch.int32)) and (out2[:, 3] == 0).all()
    # the same windows in another order, split over two calls: the same bits per window
    perm = torch.randperm(W, generator=torch.Generator().manual_seed(W)).cuda()
    cut = (2 * W) // 5
    got_o, got_s = torch.empty_like(out), torch.empty_like(sim)
    for part in (perm[:cut], perm[cut:]):
        if part.numel():
            o, s = _tail(last[part].contiguous(), head[part].contiguous(), tab[part].contiguous(), hw, hb)
            got_o[part], got_s[part] = o, s
    assert torch.equal(got_o.view(torch.int32), out.view(torch.int32)) and torch.equal(got_s, sim)


# ------------------------------------------------------------------------------------------- 2. tan_rerank_tail against fp64
@pytest.mark.parametrize("fmt", ("f32", "bf16"))
def test_rerank_tail_random_rows_fp64(fmt):
    W = 67
    ts = [(1, 20, 64, 33)[w % 4] for w in range(W)]
    g = _gen(21)
    last = (torch.randn(W, L, 512, generator=g, device="cuda") * (1 + torch.rand(W, L, 1, generator=g, device="cuda"))
            + 0.3 * torch.randn(W, 1, 512, generator=g, device="cuda")).to(DT[fmt])
    head = torch.randn(W, L, 512, generator=g, device="cuda").to(DT[fmt])
    hw, hb = torch.randn(512, generator=g, device="cuda") * 0.05, torch.randn(1, generator=g, device="cuda")
    tab = _table(ts, [0] * W)
    out, sim = _tail(last, head, tab, hw, hb)
    cos, bound, valid = _cos64(last, ts)
    frac = ((sim.double() - cos).abs()[valid] / bound[valid]).max().item()
    print(f"rerank_tail {fmt}: max |cos - fp64| / bound (2) = {frac:.4f} (bound <= {bound[valid].max().item():.3e})")
    assert frac <= 1.0
    assert (sim[~valid] == -float("inf")).all()
    cmax = torch.where(valid, cos, -2.0).amax(1)
    assert ((out[:, 0].double() - cmax).abs() <= bound.amax(1)).all()
    sec = out[:, 1].contiguous().view(torch.int32).long()
    assert ((sec >= 0) & (sec < torch.tensor(ts, device="cuda"))).all()
    assert (cos.gather(1, sec[:, None])[:, 0] >= cmax - 2 * bound.amax(1)).all()
    assert torch.equal(sec, torch.where(valid, sim, -float("inf")).argmax(1))                       # the first arg-max of its own cosines
    conf = 1.0 / torch.where(valid, ((cos - cmax[:, None]) / 0.07).exp(), 0.0).sum(1)
    cfrac = ((out[:, 2].double() - conf).abs() / (conf * (2 * bound.amax(1) / 0.07 + 2.0 ** -19 + 80 * 2.0 ** -24))).max().item()
    h64 = head[:, T].double() @ hw.double() + hb.double()
    hbound = 16 * 2.0 ** -24 * (head[:, T].double().abs() @ hw.double().abs() + hb.double().abs())
    hfrac = ((out[:, 3].double() - h64).abs() / hbound).max().item()
    print(f"rerank_tail {fmt}: confidence / bound = {cfrac:.4f}, head / bound = {hfrac:.4f}")
    assert cfrac <= 1.0 and hfrac <= 1.0


# ------------------------------------------------------------------------------------------------------- 3. tan_rerank_select
@pytest.mark.parametrize("P", (1, 7, 32))
def test_rerank_select_is_a_stable_sort(P):
    for Q in (1, 5, 130):
        g = torch.Generator().manual_seed(100 * P + Q)
        score = torch.randint(0, 5, (Q, P), generator=g).float() / 4 - 0.5                          # many equal scores
        score[0, :] = 0.25                                                                          # one query all tied
        want = np.argsort(-score.numpy(), axis=1, kind="stable")
        wide = torch.full((Q, P, 4), float("nan"))
        wide[:, :, 0] = score
        for k in sorted({1, min(3, P), P}):
            got = ops.rerank_select(score.cuda(), k)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want[:, :k]), (Q, P, k)
            assert torch.equal(ops.rerank_select(wide.cuda(), k, stride=4), got)


# ---------------------------------------------------------------------------------------------- the model, the corpus, the windows
_CACHE = {}


def _model(mode):
    if ("m", mode) not in _CACHE:
        from temporalalignnet_amd.tan_model import TemporalAligner
        m = TemporalAligner(1, 3, use_alignability_head=1, random_pos_start=0, language_model=None, compute_dtype=mode, d_video=16)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_params(77, 1, 3, True, d_video=16).items()})
        _CACHE["m", mode] = m.cuda().eval()
    return _CACHE["m", mode]


def _videos():
    rng = np.random.default_rng(5)
    return [{"vid": f"v{i}", "video": (rng.standard_normal((n, 16)) + rng.standard_normal((1, 16))).astype(np.float32)}
            for i, n in enumerate(VLENS)]


def _embed(strs):
    return torch.stack([torch.from_numpy(synth.yc2_text_embedding(s)) for s in strs]).cuda()


def _index(mode, dtype=torch.float32):
    key = ("idx", mode, str(dtype))
    if key not in _CACHE:
        from temporalalignnet_amd.search import build_index
        _CACHE[key] = build_index(_model(mode), _videos(), dtype=dtype, keep_stem=True)
    return _CACHE[key]


def _windows(moments, idx):
    """[(q, video number, s0, t)] in (query, dual rank) order from search_moments' lists."""
    from temporalalignnet_amd.search import rerank_window
    out = []
    for q, hits in enumerate(moments):
        for h in hits:
            v = idx.vids.index(h.vid)
            out.append((q, v, *rerank_window(h.second, int(idx.v_off[v + 1] - idx.v_off[v]), T)))
    return out


def _cut(rows, wins, idx, emb):
    """The torch slicing of a pass: rows [516, D] -> ([W, T, D] zero padded, vmask, text [W, 8, Dt], tmask)."""
    W = len(wins)
    x = torch.zeros(W, T, rows.shape[1], dtype=rows.dtype, device="cuda")
    vm = torch.ones(W, T, dtype=torch.bool, device="cuda")
    txt = torch.zeros(W, KP, emb.shape[1], device="cuda")
    tm = torch.ones(W, KP, dtype=torch.bool, device="cuda")
    for w, (q, v, s0, t) in enumerate(wins):
        a = int(idx.v_off[v]) + s0
        x[w, :t], vm[w, :t], txt[w, 0], tm[w, 0] = rows[a:a + t], False, emb[q], False
    return x, vm, txt, tm


def _stem_reference(mode, wins, idx, stem, per_pass=3):
    """`joint_from_stem` on host-cut stem windows, in passes of `per_pass` -> (last stage [W, L, 512] copy, head logits fp64 [W], their
    bound (head))."""
    m = _model(mode)
    emb = _embed(QUERIES)
    hw, hb = m._f("binary_head.weight").view(-1).double(), m._f("binary_head.bias").double()
    last, head = [], []
    for p0 in range(0, len(wins), per_pass):
        part = wins[p0:p0 + per_pass]
        ej = m.joint_from_stem(*_cut(stem, part, idx, emb))
        last.append(ej.stage(2).view(len(part), L, 512).clone())
        m._release_ws(ej)
    last = torch.cat(last)
    x = last[:, T].double()
    return last, x @ hw + hb, 16 * 2.0 ** -24 * (x.abs() @ hw.abs() + hb.abs())


def _reranked(mode, pool):
    """search_rerank(k = pool, windows_per_pass = 3, return_sim) next to its references, computed once per (mode, pool)."""
    key = ("rr", mode, pool)
    if key not in _CACHE:
        from temporalalignnet_amd.search import search_moments, search_rerank
        m, idx = _model(mode), _index(mode)
        kk = min(pool, len(VLENS))
        hits, sim = search_rerank(idx, m, _embed, QUERIES, k=kk, pool=pool, windows_per_pass=3, return_sim=True)
        moments = search_moments(idx, m, _embed, QUERIES, k=kk)
        wins = _windows(moments, idx)
        _CACHE[key] = dict(hits=hits, sim=sim, moments=moments, wins=wins, kk=kk)
    return _CACHE[key]


def _by_candidate(r):
    """hits re-indexed [q][dual rank] (videos are distinct within a list)."""
    return [[next(h for h in hs if h.vid == mo.vid) for mo in ms] for hs, ms in zip(r["hits"], r["moments"])]


# ------------------------------------------------------------------------------------------------ 4. stem and composition
def test_keep_stem_leaves_the_index_as_it_is():
    from temporalalignnet_amd.search import build_index
    m = _model("fp32")
    for dtype in (torch.float32, torch.bfloat16, "e4m3"):
        plain, kept = build_index(m, _videos(), dtype=dtype), build_index(m, _videos(), dtype=dtype, keep_stem=True)
        assert plain.stem is None and torch.equal(kept.feat, plain.feat) and kept.vids == plain.vids
        assert kept.v_off.tolist() == plain.v_off.tolist() and (plain.scale is None or torch.equal(kept.scale, plain.scale))
        assert kept.stem.shape == (sum(VLENS), 512) and kept.stem.dtype == torch.float32
    raw = torch.cat([torch.from_numpy(v["video"]) for v in _videos()]).cuda()
    want = raw.double() @ m._f("video_pre_proj.weight").double().T
    assert (kept.stem.double() - want).abs().max().item() <= 16 * 2.0 ** -23 * (raw.double().abs() @ m._f("video_pre_proj.weight").double().abs().T).max().item()
    assert torch.equal(kept.stem, m.video_stem(raw)) and kept.quantize().stem is kept.stem
    assert _index("bf16").stem.dtype == torch.bfloat16


@pytest.mark.parametrize("pool", (4, 32))
@pytest.mark.parametrize("mode", ("fp32", "bf16"))
def test_search_rerank_sim_is_the_joint_stack_on_host_cut_stem_windows(mode, pool):
    r, idx = _reranked(mode, pool), _index(mode)
    wins = r["wins"]
    assert r["kk"] == min(pool, 7) and r["sim"].shape == (5, r["kk"], T) and len(wins) == 5 * r["kk"] > 3 * 6
    last, head64, hbound = _stem_reference(mode, wins, idx, idx.stem)
    ts = [w[3] for w in wins]
    cos, bound, valid = _cos64(last, ts)
    sim = torch.from_numpy(r["sim"]).cuda().view(len(wins), T)
    frac = ((sim.double() - cos).abs()[valid] / bound[valid]).max().item()
    print(f"search_rerank {mode} pool={pool}: max |sim - fp64 of joint_from_stem| / bound (2) = {frac:.4f}")
    assert frac <= 1.0 and (sim[~valid] == -float("inf")).all()
    if pool == 32:                                                  # every video is a candidate: short windows, and clamped / moved ones
        assert {t for t in ts} >= {1, 20, 33, 64} and any(w[2] > 0 for w in wins)
    cand = _by_candidate(r)
    for w, (q, v, s0, t) in enumerate(wins):
        h = cand[q][w % r["kk"]]
        assert h.score == float(sim[w, :t].max()) and h.second == s0 + int(sim[w, :t].argmax())
        assert abs(h.alignability - head64[w].item()) <= hbound[w].item()
        assert 0 < h.confidence <= 1.0 + 1e-6


# ---------------------------------------------------------------------------------- 5. against the existing evaluation path, fp32
def _eval_windows_ref(mode, wins, idx):
    m = _model(mode)
    raw = torch.cat([torch.from_numpy(v["video"]) for v in _videos()]).cuda()
    r = m.eval_windows(*[t for t in _reorder(_cut(raw, wins, idx, _embed(QUERIES)))])
    return r["sim"][:, -1, :, 0].clone(), r["alignability-joint"][:, 2, 0, 0].clone()


def _reorder(cut):
    x, vm, txt, tm = cut
    return x, txt, vm, tm


def test_search_rerank_matches_eval_windows_fp32():
    r, idx = _reranked("fp32", 32), _index("fp32")
    wins = r["wins"]
    ref_sim, ref_head = _eval_windows_ref("fp32", wins, idx)
    sim = torch.from_numpy(r["sim"]).cuda().view(len(wins), T)
    cand = _by_candidate(r)
    worst = 0.0
    for w, (q, v, s0, t) in enumerate(wins):
        got, want = sim[w, :t] / 0.07, ref_sim[w, :t] / 0.07
        worst = max(worst, (got - want).abs().max().item())
        torch.testing.assert_close(got, want, rtol=1e-4, atol=2e-4)
        h = cand[q][w % r["kk"]]
        torch.testing.assert_close(torch.tensor(h.alignability), ref_head[w].cpu(), rtol=1e-4, atol=1e-5)
        top = torch.topk(want, min(2, t)).values
        if t == 1 or (top[0] - top[1]).item() > 2 * (2e-4 + 1e-4 * top[0].abs().item()):           # the maximum is not tied within the tolerance
            assert h.second == s0 + int(want.argmax()), (w, h)
    print(f"search_rerank fp32 vs eval_windows: max |sim / 0.07 difference| = {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------ 6. bf16 mode
def test_rerank_bf16_stays_within_twice_the_existing_paths_distance():
    r, idx32, idx16 = _reranked("fp32", 32), _index("fp32"), _index("bf16")
    wins = r["wins"]
    ts = [w[3] for w in wins]
    tab = _table(ts, [w[2] for w in wins])
    valid = torch.arange(T, device="cuda")[None] < torch.tensor(ts, device="cuda")[:, None]
    e32, _ = _eval_windows_ref("fp32", wins, idx32)
    e16, _ = _eval_windows_ref("bf16", wins, idx32)
    d_ref = (e16 - e32).abs()[valid].max().item()
    sims = {}
    for mode, idx in (("fp32", idx32), ("bf16", idx16)):
        last = _stem_reference(mode, wins, idx, idx.stem, per_pass=len(wins))[0]
        sims[mode] = _tail(last, None, tab)[1]
    d = (sims["bf16"] - sims["fp32"]).abs()[valid].max().item()
    print(f"bf16 vs fp32 cosines on {len(wins)} windows: rerank {d:.3e}, eval_windows {d_ref:.3e}")
    assert d <= 2 * d_ref


# ------------------------------------------------------------------------------------------------------------ 7. end to end
def _check_lists(hits, sim, moments, k):
    for q, (hs, ms) in enumerate(zip(hits, moments)):
        assert len(hs) == k
        peak = sim[q].max(axis=1)                                                                 # per candidate, dual rank order
        order = np.argsort(-peak, kind="stable")[:k]
        assert [h.vid for h in hs] == [ms[i].vid for i in order], q
        for h, i in zip(hs, order):
            assert (h.dual_second, h.dual_score) == (ms[i].second, ms[i].score) and h.score == float(peak[i])


@pytest.mark.parametrize("pool", (4, 32))
def test_search_rerank_reorders_search_moments_candidates(pool):
    from temporalalignnet_amd.search import Reranked, search_rerank
    r, m, idx = _reranked("fp32", pool), _model("fp32"), _index("fp32")
    assert all(isinstance(h, Reranked) for hs in r["hits"] for h in hs)
    _check_lists(r["hits"], r["sim"], r["moments"], r["kk"])
    for hs, ms in zip(r["hits"], r["moments"]):
        assert sorted((h.vid, h.dual_second, h.dual_score) for h in hs) == sorted((mo.vid, mo.second, mo.score) for mo in ms)
    few = search_rerank(idx, m, _embed, QUERIES, k=2, pool=pool, windows_per_pass=3)             # k < pool, no sim: the same launches
    assert few == [hs[:2] for hs in r["hits"]]
    one = search_rerank(idx, m, _embed, QUERIES, k=r["kk"], pool=pool)                            # all windows in one pass
    for hs, ms in zip(one, r["moments"]):
        assert sorted(h.vid for h in hs) == sorted(mo.vid for mo in ms) and [h.score for h in hs] == sorted((h.score for h in hs), reverse=True)
    assert search_rerank(idx, m, _embed, [], k=2, pool=pool) == []


def test_search_rerank_over_an_e4m3_index_and_the_refusals():
    from temporalalignnet_amd.search import VideoIndex, search_moments, search_rerank
    from temporalalignnet_amd.tan_model import TemporalAligner
    m = _model("fp32")
    idx = _index("fp32", "e4m3")
    assert idx.e4m3 and idx.stem is not None
    hits, sim = search_rerank(idx, m, _embed, QUERIES, k=7, pool=32, windows_per_pass=3, return_sim=True)
    _check_lists(hits, sim, search_moments(idx, m, _embed, QUERIES, k=7), 7)
    assert all(-1.0 <= h.score <= 1.0 and isinstance(h.alignability, float) for hs in hits for h in hs)
    with pytest.raises(ValueError):
        search_rerank(VideoIndex(idx.feat, idx.v_off, idx.vids, idx.scale), m, _embed, QUERIES)
    for bad in (dict(pool=0), dict(k=0), dict(k=5, pool=4), dict(seq_len=0), dict(windows_per_pass=0)):
        with pytest.raises(ValueError):
            search_rerank(_index("fp32"), m, _embed, QUERIES, **bad)
    shallow = TemporalAligner(1, 2, use_alignability_head=1, random_pos_start=0, language_model=None, d_video=16)
    with pytest.raises(ValueError, match="stage index 2"):
        search_rerank(_index("fp32"), shallow, _embed, QUERIES)


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_index_keep_stem_then_query_rerank(tmp_path):
    from temporalalignnet_amd import infer_align
    from temporalalignnet_amd.search import VideoIndex, search_rerank
    from temporalalignnet_amd.train import build_model, default_args
    from temporalalignnet_amd.word2vec_model import Word2VecModel, Word2VecTokenizer
    paths = synth.write_htm_fixture(str(tmp_path / "htm"), synth.htm_fixture())
    vocab = synth.w2v_vocab(40)
    np.save(str(tmp_path / "s3d_dict.npy"), vocab)
    m = build_model(default_args(model="init", num_encoder_layers=1, num_decoder_layers=3, use_alignability_head=1), compute_dtype="bf16",
                    language_model=None, random_pos_start=0)
    sd = m.state_dict()
    for k, v in synth.make_params(31, 1, 3, True).items():
        sd[k].copy_(torch.from_numpy(v))
    m.bert = Word2VecModel(num_embeddings=len(vocab) + 1, compute_dtype="bf16")
    for k, v in synth.w2v_params(32, len(vocab) + 1).items():
        m.bert.state_dict()[k].copy_(torch.from_numpy(v))
    ckpt = str(tmp_path / "ckpt.pth.tar")
    torch.save({"state_dict": m.state_dict(), "epoch": 3}, ckpt)
    common = ["--checkpoint", ckpt, "--vocab", str(tmp_path / "s3d_dict.npy")]
    out = str(tmp_path / "index.npz")

    def run(*args):
        p = subprocess.run([sys.executable, "-m", "temporalalignnet_amd.search", *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        return p.stdout

    run("index", *common, "--feature-dir", paths["features"], "--asr-json", paths["asr"], "--vlen-csv", paths["vlen"], "--out", out,
        "--index-dtype", "e4m3", "--keep-stem")
    sentences = ["stir the eggs", "w3 w7 w11"]
    rows = [ln.split("\t") for ln in run("query", *common, "--index", out, "-k", "3", "--rerank", "--pool", "5", *sentences).splitlines()]
    model = infer_align.build_aligner(ckpt, vocab, "init", "bf16")
    embed = infer_align.make_embed_text(model, Word2VecTokenizer(max_words=32, vocab=vocab))
    idx = VideoIndex.load(out)
    assert idx.e4m3 and idx.stem.dtype == torch.bfloat16 and idx.stem.shape == (len(idx), 512) and len(idx.vids) == 10
    want = search_rerank(idx, model, embed, sentences, k=3, pool=5)
    assert len(rows) == 6 and all(len(r) == 8 for r in rows)
    flat = [(s, h) for s, hs in zip(sentences, want) for h in hs]
    for r, (s, h) in zip(rows, flat):
        assert r[:3] == [s, h.vid, str(h.second)] and r[6] == str(h.dual_second)
        assert [float(x) for x in (r[3], r[4], r[5], r[7])] == [round(x, 6) for x in (h.score, h.confidence, h.alignability, h.dual_score)]
