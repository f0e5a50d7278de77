"""Corpus auto-alignment on the GPU: the pack / stitch kernels against the torch code they replace, align_corpus against the
HTM-Align golden (G6) and against the per-video evaluation, and the CLI end to end."""
import csv
import io
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from temporalalignnet_amd import ops, synth
from temporalalignnet_amd.eval_align import plan_windows
from temporalalignnet_amd.infer_align import _Chunk, align_corpus

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _videos(seed, vlens, per_s=8.0, Dv=16):
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(vlens):
        K = max(1, int(n / per_s))
        mid = np.sort(rng.uniform(0, n, K))
        dur = rng.uniform(1, 9, K)
        out.append({"vid": f"v{i}", "vlen": n, "start": np.clip(mid - dur / 2, 0, None), "end": mid + dur / 2,
                    "str": [f"v{i}s{k}" for k in range(K)], "video": rng.standard_normal((n, Dv)).astype(np.float32)})
    return out


def _plans(items):
    # a video too short for a window start (vlen <= 32) gets one window over all of it by hand, so the kernels see it too
    return [plan_windows(it["start"], it["end"], it["vlen"]) or [(0, it["vlen"], 0, len(it["str"]))] for it in items]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_window_pack_is_the_torch_slicing(dtype):
    items = _videos(1, [203, 20, 64, 150], Dv=20)      # f32 rows take the 16-byte path, 16-bit rows the 2-byte one
    ch = _Chunk(items, _plans(items), 64, 9)
    video = torch.cat([torch.from_numpy(it["video"]) for it in items]).to("cuda", dtype)
    text = torch.randn(ch.n_rows, 40, device="cuda").to(dtype)
    table = ch.table.cuda()
    for p0, p1, Kp in ch.passes:
        W, tab = p1 - p0, table[p0:p1]
        kmax = int(ch.table[p0:p1, 3].max())
        assert Kp % 8 == 0 and Kp >= kmax
        got = (torch.full((W, 64, 20), 7, dtype=dtype, device="cuda"), torch.zeros(W, 64, dtype=torch.bool, device="cuda"),
               torch.full((W, Kp, 40), 7, dtype=dtype, device="cuda"), torch.zeros(W, Kp, dtype=torch.bool, device="cuda"))
        ops.window_pack(video, text, tab, 64, Kp, *got)
        # make_batched_sim_fn's slicing
        vid = torch.zeros(W, 64, 20, device="cuda", dtype=dtype)
        vmask = torch.ones(W, 64, dtype=torch.bool, device="cuda")
        txt = torch.zeros(W, Kp, 40, device="cuda", dtype=dtype)
        tmask = torch.ones(W, Kp, dtype=torch.bool, device="cuda")
        for w, (vrow, t, krow, k, *_rest) in enumerate(ch.table[p0:p1].tolist()):
            vid[w, :t] = video[vrow:vrow + t]
            vmask[w, :t] = False
            txt[w, :k] = text[krow:krow + k]
            tmask[w, :k] = False
        for a, b in zip(got, (vid, vmask, txt, tmask)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert any(t < 64 for t in ch.table[:, 1].tolist()) and len(ch.passes) > 2


def _host_stitch(items, plans, raw, head):
    """The stitch of eval_align.test_alignment_htm, fed each window's slice of the pass outputs (dicts as make_batched_sim_fn
    returns them)."""
    out = []
    for it, plan, rs in zip(items, plans, raw):
        K, vlen, dev = len(it["str"]), it["vlen"], "cuda"
        acc_j, acc_d, cnt = (torch.zeros(K, vlen, device=dev) for _ in range(3))
        a_d, a_j, tcnt = (torch.zeros(K, device=dev) for _ in range(3))
        for (s0, e0, left, right), r in zip(plan, rs):
            m = np.zeros(K, bool)
            m[left:right] = True
            mt = torch.from_numpy(m).to(dev)
            if head:
                a_j[mt] += r["alignability-joint"][0, 2, :, 0]
            tcnt[mt] += 1
            acc_j[mt, s0:e0] += r["sim"][0, -1]
            acc_d[mt, s0:e0] += r["dual-sim"][0, -1]
            cnt[mt, s0:e0] += 1
        eps = torch.tensor(1e-5, device=dev)
        acc_j, acc_d = acc_j / torch.maximum(cnt, eps), acc_d / torch.maximum(cnt, eps)
        a_j = a_j / torch.maximum(tcnt, eps)
        sim = (acc_j + acc_d) / 2
        sim = sim.masked_fill(sim == 0, -6e4)
        prob = sim.softmax(-1)
        score = a_j if head else sim.max(-1)[0]
        out.append({"sim": sim.cpu(), "prob": prob.cpu(), "score": score.cpu(), "covered": (tcnt > 0).cpu()})
    return out


def assert_timestamps(ts, prob):
    """ts equals the host's prob.argmax(-1); where the host row has tied maxima any tied index is accepted."""
    prob = torch.as_tensor(prob)
    mx = prob.max(-1, keepdim=True).values
    ties = (prob == mx).sum(-1) > 1
    ts = torch.as_tensor(np.asarray(ts)).long()
    am = prob.argmax(-1)
    assert torch.equal(ts[~ties], am[~ties])
    assert bool((prob.gather(1, ts[:, None]) == mx).all())


@pytest.mark.parametrize("head", [True, False])
def test_window_stitch_is_the_host_loop(head):
    g = torch.Generator(device="cuda").manual_seed(5)
    items = _videos(2, [20, 64, 203, 1200, 203])
    plans = _plans(items)
    ch = _Chunk(items, plans, 64, 11)                      # 11 windows per pass: videos span passes, passes span videos
    table = ch.table.cuda()
    acc_j, acc_d, cnt = (torch.zeros(ch.n_acc, device="cuda") for _ in range(3))
    tcnt = torch.zeros(ch.n_rows, device="cuda")
    a_sum = torch.zeros(ch.n_rows, device="cuda") if head else None
    per_window = []
    for p0, p1, Kp in ch.passes:
        W = p1 - p0
        # eval_windows' layout: [S][W][T][Kp] raw cosines, [S][W][Kp][1] head logits, then the [B,S,...] permuted views
        sj = torch.rand(3, W, 64, Kp, device="cuda", generator=g) * 2 - 1
        sd = torch.rand(2, W, 64, Kp, device="cuda", generator=g) * 2 - 1
        aj = torch.randn(3, W, Kp, 1, device="cuda", generator=g)
        r = {"sim": sj.permute(1, 0, 2, 3), "dual-sim": sd.permute(1, 0, 2, 3), "alignability-joint": aj.permute(1, 0, 2, 3)}
        ops.window_stitch_acc(sj[-1], sd[-1], aj[2].view(W, Kp) if head else None, table[p0:p1], acc_j, acc_d, cnt, tcnt, a_sum)
        sim_j = r["sim"].transpose(-1, -2) / 0.07                    # make_batched_sim_fn
        sim_d = r["dual-sim"].transpose(-1, -2) / 0.07
        for w, (_, t, _, k, *_r) in enumerate(ch.table[p0:p1].tolist()):
            per_window.append({"sim": sim_j[w:w + 1, :, :k, :t], "dual-sim": sim_d[w:w + 1, :, :k, :t],
                               "alignability-joint": r["alignability-joint"][w:w + 1, :, :k]})
    res = torch.empty(4, ch.n_rows, device="cuda")
    ops.window_stitch_final(acc_j, acc_d, cnt, tcnt, a_sum, ch.rows.cuda(), res)
    res, acc_j = res.cpu(), acc_j.cpu()
    nw = np.cumsum([0] + [len(p) for p in plans])
    host = _host_stitch(items, plans, [per_window[a:b] for a, b in zip(nw[:-1], nw[1:])], head)
    for i, (it, h) in enumerate(zip(items, host)):
        k0, k1 = ch.k_off[i], ch.k_off[i + 1]
        sim = acc_j[ch.a_off[i]:ch.a_off[i + 1]].view(k1 - k0, it["vlen"])
        assert torch.equal(sim, h["sim"]), it["vid"]                # bit-identical in fp32
        assert_timestamps(res[0, k0:k1], h["prob"])
        torch.testing.assert_close(res[1, k0:k1], h["prob"].max(-1).values, rtol=1e-6, atol=0)
        torch.testing.assert_close(res[2, k0:k1], h["score"], rtol=1e-6, atol=0)
        assert torch.equal(res[3, k0:k1] > 0, h["covered"])


def _g6_model():
    from temporalalignnet_amd.tan_model import TemporalAligner
    m = TemporalAligner(1, 3, use_alignability_head=1, random_pos_start=0, language_model=None)
    sd = m.state_dict()
    for k, v in synth.make_params(108, 1, 3, True).items():
        sd[k].copy_(torch.from_numpy(v))
    return m.cuda().eval()


def _g6_embed(videos):
    emb = {s: torch.from_numpy(e).cuda() for v in videos for s, e in zip(v["str"], v["emb"])}
    return lambda strs: torch.stack([emb[s] for s in strs])


@pytest.mark.parametrize("windows_per_pass", [256, 5])
def test_g6_golden_through_align_corpus(golden, windows_per_pass):
    g = golden("g6_eval_harness")
    m = _g6_model()
    videos = synth.align_videos()
    res = list(align_corpus(m, videos, _g6_embed(videos), windows_per_pass=windows_per_pass, return_sim=True,
                            candidates=lambda v: ~np.asarray(v["aligned"]).astype(bool)))
    assert [r["vid"] for r in res] == [v["vid"] for v in videos]
    for i, (v, r) in enumerate(zip(videos, res)):
        al = np.asarray(v["aligned"]).astype(bool)
        assert (r["timestamp"][al] == g[f"v{i}/argmax"]).all()
        np.testing.assert_allclose(r["sim"][al], g[f"v{i}/sim_aligned"], rtol=1e-4, atol=2e-4)
        np.testing.assert_allclose(r["score"], g[f"v{i}/align_score"], rtol=1e-4, atol=1e-5)
        assert r["covered"].all()


def test_all_sentence_mode_is_the_per_video_evaluation():
    from temporalalignnet_amd.eval_align import make_batched_sim_fn, test_alignment_htm
    m = _g6_model()
    videos = synth.align_videos()
    for v in videos:
        v["aligned"] = np.zeros_like(v["aligned"])
    embed = _g6_embed(videos)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")                             # Recall / AUC over no aligned sentence: NaN, ignored
        _, pv = test_alignment_htm(None, videos, return_per_video=True, batched_sim=make_batched_sim_fn(m, embed))
    res = list(align_corpus(m, videos, embed, windows_per_pass=7, return_sim=True))
    for v, r, h in zip(videos, res, pv):
        np.testing.assert_allclose(r["sim"], h["sim"].numpy(), rtol=1e-4, atol=2e-4)
        assert_timestamps(r["timestamp"], h["sim"].softmax(-1))
        np.testing.assert_allclose(r["score"], h["score"].numpy(), rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------------- CLI end to end
@pytest.fixture(scope="module")
def cli_setup(tmp_path_factory):
    from temporalalignnet_amd.train import build_model, default_args
    from temporalalignnet_amd.word2vec_model import Word2VecModel
    tmp = tmp_path_factory.mktemp("htmaa")
    paths = synth.write_htm_fixture(str(tmp / "htm"), synth.htm_fixture())
    vocab = synth.w2v_vocab(40)
    np.save(str(tmp / "s3d_dict.npy"), vocab)
    m = build_model(default_args(model="init", num_encoder_layers=3, num_decoder_layers=3), compute_dtype="bf16",
                    language_model=None, random_pos_start=0)
    sd = m.state_dict()
    for k, v in synth.make_params(31, 3, 3, False).items():
        sd[k].copy_(torch.from_numpy(v))
    m.bert = Word2VecModel(num_embeddings=len(vocab) + 1, compute_dtype="bf16")
    for k, v in synth.w2v_params(32, len(vocab) + 1).items():
        m.bert.state_dict()[k].copy_(torch.from_numpy(v))
    ckpt = str(tmp / "ckpt.pth.tar")
    torch.save({"state_dict": m.state_dict(), "epoch": 3}, ckpt)
    args = ["--checkpoint", ckpt, "--feature-dir", paths["features"], "--asr-json", paths["asr"], "--vlen-csv", paths["vlen"],
            "--vocab", str(tmp / "s3d_dict.npy")]
    return tmp, paths, args


def _run_cli(args, out):
    p = subprocess.run([sys.executable, "-m", "temporalalignnet_amd.infer_align", *args, "--out", out], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["vid", "timestamp", "text", "score", "confidence"]
    return rows[1:]


def test_cli_end_to_end(cli_setup):
    from temporalalignnet_amd import infer_align
    from temporalalignnet_amd.word2vec_model import Word2VecTokenizer
    tmp, paths, args = cli_setup
    rows = _run_cli(args, str(tmp / "all.csv"))
    shards = [_run_cli(args + ["--worker-id", str(i), "--num-workers", "2"], str(tmp / f"w{i}.csv")) for i in range(2)]
    assert sorted(shards[0] + shards[1]) == sorted(rows)
    assert not {r[0] for r in shards[0]} & {r[0] for r in shards[1]}
    # the same corpus in process
    vocab = np.load(str(tmp / "s3d_dict.npy"))
    model = infer_align.build_aligner(args[1], vocab, "init", "bf16")
    embed = infer_align.make_embed_text(model, Word2VecTokenizer(max_words=32, vocab=vocab))
    corpus = lambda: infer_align.read_corpus(paths["features"], paths["asr"], paths["vlen"])     # noqa: E731
    allocated = []
    for rep in range(3):
        buf = io.StringIO(newline="")
        w = csv.writer(buf)
        n_cov = 0
        for r in align_corpus(model, corpus(), embed):
            infer_align.write_rows(w, r)
            n_cov += int(r["covered"].sum())
        mine = list(csv.reader(io.StringIO(buf.getvalue(), newline="")))
        assert len(mine) == n_cov and mine == rows, rep
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        allocated.append(torch.cuda.memory_allocated())
    assert allocated[1] == allocated[2]
    # texts with newlines come back whole; every video with a window start has covered sentences
    assert any("\n" in r[2] for r in rows)
    assert {r[0] for r in rows} >= {"vidA0001", "vidH0008", "vidI0009", "vidG0007"}
    # threshold keeps score > t
    t = float(np.median([float(r[3]) for r in rows]))
    kept = _run_cli(args + ["--threshold", str(t)], str(tmp / "thr.csv"))
    assert kept == [r for r in rows if float(r[3]) > t] and 0 < len(kept) < len(rows)
