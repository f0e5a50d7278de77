"""HTM-Align zero-shot alignment evaluation: counterpart of eval/eval_zeroshot_align.py:test_alignment_htm (97-252)
and of the `get_text_visual_sim` closure in train/main.py:171-189.

64-s windows with stride 16 over each video; the active sentences of a window are chosen from the NON-alignable
sentences' ASR timestamps only (no ground-truth leak, :149-167); last-stage joint and dual similarities are stitched
and averaged (:197-205), zeros -> -6e4, softmax over time, arg-max inside [floor(start), ceil(end)] -> R@1; the joint
alignability head (stage index 2, :186) -> ROC-AUC.  Model calls run on the HIP path; the per-video bookkeeping is
host-side index arithmetic on [K, vlen] tensors.
"""
from __future__ import annotations

import math

import numpy as np
import torch


def roc_auc_score(y_true, y_score) -> float:
    """ROC-AUC by the rank statistic with average ranks for ties (= sklearn.metrics.roc_auc_score, :248)."""
    y = np.asarray(y_true).astype(bool)
    s = np.asarray(y_score, dtype=np.float64)
    order = np.argsort(s, kind="mergesort")
    ss = s[order]
    ranks = np.empty(len(s))
    bounds = np.flatnonzero(np.r_[True, ss[1:] != ss[:-1], True])
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ranks[order[lo:hi]] = 0.5 * (lo + hi - 1) + 1.0
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    return float((ranks[y].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def make_sim_fn(model, embed_text, use_alignability_head=True):
    """The closure of train/main.py:171-189: `embed_text(list[str]) -> [K, 512]` stands for tokenizer + language model."""

    @torch.no_grad()
    def get_text_visual_sim(video_embed, text_str, interpolate_from=None, abs_text_pos=None):
        text_embed = embed_text(text_str)[None]
        out = {"sim": model.get_text_visual_sim_joint(video_embed, text_embed, interpolate_from).transpose(-1, -2) / 0.07,
               "dual-sim": model.get_text_visual_sim_dual(video_embed, text_embed, interpolate_from).transpose(-1, -2) / 0.07}
        if use_alignability_head:
            out.update(model.get_alignability(video_embed, text_embed, interpolate_from, abs_text_pos))
        return out

    return get_text_visual_sim


def make_batched_sim_fn(model, embed_text, use_alignability_head=True, max_windows=256):
    """Batched counterpart of make_sim_fn for `test_alignment_htm(batched_sim=...)`: all windows of a video go through
    `model.eval_windows` in chunks of `max_windows` (one pass of each stack per chunk instead of four B=1 passes per window).
    `run(video [1,vlen,Dv], text list[str], windows [(s0, e0, bool mask [K])], seq_len)` returns, per window, the dict
    `get_text_visual_sim` would have returned for it."""

    @torch.no_grad()
    def run(video, text_str, windows, seq_len):
        dev = video.device
        emb = embed_text(list(text_str))                                  # [K, 512]: sentences are embedded independently
        out = []
        for c0 in range(0, len(windows), max_windows):
            chunk = windows[c0:c0 + max_windows]
            W, kmax = len(chunk), max(int(m.sum()) for _, _, m in chunk)
            vid = torch.zeros(W, seq_len, video.shape[-1], device=dev, dtype=video.dtype)
            vmask = torch.ones(W, seq_len, dtype=torch.bool, device=dev)
            txt = torch.zeros(W, kmax, emb.shape[-1], device=dev, dtype=emb.dtype)
            tmask = torch.ones(W, kmax, dtype=torch.bool, device=dev)
            for w, (s0, e0, m) in enumerate(chunk):
                k = int(m.sum())
                vid[w, :e0 - s0] = video[0, s0:e0]
                vmask[w, :e0 - s0] = False
                txt[w, :k] = emb[torch.from_numpy(m).to(dev)]
                tmask[w, :k] = False
            r = model.eval_windows(vid, txt, vmask, tmask)
            sim_j = r["sim"].transpose(-1, -2) / 0.07                     # [W,S,K,T]
            sim_d = r["dual-sim"].transpose(-1, -2) / 0.07
            for w, (s0, e0, m) in enumerate(chunk):
                k, t = int(m.sum()), e0 - s0
                d = {"sim": sim_j[w:w + 1, :, :k, :t], "dual-sim": sim_d[w:w + 1, :, :k, :t]}
                if use_alignability_head:
                    d["alignability-dual"] = r["alignability-dual"][w:w + 1, :k]
                    d["alignability-joint"] = r["alignability-joint"][w:w + 1, :, :k]
                out.append(d)
        return out

    return run


def plan_windows(start, end, vlen, seq_len=64, candidates=None, *, max_sentences=None, vid=None):
    """The windows of one video, as eval/eval_zeroshot_align.py:129-170 forms them: [(s0, e0, left, right_excl)].

    Window starts are `arange(0, vlen - seq_len // 2, seq_len // 4)`; a window is active when the midpoint of at least one CANDIDATE
    sentence lies in [s0 - seq_len, s0 + 2 * seq_len], and then holds the sentences left..right of the active ones (every sentence in
    between, candidate or not).  Edge rule: the first four windows start at sentence 0, the last four run to the end (`right = vlen`,
    so a slice up to vlen + 1 -- every sentence when K <= vlen + 1).  e0 = min(vlen, s0 + seq_len).  `candidates` (bool [K]): the
    evaluation passes the NON-alignable sentences (~aligned, no ground-truth leak); None = every sentence (corpus inference).
    `max_sentences`: a window holding more sentences than the joint stack accepts raises ValueError naming `vid` (sentences are
    never dropped silently)."""
    start, end = np.asarray(start, dtype=np.float64), np.asarray(end, dtype=np.float64)
    K = len(start)
    cand = np.ones(K, bool) if candidates is None else np.asarray(candidates).astype(bool)
    steps = np.arange(0, vlen - seq_len // 2, seq_len // 4)
    mid = (start + end) / 2
    c_idx, c_mid = np.arange(K)[cand], mid[cand]
    out = []
    for i, s0 in enumerate(steps):
        act = c_idx[(s0 - seq_len <= c_mid) & (c_mid <= s0 + 2 * seq_len)]
        if len(act) == 0:
            continue
        left, right = int(act.min()), int(act.max())
        if i <= 3:
            left = 0
        elif i >= len(steps) - 4:
            right = int(vlen)
        right_excl = min(right + 1, K)
        if right_excl <= left:
            continue
        if max_sentences is not None and right_excl - left > max_sentences:
            raise ValueError(f"{vid}: the window at {int(s0)} s holds {right_excl - left} sentences, the joint stack takes at most "
                             f"{max_sentences} beside {seq_len} frames")
        out.append((int(s0), int(min(vlen, s0 + seq_len)), left, right_excl))
    return out


@torch.no_grad()
def monotonic_seconds(sim, start, keep=None):
    """One video's order-preserving timestamps (tan_monotonic_decode): sim [K, vlen] f32 on the device, `start` [K] the ASR starts
    that order the sentences (equal starts by sentence index), keep [K] bool or None = all.  Returns ([K] int64 on the host, -1
    where not kept; the path's score).  A constant added to a row does not move the path: decoding `sim` is decoding its
    log-softmax over time, the quantity the reference arg-maxes row by row."""
    from . import ops
    K, vlen = sim.shape
    if K == 0:
        return torch.zeros(0, dtype=torch.int64), 0.0
    dev = sim.device
    sim = sim.float().contiguous()
    tab = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)                 # noqa: E731
    rows = tab(np.stack([np.arange(K) * vlen, np.full(K, vlen)], 1))
    order = tab(np.argsort(np.asarray(start, dtype=np.float64), kind="stable"))
    keep_d = None if keep is None else torch.from_numpy(np.asarray(keep).astype(bool)).to(dev)
    ts = torch.empty(K, dtype=torch.int32, device=dev)
    path = torch.empty(1, device=dev)
    ops.monotonic_decode(sim.view(-1), rows, order, tab([[0, K, 0]]), keep_d, torch.empty(K * vlen, dtype=torch.int32, device=dev),
                         torch.empty(vlen, device=dev), ts, path)
    return ts.cpu().long(), float(path)


def check_width(width):
    """The segmental decode's `width`, as a float; negative or NaN raises ValueError."""
    width = float(width)
    if not width >= 0:
        raise ValueError(f"width: a non-negative number of logits, not {width!r}")
    return width


@torch.no_grad()
def segment_seconds(sim, start, keep=None, width=1.0):
    """One video's aligned intervals (tan_segment_decode): sim [K, vlen] f32 on the device, `start` [K] the ASR starts that order the
    sentences (equal starts by sentence index), keep [K] bool or None = all.  Returns ([K, 2] int64 on the host: inclusive (start, end)
    seconds, ordered and disjoint, (-1, -1) where not kept or when more sentences are kept than the video has seconds; the path's
    score).  A second adds sim - (row maximum - width) to its sentence's segment: `width` (logits) is how far below its row's peak a
    second may lie and still pay.  The default 1.0 is `search_moments`' default (its TEMPERATURE, 0.07 in cosine) on the stitched
    rows' 1/0.07 scale: a convention, tuned on nothing."""
    from . import ops
    width = check_width(width)
    K, vlen = sim.shape
    if K == 0:
        return torch.zeros(0, 2, dtype=torch.int64), 0.0
    dev = sim.device
    sim = sim.float().contiguous()
    tab = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)                 # noqa: E731
    rows = tab(np.stack([np.arange(K) * vlen, np.full(K, vlen)], 1))
    order = tab(np.argsort(np.asarray(start, dtype=np.float64), kind="stable"))
    keep_d = None if keep is None else torch.from_numpy(np.asarray(keep).astype(bool)).to(dev)
    bias = sim.max(-1).values - torch.full((), width, dtype=torch.float32, device=dev)                 # one f32 subtraction
    seg = torch.empty(K, 2, dtype=torch.int32, device=dev)
    path = torch.empty(1, device=dev)
    ops.segment_decode(sim.view(-1), rows, order, tab([[0, K, 0]]), keep_d, bias, torch.empty(2 * K * vlen, dtype=torch.int32, device=dev),
                       torch.empty(vlen, device=dev), seg, path)
    return seg.cpu().long(), float(path)


def temporal_iou(seg_start, seg_end, start, end):
    """IoU of the decoded seconds [seg_start, seg_end + 1) with the annotated [floor(start), ceil(end)]; 0 without a segment."""
    if seg_start < 0:
        return 0.0
    lo, hi = math.floor(start), math.ceil(end)
    inter = max(0, min(seg_end + 1, hi) - max(seg_start, lo))
    return inter / ((seg_end + 1 - seg_start) + (hi - lo) - inter)


@torch.no_grad()
def test_alignment_htm(get_text_visual_sim, videos, device="cuda", seq_len=64, use_alignability_head=True,
                       method="overlap-seq", return_per_video=False, batched_sim=None, decode=None, width=1.0):
    """`videos`: iterable of {'video' [vlen, Dv], 'start' [K], 'end' [K], 'aligned' [K] 0/1, 'str' list[str]}
    (htm_align.json schema, htm_align/readme.md:11-20).  Returns {'Recall', 'AUC'}.  `batched_sim` (make_batched_sim_fn): the
    windows of a video are evaluated together instead of one model call per window (same results, see the GPU tests).
    `decode="monotonic"` (either method): the aligned sentences' seconds come from `monotonic_seconds` -- non-decreasing in ASR start
    order -- instead of each row's own arg-max (:222,237), so Recall shows what the ordering does to R@1; AUC is not affected.
    `decode="segments"` (either method): the aligned sentences get ordered, disjoint intervals from `segment_seconds(.., width)`; a
    sentence's second is the best one inside its interval (the first arg-max of sim[k, s:e+1]; -1 without an interval), the metric
    gains 'IoU' -- the mean `temporal_iou` of [s, e + 1) with [floor(start), ceil(end)] over the aligned sentences -- and the
    per-video dicts gain 'segments' ([n_aligned, 2] int64)."""
    if decode not in (None, "monotonic", "segments"):
        raise ValueError(f"decode: None, 'monotonic' or 'segments', not {decode!r}")
    if decode == "segments":
        width = check_width(width)
    recall, ious, scores, tgts, per_video = [], [], [], [], []
    for item in videos:
        video = torch.as_tensor(item["video"]).float().to(device)[None]
        text = list(item["str"])
        aligned = np.asarray(item["aligned"]).astype(bool)
        start = np.asarray(item["start"], dtype=np.float64)
        end = np.asarray(item["end"], dtype=np.float64)
        K, vlen = len(text), video.shape[1]
        abs_pos = torch.stack((torch.as_tensor(item["start"]), torch.as_tensor(item["end"])), -1).div(vlen).to(device)
        if method == "overlap-seq":
            acc_j = torch.zeros(K, vlen, device=device)
            acc_d = torch.zeros(K, vlen, device=device)
            cnt = torch.zeros(K, vlen, device=device)
            a_d, a_j, tcnt = (torch.zeros(K, device=device) for _ in range(3))
            windows = []
            for s0, e0, left, right in plan_windows(start, end, vlen, seq_len, candidates=~aligned):
                m = np.zeros(K, bool)
                m[left:right] = True
                windows.append((s0, e0, m))
            if batched_sim is not None:
                results = batched_sim(video, text, windows, seq_len)
            else:
                results = (get_text_visual_sim(video[:, s0:e0], [t for t, k in zip(text, m) if k],
                                               abs_text_pos=abs_pos[torch.from_numpy(m).to(device)][None])
                           for s0, e0, m in windows)
            for (s0, e0, m), r in zip(windows, results):
                mt = torch.from_numpy(m).to(device)
                if use_alignability_head:
                    a_d[mt] += r["alignability-dual"][0, :, 0]
                    a_j[mt] += r["alignability-joint"][0, 2, :, 0]
                else:
                    a_d[mt] += r["dual-sim"][0, -1].max(-1).values
                    a_j[mt] += r["sim"][0, -1].max(-1).values
                tcnt[mt] += 1
                acc_j[mt, s0:e0] += r["sim"][0, -1]
                acc_d[mt, s0:e0] += r["dual-sim"][0, -1]
                cnt[mt, s0:e0] += 1
            eps = torch.tensor(1e-5, device=device)
            acc_j, acc_d = acc_j / torch.maximum(cnt, eps), acc_d / torch.maximum(cnt, eps)
            a_j = a_j / torch.maximum(tcnt, eps)
            sim = (acc_j + acc_d) / 2
        elif method == "global":
            r = get_text_visual_sim(video, text, interpolate_from=seq_len)
            sim = r["sim"][0, -1].clone()
            a_j = r["alignability-joint"][0, -1, :, 0] if use_alignability_head else r["sim"][0, -1].max(-1).values
        else:
            raise ValueError(method)
        sim = sim.masked_fill(sim == 0, -6e4)
        prob = sim.softmax(-1)
        score = a_j if use_alignability_head else sim.max(-1)[0]
        scores.append(score.cpu().numpy().copy())
        tgts.append(aligned.astype(np.int64))
        if decode is None:
            am = prob[torch.from_numpy(aligned).to(device)].argmax(-1).cpu()
        elif decode == "monotonic":
            am = monotonic_seconds(sim, start, aligned)[0][torch.from_numpy(aligned)]
        else:
            segs = segment_seconds(sim, start, aligned, width)[0][torch.from_numpy(aligned)]
            rows = sim[torch.from_numpy(aligned).to(device)].cpu()
            am = torch.tensor([int(a) + int(r[a:b + 1].argmax()) if a >= 0 else -1 for r, (a, b) in zip(rows, segs.tolist())],
                              dtype=torch.int64)
            ious += [temporal_iou(a, b, s, e) for (a, b), s, e in zip(segs.tolist(), start[aligned], end[aligned])]
        for k, (s, e) in enumerate(zip(start[aligned], end[aligned])):
            recall.append(math.floor(s) <= int(am[k]) <= math.ceil(e))
        per_video.append({"sim": sim.cpu(), "argmax": am, "score": score.cpu()})
        if decode == "segments":
            per_video[-1]["segments"] = segs
    metric = {"Recall": float(np.mean(recall)), "AUC": roc_auc_score(np.concatenate(tgts), np.concatenate(scores))}
    if decode == "segments":
        metric["IoU"] = float(np.mean(ious))
    return (metric, per_video) if return_per_video else metric
