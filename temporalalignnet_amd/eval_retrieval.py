"""YouCook2 zero-shot text->video retrieval: counterpart of eval/eval_zeroshot_retrieval.py:
`compute_metrics` (:13-27), the window selection of `YouCook2_Feature._get_video_feature` (:104-148) and `test_retrieval_yc2`
(:157-256).  The model is only reached through `get_visual_feature(video, mask, interpolate_from=)` and
`get_textual_feature(lang_embed)` (tan_model.py:152,231) -- HIP path; everything else here is host-side index arithmetic on
per-clip features and a [n_clips, n_clips] similarity matrix.
"""
from __future__ import annotations

import numpy as np
import torch


def compute_metrics(x) -> dict:
    """Recall@{1,5,10} and median rank of the diagonal of a text x video similarity matrix (:13-27, after MIL-NCE's metrics.py):
    every position where the descending-sorted row equals the diagonal entry counts (ties give several hits per row)."""
    x = np.asarray(x)
    sx = np.sort(-x, axis=1)
    d = np.diag(-x)[:, np.newaxis]
    ind = np.where(sx - d == 0)[1]
    return {"R1": np.array(float(np.sum(ind == 0)) / len(ind)), "R5": np.array(float(np.sum(ind < 5)) / len(ind)),
            "R10": np.array(float(np.sum(ind < 10)) / len(ind)), "MR": np.array(np.median(ind) + 1)}


def clip_windows(vlen: int, start, end, num_clips: int = 10, seq_len: int = -1):
    """Frame indices [num_clips, window] of the windows evaluated for one annotated segment, and the segment's position inside
    every window (start_idx, end_idx), exactly as `_get_video_feature` picks them (:104-148).
    seq_len == -1 (what test_retrieval_yc2 uses): window = clip(2 * floor(end - start), 32, 256) frames; if it is at least as long
    as the segment the windows START `lead` frames before it with lead spread over [25 %, 75 %] of the slack, otherwise they
    start inside the segment with the lag spread the same way.  Indices are clipped to the video."""
    if seq_len == -1:
        duration = np.floor(end - start).astype(int)
        win = int(np.clip(duration * 2, a_min=32, a_max=256))
        if win >= duration:
            lead = np.floor(np.linspace(0.25 * (win - duration), 0.75 * (win - duration), num_clips)).astype(int)
            first, s_idx, e_idx = start - lead, lead, lead + duration
        else:
            lag = np.floor(np.linspace(0.25 * (duration - win), 0.75 * (duration - win), num_clips)).astype(int)
            first, s_idx, e_idx = start + lag, np.zeros_like(lag), np.zeros_like(lag) + win
    else:
        win = int(seq_len)
        first = np.floor(np.linspace(0, end - start - seq_len - 1, num_clips)).astype(int) + start
        s_idx = e_idx = None
    idx = np.clip(np.expand_dims(first, 1) + np.arange(win).astype(int)[None], a_min=0, a_max=vlen - 1)
    return idx, s_idx, e_idx


@torch.no_grad()
def test_retrieval(clips, get_visual_feature, get_text_feature, embed_text, *, sim: str = "cos", seq_len: int = 64,
                   num_clips: int = 10, device="cuda", return_sim: bool = False):
    """test_retrieval_yc2 (:157-256).  `clips`: iterable of {'feature' [vlen, D] float array (per-second features of the clip's
    video), 'start', 'end' (segment, seconds), 'str'}; `embed_text(list[str]) -> [n, 512]` stands for tokenizer + language model.
    Per clip: ten windows through `get_visual_feature` (position table interpolated from `seq_len` when the window is at least that
    long, :180-184), last stage, the segment's frames of every window, L2-normalised, averaged over time and windows,
    normalised again (:197-214); text through `get_text_feature`, normalised.  Metrics on text x video, then on centred and on
    standardised features (:233-256)."""
    vis, txt = [], []
    for item in clips:
        feat = torch.as_tensor(item["feature"])
        idx, s_idx, e_idx = clip_windows(feat.shape[0], item["start"], item["end"], num_clips, -1)
        video = feat[torch.as_tensor(idx)].to(device)                                   # [num_clips, window, D]
        v = get_visual_feature(video, torch.zeros(video.shape[:2], device=device, dtype=torch.bool),
                               interpolate_from=seq_len if video.shape[1] >= seq_len else None)
        if v.dim() == 4:
            v = v[:, -1]                                                                # last deep-supervision stage
        v = torch.stack([v[i, int(s_idx[i]):int(e_idx[i])] for i in range(v.shape[0])], 0).float()
        if sim == "cos":
            v = v / v.norm(dim=-1, keepdim=True)
        v = v.mean(0).mean(0, keepdim=True)
        t = get_text_feature(embed_text([item["str"]]).to(device)).float()
        if sim == "cos":
            v = v / v.norm(dim=-1, keepdim=True)
            t = t / t.norm(dim=-1, keepdim=True)
        vis.append(v.cpu())
        txt.append(t.reshape(1, -1).cpu())
    V, T = torch.cat(vis, 0).numpy(), torch.cat(txt, 0).numpy()
    s = np.dot(T, V.T)
    metrics = compute_metrics(s)
    Vc, Tc = V - V.mean(0, keepdims=True), T - T.mean(0, keepdims=True)
    mc = compute_metrics(np.dot(Tc, Vc.T))
    ms = compute_metrics(np.dot(Tc / Tc.std(0, keepdims=True), (Vc / Vc.std(0, keepdims=True)).T))
    for tag, m in (("C", mc), ("S", ms)):
        for k in ("R1", "R5", "R10", "MR"):
            metrics[f"{tag}-{k}"] = m[k]
    return (metrics, s) if return_sim else metrics


# ------------------------------------------------------------------------------------------------ the batched harness (device path)
def metrics_from_counts(higher, ties) -> dict:
    """`compute_metrics` from per-row counts: higher[i] / ties[i] = how many columns score strictly above / exactly equal to the
    diagonal entry of row i (the tie count includes the diagonal itself).  The sorted row equals the diagonal entry at positions
    higher .. higher + ties - 1 and every one of them is a hit; the median runs over all hits."""
    higher, ties = np.asarray(higher, dtype=np.int64), np.asarray(ties, dtype=np.int64)
    ind = np.repeat(higher, ties) + (np.arange(int(ties.sum())) - np.repeat(np.cumsum(ties) - ties, ties))
    return {"R1": np.array(float(np.sum(ind == 0)) / len(ind)), "R5": np.array(float(np.sum(ind < 5)) / len(ind)),
            "R10": np.array(float(np.sum(ind < 10)) / len(ind)), "MR": np.array(np.median(ind) + 1)}


def _clip_vlen(item) -> int:
    return int(item["vlen"]) if "vlen" in item else int(np.shape(item["feature"])[0])


def plan_clip_groups(clips, num_clips: int = 10, max_windows: int = 256):
    """Model calls for `test_retrieval_batched`: the windows of all clips (`clip_windows`, seq_len == -1) grouped by window length
    -- the position table is interpolated per length, so the windows of one `get_visual_feature` call must share it -- and each
    group cut into calls of at most `max_windows` windows.  Pure host function.  Returns a list of
    {'win', 'clip' [w], 'window' [w], 'idx' [w, win] frame indices inside the clip's own video, 's_idx' [w], 'e_idx' [w]}
    (int64 arrays); groups by ascending window length, windows in clip order inside a group."""
    if max_windows < 1:
        raise ValueError("max_windows must be positive")
    groups = {}
    for c, item in enumerate(clips):
        idx, s_idx, e_idx = clip_windows(_clip_vlen(item), item["start"], item["end"], num_clips, -1)
        g = groups.setdefault(idx.shape[1], {"clip": [], "window": [], "idx": [], "s_idx": [], "e_idx": []})
        g["clip"].append(np.full(num_clips, c, dtype=np.int64))
        g["window"].append(np.arange(num_clips, dtype=np.int64))
        g["idx"].append(idx.astype(np.int64))
        g["s_idx"].append(np.asarray(s_idx, dtype=np.int64))
        g["e_idx"].append(np.asarray(e_idx, dtype=np.int64))
    calls = []
    for win in sorted(groups):
        g = {k: np.concatenate(v, 0) for k, v in groups[win].items()}
        for a in range(0, len(g["clip"]), max_windows):
            calls.append({"win": int(win), **{k: v[a:a + max_windows] for k, v in g.items()}})
    return calls


@torch.no_grad()
def test_retrieval_batched(clips, model, embed_text, *, sim: str = "cos", seq_len: int = 64, num_clips: int = 10,
                           max_windows: int = 256, return_sim: bool = False, text_batch: int = 1024, return_features: bool = False):
    """`test_retrieval` without the per-clip loop: the same twelve metrics.  Every video's features go to the device once, frames
    are gathered there, one `get_visual_feature` call per planned group of windows (`plan_clip_groups`), clip pooling by
    tan_segment_pool_*, text embedded in batches, centring / standardising as [n, 512] device steps, and the three rankings by
    tan_rank_topk with pair = arange(n) -- no [n, n] matrix and one read-back at the end.  `return_sim` adds the [n, n] text x video
    matrix (for tests), `return_features` the pooled clip and text features (device tensors)."""
    from . import ops
    clips = list(clips)
    n, dev = len(clips), torch.device("cuda", torch.cuda.current_device())
    cos = sim == "cos"
    # every distinct feature array once
    slot, feats, base, rows = {}, [], [], 0
    for item in clips:
        key = id(item["feature"])
        if key not in slot:
            slot[key] = len(feats)
            feats.append(torch.as_tensor(item["feature"]))
            base.append(rows)
            rows += feats[-1].shape[0]
    packed = torch.cat(feats, 0).to(dev)
    clip_base = np.array([base[slot[id(item["feature"])]] for item in clips], dtype=np.int64)
    acc = torch.zeros(n, 512, device=dev)
    cnt = torch.zeros(n, device=dev)
    for call in plan_clip_groups(clips, num_clips, max_windows):
        w, win = call["idx"].shape
        gidx = torch.from_numpy(call["idx"] + clip_base[call["clip"]][:, None]).to(dev)
        video = packed.index_select(0, gidx.view(-1)).view(w, win, packed.shape[1])
        v = model.get_visual_feature(video, torch.zeros(w, win, device=dev, dtype=torch.bool),
                                     interpolate_from=seq_len if win >= seq_len else None)
        stage = v[:, -1] if v.dim() == 4 else v                                     # last deep-supervision stage, in place
        table = torch.from_numpy(np.stack([call["clip"], call["s_idx"], call["e_idx"] - call["s_idx"]], 1).astype(np.int32)).to(dev)
        ops.segment_pool_acc(stage, table, acc, cnt, normalize=cos)
    V = ops.segment_pool_final(acc, cnt, torch.empty(n, 512, device=dev), normalize=cos)
    strs = [item["str"] for item in clips]
    T = torch.cat([model.get_textual_feature(embed_text(strs[a:a + text_batch]).to(dev)).float().reshape(-1, 512)
                   for a in range(0, n, text_batch)], 0).contiguous()
    if cos:
        T = ops.l2norm_fwd(T, torch.empty_like(T), None, n, 512)
    Vc, Tc = V - V.mean(0, keepdim=True), T - T.mean(0, keepdim=True)
    Vs, Ts = Vc / Vc.std(0, unbiased=False, keepdim=True), Tc / Tc.std(0, unbiased=False, keepdim=True)
    pair = torch.arange(n, dtype=torch.int32, device=dev)
    counts = torch.empty(6, n, dtype=torch.int32, device=dev)
    for i, (t, v) in enumerate(((T, V), (Tc, Vc), (Ts, Vs))):
        ops.rank_topk(t.contiguous(), v.contiguous(), pair, 0, out=(counts[2 * i], counts[2 * i + 1], None, None))
    out = [None]
    if return_sim:
        s = torch.empty(n, n, device=dev)
        ops.gemm(T, V, s, M=n, N=n, K=512)
        out.append(s)
    counts_h = counts.cpu().numpy()                                                 # the one read-back the metrics need
    metrics = metrics_from_counts(counts_h[0], counts_h[1])
    for tag, i in (("C", 1), ("S", 2)):
        m = metrics_from_counts(counts_h[2 * i], counts_h[2 * i + 1])
        for k in ("R1", "R5", "R10", "MR"):
            metrics[f"{tag}-{k}"] = m[k]
    out[0] = metrics
    if return_sim:
        out[1] = out[1].cpu().numpy()
    if return_features:
        out.append((V, T))
    return out[0] if len(out) == 1 else tuple(out)
