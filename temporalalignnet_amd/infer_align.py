"""Corpus auto-alignment (HTM-AA): a trained aligner over a corpus of long videos -> every sentence's alignability score and
aligned timestamp.  The reference switches this on with `--inference 1 --worker_id N` (train/config.py:50-51, train/main.py:226-251,
424-426) and calls `eval.inference_zeroshot_align.inference_alignment_htm`, a module its release does not ship; HTM-AA-v1 is that
module's output (htm_aa/readme.md:3,24-32).  What it must compute is the evaluation loop of eval/eval_zeroshot_align.py:129-223 with
every sentence as a window candidate (a corpus has no ground truth):

  * windows: `eval_align.plan_windows` -- the rule the HTM-Align evaluation uses too;
  * passes of up to `windows_per_pass` windows, cut across video boundaries (a long video spans passes): one `tan_window_pack`
    launch builds the pass's batch from the chunk's packed features and sentence embeddings, one `model.eval_windows` call runs
    both stacks, one `tan_window_stitch_acc` launch folds the last-stage similarities into the chunk's [K, vlen] accumulators;
  * per chunk of videos: one `tan_window_stitch_final` launch (stitched rows, first arg-max, softmax maximum, score, coverage) and
    one read-back.  Sentences are embedded once per chunk; the next chunk's feature files are read on a background thread into
    pinned memory and copied on a side stream while the current chunk computes.
  * on request (`decode="monotonic"`, `--decode monotonic`): one `tan_monotonic_decode` launch per chunk between the two, a
    dynamic program over the stitched rows that gives every video's sentences non-decreasing seconds in ASR start order.
  * on request (`decode="segments"`, `--decode segments [--width W]`): one `tan_segment_decode` launch per chunk instead, which
    gives every video's sentences ordered, disjoint intervals of seconds.

    python -m temporalalignnet_amd.infer_align --checkpoint C --feature-dir F --asr-json A --vlen-csv V --vocab s3d_dict.npy --out X.csv
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import queue
import sys
import threading

import numpy as np
import torch

from . import ops
from .data_htm import read_vlen_csv
from .eval_align import check_width, plan_windows

# include/tan_hip.h, tan_attn_*: the joint stack's sequence (seq_len frames + the window's sentences) is at most 448 (f32) / 320 (bf16)
JOINT_MAX_LEN = {torch.float32: 448, torch.bfloat16: 320}
PASSES_PER_CHUNK = 4            # a chunk closes once it holds this many full passes of windows (or the corpus ends)
WIN_FIELDS = 8                  # TAN_WIN_FIELDS


def _round8(n):
    return (n + 7) // 8 * 8


def _aligner(model):
    return getattr(model, "online", model)            # TwinTemporalAligner: the online model answers eval_windows


class _Chunk:
    """Videos evaluated together: their windows (table rows in plan order), packed features and accumulator layout."""

    def __init__(self, items, plans, seq_len, windows_per_pass, ordered=False):
        self.items, self.ordered = items, ordered
        K = np.array([len(it["str"]) for it in items], dtype=np.int64)
        V = np.array([it["vlen"] for it in items], dtype=np.int64)
        self.k_off = np.concatenate([[0], np.cumsum(K)])
        self.v_off = np.concatenate([[0], np.cumsum(V)])
        self.a_off = np.concatenate([[0], np.cumsum(K * V)])
        self.n_rows, self.n_acc = int(self.k_off[-1]), int(self.a_off[-1])
        if max(self.n_acc, int(self.v_off[-1])) >= 2 ** 31:
            raise ValueError(f"chunk of {[it['vid'] for it in items]} exceeds the int32 window table")
        tab = [(self.v_off[i] + s0, e0 - s0, self.k_off[i] + left, right - left, s0, V[i], self.a_off[i], self.k_off[i])
               for i, plan in enumerate(plans) for s0, e0, left, right in plan]
        self.table = torch.from_numpy(np.asarray(tab, dtype=np.int32).reshape(-1, WIN_FIELDS))
        rows = np.zeros((self.n_rows, 2), dtype=np.int32)
        for i in range(len(items)):
            k0, k1 = self.k_off[i], self.k_off[i + 1]
            rows[k0:k1, 0] = self.a_off[i] + np.arange(k1 - k0) * V[i]
            rows[k0:k1, 1] = V[i]
        self.rows = torch.from_numpy(rows)
        self.passes = []
        for p0 in range(0, len(tab), windows_per_pass):
            p1 = min(p0 + windows_per_pass, len(tab))
            self.passes.append((p0, p1, _round8(int(self.table[p0:p1, 3].max()))))
        self.seq_len = seq_len

    # the monotonic decode's tables (tan_monotonic_decode), built when asked for: a run without the decode does not pay for them
    @property
    def order(self):
        """[n_rows] int32: per video its packed rows by ASR start, equal starts by sentence index."""
        order = [self.k_off[i] + np.argsort(np.asarray(it["start"], dtype=np.float64), kind="stable") for i, it in enumerate(self.items)]
        return torch.from_numpy(np.concatenate(order + [np.zeros(0, np.int64)]).astype(np.int32))

    @property
    def vtab(self):
        """[n_videos, 3] int32: first index into order, count, offset of the video's row in the [sum vlen] scratch."""
        return torch.from_numpy(np.stack([self.k_off[:-1], np.diff(self.k_off), self.v_off[:-1]], 1).astype(np.int32).reshape(-1, 3))

    def load(self, device, stream):
        """Feature files -> one pinned [sum vlen, Dv] buffer -> device on `stream` (the prefetch thread)."""
        host = load_packed(self.items, self.v_off)
        self.host = (host, self.table.pin_memory(), self.rows.pin_memory())     # alive until the copies have run
        if self.ordered:
            self.host += (self.order.pin_memory(), self.vtab.pin_memory())
        with torch.cuda.stream(stream):
            self.tensors = tuple(t.to(device, non_blocking=True) for t in self.host)
            self.video, self.table_d, self.rows_d = self.tensors[:3]
            self.order_d, self.vtab_d = self.tensors[3:] if self.ordered else (None, None)
            self.ready = torch.cuda.Event()
            self.ready.record(stream)


def load_packed(items, v_off):
    """The items' feature arrays (or the callables that read them) -> one pinned [sum vlen, Dv] buffer."""
    feats = []
    for it in items:
        v = it["video"]() if callable(it["video"]) else it["video"]
        v = torch.as_tensor(v)
        if v.dim() != 2 or v.shape[0] != it["vlen"]:
            raise ValueError(f"{it['vid']}: features {tuple(v.shape)}, expected [{it['vlen']}, Dv]")
        feats.append(v)
    dtype = feats[0].dtype
    for f in feats[1:]:
        dtype = torch.promote_types(dtype, f.dtype)
    host = torch.empty((int(v_off[-1]), feats[0].shape[1]), dtype=dtype, pin_memory=True)
    for f, a, b in zip(feats, v_off[:-1], v_off[1:]):
        host[a:b].copy_(f)
    return host


def _chunks(videos, seq_len, windows_per_pass, candidates, max_sentences, on_reject, ordered=False):
    items, plans, n = [], [], 0
    for it in videos:
        it = dict(it)
        it["str"] = list(it["str"])
        if "vlen" not in it:
            it["vlen"] = int(len(it["video"]))
        try:
            plan = plan_windows(it["start"], it["end"], it["vlen"], seq_len, None if candidates is None else candidates(it),
                                max_sentences=max_sentences, vid=it.get("vid"))
        except ValueError as e:
            if on_reject is None:
                raise
            on_reject(it.get("vid"), str(e))
            continue
        items.append(it)
        plans.append(plan)
        n += len(plan)
        if n >= windows_per_pass * PASSES_PER_CHUNK:
            yield _Chunk(items, plans, seq_len, windows_per_pass, ordered)
            items, plans, n = [], [], 0
    if items:
        yield _Chunk(items, plans, seq_len, windows_per_pass, ordered)


def _prefetch(chunks, device):
    """Plans and loads the next chunk on a background thread while the current one computes (data_htm.DevicePrefetcher idiom)."""
    q: queue.Queue = queue.Queue(maxsize=1)
    stop = threading.Event()
    stream = torch.cuda.Stream(device)

    def producer():
        try:
            torch.cuda.set_device(device)
            for ch in chunks:
                if stop.is_set():
                    return
                ch.load(device, stream)
                q.put(ch)
            q.put(None)
        except BaseException as e:                    # surfaces on the consuming thread
            q.put(e)

    th = threading.Thread(target=producer, daemon=True)
    th.start()
    try:
        while True:
            ch = q.get()
            if ch is None:
                return
            if isinstance(ch, BaseException):
                raise ch
            cur = torch.cuda.current_stream(device)
            cur.wait_event(ch.ready)
            for t in ch.tensors:                      # whatever the chunk's load() put on the device
                t.record_stream(cur)
            yield ch
    finally:
        stop.set()
        while th.is_alive():
            try:
                q.get_nowait()
            except queue.Empty:
                th.join(timeout=0.05)


@torch.no_grad()
def align_corpus(model, videos, embed_text, seq_len=64, windows_per_pass=256, candidates=None, return_sim=False, on_reject=None,
                 decode=None, keep_threshold=None, width=1.0):
    """Yield per video {'vid', 'str', 'timestamp' [K] int64, 'confidence' [K], 'score' [K], 'covered' [K] bool, ('sim' [K, vlen])}.

    `videos`: iterable of {'vid', 'start' [K], 'end' [K], 'str' [K], 'video'} -- 'video' is [vlen, Dv] (array / tensor, f32 / f16 /
    bf16) or a callable that reads it, then 'vlen' is required (the corpus reader's items: files are read on the prefetch thread).
    `embed_text(list[str]) -> [K, Dt]` device tensor.  `candidates(item) -> bool [K]`: the sentences that activate a window (the
    HTM-Align evaluation's ~aligned); None = every sentence.  timestamp = first arg-max of the stitched row, confidence = max of its
    softmax over time, score = mean joint alignability logit over the windows holding the sentence (with the alignability head)
    else the row maximum (eval_zeroshot_align.py:219-223); covered = some window holds the sentence.  A video whose windows would
    hold more sentences than the joint stack accepts raises ValueError, or is passed to `on_reject(vid, message)` and skipped.

    `decode="monotonic"`: order-preserving timestamps on top of the above (one `tan_monotonic_decode` launch per chunk).  Per video,
    the kept sentences -- covered, and with `keep_threshold` also score > keep_threshold -- taken by ASR start (equal starts by
    sentence index) get the non-decreasing seconds t_0 <= t_1 <= ... that maximise the summed stitched similarity sum_i sim[i][t_i];
    ties go to the earliest seconds, last sentence first (include/tan_hip.h has the recurrence).  A constant added to a row does
    not move the path, so it is also the Viterbi path under each row's log-softmax over time, the quantity 'timestamp' arg-maxes.
    Results gain 'ordered_timestamp' [K] int64 (-1 where not kept), 'ordered' [K] bool (kept) and 'path_score' (float, the sum
    along the path; 0.0 without a kept sentence); the other keys are what they are without `decode`.

    `decode="segments"`: aligned intervals on top of the above (one `tan_segment_decode` launch per chunk).  Per video, the same kept
    sentences in the same order as for "monotonic" get inclusive intervals [segment_start, segment_end] of seconds that are ordered
    and disjoint (gaps allowed) and maximise the summed gain sim[i][t] - bias[i] over their seconds, bias[i] = sim[i][timestamp_i] -
    width: a second pays while it lies within `width` logits of its row's peak (include/tan_hip.h has the recurrence and the tie
    rule).  `width` >= 0 (else ValueError); the default 1.0 is `search_moments`' default (its TEMPERATURE, 0.07 in cosine) on the
    stitched rows' 1/0.07 scale -- a convention, tuned on nothing (no real data was available when it was chosen).  Results gain
    'segment_start' / 'segment_end' [K] int64 (-1 where not kept, or when the video has more kept sentences than seconds),
    'segmented' [K] bool (kept) and 'path_score' (float; 0.0 without a kept sentence, -inf for such an infeasible video); the
    other keys are what they are without `decode`."""
    if decode not in (None, "monotonic", "segments"):
        raise ValueError(f"decode: None, 'monotonic' or 'segments', not {decode!r}")
    if decode == "segments":
        width = check_width(width)
    ordered = decode is not None                      # either decode reads the chunk's order / vtab tables
    empty = {None: None, "monotonic": (np.zeros(0, np.int32), 0.0),
             "segments": (np.zeros((0, 2), np.int32), 0.0, np.zeros(0, bool))}[decode]
    net = _aligner(model)
    head = bool(net.use_alignability_head)
    if head and net.num_decoder_layers < 3:
        raise ValueError("the alignability score reads joint stage index 2 (eval_zeroshot_align.py:186): >= 3 decoder layers")
    max_sentences = (JOINT_MAX_LEN[net.compute_dtype] - seq_len) // 8 * 8
    device = torch.device("cuda", torch.cuda.current_device())
    T = seq_len
    chunks = _chunks(videos, seq_len, windows_per_pass, candidates, max_sentences, on_reject, ordered)
    for ch in _prefetch(chunks, device):
        if ch.n_rows == 0:
            for it in ch.items:
                yield _result(it, np.zeros((4, 0), np.float32), None if not return_sim else np.zeros((0, it["vlen"]), np.float32),
                              decode, empty)
            continue
        emb = embed_text([s for it in ch.items for s in it["str"]]).contiguous()
        acc_j, acc_d, cnt = (torch.zeros(ch.n_acc, device=device) for _ in range(3))
        tcnt = torch.zeros(ch.n_rows, device=device)
        a_sum = torch.zeros(ch.n_rows, device=device) if head else None
        for p0, p1, Kp in ch.passes:
            W, tab = p1 - p0, ch.table_d[p0:p1]
            vid = torch.empty(W, T, ch.video.shape[1], dtype=ch.video.dtype, device=device)
            txt = torch.empty(W, Kp, emb.shape[1], dtype=emb.dtype, device=device)
            vm = torch.empty(W, T, dtype=torch.bool, device=device)
            tm = torch.empty(W, Kp, dtype=torch.bool, device=device)
            ops.window_pack(ch.video, emb, tab, T, Kp, vid, vm, txt, tm)
            r = model.eval_windows(vid, txt, vm, tm)
            last = lambda x: x.permute(1, 0, 2, 3)[-1]                           # noqa: E731  [W,S,T,Kp] view of [S][W][T][Kp]
            a_j = r["alignability-joint"].permute(1, 0, 2, 3)[2].view(W, Kp) if head else None
            ops.window_stitch_acc(last(r["sim"]), last(r["dual-sim"]), a_j, tab, acc_j, acc_d, cnt, tcnt, a_sum)
        res = torch.empty(4, ch.n_rows, device=device)
        ops.window_stitch_final(acc_j, acc_d, cnt, tcnt, a_sum, ch.rows_d, res)
        if ordered:
            keep = res[3] > 0                         # covered; the threshold compares as write_rows does, in f64
            if keep_threshold is not None:
                keep = keep & (res[2].double() > float(keep_threshold))
            path = torch.empty(len(ch.items), device=device)
            run = torch.empty(int(ch.v_off[-1]), device=device)
        if decode == "monotonic":
            ts = torch.empty(ch.n_rows, dtype=torch.int32, device=device)
            ops.monotonic_decode(acc_j, ch.rows_d, ch.order_d, ch.vtab_d, keep, torch.empty(ch.n_acc, dtype=torch.int32, device=device),
                                 run, ts, path)
        elif decode == "segments":
            # bias = the row's maximum (the stitched row at its first arg-max, res[0]) - width: a gather and one f32 subtraction
            bias = acc_j[ch.rows_d[:, 0].long() + res[0].long()] - torch.full((), width, dtype=torch.float32, device=device)
            ts = torch.empty(ch.n_rows, 2, dtype=torch.int32, device=device)
            ops.segment_decode(acc_j, ch.rows_d, ch.order_d, ch.vtab_d, keep, bias,
                               torch.empty(2 * ch.n_acc, dtype=torch.int32, device=device), run, ts, path)
        res_h = torch.empty(res.shape, pin_memory=True)
        res_h.copy_(res, non_blocking=True)
        if return_sim:
            sim_h = torch.empty(acc_j.shape, pin_memory=True)
            sim_h.copy_(acc_j, non_blocking=True)
        if ordered:
            ts_h, path_h = torch.empty(ts.shape, dtype=ts.dtype, pin_memory=True), torch.empty(path.shape, pin_memory=True)
            ts_h.copy_(ts, non_blocking=True)
            path_h.copy_(path, non_blocking=True)
        if decode == "segments":                      # the mask the kernel read: an infeasible video's kept rows carry no segment
            keep_h = torch.empty(keep.shape, dtype=torch.bool, pin_memory=True)
            keep_h.copy_(keep, non_blocking=True)
        torch.cuda.current_stream(device).synchronize()
        res_h = res_h.numpy()
        for i, it in enumerate(ch.items):
            k0, k1 = ch.k_off[i], ch.k_off[i + 1]
            sim = sim_h.numpy()[ch.a_off[i]:ch.a_off[i + 1]].reshape(k1 - k0, it["vlen"]).copy() if return_sim else None
            decoded = (ts_h.numpy()[k0:k1], float(path_h[i])) if ordered else None
            if decode == "segments":
                decoded += (keep_h.numpy()[k0:k1],)
            yield _result(it, res_h[:, k0:k1], sim, decode, decoded)


def _result(it, res, sim, decode=None, decoded=None):
    """`decoded`, for decode="monotonic": (seconds [K] int32 with -1 where not kept, path score); for decode="segments": ((start, end)
    [K, 2] int32 with (-1, -1) where not kept or infeasible, path score, kept [K] bool)."""
    out = {"vid": it.get("vid"), "str": it["str"], "timestamp": res[0].astype(np.int64), "confidence": res[1].copy(),
           "score": res[2].copy(), "covered": res[3] > 0}
    if sim is not None:
        out["sim"] = sim
    if decode == "monotonic":
        out["ordered_timestamp"] = decoded[0].astype(np.int64)
        out["ordered"] = decoded[0] >= 0
        out["path_score"] = decoded[1]
    elif decode == "segments":
        out["segment_start"], out["segment_end"] = decoded[0][:, 0].astype(np.int64), decoded[0][:, 1].astype(np.int64)
        out["segmented"] = decoded[2].copy()
        out["path_score"] = decoded[1]
    return out


# ---------------------------------------------------------------------------------------------------------------- the corpus on disk
def feature_path(feature_dir, vid):
    """`{vid}.mp4.npy`, else `{vid}.webm.npy` (data/loader_htm.py:136-143)."""
    p = os.path.join(feature_dir, f"{vid}.mp4.npy")
    return p if os.path.exists(p) else os.path.join(feature_dir, f"{vid}.webm.npy")


def load_features(feature_dir, vid, vlen):
    """[vlen, Dv] float32 / float16 features of one video as stored (the first `vlen` rows)."""
    f = np.load(feature_path(feature_dir, vid))
    if f.shape[0] < vlen:
        raise ValueError(f"{vid}: {f.shape[0]} feature rows, htm_vlen.csv says {vlen}")
    return f[:vlen]


def read_corpus(feature_dir, asr_json, vlen_csv, worker_id=0, num_workers=1):
    """Items for `align_corpus` from the on-disk formats data_htm.py documents: the videos listed in both the vlen csv and the
    sentencified ASR json, sorted by vid, shard `[worker_id::num_workers]` (the reference's --worker_id).  vlen comes from the csv.
    Sentences that start at or after vlen are dropped (no frame of the video can hold them); the rest keep their ASR text as is.
    Features are read lazily (`item['video']()`), on align_corpus's prefetch thread."""
    with open(asr_json) as f:
        asr = json.load(f)
    vlen = read_vlen_csv(vlen_csv)
    for vid in sorted(v for v in vlen if v in asr)[worker_id::num_workers]:
        n, d = vlen[vid], asr[vid]
        keep = [i for i, s in enumerate(d["start"]) if float(s) < n]
        yield {"vid": vid, "vlen": n, "start": np.array([d["start"][i] for i in keep], dtype=np.float64),
               "end": np.array([d["end"][i] for i in keep], dtype=np.float64), "str": [str(d["text"][i]) for i in keep],
               "video": lambda vid=vid, n=n: load_features(feature_dir, vid, n)}


CSV_COLUMNS = ("vid", "timestamp", "text", "score", "confidence")
SEGMENT_COLUMNS = ("start", "end")                    # appended by --decode segments


def write_rows(writer, result, threshold=None):
    """HTM-AA rows of one video: covered sentences only, and with `threshold` only those with score > threshold.  A result of
    `align_corpus(decode="monotonic")` writes its ordered timestamps in the `timestamp` column (decode it with the same threshold as
    `keep_threshold`: the rows written are then exactly the decoded ones); rows and columns are the same either way.  A result of
    `align_corpus(decode="segments")` keeps every column as it is without a decode and appends SEGMENT_COLUMNS, the interval's
    inclusive first and last second (-1 -1 for a video with more rows than seconds), again for the decoded rows under the same threshold."""
    stamp = result["ordered_timestamp"] if "ordered_timestamp" in result else result["timestamp"]
    n = 0
    for k, text in enumerate(result["str"]):
        if not result["covered"][k] or (threshold is not None and not float(result["score"][k]) > threshold):
            continue
        row = [result["vid"], int(stamp[k]), text, repr(float(result["score"][k])), repr(float(result["confidence"][k]))]
        if "segment_start" in result:
            row += [int(result["segment_start"][k]), int(result["segment_end"][k])]
        writer.writerow(row)
        n += 1
    return n


def _infer_arch(state_dict):
    keys = [k[len("module."):] if k.startswith("module.") else k for k in state_dict]
    keys = [k[len("online."):] for k in keys if k.startswith("online.")] or keys
    count = lambda p: len({k.split(".")[2] for k in keys if k.startswith(p + ".resblocks.")})      # noqa: E731
    return count("video_temporal_encoder"), count("joint_temporal_encoder"), int(any(k.startswith("binary_head.") for k in keys))


def build_aligner(checkpoint, vocab, model="init", dtype="bf16"):
    """A TemporalAligner / TwinTemporalAligner with a Word2Vec language model sized to `vocab`, loaded by checkpoint.load_for_test.
    Layer counts and the alignability head are read off the checkpoint.  Position offsets are not drawn (random_pos_start = 0):
    the random offset is a training augmentation and would make the output depend on the RNG."""
    from .checkpoint import load_for_test
    from .train import build_model, default_args
    from .word2vec_model import Word2VecModel
    sd = torch.load(checkpoint, map_location="cpu", weights_only=False)["state_dict"]
    E, D, head = _infer_arch(sd)
    args = default_args(model=model, num_encoder_layers=E, num_decoder_layers=D, use_alignability_head=head)
    m = build_model(args, compute_dtype=dtype, language_model=None, random_pos_start=0)
    V = len(vocab) + 1
    if model == "cotrain":
        m.online.bert, m.target.bert = Word2VecModel(num_embeddings=V, compute_dtype=dtype), Word2VecModel(num_embeddings=V, compute_dtype=dtype)
        m.bert = m.online.bert
    else:
        m.bert = Word2VecModel(num_embeddings=V, compute_dtype=dtype)
    m.cuda().eval()
    _, missing, unexpected = load_for_test(m, checkpoint)
    if missing or unexpected:
        raise ValueError(f"{checkpoint}: missing {missing[:5]}, unexpected {unexpected[:5]}")
    return m


def make_embed_text(model, tokenizer):
    def embed_text(sentences):
        t = tokenizer(sentences, return_tensors="pt")
        return model.lang_model(t["input_ids"].cuda(), t["attention_mask"].cuda())["pooler_output"].float()
    return embed_text


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--feature-dir", required=True)
    ap.add_argument("--asr-json", required=True)
    ap.add_argument("--vlen-csv", required=True)
    ap.add_argument("--vocab", required=True, help="s3d_dict.npy (the Word2Vec vocabulary)")
    ap.add_argument("--out", required=True, help="csv: vid,timestamp,text,score,confidence")
    ap.add_argument("--worker-id", type=int, default=0)
    ap.add_argument("--num-workers", type=int, default=1)
    ap.add_argument("--threshold", type=float, default=None, help="keep rows with score > threshold (default: every covered sentence)")
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--model", choices=("init", "cotrain"), default="init")
    ap.add_argument("--decode", choices=("argmax", "monotonic", "segments"), default="argmax",
                    help="timestamp column: each sentence's own arg-max (default), or per video the non-decreasing seconds in ASR "
                         "start order with the largest summed similarity over the rows written (--threshold picks them); "
                         "segments: the arg-max column, and appended columns start,end -- per video ordered, disjoint intervals "
                         "of inclusive seconds for the rows written")
    ap.add_argument("--width", type=float, default=1.0,
                    help="--decode segments: a second counts for its sentence while its similarity lies within this many logits "
                         "of the row's peak (>= 0; the default is a convention, tuned on nothing)")
    a = ap.parse_args(argv)
    if not 0 <= a.worker_id < a.num_workers:
        ap.error("--worker-id must lie in [0, --num-workers)")
    if not a.width >= 0:
        ap.error("--width must be a non-negative number")
    return a


def main(argv=None):
    a = parse_args(argv)
    from .word2vec_model import Word2VecTokenizer
    vocab = np.load(a.vocab)
    model = build_aligner(a.checkpoint, vocab, a.model, a.dtype)
    embed = make_embed_text(model, Word2VecTokenizer(max_words=32, vocab=vocab))
    corpus = read_corpus(a.feature_dir, a.asr_json, a.vlen_csv, a.worker_id, a.num_workers)
    rejected = []

    def on_reject(vid, msg):
        rejected.append(vid)
        print(f"skipped {vid}: {msg}", file=sys.stderr)

    n_vid = n_rows = 0
    with open(a.out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS + (SEGMENT_COLUMNS if a.decode == "segments" else ()))
        for res in align_corpus(model, corpus, embed, on_reject=on_reject, decode=None if a.decode == "argmax" else a.decode,
                                keep_threshold=a.threshold if a.decode != "argmax" else None, width=a.width):
            n_rows += write_rows(w, res, a.threshold)
            n_vid += 1
    print(f"{a.out}: {n_rows} sentences from {n_vid} videos" + (f", {len(rejected)} skipped" if rejected else ""), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
