"""Corpus search with the dual encoder: "which seconds of which videos match this sentence".

The reference's `get_visual_feature` "can be used for retrieval setting" (model/tan_model.py:152); `infer_align.align_corpus` asks
the dual encoder only about a video's own ASR sentences.  Here the video side is computed ONCE into a per-second index and any
sentence is ranked against all of it:

  * `build_index`: the window stepping of `eval_align.plan_windows` with every second covered (no sentences involved), passes of up
    to `windows_per_pass` windows cut across video boundaries and packed by `tan_window_pack`, the video stack only, then
    `tan_window_feat_acc / _final`: index[t] = the mean over the windows covering second t of the L2-normalised last-stage feature.
    The text side of the dual similarity is the same unit vector t_hat in every window, so <index[t], t_hat> / 0.07 is the stitched
    dual similarity of eval_zeroshot_align.py:198,201 -- computed without knowing the sentence.
  * `search`: sentences -> `get_textual_feature`, normalised -> `tan_rank_topk` against the index (no [Q, N] score matrix) -> rows
    mapped to (vid, second) on the host.
  * an e4m3 index (`build_index(dtype="e4m3")`, `VideoIndex.quantize`, `--index-dtype e4m3`) keeps a row as 512 OCP e4m3fn codes
    and one power-of-two f32 scale (include/tan_hip.h): 516 bytes per second of video instead of 1 KiB.  The query is quantised by
    the same kernel and `tan_rank_topk_e4m3` sweeps the codes.
  * `search_moments`: neighbouring seconds of a video score almost alike, so the k best ROWS are a few videos' adjacent seconds.
    `tan_rank_topk_video` ranks VIDEOS by their best second in the same matrix-free sweep, and `tan_moment_extent` measures how
    far the matching moment extends around that second (`query --moments`).
  * `search_sequences`: "which videos show these steps, in this order, and when?"  `tan_sequence_topk` scores every video of the
    index by the best non-decreasing assignment of seconds to an ordered list of sentences -- `tan_monotonic_decode`'s path, fused
    into the same matrix-free sweep -- and keeps the k best videos; `tan_sequence_scores` and the decode itself then give the
    winners' seconds (`query --sequence`).
  * `search_rerank`: two stages.  The dual sweep (`tan_rank_topk_video`) proposes `pool` videos per sentence; one 64-second window
    around each candidate's best second is cut out of the index's STEM store (`build_index(keep_stem=True)`: video_pre_proj of
    every second, the part of the video input that depends on neither window nor text), run through the joint stack
    (`TemporalAligner.joint_from_stem`) and reduced by `tan_rerank_tail` to the joint cosine, the second the joint encoder picks,
    its softmax confidence and the alignability logit; `tan_rerank_select` orders the candidates (`query --rerank`).
  * `ShardedIndex`: several index files (one per `index --worker-id`) searched together, or one corpus larger than the card streamed
    from pinned host memory.  Every shard is swept on its own and `tan_topk_fold` folds the per-shard lists on the device under the
    sweeps' own order: `search`, `search_moments` and `search_sequences` return what they return for `VideoIndex.concat` of the
    shards, bit for bit (`query --shard`, `query --host-resident`, `merge`).
  * `restrict`: `index.restrict(videos=, exclude=, windows=)` gives a `RowFilter` -- a playlist, the videos already shown, known
    time windows -- that `search`, `search_moments` and `search_rerank` take as `restrict=`.  The sweep walks only the 64-row tiles
    that hold an admitted row (`tan_row_filter_build`, `tan_rank_topk_filtered`) and returns those rows with the unrestricted
    sweep's scores; a host-resident shard without an admitted row is not copied (`query --only / --exclude / --within`).
  * `annotate`: the transposed question -- given a fixed vocabulary of step or action descriptions, which label does every second
    of every video show?  `tan_label_topk` keeps a tile of index rows resident and streams the LABEL matrix past it, so every row's
    k best labels come out of one launch without scratch; `Annotation.segments` turns the best labels into (video, start, end,
    label) runs on the device (`tan_label_runs`) and `Annotation.label_seconds` counts the seconds of every label (`annotate`).
    Neighbouring seconds score almost alike, so the best label flickers; `Annotation.decode` (`tan_label_decode`) is a per-video
    Viterbi decode over the kept lists that pays a penalty per label change, and `segments(..., switch=)` builds its runs from
    the decoded labels (`annotate --smooth PENALTY`).
  * `search_clips`: the questions that start from VIDEO -- "where else does this clip appear?" (re-uploads, compilations), "more
    like these twenty seconds".  A clip is up to 32 index rows (seconds of an indexed video, or rows of a freshly indexed one);
    `tan_clip_topk` lays it over every video second for second -- a diagonal sum over the same matrix-free score tile -- and keeps
    per clip the k videos with the best placement and where it starts (`similar`; no model is loaded).
  * `align_spans` / `search_copies`: the second stage of clip search, for a copy that was re-timed or re-cut.  A query of up to
    4096 seconds and a video give one [m, V] block of scores (`tan_sequence_scores`, the query as 32-row pieces), and
    `tan_local_align` finds the best LOCAL alignment in it -- steps along either axis allowed at a price, unrelated cells bridged
    at a price -- with its extent in both videos.  `search_copies` proposes the candidate videos by one `tan_clip_topk` sweep over
    the query's pieces and ranks them by that alignment (`similar --align`).
  * `align_paths` / `search_copies(paths=True)`: the same alignment with its second-to-second time map -- which seconds of the copy
    show each second of the query (`tan_local_align_path` records every step's decision and walks the best path back).
    `copy_interval`, `copy_inverse` and `transfer_segments` carry timestamps, chapter marks or `Annotation.segments` from the
    original onto the copy (`similar --align --map OUT.csv`).

    python -m temporalalignnet_amd.search index --checkpoint C --feature-dir F --asr-json A --vlen-csv V --vocab s3d_dict.npy --out I.npz
    python -m temporalalignnet_amd.search query --checkpoint C --vocab s3d_dict.npy --index I.npz -k 10 "crack two eggs" ...
    python -m temporalalignnet_amd.search query ... --moments [--width 0.07] "crack two eggs" ...
    python -m temporalalignnet_amd.search query ... --sequence "crack two eggs" "whisk them" "pour into the pan"
    python -m temporalalignnet_amd.search index ... --keep-stem;  ... query ... --rerank [--pool 32] "crack two eggs" ...
    python -m temporalalignnet_amd.search query ... --index I0.npz --shard I1.npz --shard I2.npz [--host-resident] "crack two eggs" ...
    python -m temporalalignnet_amd.search query ... --only VID --only-file vids.txt --exclude VID --within VID:30-90 "crack two eggs" ...
    python -m temporalalignnet_amd.search merge --out I.npz I0.npz I1.npz ...
    python -m temporalalignnet_amd.search annotate --checkpoint C --vocab s3d_dict.npy --index I.npz --labels steps.txt [-k K]
        [--threshold X] [--min-len M] [--smooth PENALTY] [--per-second] --out segments.csv
    python -m temporalalignnet_amd.search similar --index I.npz [--shard I1.npz ...] [--host-resident] --clip VID:10-29 [-k K] [--keep-source]
    python -m temporalalignnet_amd.search similar --index I.npz --clip VID:0-599 --align --threshold X [--skew Y] [--pool P] [--piece S] [-k K]
    python -m temporalalignnet_amd.search similar --index I.npz --clip VID:0-599 --align --threshold X --map OUT.csv
"""
from __future__ import annotations

import argparse
import sys
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .infer_align import JOINT_MAX_LEN, PASSES_PER_CHUNK, WIN_FIELDS, _aligner, _prefetch, load_packed

TEMPERATURE = 0.07
E4M3 = "e4m3"

# one hit of `search_moments`: the video, the moment's first / last second (inclusive), the best second, and its score
Moment = namedtuple("Moment", ("vid", "start", "end", "second", "score"))

# one hit of `search_sequences`: the video, the second of every step (non-decreasing), and the path score
SequenceHit = namedtuple("SequenceHit", ("vid", "seconds", "score"))

# one hit of `search_rerank`: the video, the second / cosine / softmax confidence / alignability logit (None without the head) of the
# joint encoder on the window around the dual encoder's best second, and that second and its dual score
Reranked = namedtuple("Reranked", ("vid", "second", "score", "confidence", "alignability", "dual_second", "dual_score"))
# one hit of `search_clips`: the video, the first / last second (inclusive) of the clip's best placement in it, and the mean score
# per second along that placement
ClipHit = namedtuple("ClipHit", ("vid", "start", "end", "score"))
MAX_CLIP_SECONDS = 32           # a clip's rows are one wave's 32 resident query columns (tan_clip_topk)
# one hit of `align_spans` / `search_copies`: the video, the first / last second (inclusive) of the copy in it, the first / last
# second of the QUERY that the copy shows, the alignment's score (the sum of score - threshold over its cells, minus skew per step
# along one axis alone) and the number of its cells
CopyHit = namedtuple("CopyHit", ("vid", "start", "end", "q_start", "q_end", "score", "cells"))
# one hit of `align_paths` / `search_copies(paths=True)`: the CopyHit, and int32 [q_end - q_start + 1, 2]: the first / last second of
# the video shown for each query second from q_start on
CopyPath = namedtuple("CopyPath", ("hit", "seconds"))
MAX_ALIGN_SECONDS = 4096        # a query of `align_spans`: 12 bits of tan_local_align's packed origin
PIECE_ROWS = 32                 # `align_spans` hands a query to tan_sequence_scores as sequences of this many rows
EMPTY_ROW = 0x7fffffff          # the row of an empty top-k slot (include/tan_hip.h)
RERANK_TEXT_SLOTS = 8         # a rerank window holds one sentence; `align_corpus` pads the text side to multiples of 8


def _is_e4m3(dtype):
    return dtype == E4M3 or dtype == torch.float8_e4m3fn


def plan_index_windows(vlen, seq_len=64):
    """[(s0, e0)]: window starts `arange(0, vlen - seq_len // 2, seq_len // 4)` as eval/eval_zeroshot_align.py:129-133 steps them,
    e0 = min(vlen, s0 + seq_len); a video of at most seq_len // 2 seconds, which that rule gives no window, gets one."""
    steps = np.arange(0, max(int(vlen) - seq_len // 2, 1), seq_len // 4)
    return [(int(s0), int(min(vlen, s0 + seq_len))) for s0 in steps]


class _IndexChunk:
    def __init__(self, items, seq_len, windows_per_pass):
        self.items = items
        V = np.array([it["vlen"] for it in items], dtype=np.int64)
        self.v_off = np.concatenate([[0], np.cumsum(V)])
        if int(self.v_off[-1]) >= 2 ** 31:
            raise ValueError("chunk exceeds the int32 window table")
        tab = [(self.v_off[i] + s0, e0 - s0, 0, 0, s0, V[i], 0, 0) for i, it in enumerate(items)
               for s0, e0 in plan_index_windows(it["vlen"], seq_len)]
        self.table = torch.from_numpy(np.asarray(tab, dtype=np.int32).reshape(-1, WIN_FIELDS))
        self.passes = [(p0, min(p0 + windows_per_pass, len(tab))) for p0 in range(0, len(tab), windows_per_pass)]

    def load(self, device, stream):
        self.host = (load_packed(self.items, self.v_off), self.table.pin_memory())
        with torch.cuda.stream(stream):
            self.video, self.table_d = self.tensors = tuple(t.to(device, non_blocking=True) for t in self.host)
            self.ready = torch.cuda.Event()
            self.ready.record(stream)


def _index_chunks(videos, seq_len, windows_per_pass):
    items, n = [], 0
    for it in videos:
        it = dict(it)
        if "vlen" not in it:
            it["vlen"] = int(len(it["video"]))
        if it["vlen"] < 1:
            raise ValueError(f"{it.get('vid')}: empty video")
        items.append(it)
        n += len(plan_index_windows(it["vlen"], seq_len))
        if n >= windows_per_pass * PASSES_PER_CHUNK:
            yield _IndexChunk(items, seq_len, windows_per_pass)
            items, n = [], 0
    if items:
        yield _IndexChunk(items, seq_len, windows_per_pass)


def _video_numbers(vids, names, what):
    """Video numbers named by `names` (vid strings: EVERY video that carries the string; or video numbers), ascending, distinct."""
    by_name = None
    out = set()
    for name in names:
        if isinstance(name, str):
            if by_name is None:
                by_name = {}
                for v, s in enumerate(vids):
                    by_name.setdefault(s, []).append(v)
            if name not in by_name:
                raise KeyError(f"{what}: no video {name!r} in the index")
            out.update(by_name[name])
        else:
            v = int(name)
            if v != name or not 0 <= v < len(vids):
                raise KeyError(f"{what}: no video number {name!r} in the index")
            out.add(v)
    return sorted(out)


def restrict_spans(v_off, vids, videos=None, exclude=None, windows=None):
    """(spans int64 [n, 2]: the admitted global rows as merged [lo, hi) spans, ascending; n_videos: videos with an admitted row) --
    the arithmetic of `VideoIndex.restrict` / `ShardedIndex.restrict`, on the host."""
    v_off = np.asarray(v_off, dtype=np.int64)
    admitted = list(range(len(vids))) if videos is None else _video_numbers(vids, videos, "restrict(videos)")
    if exclude is not None:
        drop = set(_video_numbers(vids, exclude, "restrict(exclude)"))
        admitted = [v for v in admitted if v not in drop]
    cut = {}
    for name, first, last in (windows or ()):
        for v in _video_numbers(vids, [name], "restrict(windows)"):
            vlen = int(v_off[v + 1] - v_off[v])
            a, b = max(int(first), 0), min(int(last), vlen - 1)
            cut.setdefault(v, [])
            if a <= b:
                cut[v].append((int(v_off[v]) + a, int(v_off[v]) + b + 1))
    spans, n_videos = [], 0
    for v in admitted:
        mine = sorted(cut[v]) if v in cut else [(int(v_off[v]), int(v_off[v + 1]))]
        n_videos += bool(mine)
        for lo, hi in mine:
            if spans and lo <= spans[-1][1]:
                spans[-1][1] = max(spans[-1][1], hi)
            else:
                spans.append([lo, hi])
    return np.asarray(spans, dtype=np.int64).reshape(-1, 2), n_videos


class RowFilter:
    """What `index.restrict(...)` returns and `search(..., restrict=)` takes: the rows of ONE index a search may return.
      spans [n, 2]   int64, global rows [lo, hi), ascending, merged (adjacent videos and overlapping windows give one span)
      n_rows         admitted rows;  n_videos: videos with an admitted row
      windowed       built with `windows`: `search_rerank` refuses it
      shards()       the shards that hold an admitted row, ascending (a `VideoIndex` is shard 0)
      shard_spans(s) / shard_rows(s) / shard_videos(s)   shard s's part: spans in the shard's OWN rows, admitted rows and videos
      image(s)       the device image of shard s's spans (`ops.row_filter_build`), built on first use and kept
    It belongs to the index that made it and refuses any other."""

    def __init__(self, index, spans, n_videos, windowed):
        self._index, self.spans, self.n_videos, self.windowed = index, spans, int(n_videos), bool(windowed)
        self.n_rows = int((spans[:, 1] - spans[:, 0]).sum())
        if self.n_rows == 0:
            raise ValueError("restrict: the filter admits no row")
        row_base, shard_v_off = index.row_base, [sh.v_off for sh in index.shards]
        self._parts, self._images = {}, {}
        for s in range(len(row_base) - 1):
            lo, hi = np.maximum(spans[:, 0], row_base[s]), np.minimum(spans[:, 1], row_base[s + 1])
            local = np.stack((lo, hi), 1)[lo < hi] - row_base[s]
            if len(local):
                first = np.searchsorted(shard_v_off[s], local[:, 0], side="right") - 1         # the videos a span touches
                last = np.searchsorted(shard_v_off[s], local[:, 1] - 1, side="right") - 1
                videos = int((last - first + 1).sum() - (first[1:] == last[:-1]).sum())         # spans ascend: only neighbours share one
                self._parts[s] = (local, int((local[:, 1] - local[:, 0]).sum()), videos)

    def check(self, index):
        if index is not self._index:
            raise ValueError("this RowFilter was made by another index's restrict()")

    def shards(self):
        return sorted(self._parts)

    def ready(self):
        """`shards()`, with every image built: nothing of the filter is left to do between the shards' sweeps"""
        return [s for s in self.shards() if self.image(s) is not None]

    def shard_spans(self, s):
        return self._parts[s][0]

    def shard_rows(self, s):
        return self._parts[s][1]

    def shard_videos(self, s):
        return self._parts[s][2]

    def image(self, s=0):
        if s not in self._images:
            spans = torch.from_numpy(self.shard_spans(s).astype(np.int32)).to(self._index.device)
            self._images[s] = ops.row_filter_build(spans, len(self._index.shards[s]))
        return self._images[s]

    def clip(self, row, start, end):
        """Global rows: [start, end] cut to the admitted span that holds `row`."""
        i = np.searchsorted(self.spans[:, 0], row, side="right") - 1
        return np.maximum(start, self.spans[i, 0]), np.minimum(end, self.spans[i, 1] - 1)


def _restrict(index, videos, exclude, windows):
    spans, n_videos = restrict_spans(index.v_off, index.vids, videos, exclude, windows)
    return RowFilter(index, spans, n_videos, windows is not None)


def _locate(index, shard, row):
    """(shard, shard-local row) of either kind of index -> (global video number, second)"""
    g = index.row_base[np.asarray(shard, dtype=np.int64)] + np.asarray(row, dtype=np.int64)
    v = np.searchsorted(index.v_off, g, side="right") - 1
    return v, g - index.v_off[v]


_RESTRICT_DOC = """The `RowFilter` that admits only some of this index's rows, for `search`, `search_moments` and `search_rerank`
        (`restrict=`).  videos: the videos to search (default: all); exclude: videos to leave out; both iterables of vid strings or
        video numbers -- a string names EVERY video that carries it (equal strings are distinct videos), an unknown one raises
        KeyError.  windows: iterable of (video, first_second, last_second), inclusive, clamped to the video; several windows of a
        video are merged; an admitted video that `windows` names is narrowed to them, the others stay whole.  ValueError when
        nothing is admitted."""


class VideoIndex:
    """feat [sum vlen, 512] (device, bf16 or f32): one row per second; v_off [n_videos + 1]: each video's first row; vids.
    An e4m3 index holds feat as uint8 codes and scale [sum vlen] f32, one power of two per row; scale is None otherwise.
    stem [sum vlen, 512] (bf16 or f32, the model's compute dtype) or None: `TemporalAligner.video_stem` of every second, what
    `search_rerank` cuts its windows from.  A bf16 stem adds 1 KiB per second: an e4m3 index with a stem is 516 + 1024 bytes per
    second, a bf16 one 2 KiB."""

    def __init__(self, feat, v_off, vids, scale=None, stem=None):
        self.feat, self.v_off, self.vids, self.scale = feat, np.asarray(v_off, dtype=np.int64), list(vids), scale
        self.stem = stem
        assert (scale is not None) == (feat.dtype == torch.uint8)
        assert stem is None or (stem.shape == (feat.shape[0], 512) and stem.dtype in (torch.bfloat16, torch.float32))
        self._v_off_dev = None
        # to the searches this is a `ShardedIndex` of one shard, itself (`shards`, `shard_views`): its rows and videos are the global ones
        self.row_base, self.video_base = (np.array([0, n], dtype=np.int64) for n in (feat.shape[0], len(self.vids)))

    @property
    def v_off_device(self):
        """v_off as int32 on feat's device, made on first use and kept (it is not part of the file format)."""
        if self._v_off_dev is None:
            self._v_off_dev = torch.from_numpy(self.v_off.astype(np.int32)).to(self.feat.device)
        return self._v_off_dev

    @property
    def e4m3(self):
        return self.scale is not None

    @property
    def device(self):
        return self.feat.device

    @property
    def row_dtype(self):
        """torch.float32, torch.bfloat16, or torch.uint8 for e4m3 codes"""
        return self.feat.dtype

    @classmethod
    def concat(cls, indices):
        """One index holding the rows, scales, stems, vids and v_off of `indices` one after the other, on the device of the first
        (CPU tensors work: `load(path, device="cpu")`).  Equal vid strings stay separate videos.  ValueError unless all share one
        row format (f32, bf16 or e4m3) and either all have a stem of one dtype or none has one, and for 2^31 rows or more."""
        indices = list(indices)
        if not indices:
            raise ValueError("VideoIndex.concat: no indices")
        head = indices[0]
        dev = head.feat.device
        if any(ix.feat.dtype != head.feat.dtype for ix in indices):
            raise ValueError("VideoIndex.concat: the indices differ in row format (f32 / bf16 / e4m3)")
        if any((ix.stem is None) != (head.stem is None) or (ix.stem is not None and ix.stem.dtype != head.stem.dtype) for ix in indices):
            raise ValueError("VideoIndex.concat: either every index has a stem of one dtype or none has one")
        base = np.concatenate([[0], np.cumsum([len(ix) for ix in indices])]).astype(np.int64)
        if int(base[-1]) >= 2 ** 31:
            raise ValueError("VideoIndex.concat: 2^31 rows or more; query the files together as a ShardedIndex instead")
        cat = lambda ts: torch.cat([t.to(dev) for t in ts], 0).contiguous()                       # noqa: E731
        v_off = np.concatenate([ix.v_off[:-1] + b for ix, b in zip(indices, base)] + [base[-1:]])
        return cls(cat([ix.feat for ix in indices]), v_off, [v for ix in indices for v in ix.vids],
                   cat([ix.scale for ix in indices]) if head.e4m3 else None,
                   cat([ix.stem for ix in indices]) if head.stem is not None else None)

    def quantize(self):
        """The e4m3 index of this bf16 / f32 one (tan_quantize_rows_e4m3), with the same stem; an e4m3 index is returned as it is."""
        if self.e4m3:
            return self
        codes, scale = ops.quantize_rows_e4m3(self.feat.contiguous())
        return VideoIndex(codes, self.v_off, self.vids, scale, self.stem)

    def __len__(self):
        return int(self.feat.shape[0])

    def restrict(self, videos=None, exclude=None, windows=None):
        return _restrict(self, videos, exclude, windows)

    restrict.__doc__ = _RESTRICT_DOC

    def locate(self, rows):
        """index rows -> (video number, second)"""
        return _locate(self, 0, rows)

    @property
    def shards(self):
        return [self]

    def shard_views(self, order=None):
        """`ShardedIndex.shard_views` of the one shard: yields (0, feat, scale, v_off_device), once unless `order` is empty"""
        for s in ([0] if order is None else order):
            yield s, self.feat, self.scale, self.v_off_device

    def save(self, path):
        """One .npz of plain arrays (bf16 rows as their uint16 bit patterns; e4m3 rows as uint8 codes plus `scale`; `stem`, bf16 as
        uint16 bits too, only when the index has one: without it the file is what it was before stems existed)."""
        f = self.feat.cpu()
        bf16 = f.dtype == torch.bfloat16
        more = dict(scale=self.scale.cpu().numpy()) if self.e4m3 else {}
        if self.stem is not None:
            st = self.stem.cpu().contiguous()
            more["stem"] = st.view(torch.int16).numpy().view(np.uint16) if st.dtype == torch.bfloat16 else st.numpy()
        with open(path, "wb") as fh:
            np.savez(fh, feat=(f.view(torch.int16).numpy().view(np.uint16) if bf16 else f.numpy()), bf16=np.array(bf16),
                     e4m3=np.array(self.e4m3), v_off=self.v_off, vids=np.array(self.vids, dtype=np.str_), **more)

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path, allow_pickle=False) as z:
            f = torch.from_numpy(z["feat"].view(np.int16)).view(torch.bfloat16) if bool(z["bf16"]) else torch.from_numpy(z["feat"])
            e4m3 = "e4m3" in z.files and bool(z["e4m3"])                  # files written before the e4m3 format have no such key
            scale = torch.from_numpy(z["scale"]).to(device).contiguous() if e4m3 else None
            stem = None
            if "stem" in z.files:                                         # uint16: bf16 bit patterns
                st = z["stem"]
                stem = torch.from_numpy(st.view(np.int16)).view(torch.bfloat16) if st.dtype == np.uint16 else torch.from_numpy(st)
                stem = stem.to(device).contiguous()
            return cls(f.to(device).contiguous(), z["v_off"], [str(v) for v in z["vids"]], scale, stem)


class ShardedIndex:
    """Several `VideoIndex` shards (whole videos each; the files `index --worker-id i --num-workers n` writes) searched together:
    `search`, `search_moments` and `search_sequences` return for it exactly what they return for `VideoIndex.concat(shards)` --
    every shard is swept on its own and the per-shard lists are folded on the device by `tan_topk_fold`.  Equal vid
    strings in two shards are two videos, as inside one index.  Every shard holds fewer than 2^31 rows; their total may exceed it.
    `annotate` takes one too (one `tan_label_topk` per shard); its `Annotation` needs fewer than 2^31 rows in all for `segments`.
      vids                      every shard's, in shard order
      v_off [n_videos + 1]      int64, global: each video's first row
      row_base / video_base     int64 [S + 1]: the rows / videos before shard s; the last entry is the total
      locate(shard, row)        shard-local rows -> (global video number, second)
    resident="device": the shards' rows are where the caller put them, all on one device (files from several workers).
    resident="host":   rows and scales stay in PINNED host memory and only each shard's int32 v_off lives on `device`; a search
      streams the shards through two device slots sized to the largest shard, the copy of the next shard running under the sweep of
      the current one (`shard_views`).  This is for a corpus larger than the card.  Every call then moves the whole index over the
      host link (PCIe Gen5 x16: 63 GB/s by its specification), which bounds it whatever the sweeps cost -- accepted, and the reason
      to batch many queries per call.  Unpinned host rows raise: a pageable copy would synchronise silently.
    Stems are not used (`search_rerank` refuses a ShardedIndex)."""

    def __init__(self, shards, resident="device", device=None):
        self.shards = list(shards)
        if not self.shards:
            raise ValueError("ShardedIndex: no shards")
        if resident not in ("device", "host"):
            raise ValueError("ShardedIndex: resident is 'device' or 'host'")
        head = self.shards[0]
        if any(sh.feat.dtype != head.feat.dtype for sh in self.shards):
            raise ValueError("ShardedIndex: the shards differ in row format (f32 / bf16 / e4m3)")
        if any(len(sh) < 1 or len(sh) >= 2 ** 31 for sh in self.shards):
            raise ValueError("ShardedIndex: a shard holds 1 to 2^31 - 1 rows")
        self.resident = resident
        if resident == "host":
            self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            for sh in self.shards:
                if any(t.is_cuda or not t.is_pinned() for t in (sh.feat, sh.scale) if t is not None):
                    raise ValueError("ShardedIndex: resident='host' needs rows and scales in pinned host memory (ShardedIndex.load "
                                     "pins them); a pageable copy would not run under the sweeps")
            self._v_off_dev = [torch.from_numpy(sh.v_off.astype(np.int32)).to(self.device) for sh in self.shards]
        else:
            self.device = head.feat.device
            if any(sh.feat.device != self.device for sh in self.shards) or (device is not None and torch.device(device) != self.device):
                raise ValueError("ShardedIndex: resident='device' needs every shard on one device")
        self.row_dtype = head.feat.dtype
        self.e4m3 = head.e4m3
        self.row_base = np.concatenate([[0], np.cumsum([len(sh) for sh in self.shards])]).astype(np.int64)
        self.video_base = np.concatenate([[0], np.cumsum([len(sh.vids) for sh in self.shards])]).astype(np.int64)
        self.vids = [v for sh in self.shards for v in sh.vids]
        self.v_off = np.concatenate([sh.v_off[:-1] + b for sh, b in zip(self.shards, self.row_base)] + [self.row_base[-1:]])
        self._slots = self._side = None
        self._free = [None, None]

    @classmethod
    def load(cls, paths, device="cuda", resident="device"):
        """The index files `paths`, in this order.  resident="host": rows and scales are read into pinned host memory."""
        if resident != "host":
            return cls([VideoIndex.load(p, device) for p in paths], resident)
        shards = []
        for p in paths:
            ix = VideoIndex.load(p, "cpu")
            shards.append(VideoIndex(ix.feat.pin_memory(), ix.v_off, ix.vids, ix.scale.pin_memory() if ix.e4m3 else None, ix.stem))
        return cls(shards, resident, device)

    def __len__(self):
        return int(self.row_base[-1])

    def restrict(self, videos=None, exclude=None, windows=None):
        return _restrict(self, videos, exclude, windows)

    restrict.__doc__ = _RESTRICT_DOC + """  Videos count over all shards, in shard order; the spans are cut per shard, and a search
        leaves out the shards without an admitted row (resident="host": they are not copied)."""

    def locate(self, shard, row):
        """(shard, shard-local row) -> (global video number, second)"""
        return _locate(self, shard, row)

    def shard_views(self, order=None):
        """Yields (s, feat, scale, v_off) -- device tensors of shard s, v_off its int32 offsets -- for s in `order` (default: every
        shard).  The caller issues EVERY kernel that reads a shard's views on the current stream before it asks for the next shard.
        resident="host": shard order[i] lives in slot i % 2 while it is swept; the copy of order[i + 1] into the other slot is issued
        on a side stream before shard i is handed out, so it runs under shard i's sweep."""
        order = list(range(len(self.shards))) if order is None else list(order)
        if self.resident == "device":
            for s in order:
                sh = self.shards[s]
                yield s, sh.feat, sh.scale, sh.v_off_device
            return
        comp = torch.cuda.current_stream(self.device)
        if self._slots is None:
            rows = max(len(sh) for sh in self.shards)
            self._slots = [(torch.empty(rows, 512, dtype=self.row_dtype, device=self.device),
                            torch.empty(rows, dtype=torch.float32, device=self.device) if self.e4m3 else None) for _ in range(2)]
            self._side = torch.cuda.Stream(device=self.device)
            self._side.wait_stream(comp)               # the allocator may hand out memory that work queued on `comp` still uses
        side, in_flight = self._side, {}

        def issue(i):
            sh, (feat, scale) = self.shards[order[i]], self._slots[i % 2]
            n = len(sh)
            if not sh.feat.is_pinned() or (self.e4m3 and not sh.scale.is_pinned()):
                raise ValueError("ShardedIndex: a host-resident shard is not in pinned memory")
            if self._free[i % 2] is not None:
                side.wait_event(self._free[i % 2])     # the slot's previous shard has been read to the end (see below)
            with torch.cuda.stream(side):
                feat[:n].copy_(sh.feat, non_blocking=True)
                if self.e4m3:
                    scale[:n].copy_(sh.scale, non_blocking=True)
                in_flight[i] = torch.cuda.Event()
                in_flight[i].record(side)
            return feat[:n], (scale[:n] if self.e4m3 else None)

        try:
            nxt = issue(0) if order else None
            for i, s in enumerate(order):
                cur, nxt = nxt, (issue(i + 1) if i + 1 < len(order) else None)
                comp.wait_event(in_flight.pop(i))
                try:
                    yield s, cur[0], cur[1], self._v_off_dev[s]
                finally:
                    # The copy of a LATER shard into this slot must not start before the last kernel that read this one has
                    # finished.  The caller has issued all of them by now (the fold; for moments the extent, for sequence phase 2
                    # the score blocks), so an event recorded on the compute stream HERE is behind them; the next copy into the
                    # slot, in this call or a later one, waits on it on the side stream.
                    self._free[i % 2] = torch.cuda.Event()
                    self._free[i % 2].record(comp)
        finally:
            for ev in in_flight.values():              # an early exit: no slot is left being written behind the caller's back
                comp.wait_event(ev)


@torch.no_grad()
def build_index(model, videos, seq_len=64, windows_per_pass=256, dtype=torch.bfloat16, keep_stem=False):
    """`videos`: iterable of {'vid', 'video' [vlen, Dv] (array / tensor) or a callable that reads it (then 'vlen' is required)} --
    `infer_align.read_corpus` items work as they are.  Every second of every video gets one row (see the module docstring); the rows
    do not depend on how the windows are cut into passes.  dtype: torch.bfloat16, torch.float32, or "e4m3" (torch.float8_e4m3fn):
    each chunk's rows are finished in f32 and quantised at once; only codes and scales are kept.
    keep_stem: also keep `model.video_stem` of every second (`VideoIndex.stem`, in the model's compute dtype: 1 KiB per second in
    bf16, so an e4m3 index with a stem is 516 + 1024 bytes per second) for `search_rerank`.  A second is projected once per chunk,
    not once per covering window; feat, scale, v_off and vids are what they are without the option."""
    e4m3 = _is_e4m3(dtype)
    net = _aligner(model)
    device = torch.device("cuda", torch.cuda.current_device())
    T = seq_len
    feats, scales, stems, vlens, vids = [], [], [], [], []
    no_text = torch.zeros(1, 8, device=device)
    for ch in _prefetch(_index_chunks(videos, seq_len, windows_per_pass), device):
        n_rows = int(ch.v_off[-1])
        acc = torch.zeros(n_rows, 512, device=device)
        cnt = torch.zeros(n_rows, device=device)
        if keep_stem:
            stems.append(net.video_stem(ch.video))
        for p0, p1 in ch.passes:
            W, tab = p1 - p0, ch.table_d[p0:p1]
            vid = torch.empty(W, T, ch.video.shape[1], dtype=ch.video.dtype, device=device)
            vm = torch.empty(W, T, dtype=torch.bool, device=device)
            txt = torch.empty(W, 1, 8, device=device)
            tm = torch.empty(W, 1, dtype=torch.bool, device=device)
            ops.window_pack(ch.video, no_text, tab, T, 1, vid, vm, txt, tm)
            v = net.get_visual_feature(vid, vm)                                     # [W, S, T, 512]
            ops.window_feat_acc(v[:, -1], tab, acc, cnt)
        if e4m3:
            codes, scale = ops.quantize_rows_e4m3(ops.window_feat_final(acc, cnt, torch.empty(n_rows, 512, device=device)))
            feats.append(codes)
            scales.append(scale)
        else:
            feats.append(ops.window_feat_final(acc, cnt, torch.empty(n_rows, 512, dtype=dtype, device=device)))
        vlens += [it["vlen"] for it in ch.items]
        vids += [it.get("vid") for it in ch.items]
    if not feats:
        raise ValueError("build_index: no videos")
    return VideoIndex(torch.cat(feats, 0), np.concatenate([[0], np.cumsum(vlens)]), vids, torch.cat(scales, 0) if e4m3 else None,
                      torch.cat(stems, 0) if keep_stem else None)


@torch.no_grad()
def query_features(index, model, embed_text, queries, text_batch=1024):
    """Unit text features [Q, 512] in the index's dtype; for an e4m3 index (codes uint8 [Q, 512], scale f32 [Q])."""
    net = _aligner(model)
    dev = index.device
    t = torch.cat([net.get_textual_feature(embed_text(list(queries[a:a + text_batch])).to(dev)).float().reshape(-1, 512)
                   for a in range(0, len(queries), text_batch)], 0).contiguous()
    t = ops.l2norm_fwd(t, torch.empty_like(t), None, t.shape[0], 512)
    if index.e4m3:
        return ops.quantize_rows_e4m3(t)
    return t if index.row_dtype == torch.float32 else ops.cast(t, torch.empty(t.shape, dtype=index.row_dtype, device=dev))


class _Sweep:
    """The query side of one search call, made once from `query_features`' result (for an e4m3 index: codes and scales), and the
    ONE place that chooses the sweep of a shard view from (e4m3, restrict)."""

    def __init__(self, index, tq, restrict=None, splits=0):
        self.e4m3, self.restrict, self.splits = index.e4m3, restrict, splits
        self.tq, self.q_scale = tq if index.e4m3 else (tq, None)

    def scales(self, v_scale):
        """the scale keywords of an `ops` call over a view whose row scales are v_scale"""
        return dict(q_scale=self.q_scale, v_scale=v_scale) if self.e4m3 else {}

    def rows(self, s, feat, scale, k):
        """(score, row): the k best rows of shard s's view -- of its admitted rows under a filter; k is clamped to them"""
        if self.restrict is not None:
            return ops.rank_topk_filtered(self.tq, feat, self.restrict.image(s), min(k, self.restrict.shard_rows(s)), splits=self.splits,
                                          **self.scales(scale))
        if self.e4m3:
            return ops.rank_topk_e4m3(self.tq, self.q_scale, feat, scale, None, min(k, feat.shape[0]), splits=self.splits)[2:]
        return ops.rank_topk(self.tq, feat, None, min(k, feat.shape[0]), splits=self.splits)[2:]

    def videos(self, s, feat, scale, v_off, k):
        """(score, row, video): the k best distinct videos of shard s's view, each by its best (admitted) row; k is clamped"""
        if self.restrict is not None:
            return ops.rank_topk_video_filtered(self.tq, feat, v_off, self.restrict.image(s), min(k, self.restrict.shard_videos(s)),
                                                splits=self.splits, **self.scales(scale))
        return ops.rank_topk_video(self.tq, feat, v_off, min(k, v_off.numel() - 1), splits=self.splits, **self.scales(scale))


class _TopLists:
    """The k best of a search over the views of an index.  A `ShardedIndex`: every shard's lists are folded into running ones on
    the device (`ops.topk_fold`, once per shard).  A `VideoIndex`: its one view's lists ARE the result, and no fold is launched.
    lists: (score f32, shard int32 -- None for a `VideoIndex`: all 0 --, row, *payload int32), [Q, k] each, on the device."""

    def __init__(self, index, Q, k, n_aux):
        self.run = self.lists = None
        if isinstance(index, ShardedIndex):        # `ops.topk_fold`'s running lists, uninitialised: the first fold resets them
            i32 = dict(dtype=torch.int32, device=index.device)
            self.run = (torch.empty(Q, k, dtype=torch.float32, device=index.device), torch.empty(Q, k, **i32), torch.empty(Q, k, **i32),
                        torch.empty(n_aux, Q, k, **i32) if n_aux else None)

    def add(self, s, lists):
        """lists = (score, row, *payload) of shard s, shard-local"""
        if self.run is None:
            self.lists = (lists[0], None, *lists[1:])
        else:
            ops.topk_fold(self.run, lists, s, reset=self.lists is None)
            self.lists = (*self.run[:3], *(() if self.run[3] is None else self.run[3]))

    def winners(self):
        """A read-back of (shard, row) alone, flat int64: `search_sequences` sizes its score blocks from them"""
        if self.run is None:
            row = self.lists[2].cpu().numpy().reshape(-1).astype(np.int64)
            return np.zeros_like(row), row
        return tuple(a.reshape(-1).astype(np.int64) for a in torch.stack(self.lists[1:3]).cpu().numpy())

    def read(self):
        """The one read-back: (score [Q, k] f32, which travels as its bit pattern, shard [Q, k], (row, *payload) int32 [Q, k])"""
        ints = torch.stack(self.lists[2 if self.run is None else 1:])
        back = torch.cat((self.lists[0].view(torch.int32)[None], ints)).cpu().numpy()
        shard, ints = (np.zeros_like(back[1]), back[1:]) if self.run is None else (back[1], back[2:])
        return back[0].view(np.float32), shard, ints


@torch.no_grad()
def search(index, model, embed_text, queries, k=10, splits=0, restrict=None):
    """Per query the k best seconds of the corpus: [[(vid, second, score)] * k] * len(queries), by descending score (equal scores
    by index row).  score = <index row, unit text feature>: the stitched dual cosine; / 0.07 gives the evaluation's logit.
    `index`: a `VideoIndex`, or a `ShardedIndex` -- then exactly what `VideoIndex.concat` of its shards gives (as for
    `search_moments` and `search_sequences`): one sweep and one `tan_topk_fold` per shard.  One read-back at the end for either.
    restrict: a `RowFilter` of this index (`index.restrict(...)`): only its rows are swept (`tan_rank_topk_filtered`) and returned,
    with the scores and the order the unrestricted call gives them; k is clamped to the admitted rows."""
    queries = list(queries)
    if not queries:
        return []
    if restrict is not None:
        restrict.check(index)
    k = min(int(k), len(index) if restrict is None else restrict.n_rows)
    if not 1 <= k <= 32:
        raise ValueError("search: k must lie in [1, 32]")
    sweep = _Sweep(index, query_features(index, model, embed_text, queries), restrict, splits)
    top = _TopLists(index, len(queries), k, 0)
    for s, feat, scale, _ in index.shard_views(None if restrict is None else restrict.ready()):
        top.add(s, sweep.rows(s, feat, scale, k))
    score, shard, (row,) = top.read()
    v, sec = _locate(index, shard, row)
    return [[(index.vids[v[q, i]], int(sec[q, i]), float(score[q, i])) for i in range(k)] for q in range(len(queries))]


@torch.no_grad()
def search_moments(index, model, embed_text, queries, k=10, width=TEMPERATURE, splits=0, restrict=None):
    """Per query the k best DISTINCT videos of the corpus, [[Moment(vid, start, end, second, score)] * k] * len(queries), by
    descending score (equal scores by index row).  `second` is where the sentence fits the video best and `score` its score, as
    `search` defines it; [start, end] (seconds of the video, inclusive) is the contiguous run around `second` whose scores stay
    >= score - width.  k is clamped to the number of videos and must lie in [1, 32].
    The default width = 0.07 is one unit of the evaluation's logit score / 0.07: the seconds whose softmax-over-time weight is at
    least e^-1 of the peak's.  That is a definition chosen here, not a measurement of where moments end.
    restrict: a `RowFilter` of this index: a video's peak is its best ADMITTED second (`tan_rank_topk_video_filtered`), a video
    without one never appears, k is clamped to the admitted videos, and [start, end] is the extent as defined above cut to the
    admitted span that holds the peak (a clip on the host; the extent walk itself does not know the filter)."""
    queries = list(queries)
    if not queries:
        return []
    if restrict is not None:
        restrict.check(index)
    k = min(int(k), len(index.vids) if restrict is None else restrict.n_videos)
    if not 1 <= k <= 32:
        raise ValueError("search_moments: k must lie in [1, 32]")
    if not width >= 0:
        raise ValueError("search_moments: width must be >= 0")
    sweep = _Sweep(index, query_features(index, model, embed_text, queries), restrict, splits)
    top = _TopLists(index, len(queries), k, 3)
    for s, feat, scale, v_off in index.shard_views(None if restrict is None else restrict.ready()):
        score, row, video = sweep.videos(s, feat, scale, v_off, k)
        # the extents of the shard's OWN list, before the fold: the shard's rows are passed over once (and are gone afterwards
        # when they are streamed), at the price of extents for hits the fold drops
        start, end = ops.moment_extent(sweep.tq, feat, v_off, score, row, video, width, **sweep.scales(scale))
        top.add(s, (score, row, video, start, end))
    score, shard, (row, video, start, end) = top.read()                    # all shard-local
    first = np.zeros_like(row)
    for s in np.unique(shard):
        first[shard == s] = index.shards[s].v_off[video[shard == s]]
    gv = index.video_base[shard] + video
    if restrict is not None:
        base = index.row_base[shard]
        start, end = (a - base for a in restrict.clip(base + row, base + start, base + end))
    return [[Moment(index.vids[gv[q, i]], int(start[q, i] - first[q, i]), int(end[q, i] - first[q, i]),
                    int(row[q, i] - first[q, i]), float(score[q, i])) for i in range(k)] for q in range(len(queries))]


@torch.no_grad()
def search_sequences(index, model, embed_text, sequences, k=10, splits=0):
    """Per SEQUENCE (an ordered list of 1 to 32 sentences) the k videos of the corpus that show its steps best IN ORDER:
    [[SequenceHit(vid, seconds, score)] * k] * len(sequences), by descending score (equal scores by video number).  `seconds` holds
    one second of the video per step, non-decreasing (equal seconds allowed): the assignment with the largest summed score, ties to
    the smallest last second, then the smallest second to last, as `align_corpus(decode="monotonic")` breaks them.  `score` is that
    sum of the steps' stitched dual cosines (`search`'s score); / 0.07 gives the summed logit.  k is clamped to the number of
    videos and must lie in [1, 32].  Two read-backs: the winning videos (to size the score blocks), then seconds and scores.
    There is no `restrict=` here: a `RowFilter` is not taken by this call (a path needs its whole video, and whole-video filters
    for the sequence sweep are not built)."""
    sequences = [list(seq) for seq in sequences]
    if not sequences:
        return []
    if any(not 1 <= len(seq) <= 32 for seq in sequences):
        raise ValueError("search_sequences: a sequence holds 1 to 32 sentences")
    k = min(int(k), len(index.vids))
    if not 1 <= k <= 32:
        raise ValueError("search_sequences: k must lie in [1, 32]")
    dev = index.device
    m = np.array([len(seq) for seq in sequences], dtype=np.int64)
    s_off = torch.from_numpy(np.concatenate([[0], np.cumsum(m)]).astype(np.int32)).to(dev)
    sweep = _Sweep(index, query_features(index, model, embed_text, [sentence for seq in sequences for sentence in seq]), splits=splits)
    n_seq = len(sequences)
    # phase 1: every shard's best videos, with row = the shard-local video number
    top = _TopLists(index, n_seq, k, 0)
    for s, feat, scale, v_off in index.shard_views():
        top.add(s, ops.sequence_topk(sweep.tq, feat, s_off, v_off, min(k, v_off.numel() - 1), splits=splits, **sweep.scales(scale)))
    shard, video = top.winners()                                           # read-back 1
    # phase 2: the seconds, shard by shard over the shards that hold winners (a `VideoIndex`: all in shard 0), each over its own hits
    seq_of_hit = np.repeat(np.arange(n_seq), k)
    parts = []
    for s, feat, scale, v_off in index.shard_views([int(s) for s in np.unique(shard)]):
        at = np.flatnonzero(shard == s)
        parts.append((at, *_sequence_seconds(sweep.tq, feat, s_off, v_off, index.shards[s].v_off, m, seq_of_hit[at], video[at],
                                             sweep.scales(scale))))
    back = torch.cat([top.lists[0].reshape(-1).view(torch.int32)] + [ts for _, ts, _ in parts]).cpu().numpy()   # read-back 2
    score, a0 = back[:n_seq * k].view(np.float32), n_seq * k
    seconds = [None] * (n_seq * k)
    for at, ts, first in parts:
        for j, h in enumerate(at):
            seconds[h] = tuple(int(t) for t in back[a0 + first[j]:a0 + first[j + 1]])
        a0 += int(first[-1])
    gv = index.video_base[shard] + video
    return [[SequenceHit(index.vids[gv[p * k + i]], seconds[p * k + i], float(score[p * k + i])) for i in range(k)]
            for p in range(n_seq)]


def _sequence_seconds(tq, feat, s_off, v_off_dev, v_off, m, seq, video, scales):
    """The seconds of P hits (seq [P], video [P]: a sequence and a video of THIS index each) -- one [m, V] block of scores per hit
    (`tan_sequence_scores`) and the decode's tables: one "video" per hit, its m rows in step order.  Returns (ts: int32 on the
    device, the hits' seconds one after the other, first [P + 1]: where each hit's begin).  Nothing is read back."""
    dev, P = feat.device, len(seq)
    hm = m[seq]
    hv = v_off[video + 1] - v_off[video]
    x_off = np.concatenate([[0], np.cumsum(hm * hv)])
    if x_off[-1] >= 2 ** 31:
        raise ValueError("search_sequences: the winners' score blocks exceed the int32 decode tables; lower k or split the call")
    first = np.concatenate([[0], np.cumsum(hm)])
    hit_of_row = np.repeat(np.arange(P), hm)
    step = np.arange(first[-1]) - first[hit_of_row]
    rows = np.stack((x_off[hit_of_row] + step * hv[hit_of_row], hv[hit_of_row]), 1)
    vtab = np.stack((first[:-1], hm, np.concatenate([[0], np.cumsum(hv)])[:-1]), 1)
    hits = np.stack((seq, video), 1)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)          # noqa: E731
    x = torch.empty(int(x_off[-1]), dtype=torch.float32, device=dev)
    ops.sequence_scores(tq, feat, s_off, v_off_dev, i32(hits), torch.from_numpy(x_off[:-1].copy()).to(dev), x, **scales)
    ts = torch.empty(int(first[-1]), dtype=torch.int32, device=dev)
    path = torch.empty(P, dtype=torch.float32, device=dev)
    ops.monotonic_decode(x, i32(rows), torch.arange(int(first[-1]), dtype=torch.int32, device=dev), i32(vtab), None,
                         torch.empty(x.numel(), dtype=torch.int32, device=dev), torch.empty(int(hv.sum()), device=dev), ts, path)
    return ts, first


def _video_number(index, vid, by_name):
    """A vid string -> the FIRST video that carries it, an int -> itself; None when the index has no such video.  by_name: a dict the
    caller keeps between calls (filled on first use)."""
    if isinstance(vid, str):
        if not by_name:
            for v, s in enumerate(index.vids):
                by_name.setdefault(s, v)
        return by_name.get(vid)
    return int(vid) if isinstance(vid, (int, np.integer)) and 0 <= int(vid) < len(index.vids) else None


def clip_spans(index, clips, max_seconds=MAX_CLIP_SECONDS):
    """The host half of `clip_features`: every clip checked, [(m, source)] with source = (global video number, first second) for a
    (vid, first, last) clip and None for a tensor of rows.  A vid string names the FIRST video that carries it; an int is a video
    number.  ValueError: an unknown vid, first > last, seconds outside the video, m outside [1, max_seconds] (32 for the clip sweep;
    `align_spans` passes 4096), a tensor that is not a float [m, 512].  Needs no device."""
    by_name = {}
    out = []
    for c, clip in enumerate(clips):
        if isinstance(clip, torch.Tensor):
            if clip.dim() != 2 or clip.shape[1] != 512 or not clip.is_floating_point():
                raise ValueError(f"clip {c}: a tensor clip holds float index-style rows [m, 512], not {tuple(clip.shape)} {clip.dtype}")
            m, source = int(clip.shape[0]), None
        else:
            try:
                vid, first, last = clip
                first, last = int(first), int(last)
            except (TypeError, ValueError):
                raise ValueError(f"clip {c}: (vid, first_second, last_second) or a tensor [m, 512]") from None
            v = _video_number(index, vid, by_name)
            if v is None:
                raise ValueError(f"clip {c}: no video {vid!r} in the index")
            vlen = int(index.v_off[v + 1] - index.v_off[v])
            if first > last:
                raise ValueError(f"clip {c}: first second {first} > last second {last}")
            if first < 0 or last >= vlen:
                raise ValueError(f"clip {c}: seconds {first}..{last} lie outside video {vid!r} of {vlen} seconds")
            m, source = last - first + 1, (v, first)
        if not 1 <= m <= max_seconds:
            raise ValueError(f"clip {c}: {m} seconds; a clip holds 1 to {max_seconds} (cut a longer one into pieces)")
        out.append((m, source))
    return out


def _index_rows(index, lo, hi, dev):
    """The global rows [lo, hi) of ONE video of either kind of index as f32 on `dev`, from whichever shard holds them
    (host-resident included); e4m3 rows dequantised (code value x power-of-two scale: exact)."""
    s = int(np.searchsorted(index.row_base, lo, side="right")) - 1
    sh, a, b = index.shards[s], lo - int(index.row_base[s]), hi - int(index.row_base[s])
    rows = sh.feat[a:b].to(dev)
    if sh.scale is None:
        return rows.float()
    lut = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(dev)
    return lut[rows.long()] * sh.scale[a:b].to(dev)[:, None]


@torch.no_grad()
def clip_features(index, clips, max_seconds=MAX_CLIP_SECONDS):
    """The query side of `search_clips`: (rows, c_off).  Each clip is (vid, first, last) -- the seconds first..last, inclusive, of a
    video OF THIS INDEX (a `VideoIndex` or a `ShardedIndex`; see `clip_spans` for how a vid is resolved) -- or a float tensor
    [m, 512] of index-style rows, e.g. `build_index(model, [video]).feat[a:b]`; 1 <= m <= 32.  The rows are L2-normalised in f32 and
    then cast to the index's row dtype or quantised (`ops.quantize_rows_e4m3`), exactly as `query_features` treats text: rows
    [Qt, 512] in the index's dtype, for an e4m3 index (codes uint8 [Qt, 512], scale f32 [Qt]).  c_off [n_clip + 1] int32 on the
    device: each clip's first row, then Qt.  ValueError as `clip_spans` raises it, before anything touches the device.
    max_seconds: the longest clip taken (`align_spans`: 4096); c_off is tan_clip_topk's only while every clip holds at most 32."""
    clips = list(clips)
    spans = clip_spans(index, clips, max_seconds)
    if not clips:
        raise ValueError("clip_features: no clips")
    dev = index.device
    parts = []
    for clip, (m, source) in zip(clips, spans):
        if source is None:
            parts.append(clip.to(dev).float())
        else:
            lo = int(index.v_off[source[0]]) + source[1]
            parts.append(_index_rows(index, lo, lo + m, dev))
    t = torch.cat(parts, 0).contiguous()
    t = ops.l2norm_fwd(t, torch.empty_like(t), None, t.shape[0], 512)
    c_off = torch.from_numpy(np.concatenate([[0], np.cumsum([m for m, _ in spans])]).astype(np.int32)).to(dev)
    if index.e4m3:
        return ops.quantize_rows_e4m3(t), c_off
    return (t if index.row_dtype == torch.float32 else ops.cast(t, torch.empty(t.shape, dtype=index.row_dtype, device=dev))), c_off


def drop_source(entries, source, k):
    """`search_clips(exclude_source=True)` on the host: entries = one clip's hits, best first, out of a sweep asked for k + 1, each a
    tuple whose first element is the hit's global video number; source = the clip's own video number, or None for a tensor clip.
    The source is removed where it is listed, otherwise the list is cut to k: the order is total, so either way these are the k
    best of the other videos."""
    if source is not None:
        kept = [e for e in entries if e[0] != source]
        if len(kept) < len(entries):
            return kept
    return entries[:k]


@torch.no_grad()
def search_clips(index, clips, k=10, splits=0, exclude_source=False):
    """Video to video: per CLIP (see `clip_features`: (vid, first, last) of this index, or a tensor [m, 512]; 1 to 32 seconds) the
    videos of the corpus in which it appears best SECOND FOR SECOND, and where: [[ClipHit(vid, start, end, score)]] per clip, by
    descending score (equal scores by index row).  [start, end] are seconds of the hit's video, inclusive, end = start + m - 1: the
    placement of the clip with the largest summed score (`tan_clip_topk`; the smallest such start), and score is that sum / m --
    the mean stitched dual cosine per second, `search`'s score, so / 0.07 gives the mean logit.  Unlike `search_sequences` the
    seconds advance in lockstep: a video that merely holds the clip's best second once scores one good second out of m.
    k is clamped to the number of videos and must lie in [1, 32]; a video shorter than the clip cannot hold it, so a list is SHORTER
    than k when fewer videos are long enough.  exclude_source: leave out the video a (vid, first, last) clip was cut from (a tensor
    clip has none); the sweep is asked for k + 1, so k <= 31.
    `index`: a `VideoIndex`, or a `ShardedIndex` -- one sweep and one `tan_topk_fold` per shard, exactly what `VideoIndex.concat`
    of its shards gives.  One read-back.  There is no `restrict=` here: a `RowFilter` is not taken by this call (a placement needs
    consecutive rows of its video, and whole-video filters for this sweep are not built)."""
    clips = list(clips)
    if not clips:
        return []
    spans = clip_spans(index, clips)
    k = min(int(k), len(index.vids))
    kk = min(k + 1, len(index.vids)) if exclude_source else k
    if not 1 <= k <= kk <= 32:
        raise ValueError("search_clips: k must lie in [1, 32], and in [1, 31] with exclude_source")
    tq, c_off = clip_features(index, clips)
    sweep = _Sweep(index, tq, splits=splits)
    top = _TopLists(index, len(clips), kk, 1)
    for s, feat, scale, v_off in index.shard_views():
        top.add(s, ops.clip_topk(sweep.tq, feat, c_off, v_off, min(kk, v_off.numel() - 1), splits=splits, **sweep.scales(scale)))
    score, shard, (row, video) = top.read()                                # shard-local; an empty slot has row 0x7fffffff
    out = []
    for p, (m, source) in enumerate(spans):
        entries = []
        for i in range(kk):
            if row[p, i] == EMPTY_ROW:
                break                                                      # empty slots sort last
            s, v = int(shard[p, i]), int(video[p, i])
            entries.append((int(index.video_base[s]) + v, int(row[p, i] - index.shards[s].v_off[v]), float(score[p, i])))
        if exclude_source:
            entries = drop_source(entries, None if source is None else source[0], k)
        out.append([ClipHit(index.vids[gv], start, start + m - 1, S / m) for gv, start, S in entries])
    return out


def piece_offsets(ms, piece=PIECE_ROWS):
    """Queries of ms[q] rows, one after the other, cut into pieces of `piece` rows (each query's last piece shorter): (s_off
    [n_pieces + 1] int64: every piece's first row, then the total -- tan_sequence_scores' s_off --, first [Q + 1] int64: the number
    of each query's first piece).  No piece straddles two queries."""
    ms = np.asarray(ms, dtype=np.int64)
    n = (ms + piece - 1) // piece
    first = np.concatenate([[0], np.cumsum(n)])
    row0 = np.concatenate([[0], np.cumsum(ms)])
    q_of = np.repeat(np.arange(len(ms)), n)
    s_off = row0[q_of] + (np.arange(first[-1]) - first[q_of]) * piece
    return np.concatenate([s_off, row0[-1:]]).astype(np.int64), first.astype(np.int64)


def align_tables(ms, Vs, first, videos, piece=PIECE_ROWS):
    """The tables of P pairs for `ops.sequence_scores` and `ops.local_align`: pair h is a query of ms[h] rows whose pieces are the
    sequences first[h], first[h] + 1, ... and a video `videos[h]` of Vs[h] rows.  Returns (hits [n, 2] = (sequence, video) per
    (pair, piece), hit_off [n]: consecutive element offsets, so a pair's pieces fill ONE row-major [m, V] block, x_off [P]: each
    pair's block, table [P, 3] = (m, V, first boundary slot), n_x, sum_V), all int64."""
    ms, Vs, first, videos = (np.asarray(a, dtype=np.int64) for a in (ms, Vs, first, videos))
    x_off = np.concatenate([[0], np.cumsum(ms * Vs)])
    slot = np.concatenate([[0], np.cumsum(Vs)])
    n = (ms + piece - 1) // piece
    pair_of = np.repeat(np.arange(len(ms)), n)
    a = np.arange(int(n.sum())) - np.concatenate([[0], np.cumsum(n)])[pair_of]           # the piece's number inside its query
    hits = np.stack((first[pair_of] + a, videos[pair_of]), 1)
    hit_off = x_off[pair_of] + a * piece * Vs[pair_of]
    return hits, hit_off, x_off[:-1], np.stack((ms, Vs, slot[:-1]), 1), int(x_off[-1]), int(slot[-1])


def _align_prices(what, threshold, skew):
    threshold, skew = float(threshold), float(skew)
    if not np.isfinite(threshold) or not (skew >= 0 and np.isfinite(skew)):
        raise ValueError(f"{what}: threshold must be finite and skew in [0, +inf)")
    return threshold, skew


@torch.no_grad()
def align_spans(index, pairs, threshold, skew=0.0):
    """Where, and how much of it, a re-timed or re-cut copy of a query appears in a given video: per pair (query, vid) one
    CopyHit(vid, start, end, q_start, q_end, score, cells) or None.  `query` is what `clip_features` takes -- (vid, first, last) of
    this index or a float tensor [m, 512] -- with 1 to 4096 seconds; `vid` a video of this index (a string: the first that carries
    it; an int: a global video number).  The hit is the best LOCAL alignment of the query's seconds with the video's
    (`tan_local_align`, defined in include/tan_hip.h): a cell gains score - threshold, with `search`'s score (the stitched dual
    cosine); a step along one axis alone -- the copy slowed down or sped up -- costs `skew`; a few unrelated seconds are bridged at
    threshold - score each.  [start, end] are seconds of the video, [q_start, q_end] the seconds OF THE QUERY (0 = its first) they
    show, both inclusive; cells is the length of the path, score its sum.  None: no second of the pair scores above the threshold.
    `threshold` has no default: it depends on the features, and nobody has measured it.
    `index`: a `VideoIndex` or a `ShardedIndex` (host-resident too): the pairs are grouped by the shard that holds their video, a
    shard without one is not visited, and each visited shard costs one `tan_sequence_scores` and one `tan_local_align`.  One
    read-back at the end.  The score blocks of a shard's pairs (4 bytes x query seconds x video seconds) are held at once:
    ValueError from 2^31 elements on -- split the call."""
    return _align_pairs("align_spans", index, pairs, threshold, skew, False)


def _align_pairs(what, index, pairs, threshold, skew, paths):
    """`align_spans` (paths False: CopyHit or None per pair) and `align_paths` (paths True: CopyPath or None)"""
    pairs = list(pairs)
    threshold, skew = _align_prices(what, threshold, skew)
    if not pairs:
        return []
    # every distinct query once: `search_copies` pairs one query with many videos
    uniq, q_of, seen, by_name, gvs = [], [], {}, {}, []
    for n, pair in enumerate(pairs):
        try:
            query, vid = pair
        except (TypeError, ValueError):
            raise ValueError(f"pair {n}: (query, vid)") from None
        key = id(query) if isinstance(query, torch.Tensor) else query
        try:
            at = seen.get(key)
        except TypeError:                              # an unhashable query: `clip_spans` says what is wrong with it
            at = None
        if at is None:
            at = len(uniq)
            uniq.append(query)
            try:
                seen[key] = at
            except TypeError:
                pass
        q_of.append(at)
        gv = _video_number(index, vid, by_name)
        if gv is None:
            raise ValueError(f"pair {n}: no video {vid!r} in the index")
        gvs.append(gv)
    ms = np.array([m for m, _ in clip_spans(index, uniq, MAX_ALIGN_SECONDS)], dtype=np.int64)
    tq, _ = clip_features(index, uniq, MAX_ALIGN_SECONDS)
    dev = index.device
    s_off, first = piece_offsets(ms)
    s_off_dev = torch.from_numpy(s_off.astype(np.int32)).to(dev)
    sweep = _Sweep(index, tq)
    q_of, gvs = np.asarray(q_of, dtype=np.int64), np.asarray(gvs, dtype=np.int64)
    shard = np.searchsorted(index.video_base, gvs, side="right") - 1
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)          # noqa: E731
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)          # noqa: E731
    parts, maps = [], []
    for s, feat, scale, v_off in index.shard_views([int(s) for s in np.unique(shard)]):
        at = np.flatnonzero(shard == s)
        local = gvs[at] - index.video_base[s]
        sv = index.shards[s].v_off
        hits, hit_off, x_off, table, n_x, sum_V = align_tables(ms[q_of[at]], sv[local + 1] - sv[local], first[q_of[at]], local)
        if n_x >= 2 ** 31:
            raise ValueError(f"{what}: the score blocks of one shard's pairs reach 2^31 elements; split the call")
        x = torch.empty(n_x, dtype=torch.float32, device=dev)
        ops.sequence_scores(sweep.tq, feat, s_off_dev, v_off, i32(hits), i64(hit_off), x, **sweep.scales(scale))
        if paths:
            path_off, n_map, n_trace = path_tables(table[:, 0], table[:, 1])
            score, span, qmap = ops.local_align_path(x, i64(x_off), i32(table), threshold, skew, i64(path_off), sum_V=sum_V, n_map=n_map,
                                                     n_trace=n_trace)
            maps.append((path_off[:, 0], qmap.view(-1)))
        else:
            score, span = ops.local_align(x, i64(x_off), i32(table), threshold, skew, sum_V=sum_V)
        parts.append((at, torch.cat((score.view(torch.int32)[:, None], span), 1)))
    n_head = 6 * sum(len(at) for at, _ in parts)
    back = torch.cat([t.view(-1) for _, t in parts] + [q for _, q in maps]).cpu().numpy()       # the one read-back
    head, tail = back[:n_head].reshape(-1, 6), back[n_head:].reshape(-1, 2)
    out, a0, r0 = [None] * len(pairs), 0, 0
    for n, (at, _) in enumerate(parts):
        for e, (h, row) in enumerate(zip(at, head[a0:a0 + len(at)])):
            sc = float(row[:1].view(np.float32)[0])
            if sc > 0:
                out[h] = CopyHit(index.vids[gvs[h]], int(row[3]), int(row[4]), int(row[1]), int(row[2]), sc, int(row[5]))
                if paths:
                    row0 = r0 + int(maps[n][0][e])                                            # the pair's map rows, then its aligned ones
                    out[h] = CopyPath(out[h], tail[row0 + int(row[1]):row0 + int(row[2]) + 1].copy())
        a0 += len(at)
        if paths:
            r0 += maps[n][1].numel() // 2
    return out


def path_tables(ms, Vs):
    """What `ops.local_align_path` needs beside `align_tables`: (path_off [P, 2] int64 = (each pair's first map row: the running sum
    of m, its first trace entry: the running sum of ceil(m / 64) * (V + 63)), n_map, n_trace: the two totals)"""
    ms, Vs = np.asarray(ms, dtype=np.int64), np.asarray(Vs, dtype=np.int64)
    rows = np.concatenate([[0], np.cumsum(ms)])
    entries = np.concatenate([[0], np.cumsum((ms + 63) // 64 * (Vs + 63))])
    return np.stack((rows[:-1], entries[:-1]), 1), int(rows[-1]), int(entries[-1])


@torch.no_grad()
def align_paths(index, pairs, threshold, skew=0.0):
    """`align_spans` with the path: per pair (query, vid) one CopyPath(hit, seconds) or None.  `hit` is the CopyHit that
    `align_spans` returns for the pair; `seconds` is an int32 array [q_end - q_start + 1, 2]: row i = the first and the last
    second of the video that show query second q_start + i (`tan_local_align_path`, defined in include/tan_hip.h).  A second of
    the query shown for several seconds of the copy (slowed down, or seconds inserted) has first < last; consecutive query seconds
    that share one video second (sped up, or seconds dropped) repeat it.  The path is monotone and without jumps: a row's first
    is the previous row's last or the second after it.  `copy_interval`, `copy_inverse` and `transfer_segments` read the map.
    Arguments, checks and shard grouping are `align_spans`'.  Each visited shard costs one `tan_sequence_scores` and one
    `tan_local_align_path`, and the one read-back at the end carries the maps too (8 bytes per query second and pair)."""
    return _align_pairs("align_paths", index, pairs, threshold, skew, True)


def copy_interval(path, q_first, q_last):
    """The video seconds (first, last), inclusive, that show query seconds q_first .. q_last of a CopyPath, the query seconds
    clipped to the aligned [q_start, q_end]; None if they do not meet."""
    a, b = max(int(q_first), path.hit.q_start), min(int(q_last), path.hit.q_end)
    if a > b:
        return None
    return int(path.seconds[a - path.hit.q_start, 0]), int(path.seconds[b - path.hit.q_start, 1])


def copy_inverse(path):
    """The map of a CopyPath read the other way: an int32 array [end - start + 1, 2], row t = the first and the last QUERY second
    shown at video second start + t.  A step of the path advances the video by at most one second, so every video second of
    [start, end] is on it and every row is set.  Pure numpy on the host."""
    hit, sec = path.hit, np.asarray(path.seconds, dtype=np.int64)
    inv = np.empty((hit.end - hit.start + 1, 2), dtype=np.int32)
    inv[:, 0], inv[:, 1] = np.iinfo(np.int32).max, -1
    for i, (lo, hi) in enumerate(sec):
        rows = slice(lo - hit.start, hi - hit.start + 1)
        inv[rows, 0] = np.minimum(inv[rows, 0], hit.q_start + i)
        inv[rows, 1] = np.maximum(inv[rows, 1], hit.q_start + i)
    return inv


def transfer_segments(path, segments):
    """Segments (start, end, label, ...) on the QUERY's timeline (seconds of the query, 0 = its first, inclusive) carried onto the
    copy's timeline through `copy_interval`: the same tuples with start and end replaced by video seconds, in their order; a
    segment that does not meet the aligned span is dropped."""
    out = []
    for seg in segments:
        at = copy_interval(path, seg[0], seg[1])
        if at is not None:
            out.append(tuple(at) + tuple(seg[2:]))
    return out


def copy_pieces(m, piece):
    """A query of m seconds cut into pieces of `piece` seconds, the last one shorter: [(first second, seconds)]"""
    return [(a, min(piece, m - a)) for a in range(0, m, piece)]


@torch.no_grad()
def search_copies(index, queries, k=10, pool=32, piece=16, *, threshold, skew=0.0, exclude_source=False, paths=False):
    """Video to video when the copy was re-timed or re-cut -- slowed down, sped up, seconds cut out or inserted: per QUERY ((vid,
    first, last) of this index, or a float tensor [m, 512]; 1 to 4096 seconds) the videos that hold the best local alignment with
    it, [[CopyHit(vid, start, end, q_start, q_end, score, cells)]] by descending score (equal scores by global video number), at
    most k per query and only hits with a positive score.  See `align_spans` for the hit, `threshold` (no default) and `skew`.
    Two stages.  Every query is cut into pieces of `piece` seconds (1 to 32, the last piece shorter) and ONE `tan_clip_topk` sweep
    -- `search_clips`' -- proposes the `pool` (1 to 32) best videos per piece; the union of a query's candidates, without the
    query's own video when exclude_source is set, goes to `align_spans`.  A copy can only be found if one of its pieces lands in
    a piece's pool: a shorter piece survives more re-timing but is less specific, a larger pool admits more videos, and both cost
    sweep time (the sweep grows with the number of pieces) and alignment time (with the candidates).  The defaults piece = 16 and
    pool = 32 have not been measured on real features.
    paths: the hits are CopyPath(hit, seconds) -- the same CopyHits in the same order, each with its second-to-second time map
    (`align_paths` in place of `align_spans`).
    `index`: a `VideoIndex` or a `ShardedIndex`.  Two read-backs: the candidates, then the alignments."""
    queries = list(queries)
    threshold, skew = _align_prices("search_copies", threshold, skew)
    if not queries:
        return []
    k, pool, piece = int(k), int(pool), int(piece)
    if k < 1 or not 1 <= pool <= 32 or not 1 <= piece <= MAX_CLIP_SECONDS:
        raise ValueError(f"search_copies: k >= 1, pool in [1, 32], piece in [1, {MAX_CLIP_SECONDS}]")
    spans = clip_spans(index, queries, MAX_ALIGN_SECONDS)
    clips, q_of = [], []
    for q, (query, (m, source)) in enumerate(zip(queries, spans)):
        for a, n in copy_pieces(m, piece):
            clips.append(query[a:a + n] if source is None else (source[0], source[1] + a, source[1] + a + n - 1))
            q_of.append(q)
    kk = min(pool, len(index.vids))
    tq, c_off = clip_features(index, clips)
    sweep = _Sweep(index, tq)
    top = _TopLists(index, len(clips), kk, 1)
    for s, feat, scale, v_off in index.shard_views():
        top.add(s, ops.clip_topk(sweep.tq, feat, c_off, v_off, min(kk, v_off.numel() - 1), **sweep.scales(scale)))
    _, shard, (row, video) = top.read()                                    # read-back 1; an empty slot has row 0x7fffffff
    cands = [set() for _ in queries]
    for p, q in enumerate(q_of):
        held = row[p] != EMPTY_ROW
        cands[q].update((index.video_base[shard[p][held]] + video[p][held]).tolist())
    pairs = []
    for q, (query, (m, source)) in enumerate(zip(queries, spans)):
        if exclude_source and source is not None:
            cands[q].discard(source[0])
        pairs += [(q, gv) for gv in sorted(cands[q])]
    found = (align_paths if paths else align_spans)(index, [(queries[q], gv) for q, gv in pairs], threshold, skew)      # read-back 2
    out = [[] for _ in queries]
    for (q, gv), hit in zip(pairs, found):
        if hit is not None:
            out[q].append((-(hit.hit if paths else hit).score, gv, hit))
    return [[hit for _, _, hit in sorted(hits, key=lambda e: e[:2])[:k]] for hits in out]


def rerank_window(sec, vlen, seq_len=64):
    """(s0, t): the window `search_rerank` gives a candidate whose best dual second is `sec` in a video of `vlen` seconds -- seq_len
    seconds centred on `sec` (sec - seq_len // 2 first), moved inside the video where it would stick out, the whole video when it is
    shorter than a window."""
    s0 = min(max(int(sec) - seq_len // 2, 0), max(int(vlen) - seq_len, 0))
    return s0, min(seq_len, int(vlen) - s0)


def _rerank_table(v_off, d_row, d_video, T):
    """One window per (query, candidate) of `rank_topk_video`'s [Q, pool] lists, on the device: TAN_WIN_FIELDS rows (vrow, t, krow = q,
    k = 1, s0, vlen, 0, 0) with `rerank_window`'s arithmetic."""
    Q, pool = d_row.shape
    v = d_video.reshape(-1).long()
    first = v_off[v]
    vlen = v_off[v + 1] - first
    s0 = torch.minimum((d_row.reshape(-1) - first - T // 2).clamp(min=0), (vlen - T).clamp(min=0))
    t = torch.clamp(vlen - s0, max=T)
    qn = torch.arange(Q, dtype=torch.int32, device=d_row.device).repeat_interleave(pool)
    zero = torch.zeros_like(qn)
    return torch.stack((first + s0, t, qn, zero + 1, s0, vlen, zero, zero), 1).to(torch.int32).contiguous()


@torch.no_grad()
def search_rerank(index, model, embed_text, queries, k=10, pool=32, seq_len=64, windows_per_pass=256, splits=0, return_sim=False,
                  restrict=None):
    """Two-stage search.  Per query the `pool` best distinct videos of the dual sweep (`search_moments`' candidates: the same
    `tan_rank_topk_video` call), each rescored by the joint encoder on ONE window of `seq_len` seconds around its best dual second
    (`rerank_window`), and the k best of them: [[Reranked(vid, second, score, confidence, alignability, dual_second, dual_score)]
    * k] * len(queries), by descending `score`, equal scores by dual rank.
      score         the largest cosine between the sentence's joint output and a frame's, last joint stage (/ 0.07: the logit)
      second        the first second of the video that attains it
      confidence    the maximum of the softmax over the window's seconds of cosine / 0.07 (`align_corpus`'s confidence)
      alignability  binary_head on the sentence's joint output of stage index 2 (tan_model.py:148, eval_zeroshot_align.py:186):
                    the model's "is this sentence visible at all" logit; None for a model without the head
      dual_second / dual_score   what `search_moments` reports as second / score
    That the order key is the joint cosine ALONE is a definition chosen here; it is not the evaluation's mean of the dual and joint
    similarities (eval_zeroshot_align.py:197-201).  The position offset of every window is 0 (`joint_from_stem`).
    The index needs a stem (`build_index(keep_stem=True)`).  pool is clamped to the number of videos and must lie in [1, 32]; k is
    clamped to the number of videos too, 1 <= k <= pool.  The Q * pool windows run in passes of `windows_per_pass`; one read-back.
    return_sim: also return every window's cosines, (hits, sim [Q, pool, seq_len] f32, candidates in dual rank order, -inf beyond
    a window's seconds), a second read-back.
    restrict: a `RowFilter` of this index made of whole videos (`videos` / `exclude`): it applies to the CANDIDATE stage
    (`tan_rank_topk_video_filtered`); pool and k are clamped to the admitted videos.  One built with `windows` raises ValueError:
    the joint window is cut around the dual second whatever the filter says."""
    if isinstance(index, ShardedIndex):
        raise ValueError("search_rerank: not built for a ShardedIndex; merge the shards")
    if restrict is not None:
        restrict.check(index)
        if restrict.windowed:
            raise ValueError("search_rerank: a filter built with windows does not go with the joint window; restrict by videos / exclude")
    net = _aligner(model)
    if index.stem is None:
        raise ValueError("search_rerank: the index has no stem store (build_index(..., keep_stem=True) / index --keep-stem)")
    head = bool(net.use_alignability_head)
    if head and net.num_decoder_layers < 3:
        raise ValueError("the alignability score reads joint stage index 2 (eval_zeroshot_align.py:186): >= 3 decoder layers")
    queries = list(queries)
    if not queries:
        return ([], np.zeros((0, 0, seq_len), np.float32)) if return_sim else []
    n_videos = len(index.vids) if restrict is None else restrict.n_videos
    pool, k = min(int(pool), n_videos), min(int(k), n_videos)
    if not 1 <= pool <= 32:
        raise ValueError("search_rerank: pool must lie in [1, 32]")
    if not 1 <= k <= pool:
        raise ValueError("search_rerank: k must lie in [1, pool]")
    T, Kp = int(seq_len), RERANK_TEXT_SLOTS
    if not 1 <= T <= JOINT_MAX_LEN[net.compute_dtype] - Kp:
        raise ValueError(f"search_rerank: seq_len must lie in [1, {JOINT_MAX_LEN[net.compute_dtype] - Kp}]")
    if windows_per_pass < 1:
        raise ValueError("search_rerank: windows_per_pass must be >= 1")
    dev, Q = index.feat.device, len(queries)
    # stage 1: the dual sweep, exactly as search_moments runs it
    v_off = index.v_off_device
    d_score, d_row, d_video = _Sweep(index, query_features(index, model, embed_text, queries), restrict, splits).videos(
        0, index.feat, index.scale, v_off, pool)
    table = _rerank_table(v_off, d_row, d_video, T)
    # stage 2: the joint stack over the stem windows, reduced per pass
    emb = embed_text(queries).to(dev).float().reshape(Q, -1).contiguous()
    net._ensure_flat()
    w_head, b_head = (net._f("binary_head.weight").view(-1), net._f("binary_head.bias")) if head else (None, None)
    n_win, Sd = Q * pool, net.num_decoder_layers
    out = torch.empty(n_win, 4, device=dev)
    sim = torch.empty(n_win, T, device=dev) if return_sim else None
    for p0 in range(0, n_win, windows_per_pass):
        p1 = min(p0 + windows_per_pass, n_win)
        W, tab = p1 - p0, table[p0:p1]
        win = torch.empty(W, T, 512, dtype=index.stem.dtype, device=dev)
        vm = torch.empty(W, T, dtype=torch.bool, device=dev)
        txt = torch.empty(W, Kp, emb.shape[1], device=dev)
        tm = torch.empty(W, Kp, dtype=torch.bool, device=dev)
        ops.window_pack(index.stem, emb, tab, T, Kp, win, vm, txt, tm)
        ej = net.joint_from_stem(win, vm, txt, tm)
        ops.rerank_tail(ej.stage(Sd - 1), ej.stage(2) if head else None, tab, T, w_head, b_head, out[p0:p1],
                        sim[p0:p1] if return_sim else None)
        net._release_ws(ej)
    order = ops.rerank_select(out.view(Q, pool, 4), k, stride=4)
    # the one read-back: f32 results as their bit patterns next to the int32 ones
    back = torch.cat((out.view(torch.int32).reshape(-1), order.reshape(-1), d_score.view(torch.int32).reshape(-1), d_row.reshape(-1),
                      d_video.reshape(-1))).cpu().numpy()
    cut = np.cumsum([0, n_win * 4, Q * k, n_win, n_win, n_win])
    res, order, d_score, d_row, d_video = (back[a:b] for a, b in zip(cut[:-1], cut[1:]))
    res, order = res.reshape(Q, pool, 4), order.reshape(Q, k)
    d_score, d_row, d_video = d_score.view(np.float32).reshape(Q, pool), d_row.reshape(Q, pool), d_video.reshape(Q, pool)
    resf = res.view(np.float32)
    hits = []
    for q in range(Q):
        row = []
        for i in order[q]:
            vnum = int(d_video[q, i])
            row.append(Reranked(index.vids[vnum], int(res[q, i, 1]), float(resf[q, i, 0]), float(resf[q, i, 2]),
                                float(resf[q, i, 3]) if head else None, int(d_row[q, i] - index.v_off[vnum]), float(d_score[q, i])))
        hits.append(row)
    if return_sim:
        return hits, sim.view(Q, pool, T).cpu().numpy()
    return hits


class Annotation:
    """What `annotate` returns: the k best labels of every second of an index.
      label / score   int32 / f32 [N, k] on the index's device, rows in the index's order (a `ShardedIndex`: shard after shard);
                      row n holds its k best labels by descending score, equal scores by ascending label number
      labels          the label texts; label[n, j] numbers them
      v_off / vids    the index's: int64 [n_videos + 1], each video's first row, and the videos' names
    `segments` and `label_seconds` read column 0 only: the best label of every second -- or, with `switch=`, the labels of
    `decode`, which may be any of a second's k labels: annotate with k >= 5 when decoding."""

    def __init__(self, label, score, labels, v_off, vids):
        self.label, self.score, self.labels = label, score, list(labels)
        self.v_off, self.vids = np.asarray(v_off, dtype=np.int64), list(vids)
        self._v_off_dev = None

    def __len__(self):
        return int(self.label.shape[0])

    @property
    def k(self):
        return int(self.label.shape[1])

    def _v_off_device(self):
        if self._v_off_dev is None:
            self._v_off_dev = torch.from_numpy(self.v_off.astype(np.int32)).to(self.label.device)
        return self._v_off_dev

    def _check(self, threshold, min_len=1):
        if threshold != threshold:
            raise ValueError("Annotation: threshold must not be NaN")
        if int(min_len) < 1:
            raise ValueError("Annotation: min_len must be >= 1")
        if len(self) >= 2 ** 31:
            raise ValueError("Annotation: 2^31 rows or more; annotate the shards one by one")

    def runs_to_segments(self, runs, peak_score):
        """`ops.label_runs`' kept runs on the host (runs int [5, n]: ops.RUN_FIELDS, global rows; peak_score [n]) ->
        [(vid, start_second, end_second, label_text, peak_second, peak_score)]"""
        video, start, end, label, peak_row = (np.asarray(c, dtype=np.int64) for c in runs)
        first = self.v_off[video]
        return [(self.vids[video[i]], int(start[i] - first[i]), int(end[i] - first[i]), self.labels[label[i]],
                 int(peak_row[i] - first[i]), float(peak_score[i])) for i in range(len(video))]

    def _check_switch(self, threshold, switch):
        if not np.isfinite(threshold):
            raise ValueError("Annotation: decoding needs a finite threshold")
        if not float(switch) >= 0:
            raise ValueError("Annotation: switch must lie in [0, +inf]")
        if len(self) >= 2 ** 31:
            raise ValueError("Annotation: 2^31 rows or more; annotate the shards one by one")

    def decode(self, threshold, switch):
        """(label int32 [N], score f32 [N]) on the device: per video, the sequence of labels -- each one of its second's k kept
        labels, or -1 for background -- that maximises the sum of (score - threshold) over the labelled seconds minus `switch`
        per change of label (`tan_label_decode`; the exact definition is in include/tan_hip.h).  score is the chosen label's own
        score at that second (below the threshold where the path bridges a dip), -inf for background.  switch = 0 is the per-second
        choice; switch = +inf gives one label, or background, per video.  A label outside a second's list cannot be chosen
        there.  One launch, nothing read back."""
        self._check_switch(threshold, switch)
        return ops.label_decode(self.score, self.label, self._v_off_device(), threshold, switch)

    def _decoded_lists(self, threshold, switch):
        """`decode`'s columns as [N, 1] lists for `tan_label_runs`, with the threshold that makes exactly the -inf rows background"""
        label, score = self.decode(threshold, switch)
        return score[:, None], label[:, None], float(np.finfo(np.float32).min)

    def segments(self, threshold, min_len=1, switch=None):
        """[(vid, start_second, end_second, label_text, peak_second, peak_score)] in index order: the maximal runs of seconds of one
        video whose best label is the same and scores >= threshold (a second below it, or with a NaN score, is background), at
        least min_len seconds long; seconds are the video's own, inclusive; the peak is the run's largest score and the first
        second that attains it.  Neighbouring runs are not bridged.  One `tan_label_runs` launch and one read-back.
        switch (a penalty in [0, +inf]; threshold finite): the runs of `decode`'s labels instead -- a run then keeps the seconds
        the path bridged, which score below the threshold, and may hold labels that were not a second's best one."""
        self._check(threshold, min_len)
        cap = max(len(self) // int(min_len), 1)                        # a kept run holds at least min_len rows
        score, label = self.score, self.label
        if switch is not None:
            score, label, threshold = self._decoded_lists(threshold, switch)
        n_runs, runs, peak, _ = ops.label_runs(score, label, len(self.labels), self._v_off_device(), threshold, min_len, cap=cap)
        back = torch.cat((n_runs[:1], runs.reshape(-1), peak.view(torch.int32))).cpu().numpy()
        n = int(back[0])
        return self.runs_to_segments(back[1:1 + 5 * cap].reshape(5, cap)[:, :n], back[1 + 5 * cap:].view(np.float32)[:n])

    def label_seconds(self, threshold, switch=None):
        """{label_text: seconds}: how many seconds of the corpus show each label as their best one with a score >= threshold
        (labels nobody shows included, equal texts added up).  One `tan_label_runs` launch and one read-back.
        switch: count the seconds of `decode`'s labels instead (threshold finite)."""
        self._check(threshold)
        score, label = self.score, self.label
        if switch is not None:
            score, label, threshold = self._decoded_lists(threshold, switch)
        counts = ops.label_runs(score, label, len(self.labels), self._v_off_device(), threshold, 1, cap=0, label_rows=True)[3]
        out = {}
        for text, c in zip(self.labels, counts.cpu().numpy()):
            out[text] = out.get(text, 0) + int(c)
        return out


@torch.no_grad()
def annotate(index, model, embed_text, labels, k=1):
    """The transposed search: for a fixed vocabulary `labels` (step descriptions, tags), the k best labels of EVERY second of the
    index -- an `Annotation`.  score = <index row, unit label feature>, `search`'s score; the label features come from
    `query_features`, so an e4m3 index gets e4m3 labels.  One `tan_label_topk` launch: every index row is read once, the label
    matrix is streamed per 128 rows, and no [N, L] score matrix is stored.  1 <= k <= min(32, len(labels)).
    `index`: a `VideoIndex`, or a `ShardedIndex` -- one launch per shard into the shard's slice of the outputs (host-resident
    shards stream through the two slots), exactly what `VideoIndex.concat` of the shards gives.  The outputs stay on the device:
    k * 8 bytes per row.  There is no `restrict=` here."""
    labels = list(labels)
    if not labels:
        raise ValueError("annotate: no labels")
    k = int(k)
    if not 1 <= k <= min(32, len(labels)):
        raise ValueError("annotate: k must lie in [1, min(32, len(labels))]")
    N, dev = len(index), index.device
    tl = query_features(index, model, embed_text, labels)
    score = torch.empty(N, k, dtype=torch.float32, device=dev)
    label = torch.empty(N, k, dtype=torch.int32, device=dev)
    for s, feat, scale, _ in index.shard_views():
        out = tuple(t[int(index.row_base[s]):int(index.row_base[s + 1])] for t in (score, label))      # the view's slice of the outputs
        if index.e4m3:
            ops.label_topk_e4m3(*tl, feat, scale, k, out=out)
        else:
            ops.label_topk(tl, feat, k, out=out)
    return Annotation(label, score, labels, index.v_off, index.vids)


def write_segments_csv(f, segments):
    """`Annotation.segments`' tuples -> csv rows vid,start,end,label,peak,score under that header"""
    import csv
    w = csv.writer(f, lineterminator="\n")
    w.writerow(("vid", "start", "end", "label", "peak", "score"))
    for vid, start, end, label, peak, score in segments:
        w.writerow((vid, start, end, label, peak, f"{score:.6f}"))


def write_per_second_csv(f, ann):
    """An `Annotation` -> csv rows vid,second,label,score under that header: k rows per second, best label first"""
    import csv
    w = csv.writer(f, lineterminator="\n")
    w.writerow(("vid", "second", "label", "score"))
    label, score = ann.label.cpu().numpy(), ann.score.cpu().numpy()
    for v, vid in enumerate(ann.vids):
        for n in range(int(ann.v_off[v]), int(ann.v_off[v + 1])):
            for j in range(label.shape[1]):
                w.writerow((vid, n - int(ann.v_off[v]), ann.labels[label[n, j]], f"{score[n, j]:.6f}"))


def _parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("index", "query", "annotate"):
        p = sub.add_parser(name)
        p.add_argument("--checkpoint", required=True)
        p.add_argument("--vocab", required=True, help="s3d_dict.npy (the Word2Vec vocabulary)")
        p.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
        p.add_argument("--model", choices=("init", "cotrain"), default="init")
    p = sub.choices["index"]
    p.add_argument("--feature-dir", required=True)
    p.add_argument("--asr-json", required=True)
    p.add_argument("--vlen-csv", required=True)
    p.add_argument("--out", required=True, help="index file (.npz)")
    p.add_argument("--index-dtype", choices=("bf16", "fp32", "e4m3"), default=None,
                   help="row format of the index (default: --dtype); e4m3: 516 bytes per second instead of 1 KiB")
    p.add_argument("--keep-stem", action="store_true",
                   help="also keep video_pre_proj of every second (what `query --rerank` needs): + 1 KiB per second in bf16")
    p.add_argument("--worker-id", type=int, default=0)
    p.add_argument("--num-workers", type=int, default=1)
    for name in ("query", "annotate"):
        p = sub.choices[name]
        p.add_argument("--index", required=True)
        p.add_argument("--shard", action="append", default=None, metavar="PATH",
                       help="a further index file searched together with --index, in the order given (repeatable)")
        p.add_argument("--host-resident", action="store_true",
                       help="keep the rows in pinned host memory and stream them through the card: for an index larger than the card")
    p = sub.choices["annotate"]
    p.add_argument("--labels", required=True, metavar="FILE", help="the vocabulary: one label text per line, blank lines skipped")
    p.add_argument("-k", type=int, default=1, help="labels kept per second, 1 to 32 (segments use the best one)")
    p.add_argument("--threshold", type=float, default=None,
                   help="a second whose best score is below this is background (default: none is)")
    p.add_argument("--min-len", type=int, default=None, help="drop segments shorter than this many seconds (default 1)")
    p.add_argument("--smooth", type=float, default=None, metavar="PENALTY",
                   help="decode every video's labels with this penalty per label change (>= 0; needs a finite --threshold, "
                        "use -k 5 or more): segments bridge short dips and flickers")
    p.add_argument("--per-second", action="store_true", help="write vid,second,label,score for the k labels of every second instead")
    p.add_argument("--out", required=True, metavar="CSV", help="vid,start,end,label,peak,score: one row per segment")
    p = sub.choices["query"]
    p.add_argument("-k", type=int, default=10)
    p.add_argument("--moments", action="store_true",
                   help="the k best distinct videos, each as `sentence vid start end second score` (seconds of the video)")
    p.add_argument("--width", type=float, default=None,
                   help=f"with --moments: a moment extends while the score stays within this of its peak (default {TEMPERATURE})")
    p.add_argument("--sequence", action="store_true",
                   help="the sentences are ONE ordered list of steps: the k videos that show them in order, each as "
                        "`vid score t_0 ... t_{m-1}` (seconds of the video, non-decreasing)")
    p.add_argument("--rerank", action="store_true",
                   help="two stages: the --pool best distinct videos of the dual sweep rescored by the joint encoder, the k best as "
                        "`sentence vid second score confidence alignability dual_second dual_score` (needs index --keep-stem)")
    p.add_argument("--pool", type=int, default=None, help="with --rerank: candidates per sentence, 1 to 32 (default 32)")
    p.add_argument("--only", action="append", default=None, metavar="VID", help="search only this video (repeatable)")
    p.add_argument("--only-file", default=None, metavar="PATH", help="search only the videos listed here, one vid per line")
    p.add_argument("--exclude", action="append", default=None, metavar="VID", help="leave this video out (repeatable)")
    p.add_argument("--exclude-file", default=None, metavar="PATH", help="leave out the videos listed here, one vid per line")
    p.add_argument("--within", action="append", default=None, metavar="VID:FIRST-LAST",
                   help="search this video only between these seconds, inclusive (repeatable; other videos stay whole)")
    p.add_argument("sentences", nargs="+")
    p = sub.add_parser("similar", help="where else in the corpus a piece of an indexed video appears (no checkpoint, no model)")
    p.add_argument("--index", required=True)
    p.add_argument("--shard", action="append", default=None, metavar="PATH",
                   help="a further index file searched together with --index, in the order given (repeatable)")
    p.add_argument("--host-resident", action="store_true",
                   help="keep the rows in pinned host memory and stream them through the card: for an index larger than the card")
    p.add_argument("--clip", action="append", required=True, metavar="VID:FIRST-LAST",
                   help=f"these seconds of this video of the index, inclusive, at most {MAX_CLIP_SECONDS} (repeatable)")
    p.add_argument("-k", type=int, default=10)
    p.add_argument("--keep-source", action="store_true", help="also list the video the clip was cut from (left out by default)")
    p.add_argument("--align", action="store_true",
                   help=f"find re-timed or re-cut copies: the best local alignment of the clip (then up to {MAX_ALIGN_SECONDS} seconds) "
                        "with each candidate video, as `vid start end score q_start q_end cells` (needs --threshold)")
    p.add_argument("--threshold", type=float, default=None,
                   help="with --align: a second of the alignment gains its score minus this (no default: it depends on the features)")
    p.add_argument("--skew", type=float, default=None, help="with --align: the price of a step along one video alone, >= 0 (default 0)")
    p.add_argument("--pool", type=int, default=None, help="with --align: candidate videos per piece, 1 to 32 (default 32)")
    p.add_argument("--piece", type=int, default=None,
                   help=f"with --align: the clip is cut into pieces of this many seconds for the candidate sweep, 1 to {MAX_CLIP_SECONDS} "
                        "(default 16)")
    p.add_argument("--map", default=None, metavar="OUT.csv",
                   help="with --align: write the time map of every hit, one row `query,vid,query_second,first,last` per aligned second "
                        "of the clip (query_second on the clip's own video timeline; first..last the seconds of vid that show it)")
    p = sub.add_parser("merge", help="concatenate index files into one (no checkpoint, no GPU)")
    p.add_argument("--out", required=True, help="index file (.npz)")
    p.add_argument("inputs", nargs="+", help="index files, in the order their videos get")
    return ap


def parse_args(argv=None):
    ap = _parser()
    a = ap.parse_args(argv)
    if a.cmd == "query" and a.sequence and (a.moments or a.width is not None):
        ap.error("--sequence does not go with --moments / --width")
    if a.cmd == "query" and a.sequence and len(a.sentences) > 32:
        ap.error("--sequence takes at most 32 sentences")
    if a.cmd == "query" and a.rerank and (a.sequence or a.moments):
        ap.error("--rerank does not go with --sequence / --moments")
    if a.cmd == "query" and a.rerank and (a.shard or a.host_resident):
        ap.error("--rerank does not go with --shard / --host-resident; merge the index files")
    if a.cmd == "query" and a.pool is not None and not a.rerank:
        ap.error("--pool needs --rerank")
    if a.cmd == "query" and a.pool is not None and not 1 <= a.pool <= 32:
        ap.error("--pool must lie in [1, 32]")
    if a.cmd == "query" and a.width is not None and not a.moments:
        ap.error("--width needs --moments")
    if a.cmd == "query" and a.width is not None and not a.width >= 0:
        ap.error("--width must be >= 0")
    if a.cmd == "index" and not 0 <= a.worker_id < a.num_workers:
        ap.error("--worker-id must lie in [0, --num-workers)")
    if a.cmd == "annotate":
        if not 1 <= a.k <= 32:
            ap.error("-k must lie in [1, 32]")
        if a.per_second and (a.threshold is not None or a.min_len is not None):
            ap.error("--per-second does not go with --threshold / --min-len")
        if a.threshold is not None and a.threshold != a.threshold:
            ap.error("--threshold must not be NaN")
        if a.min_len is not None and a.min_len < 1:
            ap.error("--min-len must be >= 1")
        if a.smooth is not None:
            if a.per_second:
                ap.error("--smooth does not go with --per-second")
            if not a.smooth >= 0:
                ap.error("--smooth must be >= 0")
            if a.threshold is None or not np.isfinite(a.threshold):
                ap.error("--smooth needs a finite --threshold")
    if a.cmd == "query":
        filtered = any(x is not None for x in (a.only, a.only_file, a.exclude, a.exclude_file, a.within))
        if filtered and a.sequence:
            ap.error("--only / --exclude / --within do not go with --sequence")
        if a.within is not None and a.rerank:
            ap.error("--within does not go with --rerank (the joint window is cut around the dual second)")
        try:
            a.within = None if a.within is None else [parse_within(w) for w in a.within]
        except ValueError as e:
            ap.error(str(e))
    if a.cmd == "similar":
        if not a.align and any(x is not None for x in (a.threshold, a.skew, a.pool, a.piece)):
            ap.error("--threshold / --skew / --pool / --piece need --align")
        if a.map is not None and not a.align:
            ap.error("--map needs --align")
        if a.align:
            if a.threshold is None or not np.isfinite(a.threshold):
                ap.error("--align needs a finite --threshold")
            if a.skew is not None and not (a.skew >= 0 and np.isfinite(a.skew)):
                ap.error("--skew must be >= 0 and finite")
            if a.pool is not None and not 1 <= a.pool <= 32:
                ap.error("--pool must lie in [1, 32]")
            if a.piece is not None and not 1 <= a.piece <= MAX_CLIP_SECONDS:
                ap.error(f"--piece must lie in [1, {MAX_CLIP_SECONDS}]")
            if a.k < 1:
                ap.error("-k must be >= 1")
        elif not 1 <= a.k <= (32 if a.keep_source else 31):
            ap.error("-k must lie in [1, 31], or [1, 32] with --keep-source")
        try:
            a.clip = [parse_within(c, "--clip") for c in a.clip]
        except ValueError as e:
            ap.error(str(e))
        for vid, first, last in a.clip:
            if first > last:
                ap.error(f"--clip {vid}:{first}-{last}: FIRST is after LAST")
            if last - first + 1 > (MAX_ALIGN_SECONDS if a.align else MAX_CLIP_SECONDS):
                ap.error(f"--clip {vid}:{first}-{last} holds {last - first + 1} seconds; cut it into clips of at most "
                         f"{MAX_ALIGN_SECONDS if a.align else MAX_CLIP_SECONDS} seconds")
    return a


def parse_within(text, option="--within"):
    """'VID:FIRST-LAST' -> (vid, first, last); the vid may hold colons itself"""
    vid, sep, span = text.rpartition(":")
    first, dash, last = span.partition("-")
    if not sep or not vid or not dash or not first.isdigit() or not last.isdigit():
        raise ValueError(f"{option} takes VID:FIRST-LAST (seconds, inclusive), not {text!r}")
    return vid, int(first), int(last)


def _read_vids(path):
    with open(path) as f:
        return [line.strip() for line in f if line.strip()]


def restrict_from_args(index, a):
    """The `RowFilter` of `query`'s --only / --only-file / --exclude / --exclude-file / --within, or None without any of them"""
    only = (a.only or []) + (_read_vids(a.only_file) if a.only_file else [])
    exclude = (a.exclude or []) + (_read_vids(a.exclude_file) if a.exclude_file else [])
    if not (only or exclude or a.within or a.only is not None or a.only_file):
        return None
    return index.restrict(videos=only if (a.only is not None or a.only_file) else None, exclude=exclude or None, windows=a.within)


def _load_index(a):
    """--index [--shard ...] [--host-resident] -> a `VideoIndex` or a `ShardedIndex`"""
    if a.shard or a.host_resident:
        return ShardedIndex.load([a.index] + (a.shard or []), resident="host" if a.host_resident else "device")
    return VideoIndex.load(a.index)


def main(argv=None):
    a = parse_args(argv)
    if a.cmd == "merge":
        idx = VideoIndex.concat([VideoIndex.load(p, device="cpu") for p in a.inputs])
        idx.save(a.out)
        print(f"{a.out}: {len(idx)} seconds of {len(idx.vids)} videos from {len(a.inputs)} files", file=sys.stderr)
        return 0
    if a.cmd == "similar":
        idx = _load_index(a)
        try:
            if a.align:
                found = search_copies(idx, a.clip, a.k, 32 if a.pool is None else a.pool, 16 if a.piece is None else a.piece,
                                      threshold=a.threshold, skew=a.skew or 0.0, exclude_source=not a.keep_source,
                                      paths=a.map is not None)
            else:
                found = search_clips(idx, a.clip, a.k, exclude_source=not a.keep_source)
        except ValueError as e:
            print(f"similar: {e}", file=sys.stderr)
            return 2
        if a.align:
            if a.map is not None:
                with open(a.map, "w") as f:
                    f.write("query,vid,query_second,first,last\n")
                    for (vid, first, last), hits in zip(a.clip, found):
                        for h, seconds in hits:
                            for i, (lo, hi) in enumerate(seconds.tolist()):
                                f.write(f"{vid}:{first}-{last},{h.vid},{first + h.q_start + i},{lo},{hi}\n")
                found = [[h for h, _ in hits] for hits in found]
            for hits in found:
                for h in hits:
                    print(f"{h.vid}\t{h.start}\t{h.end}\t{h.score:.6f}\t{h.q_start}\t{h.q_end}\t{h.cells}")
            return 0
        for hits in found:
            for h in hits:
                print(f"{h.vid}\t{h.start}\t{h.end}\t{h.score:.6f}")
        return 0
    from .infer_align import build_aligner, make_embed_text, read_corpus
    vocab = np.load(a.vocab)
    model = build_aligner(a.checkpoint, vocab, a.model, a.dtype)
    if a.cmd == "index":
        corpus = read_corpus(a.feature_dir, a.asr_json, a.vlen_csv, a.worker_id, a.num_workers)
        idx = build_index(model, corpus, dtype={"bf16": torch.bfloat16, "fp32": torch.float32, "e4m3": E4M3}[a.index_dtype or a.dtype],
                          keep_stem=a.keep_stem)
        idx.save(a.out)
        print(f"{a.out}: {len(idx)} seconds of {len(idx.vids)} videos", file=sys.stderr)
        return 0
    from .word2vec_model import Word2VecTokenizer
    embed = make_embed_text(model, Word2VecTokenizer(max_words=32, vocab=vocab))
    idx = _load_index(a)
    if a.cmd == "annotate":
        ann = annotate(idx, model, embed, _read_vids(a.labels), a.k)
        with open(a.out, "w", newline="") as f:
            if a.per_second:
                write_per_second_csv(f, ann)
            else:
                write_segments_csv(f, ann.segments(float("-inf") if a.threshold is None else a.threshold, a.min_len or 1, switch=a.smooth))
        print(f"{a.out}: {len(ann)} seconds of {len(ann.vids)} videos against {len(ann.labels)} labels", file=sys.stderr)
        return 0
    if a.sequence:
        for h in search_sequences(idx, model, embed, [a.sentences], a.k)[0]:
            print(f"{h.vid}\t{h.score:.6f}\t" + "\t".join(str(t) for t in h.seconds))
        return 0
    only = restrict_from_args(idx, a)
    if a.rerank:
        pool = 32 if a.pool is None else a.pool
        for sentence, hits in zip(a.sentences, search_rerank(idx, model, embed, a.sentences, min(a.k, pool), pool, restrict=only)):
            for h in hits:
                al = "" if h.alignability is None else f"{h.alignability:.6f}"
                print(f"{sentence}\t{h.vid}\t{h.second}\t{h.score:.6f}\t{h.confidence:.6f}\t{al}\t{h.dual_second}\t{h.dual_score:.6f}")
        return 0
    if a.moments:
        width = TEMPERATURE if a.width is None else a.width
        for sentence, hits in zip(a.sentences, search_moments(idx, model, embed, a.sentences, a.k, width, restrict=only)):
            for m in hits:
                print(f"{sentence}\t{m.vid}\t{m.start}\t{m.end}\t{m.second}\t{m.score:.6f}")
        return 0
    for sentence, hits in zip(a.sentences, search(idx, model, embed, a.sentences, a.k, restrict=only)):
        for vid, sec, score in hits:
            print(f"{sentence}\t{vid}\t{sec}\t{score:.6f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
