"""The per-second index of a corpus: building it, the two index classes, and the row filters.

  * `build_index`: the window stepping of `eval_align.plan_windows` with every second covered (no sentences involved), passes of up
    to `windows_per_pass` windows cut across video boundaries and packed by `tan_window_pack`, the video stack only, then
    `tan_window_feat_acc / _final`: index[t] = the mean over the windows covering second t of the L2-normalised last-stage feature.
    The text side of the dual similarity is the same unit vector t_hat in every window, so <index[t], t_hat> / 0.07 is the stitched
    dual similarity of eval_zeroshot_align.py:198,201 -- computed without knowing the sentence.
  * an e4m3 index (`build_index(dtype="e4m3")`, `VideoIndex.quantize`, `--index-dtype e4m3`) keeps a row as 512 OCP e4m3fn codes
    and one power-of-two f32 scale (include/tan_hip.h): 516 bytes per second of video instead of 1 KiB.  The query is quantised by
    the same kernel and `tan_rank_topk_e4m3` sweeps the codes.
  * `ShardedIndex`: several index files (one per `index --worker-id`) searched together, or one corpus larger than the card streamed
    from pinned host memory.  Every shard is swept on its own and `tan_topk_fold` folds the per-shard lists on the device under the
    sweeps' own order: `search`, `search_moments` and `search_sequences` return what they return for `VideoIndex.concat` of the
    shards, bit for bit (`query --shard`, `query --host-resident`, `merge`).
  * `restrict`: `index.restrict(videos=, exclude=, windows=)` gives a `RowFilter` -- a playlist, the videos already shown, known
    time windows -- that `search`, `search_moments` and `search_rerank` take as `restrict=`.  The sweep walks only the 64-row tiles
    that hold an admitted row (`tan_row_filter_build`, `tan_rank_topk_filtered`) and returns those rows with the unrestricted
    sweep's scores; a host-resident shard without an admitted row is not copied (`query --only / --exclude / --within`).
"""
from functools import cached_property

import numpy as np
import torch

from .. import ops
from ..infer_align import PASSES_PER_CHUNK, WIN_FIELDS, _aligner, _prefetch, load_packed

E4M3 = "e4m3"


def _on_device(a, dtype, dev):
    """a host array as a contiguous tensor of `dtype` (np.int32 / np.int64: the kernels' tables and offsets) on `dev`"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


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
            spans = _on_device(self.shard_spans(s), np.int32, self._index.device)
            self._images[s] = ops.row_filter_build(spans, len(self._index.shards[s]))
        return self._images[s]

    def clip(self, row, start, end):
        """Global rows: [start, end] cut to the admitted span that holds `row`."""
        i = np.searchsorted(self.spans[:, 0], row, side="right") - 1
        return np.maximum(start, self.spans[i, 0]), np.minimum(end, self.spans[i, 1] - 1)


def _restrict(index, videos=None, exclude=None, windows=None):
    """The `RowFilter` that admits only some of this index's rows, for `search`, `search_moments` and `search_rerank`
    (`restrict=`): `VideoIndex.restrict` and `ShardedIndex.restrict`.  videos: the videos to search (default: all); exclude: videos
    to leave out; both iterables of vid strings or video numbers -- a string names EVERY video that carries it (equal strings are
    distinct videos), an unknown one raises KeyError.  windows: iterable of (video, first_second, last_second), inclusive, clamped
    to the video; several windows of a video are merged; an admitted video that `windows` names is narrowed to them, the others
    stay whole.  ValueError when nothing is admitted.  A `ShardedIndex`: videos count over all shards, in shard order; the spans are
    cut per shard, and a search leaves out the shards without an admitted row (resident="host": they are not copied)."""
    spans, n_videos = restrict_spans(index.v_off, index.vids, videos, exclude, windows)
    return RowFilter(index, spans, n_videos, windows is not None)


def _locate(index, shard, row):
    """(shard, shard-local row) of either kind of index -> (global video number, second)"""
    g = index.row_base[np.asarray(shard, dtype=np.int64)] + np.asarray(row, dtype=np.int64)
    v = np.searchsorted(index.v_off, g, side="right") - 1
    return v, g - index.v_off[v]


def _locate_videos(index, shard, video):
    """(shard, shard-local video number) of either kind of index, arrays of one shape -> (global video number, the video's first row
    IN ITS SHARD: a hit's shard-local row minus it is its second).  An empty slot names no shard: the caller leaves it out."""
    shard = np.asarray(shard, dtype=np.int64)
    v = index.video_base[shard] + np.asarray(video, dtype=np.int64)
    return v, index.v_off[v] - index.row_base[shard]


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
        # to the searches this is a `ShardedIndex` of one shard, itself (`shards`, `shard_views`): its rows and videos are the global ones
        self.row_base, self.video_base = (np.array([0, n], dtype=np.int64) for n in (feat.shape[0], len(self.vids)))

    @cached_property
    def v_off_device(self):
        """v_off as int32 on feat's device, made on first use and kept (it is not part of the file format)."""
        return _on_device(self.v_off, np.int32, self.feat.device)

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

    restrict = _restrict

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
            self._v_off_dev = [_on_device(sh.v_off, np.int32, self.device) for sh in self.shards]
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

    restrict = _restrict

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
    e4m3 = dtype == E4M3 or dtype == torch.float8_e4m3fn
    net = _aligner(model)
    device = torch.device("cuda", torch.cuda.current_device())
    feats, scales, stems, vlens, vids = [], [], [], [], []
    no_text = torch.zeros(1, 8, device=device)
    for ch in _prefetch(_index_chunks(videos, seq_len, windows_per_pass), device):
        n_rows = int(ch.v_off[-1])
        acc = torch.zeros(n_rows, 512, device=device)
        cnt = torch.zeros(n_rows, device=device)
        if keep_stem:
            stems.append(net.video_stem(ch.video))
        for p0, p1 in ch.passes:
            tab = ch.table_d[p0:p1]
            vid, vm, _, _ = ops.window_pack_fresh(ch.video, no_text, tab, seq_len, 1)
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
