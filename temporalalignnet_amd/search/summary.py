"""What a video looks like, in a few seconds of it: storyboards.

  * `storyboard`: per video the k seconds that together cover it best -- thumbnails for a result list, "is this the video I
    meant" at a glance, a compact stand-in for a long video as a `search_cover` query.  Neighbouring seconds score almost alike, so
    every n-th second, or the k seconds that score best against something, are k near-identical frames; greedy facility location
    picks, second by second, the one that raises the mean over ALL the video's seconds of each second's best score to a chosen one.
    The video's own rows are both sides of `tan_sequence_scores` (one [V, V] block per video, the view's rows as the queries: no
    copy), and `tan_storyboard_select` runs the k iterations of a video in one workgroup, in 64-bit fixed point: the result depends
    on no reduction order, and a `ShardedIndex` gives what `VideoIndex.concat` of its shards gives, bit for bit.  No vocabulary, no
    model, one read-back (`storyboard`).
  * `chapters`: where a video's parts begin and end -- kernel temporal segmentation (Potapov et al., ECCV 2014).  Over the same
    [V, V] block, `tan_chapter_costs` gives the within-segment scatter of every stretch [s, e) and `tan_chapter_decode` the
    boundaries that minimise the summed scatter plus a penalty per boundary, by an exact dynamic programme in 64-bit fixed point.
    A scene that comes back later (A B A) is three chapters, where a storyboard has one entry that owns two stretches.
    `Chapters.spans` is what `transfer_segments` takes.
"""
import csv

import numpy as np
import torch

from .. import ops
from .index import _on_device, _video_numbers
from .text import hits_by_shard, read_back
from .video import _index_rows, align_tables, piece_offsets

MAX_STORYBOARD_SECONDS = ops.STORYBOARD_MAX_ROWS        # a video of `storyboard`: the rows of tan_storyboard_select's C in LDS
MAX_STORYBOARD_K = ops.STORYBOARD_MAX_K
MAX_CHAPTER_SECONDS = ops.CHAPTER_MAX_ROWS              # a video of `chapters`: the rows of tan_chapter_decode's dp in LDS
MAX_CHAPTER_K = ops.CHAPTER_MAX_K


def plan_passes(Vs, budget, what="storyboard"):
    """Videos of Vs[i] seconds, in this order, cut into passes [(a, b)] of consecutive videos [a, b) whose sum of V^2 -- the elements
    of a pass's score blocks -- stays within `budget`; a video that exceeds the budget alone gets a pass of its own.  A video is
    never split and the passes keep the order.  ValueError: a budget outside [1, 2^31), in the name of the caller `what`."""
    budget = int(budget)
    if not 1 <= budget < 2 ** 31:
        raise ValueError(f"{what}: budget (score elements per pass) must lie in [1, 2^31)")
    passes, a, held = [], 0, 0
    for i, V in enumerate(Vs):
        need = int(V) * int(V)
        if i > a and held + need > budget:
            passes.append((a, i))
            a, held = i, 0
        held += need
    if len(Vs) > a:
        passes.append((a, len(Vs)))
    return passes


def _wanted(index, videos, skip_long, what="storyboard", a_what="a storyboard", most=MAX_STORYBOARD_SECONDS):
    """(global video numbers int64, ascending; skipped: the vids of the over-long ones left out) of the `videos=` of `what`"""
    wanted = np.arange(len(index.vids), dtype=np.int64) if videos is None else \
        np.asarray(_video_numbers(index.vids, videos, f"{what}(videos)"), dtype=np.int64)
    lens = index.v_off[wanted + 1] - index.v_off[wanted]
    long = lens > most
    if long.any() and not skip_long:
        v = int(wanted[long][0])
        raise ValueError(f"{what}: video {index.vids[v]!r} (number {v}) holds {int(lens[long][0])} seconds; {a_what} takes at "
                         f"most {most} (skip_long=True leaves such videos out)")
    return wanted[~long], [index.vids[int(v)] for v in wanted[long]]


class Storyboard:
    """What `storyboard` returns: per wanted video its entries, in the order they were chosen.
      vids [n] / numbers int64 [n]   the videos, in index order: their names and global video numbers
      second int32 [n, k]            the chosen seconds of each video (0 = its first); -1 after the selection stopped
      coverage f32 [n, k]            the mean over the video's seconds of the best score to any second chosen so far; 0 where second is -1
      owner_off int64 [n + 1], owner int32 [sum V]   per second of each video the entry (0-based) that shows it best
      skipped                        the vids `skip_long=True` left out
    A vid string names the FIRST video of the storyboard that carries it; an int is a global video number."""

    def __init__(self, vids, numbers, second, coverage, owner_off, owner, skipped=()):
        self.vids, self.numbers = list(vids), np.asarray(numbers, dtype=np.int64)
        self.second, self.coverage = np.asarray(second, dtype=np.int32), np.asarray(coverage, dtype=np.float32)
        self.owner_off, self.owner = np.asarray(owner_off, dtype=np.int64), np.asarray(owner, dtype=np.int32)
        self.skipped = list(skipped)
        self._by_name = {}

    def __len__(self):
        return len(self.vids)

    def __eq__(self, other):
        return isinstance(other, Storyboard) and self.vids == other.vids and self.skipped == other.skipped and all(
            a.shape == b.shape and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                                  b.view(np.int32) if b.dtype == np.float32 else b)
            for a, b in ((getattr(self, n), getattr(other, n)) for n in ("numbers", "second", "coverage", "owner_off", "owner")))

    def _at(self, vid):
        if isinstance(vid, str):
            if not self._by_name:
                for i, s in enumerate(self.vids):
                    self._by_name.setdefault(s, i)
            i = self._by_name.get(vid)
        else:
            at = np.flatnonzero(self.numbers == int(vid))
            i = int(at[0]) if len(at) else None
        if i is None:
            raise KeyError(f"storyboard: no video {vid!r}")
        return i

    def owners(self, vid):
        """int32 [V]: per second of the video the entry that shows it best"""
        i = self._at(vid)
        return self.owner[self.owner_off[i]:self.owner_off[i + 1]]

    def frames(self, vid):
        """[(second, coverage, share)] in the order chosen: share is the number of the video's seconds the entry owns"""
        i = self._at(vid)
        n = int((self.second[i] >= 0).sum())
        share = np.bincount(self.owners(vid), minlength=n)
        return [(int(self.second[i, j]), float(self.coverage[i, j]), int(share[j])) for j in range(n)]

    def rows(self, index, vid):
        """f32 [j, 512] on the index's device: the chosen rows of the video, dequantised as `clip_features` reads a clip's -- what
        `search_cover` takes as a query"""
        i = self._at(vid)
        v = int(self.numbers[i])
        lo, hi = int(index.v_off[v]), int(index.v_off[v + 1])
        chosen = self.second[i][self.second[i] >= 0].astype(np.int64)
        return _index_rows(index, lo, hi, index.device)[torch.from_numpy(chosen).to(index.device)]

    def save(self, path):
        with open(path, "wb") as fh:
            np.savez(fh, vids=np.array(self.vids, dtype=np.str_), numbers=self.numbers, second=self.second, coverage=self.coverage,
                     owner_off=self.owner_off, owner=self.owner, skipped=np.array(self.skipped, dtype=np.str_))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls([str(v) for v in z["vids"]], z["numbers"], z["second"], z["coverage"], z["owner_off"], z["owner"],
                       [str(v) for v in z["skipped"]])


def write_storyboard_csv(f, board):
    """vid,rank,second,coverage,share: one row per entry of every video of a `Storyboard`, rank 0 = the first chosen"""
    w = csv.writer(f)
    w.writerow(("vid", "rank", "second", "coverage", "share"))
    for vid, number in zip(board.vids, board.numbers):
        for rank, (second, coverage, share) in enumerate(board.frames(int(number))):
            w.writerow((vid, rank, second, f"{coverage:.6f}", share))


def _check_storyboard(k, min_gain, budget):
    k, min_gain = int(k), float(min_gain)
    if not 1 <= k <= MAX_STORYBOARD_K:
        raise ValueError(f"storyboard: k must lie in [1, {MAX_STORYBOARD_K}]")
    if not (min_gain >= 0 and np.isfinite(min_gain)):
        raise ValueError("storyboard: min_gain must be finite and >= 0")
    plan_passes((), budget)
    return k, min_gain


@torch.no_grad()
def storyboard(index, k=8, *, videos=None, min_gain=0.0, budget=2 ** 28, skip_long=False):
    """Per video the k seconds that together show it best: a `Storyboard`.  Entry j is the second that adds most to the mean, over
    all seconds of the video, of each second's best score to a chosen one (`search`'s score between two index rows); the selection
    of a video stops early when no second adds anything, or less than `min_gain` (finite, >= 0) to that mean
    (`tan_storyboard_select`, defined bit for bit in include/tan_hip.h).  1 <= k <= 4096; a video of fewer than k seconds has fewer
    entries.  videos: the wanted videos, vid strings (EVERY video that carries the string) or global video numbers, as
    `index.restrict(videos=)` takes them (KeyError for an unknown one); default: all.  They are taken in index order.
    `index`: a `VideoIndex` or a `ShardedIndex` (host-resident too), f32 / bf16 / e4m3; a shard without a wanted video is not
    visited.  A shard's wanted videos are cut into passes whose score blocks, sum V^2 elements of 4 bytes, stay within `budget`
    (below 2^31; a video larger than the budget alone is a pass of its own): a pass costs one `tan_sequence_scores` -- the view's
    own rows as the queries, in 32-row pieces that straddle no video -- and one `tan_storyboard_select`.  One read-back at the end.
    ValueError before anything touches the device: k, min_gain or budget out of range, and a wanted video of more than 4096 seconds,
    named -- unless skip_long=True, which leaves such videos out and lists them in `Storyboard.skipped`."""
    k, min_gain = _check_storyboard(k, min_gain, budget)
    wanted, skipped = _wanted(index, videos, skip_long)
    lens = index.v_off[wanted + 1] - index.v_off[wanted]
    owner_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dev = index.device
    shard = np.searchsorted(index.video_base, wanted, side="right") - 1
    parts = []                                          # per pass, in index order: (second, coverage as bits, owner)
    for at, s, feat, scale, v_off in hits_by_shard(index, shard):
        sv = index.shards[s].v_off
        s_off, first = piece_offsets(sv[1:] - sv[:-1])                             # every video of the shard: the queries are its rows
        s_off_dev = _on_device(s_off, np.int32, dev)
        local = wanted[at] - index.video_base[s]
        Vs = lens[at]
        scales = dict(q_scale=scale, v_scale=scale) if index.e4m3 else {}
        for a, b in plan_passes(Vs, budget):
            hits, hit_off, x_off, table, n_x, sum_V = align_tables(Vs[a:b], Vs[a:b], first[local[a:b]], local[a:b])
            x = ops.sequence_scores(feat, feat, s_off_dev, v_off, _on_device(hits, np.int32, dev), _on_device(hit_off, np.int64, dev),
                                    torch.empty(n_x, dtype=torch.float32, device=dev), **scales)
            second, coverage, owner = ops.storyboard_select(x, _on_device(x_off, np.int64, dev), _on_device(table[:, 1:], np.int32, dev),
                                                            k, min_gain=min_gain, sum_V=sum_V)
            parts.append((second, coverage.view(torch.int32), owner))
    if not parts:
        return Storyboard([], wanted, np.empty((0, k), np.int32), np.empty((0, k), np.float32), owner_off, np.empty(0, np.int32), skipped)
    back = read_back([t for part in parts for t in part])                          # the one read-back
    return Storyboard([index.vids[int(v)] for v in wanted], wanted, np.concatenate(back[0::3]).reshape(-1, k),
                      np.concatenate(back[1::3]).view(np.float32).reshape(-1, k), owner_off, np.concatenate(back[2::3]), skipped)


class Chapters:
    """What `chapters` returns: per wanted video its contiguous chapters.
      vids [n] / numbers int64 [n]   the videos, in index order: their names and global video numbers
      count int32 [n]                the number of chapters of each video
      start int32 [n, k]             each chapter's first second (0 = the video's first); -1 from `count` on
      scatter f32 [n, k]             at [j - 1] the summed within-chapter scatter of the best cut into j chapters; +inf where the
                                     video cannot be cut into j chapters of min_len seconds
      chapter_off int64 [n + 1], chapter int32 [sum V]   per second of each video its chapter (0-based)
      skipped                        the vids `skip_long=True` left out
    A vid string names the FIRST video that carries it; an int is a global video number."""

    _FIELDS = ("numbers", "count", "start", "scatter", "chapter_off", "chapter")

    def __init__(self, vids, numbers, count, start, scatter, chapter_off, chapter, skipped=()):
        self.vids, self.numbers = list(vids), np.asarray(numbers, dtype=np.int64)
        self.count, self.start = np.asarray(count, dtype=np.int32), np.asarray(start, dtype=np.int32)
        self.scatter = np.asarray(scatter, dtype=np.float32)
        self.chapter_off, self.chapter = np.asarray(chapter_off, dtype=np.int64), np.asarray(chapter, dtype=np.int32)
        self.skipped = list(skipped)
        self._by_name = {}

    def __len__(self):
        return len(self.vids)

    def __eq__(self, other):
        return isinstance(other, Chapters) and self.vids == other.vids and self.skipped == other.skipped and all(
            a.shape == b.shape and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                                  b.view(np.int32) if b.dtype == np.float32 else b)
            for a, b in ((getattr(self, n), getattr(other, n)) for n in self._FIELDS))

    __hash__ = None

    def _at(self, vid):
        if isinstance(vid, str):
            if not self._by_name:
                for i, s in enumerate(self.vids):
                    self._by_name.setdefault(s, i)
            i = self._by_name.get(vid)
        else:
            at = np.flatnonzero(self.numbers == int(vid))
            i = int(at[0]) if len(at) else None
        if i is None:
            raise KeyError(f"chapters: no video {vid!r}")
        return i

    def of(self, vid):
        """int32 [V]: per second of the video its chapter"""
        i = self._at(vid)
        return self.chapter[self.chapter_off[i]:self.chapter_off[i + 1]]

    def spans(self, vid):
        """[(start, end inclusive, chapter)] in seconds of the video: the segments `transfer_segments` takes"""
        i = self._at(vid)
        n, V = int(self.count[i]), int(self.chapter_off[i + 1] - self.chapter_off[i])
        edges = [int(s) for s in self.start[i, :n]] + [V]
        return [(edges[c], edges[c + 1] - 1, c) for c in range(n)]

    def save(self, path):
        with open(path, "wb") as fh:
            np.savez(fh, vids=np.array(self.vids, dtype=np.str_), skipped=np.array(self.skipped, dtype=np.str_),
                     **{n: getattr(self, n) for n in self._FIELDS})

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls([str(v) for v in z["vids"]], *(z[n] for n in cls._FIELDS), [str(v) for v in z["skipped"]])


def write_chapters_csv(f, chaps):
    """vid,chapter,start,end,seconds: one row per chapter of every video of a `Chapters`, end inclusive"""
    w = csv.writer(f)
    w.writerow(("vid", "chapter", "start", "end", "seconds"))
    for vid, number in zip(chaps.vids, chaps.numbers):
        for start, end, c in chaps.spans(int(number)):
            w.writerow((vid, c, start, end, end - start + 1))


def _check_chapters(k, penalty, min_len, budget):
    k, penalty, min_len = int(k), float(penalty), int(min_len)
    if not 1 <= k <= MAX_CHAPTER_K:
        raise ValueError(f"chapters: k must lie in [1, {MAX_CHAPTER_K}]")
    if not (penalty >= 0 and np.isfinite(penalty)):
        raise ValueError("chapters: penalty must be finite and >= 0")
    if not 1 <= min_len <= MAX_CHAPTER_SECONDS:
        raise ValueError(f"chapters: min_len must lie in [1, {MAX_CHAPTER_SECONDS}]")
    plan_passes((), budget, "chapters")
    return k, penalty, min_len


@torch.no_grad()
def chapters(index, k=12, *, penalty, min_len=1, videos=None, budget=2 ** 27, skip_long=False):
    """Each video cut into at most k contiguous chapters: a `Chapters`.  Kernel temporal segmentation: the boundaries that minimise
    the summed within-chapter scatter of the video's seconds (`search`'s score between two index rows as the kernel) plus `penalty`
    per boundary, found exactly by dynamic programming (`tan_chapter_costs`, `tan_chapter_decode`, defined bit for bit in
    include/tan_hip.h).  penalty (finite, >= 0) has NO default: it is absolute, in score x seconds -- a boundary is kept only if
    it lowers the summed scatter by at least that much -- and its scale is the model's.  1 <= k <= 256; every chapter holds at
    least min_len seconds (1 to 4096; a shorter video is one chapter).  videos, `index`, skip_long: as `storyboard` takes them.  A
    shard's wanted videos are cut into passes whose score blocks, sum V^2 elements, stay within `budget` (below 2^31; a pass holds
    12 bytes per element: the scores and the 64-bit costs): a pass costs one `tan_sequence_scores`, one `tan_chapter_costs` and one
    `tan_chapter_decode`.  One read-back at the end.
    ValueError before anything touches the device: k, penalty, min_len or budget out of range, and a wanted video of more than 4096
    seconds, named -- unless skip_long=True, which leaves such videos out and lists them in `Chapters.skipped`."""
    k, penalty, min_len = _check_chapters(k, penalty, min_len, budget)
    wanted, skipped = _wanted(index, videos, skip_long, "chapters", "a chapter cut", MAX_CHAPTER_SECONDS)
    lens = index.v_off[wanted + 1] - index.v_off[wanted]
    chapter_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dev = index.device
    shard = np.searchsorted(index.video_base, wanted, side="right") - 1
    parts = []                                          # per pass, in index order: (count, start, scatter as bits, chapter)
    for at, s, feat, scale, v_off in hits_by_shard(index, shard):
        sv = index.shards[s].v_off
        s_off, first = piece_offsets(sv[1:] - sv[:-1])
        s_off_dev = _on_device(s_off, np.int32, dev)
        local = wanted[at] - index.video_base[s]
        Vs = lens[at]
        scales = dict(q_scale=scale, v_scale=scale) if index.e4m3 else {}
        for a, b in plan_passes(Vs, budget, "chapters"):
            hits, hit_off, x_off, table, n_x, sum_V = align_tables(Vs[a:b], Vs[a:b], first[local[a:b]], local[a:b])
            x = ops.sequence_scores(feat, feat, s_off_dev, v_off, _on_device(hits, np.int32, dev), _on_device(hit_off, np.int64, dev),
                                    torch.empty(n_x, dtype=torch.float32, device=dev), **scales)
            x_off_dev, table_dev = _on_device(x_off, np.int64, dev), _on_device(table[:, 1:], np.int32, dev)
            cost = ops.chapter_costs(x, x_off_dev, table_dev)
            count, start, scatter, chapter = ops.chapter_decode(cost, x_off_dev, table_dev, k, penalty=penalty, min_len=min_len,
                                                                sum_V=sum_V)
            parts.append((count, start, scatter.view(torch.int32), chapter))
    if not parts:
        return Chapters([], wanted, np.empty(0, np.int32), np.empty((0, k), np.int32), np.empty((0, k), np.float32), chapter_off,
                        np.empty(0, np.int32), skipped)
    back = read_back([t for part in parts for t in part])                          # the one read-back
    return Chapters([index.vids[int(v)] for v in wanted], wanted, np.concatenate(back[0::4]), np.concatenate(back[1::4]).reshape(-1, k),
                    np.concatenate(back[2::4]).view(np.float32).reshape(-1, k), chapter_off, np.concatenate(back[3::4]), skipped)
