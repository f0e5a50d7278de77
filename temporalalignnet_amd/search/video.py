"""The searches that start from VIDEO: where a clip appears in the corpus, and how a re-timed or re-cut copy lines up with it.

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
"""
from collections import namedtuple

import numpy as np
import torch

from .. import ops
from .index import _locate_videos, _on_device
from .text import _Sweep, _TopLists, hits_by_shard, read_back, unit_rows

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
# one hit of `search_cover`: the video, the score it was ranked by, and both directions of the Chamfer similarity: forward = the mean
# over the QUERY's seconds of each one's best second in the video, backward = the mean over the VIDEO's seconds of each one's best
# second of the query
CoverHit = namedtuple("CoverHit", ("vid", "score", "forward", "backward"))
MAX_COVER_SECONDS = 4096        # a query of `search_cover`: the rows of tan_cover_topk's LDS array of row maxima


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
    rows = unit_rows(index, torch.cat(parts, 0).contiguous())
    return rows, _on_device(np.concatenate([[0], np.cumsum([m for m, _ in spans])]), np.int32, dev)


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


def _clip_sweep(index, clips, kk, splits=0):
    """`search_clips`' sweep, `search_copies`' first stage: one `tan_clip_topk` per shard view, folded, and `_TopLists.read`'s lists"""
    tq, c_off = clip_features(index, clips)
    sweep = _Sweep(index, tq, splits=splits)
    top = _TopLists(index, len(clips), kk, 1)
    for s, feat, scale, v_off in index.shard_views():
        top.add(s, ops.clip_topk(sweep.tq, feat, c_off, v_off, min(kk, v_off.numel() - 1), splits=splits, **sweep.scales(scale)))
    return top.read()


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
    if not 1 <= k <= kk <= 32:                     # not `_top_k`: the sweep's kk = k + 1 has to fit as well
        raise ValueError("search_clips: k must lie in [1, 32], and in [1, 31] with exclude_source")
    score, shard, (row, video) = _clip_sweep(index, clips, kk, splits)    # shard-local; an empty slot has row 0x7fffffff
    out = []
    for p, (m, source) in enumerate(spans):
        n = int((row[p] != EMPTY_ROW).sum())                               # empty slots sort last: the first n are the hits
        number, first = _locate_videos(index, shard[p, :n], video[p, :n])
        entries = [(int(number[i]), int(row[p, i] - first[i]), float(score[p, i])) for i in range(n)]
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
    s_off_dev = _on_device(s_off, np.int32, dev)
    sweep = _Sweep(index, tq)
    q_of, gvs = np.asarray(q_of, dtype=np.int64), np.asarray(gvs, dtype=np.int64)
    shard = np.searchsorted(index.video_base, gvs, side="right") - 1
    parts, heads, maps = [], [], []
    for at, s, feat, scale, v_off in hits_by_shard(index, shard):
        local = gvs[at] - index.video_base[s]
        sv = index.shards[s].v_off
        hits, hit_off, x_off, table, n_x, sum_V = align_tables(ms[q_of[at]], sv[local + 1] - sv[local], first[q_of[at]], local)
        if n_x >= 2 ** 31:
            raise ValueError(f"{what}: the score blocks of one shard's pairs reach 2^31 elements; split the call")
        x = sweep.blocks(feat, scale, s_off_dev, v_off, hits, hit_off, n_x)
        x_off, table_dev = _on_device(x_off, np.int64, dev), _on_device(table, np.int32, dev)
        if paths:
            path_off, n_map, n_trace = path_tables(table[:, 0], table[:, 1])
            score, span, qmap = ops.local_align_path(x, x_off, table_dev, threshold, skew, _on_device(path_off, np.int64, dev),
                                                     sum_V=sum_V, n_map=n_map, n_trace=n_trace)
            maps.append(qmap)
        else:
            score, span = ops.local_align(x, x_off, table_dev, threshold, skew, sum_V=sum_V)
        parts.append((at, path_off[:, 0] if paths else None))
        heads.append(torch.cat((score.view(torch.int32)[:, None], span), 1))
    back = read_back(heads + maps)                                                                # the one read-back
    out = [None] * len(pairs)
    for n, (at, map_row) in enumerate(parts):
        tail = back[len(parts) + n].reshape(-1, 2) if paths else None                           # the shard's map rows
        for e, (h, row) in enumerate(zip(at, back[n].reshape(-1, 6))):
            sc = float(row[:1].view(np.float32)[0])
            if sc > 0:
                out[h] = CopyHit(index.vids[gvs[h]], int(row[3]), int(row[4]), int(row[1]), int(row[2]), sc, int(row[5]))
                if paths:
                    row0 = int(map_row[e])                                                    # the pair's map rows, then its aligned ones
                    out[h] = CopyPath(out[h], tail[row0 + int(row[1]):row0 + int(row[2]) + 1].copy())
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
    _, shard, (row, video) = _clip_sweep(index, clips, min(pool, len(index.vids)))          # read-back 1; an empty slot has row 0x7fffffff
    cands = [set() for _ in queries]
    for p, q in enumerate(q_of):
        held = row[p] != EMPTY_ROW
        cands[q].update(_locate_videos(index, shard[p][held], video[p][held])[0].tolist())
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


@torch.no_grad()
def search_cover(index, queries, k=10, rank="both", exclude_source=False):
    """Video to video whatever the order and the pace: per QUERY the videos of the corpus that share the most seconds with it,
    [[CoverHit(vid, score, forward, backward)]] by descending score (equal scores by index row).  A query is (vid, first, last) --
    seconds of a video of this index, inclusive --, a bare vid (the whole video; a string names the first video that carries it, an
    int is a video number) or a float tensor [m, 512] of index-style rows; 1 to 4096 seconds.  forward is the mean over the query's
    seconds of each second's best score in the hit's video ("how much of my video is in it": a long compilation that contains the
    query scores high), backward the mean over the hit's seconds of each second's best score in the query ("how much of it is in my
    video": a short excerpt of the query scores high); rank = "query" orders by forward, "video" by backward, "both" by their
    mean.  The scores are `search`'s (the stitched dual cosine), the means are `tan_cover_topk`'s: sums in 64-bit fixed point, the
    same bits whatever the tiling or the shards (include/tan_hip.h).
    k is clamped to the number of videos and must lie in [1, 32].  exclude_source: leave out the video a query was cut from (a
    tensor query has none); the sweep is asked for k + 1, so k <= 31.
    `index`: a `VideoIndex`, or a `ShardedIndex` (host-resident too) -- one sweep and one `tan_topk_fold` per shard, exactly what
    `VideoIndex.concat` of its shards gives.  One read-back.  The all-pairs forward / backward block of a shard view (8 bytes x
    queries x videos) is held on the device during its sweep.  There is no `restrict=` here.  ValueError before anything touches
    the device: an unknown rank, k out of range, and what `clip_spans` raises."""
    queries = list(queries)
    if rank not in ops.COVER_RANKS:
        raise ValueError(f"search_cover: rank must be one of {sorted(ops.COVER_RANKS)}, not {rank!r}")
    if not queries:
        return []
    whole = {}
    for q, query in enumerate(queries):                                    # a bare vid: the whole video
        if isinstance(query, (str, int, np.integer)):
            v = _video_number(index, query, whole)
            if v is None:
                raise ValueError(f"clip {q}: no video {query!r} in the index")
            queries[q] = (v, 0, int(index.v_off[v + 1] - index.v_off[v]) - 1)
    spans = clip_spans(index, queries, MAX_COVER_SECONDS)
    if len(queries) > 65535:
        raise ValueError("search_cover: at most 65535 queries per call")
    k = min(int(k), len(index.vids))
    kk = min(k + 1, len(index.vids)) if exclude_source else k
    if not 1 <= k <= kk <= 32:
        raise ValueError("search_cover: k must lie in [1, 32], and in [1, 31] with exclude_source")
    tq, q_off = clip_features(index, queries, MAX_COVER_SECONDS)
    sweep = _Sweep(index, tq)
    top = _TopLists(index, len(queries), kk, 3)
    for s, feat, scale, v_off in index.shard_views():
        score, row, video, fwd, bwd = ops.cover_topk(sweep.tq, feat, q_off, v_off, min(kk, v_off.numel() - 1), rank=rank,
                                                     **sweep.scales(scale))
        at = video.long()
        top.add(s, (score, row, video, fwd.gather(1, at).view(torch.int32), bwd.gather(1, at).view(torch.int32)))
    score, shard, (row, video, fwd, bwd) = top.read()                      # shard-local; an empty slot has row 0x7fffffff
    fwd, bwd = fwd.view(np.float32), bwd.view(np.float32)
    out = []
    for p, (m, source) in enumerate(spans):
        n = int((row[p] != EMPTY_ROW).sum())
        number, _ = _locate_videos(index, shard[p, :n], video[p, :n])
        entries = [(int(number[i]), float(score[p, i]), float(fwd[p, i]), float(bwd[p, i])) for i in range(n)]
        if exclude_source:
            entries = drop_source(entries, None if source is None else source[0], k)
        out.append([CoverHit(index.vids[gv], sc, f, b) for gv, sc, f, b in entries])
    return out
