"""The searches that start from text; above them, from `_top_k` to `read_back`, the plumbing that every search takes from here.

  * `search`: sentences -> `get_textual_feature`, normalised -> `tan_rank_topk` against the index (no [Q, N] score matrix) -> rows
    mapped to (vid, second) on the host.
  * `search_moments`: neighbouring seconds of a video score almost alike, so the k best ROWS are a few videos' adjacent seconds.
    `tan_rank_topk_video` ranks VIDEOS by their best second in the same matrix-free sweep, and `tan_moment_extent` measures how
    far the matching moment extends around that second (`query --moments`).
  * `search_sequences`: "which videos show these steps, in this order, and when?"  `tan_sequence_topk` scores every video of the
    index by the best non-decreasing assignment of seconds to an ordered list of sentences -- `tan_monotonic_decode`'s path, fused
    into the same matrix-free sweep -- and keeps the k best videos; `tan_sequence_scores` and the decode itself then give the
    winners' seconds (`query --sequence`).
  * `search_compound`: "which videos show this AND that, in whatever order, but NOT that?"  `tan_compound_topk` scores every video
    of the index by the weakest of its clauses' peaks in the same matrix-free sweep, drops the videos a banned sentence matches,
    and keeps the k best; `tan_compound_peaks` then gives the winners' per-sentence seconds and peaks (`query --all`).
  * `search_rerank`: two stages. The dual sweep (`tan_rank_topk_video`) proposes `pool` videos per sentence; one 64-second window
    around each candidate's best second is cut out of the index's STEM store (`build_index(keep_stem=True)`: video_pre_proj of
    every second, the part of the video input that depends on neither window nor text), run through the joint stack
    (`TemporalAligner.joint_from_stem`) and reduced by `tan_rerank_tail` to the joint cosine, the second the joint encoder picks,
    its softmax confidence and the alignability logit; `tan_rerank_select` orders the candidates (`query --rerank`).
"""
from collections import namedtuple
from itertools import accumulate

import numpy as np
import torch

from .. import ops
from ..infer_align import JOINT_MAX_LEN, _aligner
from . import coarse as c2f
from .index import ShardedIndex, _locate, _locate_videos, _on_device

TEMPERATURE = 0.07

# one hit of `search_moments`: the video, the moment's first / last second (inclusive), the best second, and its score
Moment = namedtuple("Moment", ("vid", "start", "end", "second", "score"))

# one hit of `search_sequences`: the video, the second of every step (non-decreasing), and the path score
SequenceHit = namedtuple("SequenceHit", ("vid", "seconds", "score"))

# one hit of `search_compound`: the video, its score (the weakest clause), every term's best second of the video and its peak (in term
# order, banned terms included), and the clause that set the score
CompoundHit = namedtuple("CompoundHit", ("vid", "score", "seconds", "scores", "weakest"))

# one hit of `search_rerank`: the video, the second / cosine / softmax confidence / alignability logit (None without the head) of the
# joint encoder on the window around the dual encoder's best second, and that second and its dual score
Reranked = namedtuple("Reranked", ("vid", "second", "score", "confidence", "alignability", "dual_second", "dual_score"))
RERANK_TEXT_SLOTS = 8         # a rerank window holds one sentence; `align_corpus` pads the text side to multiples of 8


def _top_k(what, k, n, name="k"):
    """k clamped to the n rows or videos there are; ValueError unless it then lies in [1, 32], the most a sweep keeps"""
    k = min(int(k), n)
    if not 1 <= k <= 32:
        raise ValueError(f"{what}: {name} must lie in [1, 32]")
    return k


def unit_rows(index, t):
    """f32 rows t [n, 512] (contiguous, on the index's device) as a sweep's query: unit rows in the index's row format (`query_features`)"""
    return _row_format(index, ops.l2norm_fwd(t, torch.empty_like(t), None, t.shape[0], 512))


def _row_format(index, t):
    """f32 unit rows t in the index's row format: the second half of `unit_rows`"""
    if index.e4m3:
        return ops.quantize_rows_e4m3(t)
    return t if index.row_dtype == torch.float32 else ops.cast(t, torch.empty(t.shape, dtype=index.row_dtype, device=index.device))


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

    def blocks(self, feat, scale, s_off, v_off, hits, hit_off, n_x):
        """x f32 [n_x] on the device: `ops.sequence_scores`' blocks of a view's hits [P, 2] = (sequence, video), hit h's at x[hit_off[h]:]"""
        dev = feat.device
        x = torch.empty(n_x, dtype=torch.float32, device=dev)
        return ops.sequence_scores(self.tq, feat, s_off, v_off, _on_device(hits, np.int32, dev), _on_device(hit_off, np.int64, dev), x,
                                   **self.scales(scale))


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


def hits_by_shard(index, shard):
    """A search's second phase over hits whose videos lie in the shards `shard` [n] (a `VideoIndex`: all 0): yields (at: the numbers
    of shard s's hits, s, feat, scale, v_off: its view) for the shards that hold a hit, ascending, under `shard_views`' rule."""
    for s, feat, scale, v_off in index.shard_views([int(s) for s in np.unique(shard)]):
        yield np.flatnonzero(shard == s), s, feat, scale, v_off


def read_back(tensors):
    """ONE read-back of int32 device tensors (f32 ones as their bit patterns, `.view(torch.int32)`): each one's flat host array"""
    flat = [t.reshape(-1) for t in tensors]
    back = torch.cat(flat).cpu().numpy()
    cut = [0, *accumulate(t.numel() for t in flat)]
    return [back[a:b] for a, b in zip(cut, cut[1:])]


@torch.no_grad()
def query_features(index, model, embed_text, queries, text_batch=1024):
    """Unit text features [Q, 512] in the index's dtype; for an e4m3 index (codes uint8 [Q, 512], scale f32 [Q])."""
    return unit_rows(index, _text_features(index, model, embed_text, queries, text_batch))


def _text_features(index, model, embed_text, queries, text_batch=1024):
    """The sentences' text features, f32 [Q, 512] on the index's device, not yet normalised"""
    net = _aligner(model)
    dev = index.device
    return torch.cat([net.get_textual_feature(embed_text(list(queries[a:a + text_batch])).to(dev)).float().reshape(-1, 512)
                      for a in range(0, len(queries), text_batch)], 0).contiguous()


@torch.no_grad()
def search(index, model, embed_text, queries, k=10, splits=0, restrict=None, coarse=None, pool=64):
    """Per query the k best seconds of the corpus: [[(vid, second, score)] * k] * len(queries), by descending score (equal scores
    by index row).  score = <index row, unit text feature>: the stitched dual cosine; / 0.07 gives the evaluation's logit.
    `index`: a `VideoIndex`, or a `ShardedIndex` -- then exactly what `VideoIndex.concat` of its shards gives (as for
    `search_moments` and `search_sequences`): one sweep and one `tan_topk_fold` per shard.  One read-back at the end for either.
    restrict: a `RowFilter` of this index (`index.restrict(...)`): only its rows are swept (`tan_rank_topk_filtered`) and returned,
    with the scores and the order the unrestricted call gives them; k is clamped to the admitted rows.
    coarse: a `CoarseImage` of this index (search/coarse.py): its MXFP4 rows are swept on the device for `pool` candidates per query,
    and only the candidates' full rows -- gathered, for a host-resident index over the host link, instead of every shard -- meet
    the exact sweep.  Every returned entry has the score and the relative order this call gives it without `coarse=`, and the
    results are equal whenever that call's k best lie among the candidates; k is clamped to the distinct candidates.  Not with
    `restrict`."""
    queries = list(queries)
    if not queries:
        return []
    if coarse is not None:
        if restrict is not None:
            raise ValueError("search: coarse= does not go with restrict=")
        coarse.check(index)
        k = _top_k("search", k, len(index))
        unit = _text_features(index, model, embed_text, queries)
        unit = ops.l2norm_fwd(unit, torch.empty_like(unit), None, unit.shape[0], 512)
        return c2f.locate(index, *c2f.search_coarse(index, coarse, unit, _row_format(index, unit), k, pool, splits))
    if restrict is not None:
        restrict.check(index)
    k = _top_k("search", k, len(index) if restrict is None else restrict.n_rows)
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
    k = _top_k("search_moments", k, len(index.vids) if restrict is None else restrict.n_videos)
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
    gv, first = _locate_videos(index, shard, video)
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
    k = _top_k("search_sequences", k, len(index.vids))
    m = np.array([len(seq) for seq in sequences], dtype=np.int64)
    s_off = _on_device(np.concatenate([[0], np.cumsum(m)]), np.int32, index.device)
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
    for at, s, feat, scale, v_off in hits_by_shard(index, shard):
        parts.append((at, *_sequence_seconds(sweep, feat, scale, s_off, v_off, index.shards[s].v_off, m, seq_of_hit[at], video[at])))
    score, *ts = read_back([top.lists[0].view(torch.int32)] + [ts for _, ts, _ in parts])              # read-back 2
    score = score.view(np.float32)
    seconds = [None] * (n_seq * k)
    for (at, _, first), t in zip(parts, ts):
        for j, h in enumerate(at):
            seconds[h] = tuple(int(sec) for sec in t[first[j]:first[j + 1]])
    gv, _ = _locate_videos(index, shard, video)
    return [[SequenceHit(index.vids[gv[p * k + i]], seconds[p * k + i], float(score[p * k + i])) for i in range(k)]
            for p in range(n_seq)]


def _sequence_seconds(sweep, feat, scale, s_off, v_off_dev, v_off, m, seq, video):
    """The seconds of P hits (seq [P], video [P]: a sequence and a video of THIS view each) -- one [m, V] block of scores per hit
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
    x = sweep.blocks(feat, scale, s_off, v_off_dev, np.stack((seq, video), 1), x_off[:-1], int(x_off[-1]))
    ts = torch.empty(int(first[-1]), dtype=torch.int32, device=dev)
    path = torch.empty(P, dtype=torch.float32, device=dev)
    ops.monotonic_decode(x, _on_device(rows, np.int32, dev), torch.arange(int(first[-1]), dtype=torch.int32, device=dev),
                         _on_device(vtab, np.int32, dev), None, torch.empty(x.numel(), dtype=torch.int32, device=dev),
                         torch.empty(int(hv.sum()), device=dev), ts, path)
    return ts, first


class Compound(namedtuple("Compound", ("all", "none"), defaults=((),))):
    """One query of `search_compound`: `all` lists what the video must show -- each element a sentence, or a list of alternative
    sentences (paraphrases: the best one counts) -- and `none` the sentences it must not show."""
    __slots__ = ()


def compound_tables(queries):
    """The host tables of `search_compound`: (sentences: every query's terms one after the other -- its clauses' sentences in
    clause order, then its banned ones --, t_off int64 [n + 1]: each query's first term, then their number, role int32 [terms]: the
    term's clause (its position in `all`), or -1 = banned).  ValueError: a query without a clause, an empty clause, more than 32 terms."""
    sentences, t_off, role = [], [0], []
    for q in queries:
        clauses = [[c] if isinstance(c, str) else list(c) for c in ([q.all] if isinstance(q.all, str) else q.all)]
        if not clauses:
            raise ValueError("search_compound: a query needs at least one clause in `all`")
        if any(not c for c in clauses):
            raise ValueError("search_compound: an empty clause in `all`")
        banned = [q.none] if isinstance(q.none, str) else list(q.none)
        if sum(len(c) for c in clauses) + len(banned) > 32:
            raise ValueError("search_compound: a query holds at most 32 sentences, alternatives and banned ones included")
        for j, c in enumerate(clauses):
            sentences += c
            role += [j] * len(c)
        sentences += banned
        role += [-1] * len(banned)
        t_off.append(len(sentences))
    return sentences, np.array(t_off, dtype=np.int64), np.array(role, dtype=np.int32)


def compound_weakest(peaks, role):
    """(score, clause): a video's compound score from its terms' peaks (f32 [m]) and their roles, by the definition of
    include/tan_hip.h -- a clause is worth the first of its terms that none beats under >, the video the first clause, ascending,
    that none undercuts under < -- and the clause that set it."""
    score = weakest = None
    for j in sorted({int(r) for r in role if r >= 0}):
        g = None
        for p, r in zip(peaks, role):
            if r == j and (g is None or p > g):
                g = p
        if score is None or g < score:
            score, weakest = g, j
    return score, weakest


@torch.no_grad()
def search_compound(index, model, embed_text, queries, k=10, splits=0, veto=None):
    """Per COMPOUND query -- `Compound(all=[...], none=[...])`: every element of `all` is a sentence or a list of alternative
    sentences (one clause), `none` the banned sentences; 1 to 32 sentences in all -- the k videos that show EVERY clause, in whatever
    order, and no banned sentence: [[CompoundHit(vid, score, seconds, scores, weakest)] ...] * len(queries), by descending score
    (equal scores by video number).  A sentence's peak is its best second of the video (`search`'s score), a clause is worth its
    best sentence, and `score` is the video's WEAKEST clause; a video where a banned sentence peaks at `veto` or above is left out,
    so a list may be shorter than k.  `seconds` / `scores` hold every sentence's best second of the video and its peak, in the order
    of `all` (alternatives in place) and then `none` -- the banned ones too: how close the video came to the veto.  `weakest` is
    the position in `all` of the clause that set the score.  k is clamped to the number of videos and must lie in [1, 32].
    veto has no default, like a threshold anywhere here: it is required with a `none` and refused without one.
    `index`: a `VideoIndex`, or a `ShardedIndex` (device- or host-resident) -- then exactly what `VideoIndex.concat` of its shards
    gives: one `tan_compound_topk` and one `tan_topk_fold` per shard, then `tan_compound_peaks` over the shards that hold winners.
    Two read-backs: the winning videos, then scores and peaks.
    There is no `restrict=` and no `coarse=` here: every video is scored whole by the exact sweep (whole-video filters for this
    sweep are not built, and a coarse image proposes rows for one sentence, not videos for a conjunction)."""
    queries = list(queries)
    if not queries:
        return []
    sentences, t_off_h, role_h = compound_tables(queries)
    banned = bool((role_h < 0).any())
    if banned and veto is None:
        raise ValueError("search_compound: `none` needs veto= (no default: its scale is the model's)")
    if not banned and veto is not None:
        raise ValueError("search_compound: veto= without any `none`")
    if veto is not None and veto != veto:
        raise ValueError("search_compound: veto is NaN")
    k = _top_k("search_compound", k, len(index.vids))
    n_query, dev = len(queries), index.device
    t_off, role = _on_device(t_off_h, np.int32, dev), _on_device(role_h, np.int32, dev)
    sweep = _Sweep(index, query_features(index, model, embed_text, sentences), splits=splits)
    # phase 1: every shard's best videos, with row = the shard-local video number
    top = _TopLists(index, n_query, k, 0)
    for s, feat, scale, v_off in index.shard_views():
        top.add(s, ops.compound_topk(sweep.tq, feat, t_off, role, v_off, min(k, v_off.numel() - 1),
                                     veto=float("inf") if veto is None else float(veto), splits=splits, **sweep.scales(scale)))
    shard, video = top.winners()                                           # read-back 1
    # phase 2: the peaks, shard by shard over the shards that hold winners, each over its own hits; an empty slot is no hit
    real = np.flatnonzero(video != 0x7fffffff)
    query_of_hit = np.repeat(np.arange(n_query), k)[real]
    parts = []
    for at, s, feat, scale, v_off in hits_by_shard(index, shard[real]):
        hits = _on_device(np.stack((query_of_hit[at], video[real][at]), 1), np.int32, dev)
        parts.append((at, s, *ops.compound_peaks(sweep.tq, feat, t_off, v_off, hits, **sweep.scales(scale))))
    score, *peaks = read_back([top.lists[0].view(torch.int32)] + [t.view(torch.int32) for part in parts for t in part[2:]])   # read-back 2
    score = score.view(np.float32)
    found = [[] for _ in range(n_query)]
    rows = {}
    for (at, s, *_), ps, pr in zip(parts, peaks[0::2], peaks[1::2]):
        first = index.shards[s].v_off[video[real][at]]
        for j, h in enumerate(at):
            rows[real[h]] = (ps.view(np.float32).reshape(-1, 32)[j], pr.reshape(-1, 32)[j] - first[j])
    gv, _ = _locate_videos(index, shard[real], video[real])
    for h, slot in enumerate(real):                                        # ascending: every query's hits in rank order
        q = query_of_hit[h]
        m = int(t_off_h[q + 1] - t_off_h[q])
        ps, sec = rows[slot]
        _, weakest = compound_weakest(ps[:m], role_h[t_off_h[q]:t_off_h[q + 1]])
        found[q].append(CompoundHit(index.vids[gv[h]], float(score[slot]), tuple(int(t) for t in sec[:m]),
                                    tuple(float(p) for p in ps[:m]), weakest))
    return found


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
    pool, k = _top_k("search_rerank", pool, n_videos, name="pool"), min(int(k), n_videos)
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
        tab = table[p0:p1]
        win, vm, txt, tm = ops.window_pack_fresh(index.stem, emb, tab, T, Kp)
        ej = net.joint_from_stem(win, vm, txt, tm)
        ops.rerank_tail(ej.stage(Sd - 1), ej.stage(2) if head else None, tab, T, w_head, b_head, out[p0:p1],
                        sim[p0:p1] if return_sim else None)
        net._release_ws(ej)
    order = ops.rerank_select(out.view(Q, pool, 4), k, stride=4)
    # the one read-back: f32 results as their bit patterns next to the int32 ones
    res, order, d_score, d_row, d_video = read_back((out.view(torch.int32), order, d_score.view(torch.int32), d_row, d_video))
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
