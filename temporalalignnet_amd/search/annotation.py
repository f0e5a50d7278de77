"""Annotation: the transposed search.

  * `annotate`: the transposed question -- given a fixed vocabulary of step or action descriptions, which label does every second
    of every video show?  `tan_label_topk` keeps a tile of index rows resident and streams the LABEL matrix past it, so every row's
    k best labels come out of one launch without scratch; `Annotation.segments` turns the best labels into (video, start, end,
    label) runs on the device (`tan_label_runs`) and `Annotation.label_seconds` counts the seconds of every label (`annotate`).
    Neighbouring seconds score almost alike, so the best label flickers; `Annotation.decode` (`tan_label_decode`) is a per-video
    Viterbi decode over the kept lists that pays a penalty per label change, and `segments(..., switch=)` builds its runs from
    the decoded labels (`annotate --smooth PENALTY`).
"""
import csv
from functools import cached_property

import numpy as np
import torch

from .. import ops
from .index import _on_device
from .text import query_features


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

    def __len__(self):
        return int(self.label.shape[0])

    @property
    def k(self):
        return int(self.label.shape[1])

    @cached_property
    def v_off_device(self):
        return _on_device(self.v_off, np.int32, self.label.device)         # as `VideoIndex.v_off_device`

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

    def decode(self, threshold, switch):
        """(label int32 [N], score f32 [N]) on the device: per video, the sequence of labels -- each one of its second's k kept
        labels, or -1 for background -- that maximises the sum of (score - threshold) over the labelled seconds minus `switch`
        per change of label (`tan_label_decode`; the exact definition is in include/tan_hip.h).  score is the chosen label's own
        score at that second (below the threshold where the path bridges a dip), -inf for background.  switch = 0 is the per-second
        choice; switch = +inf gives one label, or background, per video.  A label outside a second's list cannot be chosen
        there.  One launch, nothing read back."""
        if not np.isfinite(threshold):
            raise ValueError("Annotation: decoding needs a finite threshold")
        if not float(switch) >= 0:
            raise ValueError("Annotation: switch must lie in [0, +inf]")
        if len(self) >= 2 ** 31:
            raise ValueError("Annotation: 2^31 rows or more; annotate the shards one by one")
        return ops.label_decode(self.score, self.label, self.v_off_device, threshold, switch)

    def _lists(self, threshold, switch):
        """(score, label, threshold) for `tan_label_runs`: the kept lists as they are, or with `switch` `decode`'s columns as [N, 1]
        lists, with the threshold that makes exactly the -inf rows background"""
        if switch is None:
            return self.score, self.label, threshold
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
        score, label, threshold = self._lists(threshold, switch)
        n_runs, runs, peak, _ = ops.label_runs(score, label, len(self.labels), self.v_off_device, threshold, min_len, cap=cap)
        back = torch.cat((n_runs[:1], runs.reshape(-1), peak.view(torch.int32))).cpu().numpy()
        n = int(back[0])
        return self.runs_to_segments(back[1:1 + 5 * cap].reshape(5, cap)[:, :n], back[1 + 5 * cap:].view(np.float32)[:n])

    def label_seconds(self, threshold, switch=None):
        """{label_text: seconds}: how many seconds of the corpus show each label as their best one with a score >= threshold
        (labels nobody shows included, equal texts added up).  One `tan_label_runs` launch and one read-back.
        switch: count the seconds of `decode`'s labels instead (threshold finite)."""
        self._check(threshold)
        score, label, threshold = self._lists(threshold, switch)
        counts = ops.label_runs(score, label, len(self.labels), self.v_off_device, threshold, 1, cap=0, label_rows=True)[3]
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
    score, label = label_lists(index, query_features(index, model, embed_text, labels), k)
    return Annotation(label, score, labels, index.v_off, index.vids)


def label_lists(index, tl, k, each_shard=None):
    """(score f32, label int32) [N, k] on the index's device: the k best rows of tl -- label features in the index's row format, as
    `query_features` makes them (an e4m3 index: (codes, scales)) -- for every row of the index, one `tan_label_topk` launch per
    shard into the shard's slice of the outputs.  each_shard(feat, scale, score, label): called with every shard's view and its
    slices while the shard is in its slot (`discover_steps` adds the shard's rows to its sums there)."""
    N, dev = len(index), index.device
    score = torch.empty(N, k, dtype=torch.float32, device=dev)
    label = torch.empty(N, k, dtype=torch.int32, device=dev)
    for s, feat, scale, _ in index.shard_views():
        out = tuple(t[int(index.row_base[s]):int(index.row_base[s + 1])] for t in (score, label))      # the view's slice of the outputs
        if index.e4m3:
            ops.label_topk_e4m3(*tl, feat, scale, k, out=out)
        else:
            ops.label_topk(tl, feat, k, out=out)
        if each_shard is not None:
            each_shard(feat, scale, *out)
    return score, label


def write_segments_csv(f, segments):
    """`Annotation.segments`' tuples -> csv rows vid,start,end,label,peak,score under that header"""
    w = csv.writer(f, lineterminator="\n")
    w.writerow(("vid", "start", "end", "label", "peak", "score"))
    for vid, start, end, label, peak, score in segments:
        w.writerow((vid, start, end, label, peak, f"{score:.6f}"))


def write_per_second_csv(f, ann):
    """An `Annotation` -> csv rows vid,second,label,score under that header: k rows per second, best label first"""
    w = csv.writer(f, lineterminator="\n")
    w.writerow(("vid", "second", "label", "score"))
    label, score = ann.label.cpu().numpy(), ann.score.cpu().numpy()
    for v, vid in enumerate(ann.vids):
        for n in range(int(ann.v_off[v]), int(ann.v_off[v + 1])):
            for j in range(label.shape[1]):
                w.writerow((vid, n - int(ann.v_off[v]), ann.labels[label[n, j]], f"{score[n, j]:.6f}"))
