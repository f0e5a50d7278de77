"""Which `ops` calls the searches make, in which order, over a `VideoIndex` and over a `ShardedIndex`: the launch trace of `search`,
`search_moments`, `search_sequences` and `annotate`, with `search.ops` replaced by a recording stub and `query_features` by zero rows,
on CPU tensors.  A `VideoIndex` is one sweep and nothing else (never a `topk_fold`); a `ShardedIndex` is the same sweep and one fold
per shard.  The table is a statement about behaviour, not about how search.py is organised.  No device needed."""
import numpy as np
import pytest
import torch

from temporalalignnet_amd import ops, search

Q, K = 2, 2
SEQUENCES = [["a"], ["b", "c", "d"]]
LABELS = ["l%d" % i for i in range(4)]


class RecordingOps:
    """`search.ops`, as far as the searches use it: every call is recorded by name and returns zero-filled tensors of the documented
    shapes (caller-owned outputs are zero-filled in place)."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _lists(n, k, ints):
        return (torch.zeros(n, k),) + tuple(torch.zeros(n, k, dtype=torch.int32) for _ in range(ints))

    def rank_topk(self, tq, vn, pair=None, k=0, *, splits=0):
        self.calls.append("rank_topk")
        return (None, None) + self._lists(tq.shape[0], k, 1)

    def rank_topk_e4m3(self, tq, q_scale, vn, v_scale, pair=None, k=0, *, splits=0):
        self.calls.append("rank_topk_e4m3")
        return (None, None) + self._lists(tq.shape[0], k, 1)

    def row_filter_build(self, spans, N, out=None):
        self.calls.append("row_filter_build")
        return torch.zeros(16, dtype=torch.uint8)

    def rank_topk_filtered(self, tq, vn, filt, k, *, q_scale=None, v_scale=None, splits=0):
        self.calls.append("rank_topk_filtered")
        return self._lists(tq.shape[0], k, 1)

    def rank_topk_video(self, tq, vn, v_off, k, *, q_scale=None, v_scale=None, splits=0):
        self.calls.append("rank_topk_video")
        return self._lists(tq.shape[0], k, 2)

    def rank_topk_video_filtered(self, tq, vn, v_off, filt, k, *, q_scale=None, v_scale=None, splits=0):
        self.calls.append("rank_topk_video_filtered")
        return self._lists(tq.shape[0], k, 2)

    def moment_extent(self, tq, vn, v_off, top_score, top_row, top_video, width, *, q_scale=None, v_scale=None):
        self.calls.append("moment_extent")
        return torch.zeros_like(top_row), torch.zeros_like(top_row)

    def sequence_topk(self, tq, vn, s_off, v_off, k, *, q_scale=None, v_scale=None, splits=0):
        self.calls.append("sequence_topk")
        return self._lists(s_off.numel() - 1, k, 1)

    def sequence_scores(self, tq, vn, s_off, v_off, hits, x_off, x, *, q_scale=None, v_scale=None):
        self.calls.append("sequence_scores")
        return x.zero_()

    def monotonic_decode(self, sim, rows, order, vtab, keep, bp, run, ts, path):
        self.calls.append("monotonic_decode")
        ts.zero_()
        path.zero_()

    def label_topk(self, tl, vn, k=1, *, out=None):
        self.calls.append("label_topk")
        for t in out:
            t.zero_()
        return out

    def label_topk_e4m3(self, tl, l_scale, vn, v_scale, k=1, *, out=None):
        self.calls.append("label_topk_e4m3")
        for t in out:
            t.zero_()
        return out

    def topk_fold(self, run, incoming, shard, reset=False):
        self.calls.append("topk_fold")
        for t in run:
            if t is not None:
                t.zero_()
        return run


def _index(vlens, e4m3):
    n = sum(vlens)
    feat = torch.zeros(n, 512, dtype=torch.uint8 if e4m3 else torch.float32)
    return search.VideoIndex(feat, np.concatenate([[0], np.cumsum(vlens)]), ["v%d" % i for i in range(len(vlens))],
                             torch.ones(n) if e4m3 else None)


def _indices(e4m3):
    """(kind, index, the videos of its filter): the filter of the sharded index admits rows of shards 0 and 2 only"""
    return (("video", _index([5, 3, 9], e4m3), [0, 2]),
            ("sharded", search.ShardedIndex([_index(v, e4m3) for v in ([5, 3], [9], [2, 2])]), [0, 3]))


# the ordered `ops` calls of every case, a trailing _e4m3 stripped
SWEEP = {"search": ["rank_topk"], "search_moments": ["rank_topk_video", "moment_extent"]}
FILTERED = {"search": ["rank_topk_filtered"], "search_moments": ["rank_topk_video_filtered", "moment_extent"]}
WANT = {
    ("video", "search", False): SWEEP["search"],
    ("video", "search", True): ["row_filter_build"] + FILTERED["search"],
    ("video", "search_moments", False): SWEEP["search_moments"],
    ("video", "search_moments", True): FILTERED["search_moments"],                          # the images are built by now
    ("video", "search_sequences", False): ["sequence_topk", "sequence_scores", "monotonic_decode"],
    ("video", "annotate", False): ["label_topk"],
    ("sharded", "search", False): (SWEEP["search"] + ["topk_fold"]) * 3,
    ("sharded", "search", True): ["row_filter_build"] * 2 + (FILTERED["search"] + ["topk_fold"]) * 2,
    ("sharded", "search_moments", False): (SWEEP["search_moments"] + ["topk_fold"]) * 3,
    ("sharded", "search_moments", True): (FILTERED["search_moments"] + ["topk_fold"]) * 2,
    # the stub's winners all sit in shard 0: one score block and one decode, for the one shard that holds a winner
    ("sharded", "search_sequences", False): ["sequence_topk", "topk_fold"] * 3 + ["sequence_scores", "monotonic_decode"],
    ("sharded", "annotate", False): ["label_topk"] * 3,
}
# read-backs (`Tensor.cpu()` calls) a search may make at the most: (VideoIndex, ShardedIndex)
READ_BACKS = {"search": (2, 1), "search_moments": (2, 1), "search_sequences": (2, 2), "annotate": (0, 0)}


@pytest.mark.parametrize("e4m3", (False, True), ids=("f32", "e4m3"))
def test_the_searches_make_the_same_ops_calls_in_the_same_order(monkeypatch, e4m3):
    rec = RecordingOps()
    # every module of the package reaches the wrappers as attributes of the one `ops` module: the stub's functions go there
    for name in dir(rec):
        if not name.startswith("_") and callable(getattr(rec, name)):
            monkeypatch.setattr(ops, name, getattr(rec, name))

    def zero_queries(index, model, embed_text, queries, text_batch=1024):
        n = len(list(queries))
        return (torch.zeros(n, 512, dtype=torch.uint8), torch.ones(n)) if index.e4m3 else torch.zeros(n, 512)

    for module in (search.text, search.annotation):                        # where the searches and `annotate` resolve it
        monkeypatch.setattr(module, "query_features", zero_queries)
    read_backs, cpu = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **kw: read_backs.append(1) or cpu(t, *a, **kw))

    seen = {}
    for kind, index, videos in _indices(e4m3):
        filt = index.restrict(videos=videos)
        if kind == "sharded":
            assert filt.shards() == [0, 2]
        calls = [("search", False, lambda: search.search(index, None, None, ["q"] * Q, k=K)),
                 ("search", True, lambda: search.search(index, None, None, ["q"] * Q, k=K, restrict=filt)),
                 ("search_moments", False, lambda: search.search_moments(index, None, None, ["q"] * Q, k=K)),
                 ("search_moments", True, lambda: search.search_moments(index, None, None, ["q"] * Q, k=K, restrict=filt)),
                 ("search_sequences", False, lambda: search.search_sequences(index, None, None, SEQUENCES, k=K)),
                 ("annotate", False, lambda: search.annotate(index, None, None, LABELS, k=K))]
        for name, filtered, call in calls:
            del rec.calls[:], read_backs[:]
            out = call()
            got = [c[:-5] if c.endswith("_e4m3") else c for c in rec.calls]
            seen[kind, name, filtered] = got
            assert got == WANT[kind, name, filtered], (kind, name, filtered, e4m3)
            assert all(c.endswith("_e4m3") == e4m3 for c in rec.calls if c in ("rank_topk", "rank_topk_e4m3", "label_topk", "label_topk_e4m3"))
            assert len(read_backs) <= READ_BACKS[name][kind == "sharded"], (kind, name, filtered, len(read_backs))
            if kind == "video":
                assert "topk_fold" not in got
            if name == "annotate":
                assert out.label.shape == (len(index), K) and out.score.shape == (len(index), K)
            else:
                assert len(out) == 2 and all(len(hits) == K for hits in out)
    assert set(seen) == set(WANT)
