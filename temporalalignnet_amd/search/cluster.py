"""Step discovery: the search that starts from nothing.

  * `discover_steps`: which steps recur in an unlabelled corpus at all?  Spherical k-means over every second of the index, all on
    the device.  An iteration assigns every second to its best centroid with the annotation sweep (`tan_label_topk`, the centroids
    in the labels' place, k = 1), adds every shard's rows into the 64-bit fixed-point sums of their clusters
    (`tan_cluster_accumulate`) and turns the sums into new unit centroids (`tan_cluster_centroids`).  Integer sums do not depend on
    the order of the rows, so a `ShardedIndex`, device- or host-resident, gives the centroids of `VideoIndex.concat` of its shards
    bit for bit, and every run gives the same ones.
  * `StepClusters`: the centroids with every second's cluster and score.  `annotation` hands them to everything that takes a label
    matrix (`Annotation.segments`, `label_seconds`, `decode`), for the clustered index or another one; `exemplars` shows the
    seconds that fit a cluster best; `name` finds the nearest entry of a vocabulary (`discover`, `annotate --clusters`).
"""
import numpy as np
import torch

from .. import ops
from .annotation import Annotation, label_lists
from .index import _locate
from .text import _Sweep, _TopLists, _top_k, query_features

MAX_CLUSTERS = 16384


def centroid_image(index, centroids):
    """f32 centroids [K, 512] on the index's device in the index's row format, as `label_lists` and `_Sweep` take a label or
    query matrix: f32 as they are, bf16 rounded to nearest even, e4m3 as (codes, scales) of `ops.quantize_rows_e4m3`"""
    if index.e4m3:
        return ops.quantize_rows_e4m3(centroids)
    return centroids if index.row_dtype == torch.float32 else centroids.to(torch.bfloat16)


def _gather_rows(index, rows):
    """global rows [K] (ascending or not) of either kind of index -> f32 [K, 512] on the index's device; the rows of a
    host-resident shard are gathered from its pinned host tensors"""
    shard = np.searchsorted(index.row_base, rows, side="right") - 1
    out = torch.empty(len(rows), 512, dtype=torch.float32, device=index.device)
    for s in np.unique(shard):
        at = np.flatnonzero(shard == s)
        sh = index.shards[int(s)]
        local = torch.from_numpy(rows[at] - index.row_base[s]).to(sh.feat.device)
        feat = sh.feat[local].to(index.device)
        if index.e4m3:                                 # the 256 code values come from the host's float8_e4m3fn
            lut = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(index.device)
            feat = lut[feat.long()] * sh.scale[local].to(index.device)[:, None]
        out[torch.from_numpy(at).to(index.device)] = feat.float()
    return out


def _check_k(k, N):
    k = int(k)
    if not 1 <= k <= min(N, MAX_CLUSTERS):
        raise ValueError(f"discover_steps: k must lie in [1, min(N, {MAX_CLUSTERS})]")
    return k


def _init_kind(init, K, N):
    """('rows', int64 [K]) or ('centroids', the tensor) of `discover_steps`' init=; ValueError for anything else"""
    if isinstance(init, torch.Tensor) and init.is_floating_point():
        if init.dtype != torch.float32 or tuple(init.shape) != (K, 512):
            raise ValueError("discover_steps: init centroids are an f32 tensor [k, 512]")
        return "centroids", init
    rows = np.asarray(init.cpu() if isinstance(init, torch.Tensor) else init)
    if rows.dtype.kind not in "iu" or rows.shape != (K,):
        raise ValueError("discover_steps: init is None, k global rows (integers), or an f32 tensor [k, 512] of centroids")
    rows = rows.astype(np.int64)
    if rows.min() < 0 or rows.max() >= N:
        raise ValueError("discover_steps: an init row lies outside [0, N)")
    return "rows", rows


class StepClusters:
    """What `discover_steps` returns.
      centroids          f32 [K, 512] on the device: unit vectors (the f32 master; the sweeps see `centroid_image` of them)
      assign / score     int32 / f32 [N] on the device: every second's cluster and its score against the centroids' image, rows in
                         the index's order; equal scores go to the lower cluster number
      sizes / cohesion   int64 / f32 [K] on the host: the seconds of every cluster, and the mean resultant length of their rows
                         (1: they all coincide; 0 for an empty cluster, which keeps its centroid -- empty clusters are not re-seeded)
      moved / objective  per assignment pass: the seconds whose cluster changed (the first pass: N), and the mean score
      v_off / vids       the index's
      history            with history=True: [(assign, centroids)] of every assignment pass, the last one being (assign, centroids)"""

    def __init__(self, centroids, assign, score, sizes, cohesion, moved, objective, v_off, vids, history=None):
        self.centroids, self.assign, self.score = centroids, assign, score
        self.sizes, self.cohesion = np.asarray(sizes, dtype=np.int64), np.asarray(cohesion, dtype=np.float32)
        self.moved, self.objective = [int(m) for m in moved], [float(o) for o in objective]
        self.v_off, self.vids, self.history = np.asarray(v_off, dtype=np.int64), list(vids), history

    def __len__(self):
        return int(self.centroids.shape[0])

    def labels(self, names=None):
        names = [f"step {c:03d}" for c in range(len(self))] if names is None else list(names)
        if len(names) != len(self):
            raise ValueError("StepClusters: one name per cluster")
        return names

    @torch.no_grad()
    def annotation(self, index, k=1, names=None):
        """The `Annotation` of `index` -- the clustered one or any other of any row format -- with the clusters as the vocabulary:
        the k best clusters of every second (`tan_label_topk` with the centroids' image in that index's format), labelled `names`
        or "step 000", ...  `segments`, `label_seconds` and `decode` then work as for `annotate`.  1 <= k <= min(32, K)."""
        k = int(k)
        if not 1 <= k <= min(32, len(self)):
            raise ValueError("StepClusters.annotation: k must lie in [1, min(32, K)]")
        names = self.labels(names)
        score, label = label_lists(index, centroid_image(index, self.centroids.to(index.device)), k)
        return Annotation(label, score, names, index.v_off, index.vids)

    @torch.no_grad()
    def exemplars(self, index, n=3, splits=0):
        """Per cluster the n seconds of `index` that fit its centroid best, [[(vid, second, score)] * n] * K by descending score:
        `search` with the centroids' image in the query's place (`tan_rank_topk`, folded over the shards).  They are the best rows
        by score, whichever cluster they were assigned to.  n is clamped to the rows and must lie in [1, 32]."""
        n = _top_k("StepClusters.exemplars", n, len(index), name="n")
        sweep = _Sweep(index, centroid_image(index, self.centroids.to(index.device)), splits=splits)
        top = _TopLists(index, len(self), n, 0)
        for s, feat, scale, _ in index.shard_views():
            top.add(s, sweep.rows(s, feat, scale, n))
        score, shard, (row,) = top.read()
        v, sec = _locate(index, shard, row)
        return [[(index.vids[v[c, i]], int(sec[c, i]), float(score[c, i])) for i in range(n)] for c in range(len(self))]

    @torch.no_grad()
    def name(self, index, model, embed_text, labels):
        """Per cluster the nearest entry of a vocabulary, [(label_text, score)] * K: the label features come from
        `query_features(index, ...)` and `tan_label_topk` (k = 1) runs with the centroids' image in the rows' place; `index` gives
        the row format and the device."""
        labels = list(labels)
        if not labels:
            raise ValueError("StepClusters.name: no labels")
        tl = query_features(index, model, embed_text, labels)
        image = centroid_image(index, self.centroids.to(index.device))
        if index.e4m3:
            score, label = ops.label_topk_e4m3(*tl, *image, 1)
        else:
            score, label = ops.label_topk(tl, image, 1)
        back = torch.cat((label.reshape(-1), score.reshape(-1).view(torch.int32))).cpu().numpy()
        return [(labels[int(lab)], float(sc)) for lab, sc in zip(back[:len(self)], back[len(self):].view(np.float32))]

    def save(self, path):
        """One .npz of plain arrays (the history is not kept)"""
        with open(path, "wb") as fh:
            np.savez(fh, centroids=self.centroids.cpu().numpy(), assign=self.assign.cpu().numpy(), score=self.score.cpu().numpy(),
                     sizes=self.sizes, cohesion=self.cohesion, moved=np.asarray(self.moved, dtype=np.int64),
                     objective=np.asarray(self.objective, dtype=np.float64), v_off=self.v_off, vids=np.array(self.vids, dtype=np.str_))

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path, allow_pickle=False) as z:
            on = lambda a: torch.from_numpy(a).to(device).contiguous()                              # noqa: E731
            return cls(on(z["centroids"]), on(z["assign"]), on(z["score"]), z["sizes"], z["cohesion"], z["moved"], z["objective"],
                       z["v_off"], [str(v) for v in z["vids"]])


@torch.no_grad()
def discover_steps(index, k, iters=10, seed=0, init=None, history=False):
    """Spherical k-means over every second of a `VideoIndex` or a `ShardedIndex` (device- or host-resident; f32, bf16 or e4m3 rows):
    `StepClusters` of k unit centroids.  An assignment pass is, per shard and inside one `shard_views` step, `tan_label_topk` with
    k = 1 against the centroids' image in the index's row format (`centroid_image`), a stable argsort of the shard's assignment
    and `tan_cluster_accumulate` into the shared fixed-point sums; after the shards a bincount and `tan_cluster_centroids`.  At most
    `iters` (>= 1) updates are made; the loop ends early when a pass moves no second (one read-back per pass), and after the last
    update one more pass runs, so assign / score belong to the returned centroids.  Bit-identical from run to run, and for a
    `ShardedIndex` exactly what `VideoIndex.concat` of its shards gives.
    1 <= k <= min(N, 16384), N < 2^31.  init: None -- k distinct rows `np.random.default_rng(seed).choice(N, k, replace=False)`,
    sorted, normalised in f32; or k global rows (integers), treated the same way; or an f32 tensor [k, 512] of centroids, taken as
    it is.  Empty clusters keep their centroid and are not re-seeded: `sizes` shows them.  history: keep every pass's
    (assign, centroids)."""
    N = len(index)
    K = _check_k(k, N)
    iters = int(iters)
    if iters < 1:
        raise ValueError("discover_steps: iters must be >= 1")
    if N >= 2 ** 31:
        raise ValueError("discover_steps: 2^31 rows or more")
    if init is None:
        kind, init = "rows", np.sort(np.random.default_rng(seed).choice(N, K, replace=False)).astype(np.int64)
    else:
        kind, init = _init_kind(init, K, N)
    dev = index.device
    if kind == "rows":
        rows = _gather_rows(index, init)
        cent = ops.l2norm_fwd(rows, torch.empty_like(rows), None, K, 512)
    else:
        cent = init.to(dev).contiguous().clone()
    sums = torch.empty(K, 512, dtype=torch.int64, device=dev)

    def add_shard(feat, scale, score, label):
        a = label.view(-1)
        ops.cluster_accumulate(feat, a, torch.argsort(a, stable=True).int(), sums, scale)

    before = torch.full((N,), -1, dtype=torch.int32, device=dev)
    moved, objective, hist = [], [], []
    while True:
        sums.zero_()
        score, label = label_lists(index, centroid_image(index, cent), 1, add_shard)
        assign, score = label.view(N), score.view(N)
        counts = torch.bincount(assign, minlength=K).int()
        new, cohesion = ops.cluster_centroids(sums, counts, cent)
        m, obj = torch.stack(((assign != before).sum().double(), score.double().mean())).cpu().tolist()      # the pass's one read-back
        moved.append(int(m))
        objective.append(obj)
        if history:
            hist.append((assign, cent))
        if len(moved) > iters or (len(moved) > 1 and moved[-1] == 0):
            break
        cent, before = new, assign
    return StepClusters(cent, assign, score, counts.cpu().numpy(), cohesion.cpu().numpy(), moved, objective, index.v_off, index.vids,
                        hist if history else None)
