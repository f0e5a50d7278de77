"""Coarse-to-fine search: an MXFP4 image of the index on the card proposes candidates, the exact sweep rescores them.

A corpus larger than the card can only be searched as `ShardedIndex(resident="host")`, which moves every shard over the host link
for every call.  A `CoarseImage` holds the same rows at 272 bytes per second (the row format of `tan_quantize_rows_mxfp4`,
include/tan_hip.h) and stays on the device.  `search(..., coarse=image, pool=P)` then runs in two stages:

  1. `tan_rank_topk_mxfp4` sweeps the image, shard by shard, and `tan_topk_fold` folds the lists, in ceil(P / 32) rounds: every round
     after the first continues the list below the previous round's last entry (the sweep's cutoff).  Each query has P candidates.
  2. The candidates of ALL queries, unique and in index order, are gathered into one [U, 512] block -- on the device for a
     device-resident index, from pinned host memory through one staging buffer for a host-resident one (no shard is copied and
     `shard_views` is not entered) -- and the index's own exact sweep (`tan_rank_topk` / `_e4m3`) ranks the block.

Identical rows score identically wherever they sit (tan_rank_topk's contract) and the block keeps the index order, so every returned
(vid, second, score) carries the bits the uncoarsened `search` gives that row, in that call's order; and whenever the uncoarsened
top k lie among the gathered rows the two results are equal.
"""
import numpy as np
import torch

from .. import ops
from .index import ShardedIndex, _locate

EMPTY_ROW = 0x7FFFFFFF


def shard_cutoff_row(cut_shard, cut_row, s):
    """int32 [Q] (device): the cutoff rows shard s sweeps with when query q's cutoff entry is (cut_shard[q], cut_row[q]).  The
    fold's order is (score, shard, row): at an equal score a shard before the cutoff's admits no row (0x7fffffff), a shard after it
    every row (-1), the cutoff's own shard the rows after cut_row."""
    other = torch.where(cut_shard > s, torch.full_like(cut_row, EMPTY_ROW), torch.full_like(cut_row, -1))
    return torch.where(cut_shard == s, cut_row, other).contiguous()


def unique_candidates(shard, row):
    """(shard, row) int arrays of any one shape, empty slots (row 0x7fffffff) allowed -> the distinct pairs as int64 keys
    shard << 32 | row, ascending: the index order"""
    shard, row = np.asarray(shard, dtype=np.int64).reshape(-1), np.asarray(row, dtype=np.int64).reshape(-1)
    keep = row != EMPTY_ROW
    return np.unique((shard[keep] << 32) | row[keep])


def split_keys(keys):
    """keys of `unique_candidates` -> (shard int64, row int64)"""
    return keys >> 32, keys & 0xFFFFFFFF


class CoarseImage:
    """One (codes uint8 [n, 256], scales uint8 [n, 16]) pair per shard of the index it was made from, all on the device.
    `stats`: what the last `search(..., coarse=self)` did -- candidates U, bytes staged from the host, rounds."""

    def __init__(self, parts):
        self.parts = [(c.contiguous(), s.contiguous()) for c, s in parts]
        for c, s in self.parts:
            assert c.dtype == torch.uint8 and s.dtype == torch.uint8 and c.dim() == 2 and c.shape[1] == 256 and s.shape == (c.shape[0], 16)
        self.stats = {}

    @property
    def rows(self):
        """every shard's row count"""
        return [int(c.shape[0]) for c, _ in self.parts]

    @property
    def device(self):
        return self.parts[0][0].device

    def nbytes(self):
        return sum(c.numel() + s.numel() for c, s in self.parts)

    @classmethod
    @torch.no_grad()
    def build(cls, index, chunk=1 << 20):
        """The image of a `VideoIndex` or a `ShardedIndex` of any residency and row format (f32, bf16, e4m3: dequantised to f32
        first, which is exact).  A host-resident shard passes through `shard_views` once, here."""
        parts = []
        for _, feat, scale, _ in index.shard_views():
            n = feat.shape[0]
            codes = torch.empty(n, 256, dtype=torch.uint8, device=feat.device)
            scales = torch.empty(n, 16, dtype=torch.uint8, device=feat.device)
            for a in range(0, n, chunk):
                x = feat[a:a + chunk]
                if scale is not None:                  # code values times a power of two: exact in f32
                    x = x.view(torch.float8_e4m3fn).float() * scale[a:a + chunk, None]
                ops.quantize_rows_mxfp4(x.contiguous(), codes[a:a + chunk], scales[a:a + chunk])
            parts.append((codes, scales))
        return cls(parts)

    def check(self, index):
        rows = [len(sh) for sh in index.shards]
        if rows != self.rows:
            raise ValueError(f"coarse image of shards with {self.rows} rows does not fit an index of shards with {rows} rows")
        if self.device != index.device:
            raise ValueError("coarse image and index are on different devices")

    def save(self, path):
        """One .npz of plain arrays: rows [S], and codes_<s> / scales_<s> per shard"""
        arrays = {"rows": np.asarray(self.rows, dtype=np.int64)}
        for i, (c, s) in enumerate(self.parts):
            arrays[f"codes_{i}"], arrays[f"scales_{i}"] = c.cpu().numpy(), s.cpu().numpy()
        with open(path, "wb") as fh:
            np.savez(fh, **arrays)

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path, allow_pickle=False) as z:
            n = len(z["rows"])
            img = cls([(torch.from_numpy(z[f"codes_{i}"]).to(device), torch.from_numpy(z[f"scales_{i}"]).to(device)) for i in range(n)])
            if img.rows != [int(r) for r in z["rows"]]:
                raise ValueError(f"{path}: the shards' row counts do not match their arrays")
        return img


def propose(image, tq, q_scale, pool, splits=0, ops=ops):
    """Stage 1: per query the `pool` best rows of the image by coarse score under the fold's order (score, shard, row):
    (shard [Q, pool], row [Q, pool]) int32 on the device.  ceil(pool / 32) rounds of one sweep and one fold per shard."""
    Q, dev = tq.shape[0], tq.device
    i32 = dict(dtype=torch.int32, device=dev)
    found, below = [], None
    for done in range(0, pool, 32):
        k = min(32, pool - done)
        run = (torch.empty(Q, k, dtype=torch.float32, device=dev), torch.empty(Q, k, **i32), torch.empty(Q, k, **i32), None)
        for s, (codes, scales) in enumerate(image.parts):
            cut = None if below is None else (below[0], shard_cutoff_row(below[1], below[2], s))
            ops.topk_fold(run, ops.rank_topk_mxfp4(tq, q_scale, codes, scales, min(k, codes.shape[0]), splits=splits, below=cut), s,
                          reset=s == 0)
        found.append(run)
        below = tuple(t[:, -1].contiguous() for t in run[:3])
    return torch.cat([r[1] for r in found], 1), torch.cat([r[2] for r in found], 1)


def stage(index, keys, stats):
    """The rows `keys` (ascending) of the index as (feat [U, 512] in the index's row format, scale [U] or None): one `index_select`
    per shard, on the device for a device-resident index, from pinned host memory into one pinned staging buffer otherwise"""
    shard, row = split_keys(keys)
    U, dev = len(keys), index.device
    host = isinstance(index, ShardedIndex) and index.resident == "host"
    where = dict(device="cpu", pin_memory=True) if host else dict(device=dev)
    feat = torch.empty(U, 512, dtype=index.row_dtype, **where)
    scale = torch.empty(U, dtype=torch.float32, **where) if index.e4m3 else None
    cut = np.searchsorted(shard, np.arange(len(index.shards) + 1))
    for s, (a, b) in enumerate(zip(cut, cut[1:])):
        if a == b:
            continue
        sh = index.shards[s]
        at = torch.from_numpy(row[a:b]) if host else torch.from_numpy(row[a:b]).to(dev)
        torch.index_select(sh.feat, 0, at, out=feat[a:b])
        if scale is not None:
            torch.index_select(sh.scale, 0, at, out=scale[a:b])
    stats["staged_bytes"] = (feat.numel() * feat.element_size() + (0 if scale is None else 4 * U)) if host else 0
    return feat, scale


def gather(index, keys, stats):
    """Stage 2's block on the device: `stage`, and for a host-resident index one copy of the staging buffer"""
    feat, scale = stage(index, keys, stats)
    if not feat.is_cuda and index.device.type == "cuda":
        feat, scale = feat.to(index.device, non_blocking=True), None if scale is None else scale.to(index.device, non_blocking=True)
    return feat, scale


def rescore(index, image, tq_fine, cand, k, splits=0, ops=ops):
    """Stage 2: cand = (shard, row) [Q, pool] on the device -> (score [Q, k] f32, shard [Q, k], row [Q, k]) on the host, k clamped
    to the U distinct candidates: the exact sweep's k best of the gathered block, mapped back through the sorted candidates."""
    back = torch.stack(cand).cpu().numpy()             # the one read-back of the pairs
    keys = unique_candidates(back[0], back[1])
    image.stats.update(unique=len(keys))
    feat, scale = gather(index, keys, image.stats)
    k = min(k, len(keys))
    if index.e4m3:
        score, at = ops.rank_topk_e4m3(tq_fine[0], tq_fine[1], feat, scale, None, k, splits=splits)[2:]
    else:
        score, at = ops.rank_topk(tq_fine, feat, None, k, splits=splits)[2:]
    out = torch.cat((score.view(torch.int32)[None], at[None])).cpu().numpy()
    shard, row = split_keys(keys[out[1].astype(np.int64)])
    return out[0].view(np.float32), shard, row


@torch.no_grad()
def search_coarse(index, image, unit_f32, tq_fine, k, pool, splits=0, ops=ops):
    """`search` with `coarse=`: unit_f32 [Q, 512] the queries' unit features, tq_fine the same in the index's row format.  Returns
    (score, shard, row) host arrays [Q, k'], k' = k clamped to the distinct candidates.  `ops`: the kernels' wrappers."""
    image.check(index)
    pool = min(int(pool), len(index))
    if pool < 1:
        raise ValueError("search: pool must be at least 1")
    tq, q_scale = ops.quantize_rows_e4m3(unit_f32)
    image.stats = dict(pool=pool, rounds=-(-pool // 32))
    return rescore(index, image, tq_fine, propose(image, tq, q_scale, pool, splits, ops), k, splits, ops)


def locate(index, score, shard, row):
    """host lists -> [[(vid, second, score)]] as `search` returns them"""
    v, sec = _locate(index, shard, row)
    return [[(index.vids[v[q, i]], int(sec[q, i]), float(score[q, i])) for i in range(score.shape[1])] for q in range(score.shape[0])]
