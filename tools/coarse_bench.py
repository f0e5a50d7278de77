"""Coarse-to-fine search, measured on the protocol of tools/search_bench.py: one process, device events around each call, the median of
--reps after --warmup, caller-owned outputs and scratch.  Prints one JSON line; `--out` also writes it.

    python tools/coarse_bench.py [--rows 4194304] [--queries 1 64 1024] [-k 32] [--pools 32 128] [--reps 10] [--warmup 3] [--out FILE]

(a) `sweeps`: `ops.rank_topk_mxfp4` over the MXFP4 image of seeded random unit rows against `ops.rank_topk_e4m3` and the bf16
    `ops.rank_topk` over the same rows, the three alternating call by call.  4 Mi rows are 1.06 GiB of MXFP4, 2 GiB + 16 MiB of e4m3 and
    4 GiB of bf16: all far beyond the last-level cache.  `*_TBps` counts the index once per sweep, `*_of_stream` relates it to the
    6.29 TB/s streaming read measured on this part.
(b) `search`: `search.search(..., coarse=image, pool=P)` against the plain call on a HOST-RESIDENT three-shard bf16 index of the same
    rows (host clock around calls that end in their read-back; the plain call of the same run is the yardstick), and the split of
    the coarse call into its stages, each timed on its own with device events: `rounds_ms` (sweeps and folds), `read_back_ms`,
    `gather_ms` (the per-shard `index_select` into the pinned staging buffer, timed directly on the host clock), `copy_ms` (that buffer
    to the device) and `fine_ms`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from temporalalignnet_amd import ops, search  # noqa: E402
from temporalalignnet_amd.search import coarse as c2f  # noqa: E402

STREAM_TBS = 6.29
SLICE = 262144


def unit_rows(n, seed):
    x = torch.randn(n, 512, generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda")
    return x / x.norm(dim=-1, keepdim=True)


def timed_round(fns, warmup, reps):
    """Median ms of every routine, the routines alternating call by call (A B C A B C ...)"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for fn, acc in zip(fns, ms):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b))
    return [float(np.median(x)) for x in ms]


def host_clock(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


class _Identity:
    @staticmethod
    def get_textual_feature(x):
        return x


def sweeps_table(N, k, v16, v8, s8, c4, sc4, a):
    rows = []
    for Q in a.queries:
        q = unit_rows(Q, 1 << 30)
        q16 = q.to(torch.bfloat16)
        q8, qs = ops.quantize_rows_e4m3(q)
        ws = torch.empty(max(ops._lib.lib().tan_rank_topk_ws_bytes(Q, N, k), ops._lib.lib().tan_rank_topk_mxfp4_ws_bytes(Q, N, k)),
                         dtype=torch.uint8, device="cuda")
        outs = [(torch.empty(Q, k, device="cuda"), torch.empty(Q, k, dtype=torch.int32, device="cuda")) for _ in range(3)]
        t4, t8, t16 = timed_round((lambda: ops.rank_topk_mxfp4(q8, qs, c4, sc4, k, out=outs[0], ws=ws),
                                   lambda: ops.rank_topk_e4m3(q8, qs, v8, s8, None, k, out=(None, None, *outs[1]), ws=ws),
                                   lambda: ops.rank_topk(q16, v16, None, k, out=(None, None, *outs[2]), ws=ws)), a.warmup, a.reps)
        tb = lambda nbytes, ms: round(N * nbytes / ms * 1e-9, 3)                                # noqa: E731
        overlap = float(np.mean([len(set(x.tolist()) & set(y.tolist())) / k for x, y in zip(outs[0][1].cpu().numpy(), outs[2][1].cpu().numpy())]))
        rows.append({"Q": Q, "k": k, "mxfp4_ms": round(t4, 4), "e4m3_ms": round(t8, 4), "bf16_ms": round(t16, 4),
                     "mxfp4_over_e4m3": round(t4 / t8, 3), "mxfp4_over_bf16": round(t4 / t16, 3),
                     "mxfp4_TBps": tb(272, t4), "e4m3_TBps": tb(516, t8), "bf16_TBps": tb(1024, t16),
                     "mxfp4_of_stream": round(tb(272, t4) / STREAM_TBS, 3), "e4m3_of_stream": round(tb(516, t8) / STREAM_TBS, 3),
                     "bf16_of_stream": round(tb(1024, t16) / STREAM_TBS, 3), "top_k_overlap_with_bf16": round(overlap, 3)})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def search_table(N, k, v16, c4, sc4, a):
    cuts = [0, N // 3, 2 * N // 3, N]
    parts = [search.VideoIndex(v16[c0:c1].cpu().pin_memory(), [0, c1 - c0], [f"s{i}"]) for i, (c0, c1) in enumerate(zip(cuts, cuts[1:]))]
    index = search.ShardedIndex(parts, resident="host")
    image = search.CoarseImage([(c4[c0:c1], sc4[c0:c1]) for c0, c1 in zip(cuts, cuts[1:])])
    rows = []
    for Q in a.search_queries:
        q = unit_rows(Q, 1 << 30)
        embed, queries = (lambda strs: q), [""] * Q
        kk = min(k, 32)
        t_plain = host_clock(lambda: search.search(index, _Identity, embed, queries, k=kk), 1, max(3, a.reps // 3))
        plain = search.search(index, _Identity, embed, queries, k=kk)
        for pool in a.pools:
            t_coarse = host_clock(lambda: search.search(index, _Identity, embed, queries, k=kk, coarse=image, pool=pool), a.warmup, a.reps)
            got = search.search(index, _Identity, embed, queries, k=kk, coarse=image, pool=pool)
            recall = float(np.mean([len({h[:2] for h in g} & {h[:2] for h in p}) / kk for g, p in zip(got, plain)]))
            # the stages, each on its own
            q8, qs = ops.quantize_rows_e4m3(q)
            fine = q.to(torch.bfloat16)
            cand = c2f.propose(image, q8, qs, pool)
            (t_rounds,) = timed_round((lambda: c2f.propose(image, q8, qs, pool),), a.warmup, a.reps)
            t_back = host_clock(lambda: torch.stack(cand).cpu(), a.warmup, a.reps)
            back = torch.stack(cand).cpu().numpy()
            keys = c2f.unique_candidates(back[0], back[1])
            stats = {}
            t_gather = host_clock(lambda: c2f.stage(index, keys, stats), a.warmup, a.reps)     # host work only: the host clock
            pinned = c2f.stage(index, keys, stats)[0]
            dst = torch.empty(len(keys), 512, dtype=torch.bfloat16, device="cuda")
            (t_copy,) = timed_round((lambda: dst.copy_(pinned, non_blocking=True),), a.warmup, a.reps)
            (t_fine,) = timed_round((lambda: ops.rank_topk(fine, dst, None, min(kk, len(keys))),), a.warmup, a.reps)
            rows.append({"Q": Q, "k": kk, "pool": pool, "rows": N, "shards": 3, "plain_host_resident_ms": round(t_plain, 2),
                         "coarse_ms": round(t_coarse, 3), "plain_over_coarse": round(t_plain / t_coarse, 1), "unique": int(len(keys)),
                         "staged_MB": round(stats["staged_bytes"] / 1e6, 3), "index_MB": round(N * 1024 / 1e6, 1),
                         "rounds_ms": round(t_rounds, 4), "read_back_ms": round(t_back, 4),
                         "gather_ms": round(t_gather, 4), "copy_ms": round(t_copy, 4), "fine_ms": round(t_fine, 4),
                         "top_k_recall_vs_plain": round(recall, 4)})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4 * 2 ** 20)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--search-queries", type=int, nargs="+", default=[64])
    ap.add_argument("--pools", type=int, nargs="+", default=[32, 128])
    ap.add_argument("-k", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-search", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N = a.rows
    v16 = torch.empty(N, 512, dtype=torch.bfloat16, device="cuda")
    v8, s8 = torch.empty(N, 512, dtype=torch.uint8, device="cuda"), torch.empty(N, device="cuda")
    c4, sc4 = torch.empty(N, 256, dtype=torch.uint8, device="cuda"), torch.empty(N, 16, dtype=torch.uint8, device="cuda")
    for i, c0 in enumerate(range(0, N, SLICE)):
        x = unit_rows(min(SLICE, N - c0), i)
        v16[c0:c0 + SLICE] = x.to(torch.bfloat16)
        ops.quantize_rows_e4m3(x, v8[c0:c0 + SLICE], s8[c0:c0 + SLICE])
        ops.quantize_rows_mxfp4(x, c4[c0:c0 + SLICE], sc4[c0:c0 + SLICE])
    result = {"bench": "coarse", "rows": N, "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
              "sweeps": sweeps_table(N, a.k, v16, v8, s8, c4, sc4, a)}
    del v8, s8
    if not a.skip_search:
        result["search"] = search_table(N, a.k, v16, c4, sc4, a)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
