"""One iteration of step discovery (`search.discover_steps`), part by part: `ops.label_topk` with k = 1 (assign), `torch.argsort`
of the assignment (argsort), `ops.cluster_accumulate` (accumulate) and `ops.cluster_centroids` after a `bincount` (centroids), over a
synthetic index of seeded random unit rows, bf16 and e4m3, one process, device events around each call after a warm-up.  Prints one
JSON line; `--out` also writes the table.

    python tools/cluster_bench.py [--rows 1048576] [-k 256] [--reps 10] [--warmup 3] [--out FILE]

1 Mi rows are 1 GiB of bf16 and 512 MiB + 4 MiB of e4m3 codes and scales: beyond the 256 MB last-level cache, so accumulate streams
its rows from HBM.  Its read bound is N * 1 KiB (bf16) or N * 516 B (e4m3): `accumulate_TBps` counts those bytes once per call
and `of_stream` relates them to the 6.29 TB/s streaming read the project has measured on this part (tools/search_bench.py).  The
rows are gathered in cluster order, 1 KiB (512 B) contiguous each.  `accumulate_unsorted_ms` is the same call with the identity in
`order`'s place: every change of cluster flushes 512 atomics, which is what the sort saves.  The centroids are seeded random unit
vectors, so the sweep's assignment is close to uniform over the clusters.  The timed accumulate calls add into the same sums again
and again (integers wrap); the sums are zeroed before the call whose centroids are timed."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from temporalalignnet_amd import ops  # noqa: E402

STREAM_TBS = 6.29
SLICE = 262144


def unit_rows(n, seed):
    x = torch.randn(n, 512, generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda")
    return x / x.norm(dim=-1, keepdim=True)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def one_format(fmt, N, K, a):
    feat = torch.empty(N, 512, dtype=torch.uint8 if fmt == "e4m3" else torch.bfloat16, device="cuda")
    scale = torch.empty(N, device="cuda") if fmt == "e4m3" else None
    for lo in range(0, N, SLICE):                      # made in slices: the f32 rows of the whole index never exist at once
        x = unit_rows(min(SLICE, N - lo), 1000 + lo // SLICE)
        if fmt == "e4m3":
            ops.quantize_rows_e4m3(x, feat[lo:lo + len(x)], scale[lo:lo + len(x)])
        else:
            feat[lo:lo + len(x)] = x.to(torch.bfloat16)
    cent = unit_rows(K, 7).contiguous()
    image = ops.quantize_rows_e4m3(cent) if fmt == "e4m3" else cent.to(torch.bfloat16)
    out = (torch.empty(N, 1, device="cuda"), torch.empty(N, 1, dtype=torch.int32, device="cuda"))
    if fmt == "e4m3":
        assign_fn = lambda: ops.label_topk_e4m3(*image, feat, scale, 1, out=out)                    # noqa: E731
    else:
        assign_fn = lambda: ops.label_topk(image, feat, 1, out=out)                                 # noqa: E731
    row = dict(format=fmt, rows=N, k=K)
    row["assign_ms"], row["assign_min_ms"] = timed(assign_fn, a.warmup, a.reps)
    assign = out[1].view(N)
    row["argsort_ms"], row["argsort_min_ms"] = timed(lambda: torch.argsort(assign, stable=True).int(), a.warmup, a.reps)
    order = torch.argsort(assign, stable=True).int()
    sums = torch.zeros(K, 512, dtype=torch.int64, device="cuda")
    row["accumulate_ms"], row["accumulate_min_ms"] = timed(lambda: ops.cluster_accumulate(feat, assign, order, sums, scale), a.warmup, a.reps)
    identity = torch.arange(N, dtype=torch.int32, device="cuda")
    row["accumulate_unsorted_ms"], _ = timed(lambda: ops.cluster_accumulate(feat, assign, identity, sums, scale), a.warmup, a.reps)
    sums.zero_()
    ops.cluster_accumulate(feat, assign, order, sums, scale)
    new = (torch.empty(K, 512, device="cuda"), torch.empty(K, device="cuda"))

    def centroids():
        ops.cluster_centroids(sums, torch.bincount(assign, minlength=K).int(), cent, out=new)

    row["centroids_ms"], row["centroids_min_ms"] = timed(centroids, a.warmup, a.reps)
    read = N * (516 if fmt == "e4m3" else 1024)
    row["accumulate_read_bytes"] = read
    row["accumulate_TBps"] = read / (row["accumulate_ms"] * 1e-3) / 1e12
    row["of_stream"] = row["accumulate_TBps"] / STREAM_TBS
    row["bound_ms"] = read / (STREAM_TBS * 1e12) * 1e3
    row["atomics"] = int(((N + 255) // 256 + K) * 512)                  # the sorted launch's upper bound
    row["iteration_ms"] = row["assign_ms"] + row["argsort_ms"] + row["accumulate_ms"] + row["centroids_ms"]
    sizes = torch.bincount(assign, minlength=K)
    row["empty_clusters"], row["largest_cluster"] = int((sizes == 0).sum()), int(sizes.max())
    row["cohesion_mean"] = float(new[1].mean())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1048576)
    ap.add_argument("-k", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    table = [one_format(fmt, a.rows, a.k, a) for fmt in ("bf16", "e4m3")]
    res = dict(bench="cluster", device=torch.cuda.get_device_name(0), stream_TBps=STREAM_TBS, table=table)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
