"""Corpus sweep time: `ops.rank_topk` over a bf16 index against `ops.rank_topk_e4m3` over the e4m3 index of the same rows, one
process, device events around each call, caller-owned outputs and scratch.  Prints one JSON line; `--out` also writes the table.

    python tools/search_bench.py [--rows 4194304] [--queries 1 64 1024] [-k 10] [--reps 10] [--warmup 3] [--out FILE]

Rows: seeded random unit rows, made in slices.  4 Mi rows are 4 GiB of bf16 and 2 GiB + 16 MiB of e4m3 codes and scales: both far
beyond the 256 MB last-level cache, so every sweep streams its index from HBM.  Bytes per second count the index once per sweep
(at Q <= 128, one query tile, that is all a sweep reads); `of_stream` relates them to the 6.29 TB/s streaming read the project has
measured on this part.  The yardstick is the bf16 sweep of the same run."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4 * 2 ** 20)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, k = a.rows, a.k
    v16 = torch.empty(N, 512, dtype=torch.bfloat16, device="cuda")
    v8 = torch.empty(N, 512, dtype=torch.uint8, device="cuda")
    s8 = torch.empty(N, device="cuda")
    for r in range(0, N, SLICE):
        x = unit_rows(min(SLICE, N - r), r)
        v16[r:r + SLICE] = x.to(torch.bfloat16)
        ops.quantize_rows_e4m3(x, v8[r:r + SLICE], s8[r:r + SLICE])
    del x
    rows = []
    for Q in a.queries:
        q = unit_rows(Q, 1 << 30)
        q16 = q.to(torch.bfloat16)
        q8, qs8 = ops.quantize_rows_e4m3(q)
        ws = torch.empty(ops.rank_topk_ws_bytes(Q, N, k), dtype=torch.uint8, device="cuda")
        out = (None, None, torch.empty(Q, k, device="cuda"), torch.empty(Q, k, dtype=torch.int32, device="cuda"))
        t16, b16 = timed(lambda: ops.rank_topk(q16, v16, None, k, out=out, ws=ws), a.warmup, a.reps)
        top16 = out[3].clone()
        t8, b8 = timed(lambda: ops.rank_topk_e4m3(q8, qs8, v8, s8, None, k, out=out, ws=ws), a.warmup, a.reps)
        agree = float((top16[:, 0] == out[3][:, 0]).float().mean())
        by16, by8 = N * 1024, N * 516
        rows.append({"Q": Q, "bf16_ms": round(t16, 4), "bf16_min_ms": round(b16, 4), "e4m3_ms": round(t8, 4), "e4m3_min_ms": round(b8, 4),
                     "e4m3_over_bf16": round(t8 / t16, 3),
                     "bf16_TBps": round(by16 / t16 * 1e-9, 3), "e4m3_TBps": round(by8 / t8 * 1e-9, 3),
                     "bf16_of_stream": round(by16 / t16 * 1e-9 / STREAM_TBS, 3), "e4m3_of_stream": round(by8 / t8 * 1e-9 / STREAM_TBS, 3),
                     "bf16_TFLOPs": round(2.0 * Q * N * 512 / t16 * 1e-9, 1), "e4m3_TFLOPs": round(2.0 * Q * N * 512 / t8 * 1e-9, 1),
                     "top1_agree": round(agree, 4)})
    res = {"rows": N, "k": k, "reps": a.reps, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0), "stream_TBps": STREAM_TBS,
           "table": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(f"# tools/search_bench.py --rows {N} -k {k}: median of {a.reps} after {a.warmup} warm-ups, {res['gpu']}\n")
            fh.write(f"# index bytes per sweep: bf16 {N * 1024}, e4m3 {N * 516}; of_stream = bytes/s over {STREAM_TBS} TB/s\n")
            cols = list(rows[0])
            fh.write(" ".join(f"{c:>15}" for c in cols) + "\n")
            for r in rows:
                fh.write(" ".join(f"{r[c]:>15}" for c in cols) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
