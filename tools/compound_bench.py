"""Compound search against its yardstick, on the protocol of tools/coarse_bench.py: one process, device events around each call, the
median of --reps after --warmup, caller-owned outputs and scratch.  Prints one JSON line; `--out` also writes it.

    python tools/compound_bench.py [--rows 1048576] [--queries 4 64 256] [-k 10] [--format bf16] [--reps 15] [--warmup 3] [--out FILE]

One format per process, so that every step that uses the card runs under a time limit of its own and a failed step ends the chain:

    timeout -k 10 600 python tools/compound_bench.py --format bf16 --out bf16.json &&
    timeout -k 10 600 python tools/compound_bench.py --format e4m3 --out e4m3.json &&
    timeout -k 10 600 python tools/compound_bench.py --format f32 --rows 524288 --out f32.json

`ops.compound_topk` over n queries of 32 terms each (roles: 8 clauses of 3 alternatives, 8 banned terms, a veto that about half the
videos meet) against `ops.sequence_topk` over n sequences of 32 steps -- the same 32-column groups, the same index (seeded random
unit rows, videos of 60 .. 1200 rows), the same splits, the same loads and MFMAs; only the epilogue differs.  The three routines
alternate call by call: sequence, compound, sequence AGAIN -- the two sequence columns are the same code on the same data, and their
difference is the run-to-run spread against which `compound_over_sequence` is to be read.  `*_spread` is (max - min) / median of a
routine's own repetitions.  `stream_bound_ms` is the index read once per workgroup pass (one pass per four queries) at the
6.29 TB/s streaming read measured on this part, `*_of_stream` that bound over the time: a share of a bound, not a bandwidth -- the
passes of one launch share the caches."""
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
ROW_BYTES = {"bf16": 1024, "e4m3": 516, "f32": 2048}
ROLES = [j // 3 for j in range(24)] + [-1] * 8                      # 8 clauses of 3 alternatives, then 8 banned terms


def unit_rows(n, seed):
    x = torch.randn(n, 512, generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda")
    return x / x.norm(dim=-1, keepdim=True)


def stored(fmt, n, seed0):
    """n seeded unit rows in the format: (rows, scale or None)"""
    dt = {"bf16": torch.bfloat16, "f32": torch.float32, "e4m3": torch.uint8}[fmt]
    rows = torch.empty(n, 512, dtype=dt, device="cuda")
    scale = torch.empty(n, device="cuda") if fmt == "e4m3" else None
    for i, c0 in enumerate(range(0, n, SLICE)):
        x = unit_rows(min(SLICE, n - c0), seed0 + i)
        if fmt == "e4m3":
            ops.quantize_rows_e4m3(x, rows[c0:c0 + SLICE], scale[c0:c0 + SLICE])
        else:
            rows[c0:c0 + SLICE] = x.to(dt)
    return rows, scale


def timed_round(fns, warmup, reps):
    """Per routine (median ms, (max - min) / median), the routines alternating call by call (A B C A B C ...)"""
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
    return [(float(np.median(x)), float((max(x) - min(x)) / np.median(x))) for x in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2 ** 20)
    ap.add_argument("--queries", type=int, nargs="+", default=[4, 64, 256])
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--format", choices=sorted(ROW_BYTES), default="bf16")
    ap.add_argument("--splits", type=int, default=0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, k, fmt = a.rows, a.k, a.format
    lens = np.random.default_rng(0).integers(60, 1201, N // 60 + 1)
    v_off = np.minimum(np.concatenate([[0], np.cumsum(lens)]), N)
    v_off = v_off[:int(np.argmax(v_off == N)) + 1]
    nv = len(v_off) - 1
    v_dev = torch.from_numpy(v_off.astype(np.int32)).cuda()
    vn, v_scale = stored(fmt, N, 0)
    table = []
    for n in a.queries:
        tq, q_scale = stored(fmt, 32 * n, 1 << 20)
        kw = dict(q_scale=q_scale, v_scale=v_scale) if fmt == "e4m3" else {}
        t_off = torch.arange(0, 32 * n + 1, 32, dtype=torch.int32, device="cuda")
        role = torch.tensor(ROLES * n, dtype=torch.int32, device="cuda")
        ws = torch.empty(max(ops.sequence_topk_ws_bytes(n, N, k), ops.compound_topk_ws_bytes(n, N, k)), dtype=torch.uint8, device="cuda")
        outs = [(torch.empty(n, k, device="cuda"), torch.empty(n, k, dtype=torch.int32, device="cuda")) for _ in range(3)]
        # the veto: the median over videos of the first query's largest banned peak, so that about half the videos are candidates
        hits = torch.stack((torch.zeros(nv, dtype=torch.int32, device="cuda"), torch.arange(nv, dtype=torch.int32, device="cuda")), 1)
        veto = float(ops.compound_peaks(tq, vn, t_off, v_dev, hits.contiguous(), **kw)[0][:, 24:].amax(1).median())
        seq = lambda o: ops.sequence_topk(tq, vn, t_off, v_dev, k, splits=a.splits, out=outs[o], ws=ws, **kw)           # noqa: E731
        cmp_ = lambda: ops.compound_topk(tq, vn, t_off, role, v_dev, k, veto=veto, splits=a.splits, out=outs[1], ws=ws, **kw)   # noqa: E731
        (t_s, sp_s), (t_c, sp_c), (t_s2, sp_s2) = timed_round((lambda: seq(0), cmp_, lambda: seq(2)), a.warmup, a.reps)
        assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])
        kept = int((outs[1][1] != 0x7fffffff).sum())
        bound = (n + 3) // 4 * N * ROW_BYTES[fmt] / (STREAM_TBS * 1e12) * 1e3
        table.append({"queries": n, "terms": 32, "k": k, "sequence_ms": round(t_s, 4), "compound_ms": round(t_c, 4),
                      "sequence_again_ms": round(t_s2, 4), "sequence_spread": round(sp_s, 4), "compound_spread": round(sp_c, 4),
                      "sequence_again_spread": round(sp_s2, 4), "run_to_run": round(abs(t_s - t_s2) / t_s, 4),
                      "compound_over_sequence": round(t_c / t_s, 4), "passes": (n + 3) // 4, "stream_bound_ms": round(bound, 4),
                      "sequence_of_stream": round(bound / t_s, 3), "compound_of_stream": round(bound / t_c, 3),
                      "veto": veto, "list_slots_filled": kept, "list_slots": n * k})
        print(json.dumps(table[-1]), file=sys.stderr, flush=True)
    result = {"bench": "compound", "format": fmt, "rows": N, "videos": nv, "splits": a.splits, "device": torch.cuda.get_device_name(0),
              "reps": a.reps, "warmup": a.warmup, "table": table}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
