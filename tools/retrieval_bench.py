"""Zero-shot retrieval throughput: `eval_retrieval.test_retrieval_batched` against the per-clip `test_retrieval`, and `tan_rank_topk`
against `torch.matmul` + `torch.topk` over index chunks sized to 1 GB of scores.  One process, ABBA order, device-synchronised wall
clocks.  Prints one JSON line.

    python tools/retrieval_bench.py [--clips 3000] [--reps 2] [--only harness|sweep|sweep-large]

Clips: seeded, 64 videos of 200-900 s with [vlen, 1024] f32 features, segments of 3-200 s, random [n, 512] sentence embeddings
(looked up, so neither path pays for a language model).  Model: E6D6, bf16, random weights.  Sweep shapes: Q = N = 3 000 f32 with
pairs (the metrics' shape) and Q = 2 048, N = 2 M, k = 10 bf16 (corpus search); FLOP = 2 * Q * N * 512, peak = the bf16 dense MFMA
rate (2.5 PFLOP/s).  `--only sweep-large` runs the large sweep alone (for a `rocprofv3 --kernel-trace --stats` run of its own).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from temporalalignnet_amd import eval_retrieval, ops  # noqa: E402
from temporalalignnet_amd.train import build_model, default_args  # noqa: E402

BF16_PEAK = 2.5e15


def make_clips(n, seed=0):
    rng = np.random.default_rng(seed)
    vids = [(np.abs(rng.standard_normal((int(v), 1024))) * 0.3).astype(np.float32) for v in rng.integers(200, 901, 64)]
    clips = []
    for i in range(n):
        f = vids[i % len(vids)]
        s = int(rng.integers(0, f.shape[0] - 6))
        e = int(min(f.shape[0] - 1, s + rng.integers(3, 200)))
        clips.append({"feature": f, "start": s, "end": max(e, s + 2), "str": f"c{i}"})
    return clips


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def abba(paths, reps):
    for f in paths.values():                   # warm-up: code objects, workspaces, allocator
        f()
    names = list(paths)
    order = names if len(names) == 1 else [names[0], names[1], names[1], names[0]]
    times = {k: [] for k in names}
    for _ in range(reps):
        for k in order:
            times[k].append(timed(paths[k]))
    return times


def chunked_topk(tq, vn, k, pair=None):
    """The baseline on the same device: scores chunk by chunk (1 GB of f32 each), top-k per chunk, merged; counts per chunk."""
    Q, N = tq.shape[0], vn.shape[0]
    step = max(1, (1 << 30) // (4 * Q))
    best_s = best_r = None
    hi = torch.zeros(Q, dtype=torch.int64, device=tq.device)
    d = (tq.float() * vn[pair.long()].float()).sum(-1, keepdim=True) if pair is not None else None
    for a in range(0, N, step):
        s = torch.matmul(tq, vn[a:a + step].T).float()
        if d is not None:
            hi += (s > d).sum(1)
        if k:
            ts, tr = torch.topk(s, min(k, s.shape[1]), dim=1)
            tr = tr + a
            if best_s is not None:
                ts, j = torch.topk(torch.cat([best_s, ts], 1), k, dim=1)
                tr = torch.cat([best_r, tr], 1).gather(1, j)
            best_s, best_r = ts, tr
    return hi, best_s, best_r


def sweep_case(Q, N, k, dtype, with_pair, reps, alone=False):
    g = torch.Generator(device="cuda").manual_seed(1)
    vn = torch.empty(N, 512, dtype=dtype, device="cuda")
    for a in range(0, N, 250_000):
        x = torch.randn(min(250_000, N - a), 512, generator=g, device="cuda")
        vn[a:a + 250_000] = (x / x.norm(dim=-1, keepdim=True)).to(dtype)
    tq = torch.randn(Q, 512, generator=g, device="cuda")
    tq = (tq / tq.norm(dim=-1, keepdim=True)).to(dtype)
    pair = (torch.arange(Q, device="cuda") % N).int() if with_pair else None
    ws = torch.empty(ops.rank_topk_ws_bytes(Q, N, k), dtype=torch.uint8, device="cuda")
    paths = {"sweep": lambda: ops.rank_topk(tq, vn, pair, k, ws=ws)}
    if not alone:
        paths["chunked"] = lambda: chunked_topk(tq, vn, k, pair)
    times = abba(paths, reps)
    flop = 2.0 * Q * N * 512
    out = {"Q": Q, "N": N, "k": k, "dtype": str(dtype).replace("torch.", ""), "pair": with_pair}
    for name, ts in times.items():
        med = float(np.median(ts))
        out[name] = {"ms": [round(t * 1e3, 3) for t in ts], "tflops": round(flop / med / 1e12, 1), "of_bf16_peak": round(flop / med / BF16_PEAK, 4)}
    if not alone:
        out["chunked_over_sweep"] = round(float(np.median(times["chunked"]) / np.median(times["sweep"])), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=2, help="ABBA blocks")
    ap.add_argument("--only", choices=("harness", "sweep", "sweep-large"), default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    out = {"gpu": torch.cuda.get_device_name(0)}
    if a.only in (None, "harness"):
        model = build_model(default_args(model="init", num_encoder_layers=6, num_decoder_layers=6), compute_dtype="bf16",
                            random_pos_start=0).cuda().eval()
        clips = make_clips(a.clips)
        names = {c["str"]: i for i, c in enumerate(clips)}
        table = torch.randn(len(clips), 512, device="cuda")
        embed = lambda strs: table[torch.tensor([names[s] for s in strs], device="cuda")]      # noqa: E731
        times = abba({"batched": lambda: eval_retrieval.test_retrieval_batched(clips, model, embed),
                      "per_clip": lambda: eval_retrieval.test_retrieval(clips, model.get_visual_feature, model.get_textual_feature, embed)},
                     a.reps)
        out["harness"] = {"clips": len(clips), "model": "E6D6 bf16"}
        for k, ts in times.items():
            out["harness"][k] = {"s": [round(t, 4) for t in ts], "clips_per_s": round(len(clips) / float(np.median(ts)), 1)}
        out["harness"]["speedup_median"] = round(float(np.median(times["per_clip"]) / np.median(times["batched"])), 2)
    if a.only in (None, "sweep"):
        out["sweep_metrics"] = sweep_case(3000, 3000, 0, torch.float32, True, a.reps)
    if a.only in (None, "sweep", "sweep-large"):
        out["sweep_large"] = sweep_case(2048, 2_000_000, 10, torch.bfloat16, False, a.reps, alone=a.only == "sweep-large")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
