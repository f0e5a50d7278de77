"""Corpus auto-alignment throughput: `infer_align.align_corpus` against the per-video evaluation path (`test_alignment_htm` +
`make_batched_sim_fn`, every sentence a candidate), same model, same synthetic corpus, one process, ABBA order, device-synchronised
wall clocks.  Prints one JSON line.

    python tools/infer_align_bench.py [--videos 256] [--reps 2] [--only corpus] [--decode monotonic|segments]

Corpus: seeded, vlen uniform in [120, 900] s, one sentence per ~8 s, [vlen, 1024] f16 features, random [K, 512] sentence embeddings
(looked up, so neither path pays for a language model).  Model: E6D6, bf16, alignability head, random weights.
`--only corpus` runs align_corpus alone (for a `rocprofv3 --kernel-trace --stats` run of its own).
`--decode monotonic` measures instead what the order-preserving decode costs: align_corpus with it against align_corpus without,
ABBA in one process (with `--only corpus`: align_corpus with the decode alone).
`--decode segments` measures the segmental decode against both yardsticks in one process: align_corpus plain, with the monotonic decode
and with the segmental one, in alternating order (A B C C B A), medians; and the two decode launches alone over the corpus's own chunk
tables (random stitched rows, every row kept, bias = row maximum - 1), alternating, device events, median per chunk.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from temporalalignnet_amd.eval_align import make_batched_sim_fn, plan_windows, test_alignment_htm  # noqa: E402
from temporalalignnet_amd.infer_align import align_corpus  # noqa: E402
from temporalalignnet_amd.train import build_model, default_args  # noqa: E402


def corpus(n, seed=0):
    rng = np.random.default_rng(seed)
    vids = []
    for i in range(n):
        vlen = int(rng.integers(120, 901))
        K = max(1, int(round(vlen / 8)))
        mid = np.sort(rng.uniform(0, vlen, K))
        dur = rng.uniform(1, 8, K)
        vids.append({"vid": f"v{i:04d}", "video": (np.abs(rng.standard_normal((vlen, 1024))) * 0.3).astype(np.float16),
                     "start": np.clip(mid - dur / 2, 0, None), "end": np.minimum(mid + dur / 2, vlen),
                     "aligned": np.zeros(K, np.int64), "str": [f"v{i}s{k}" for k in range(K)]})
    return vids


def decode_launch_us(vids, windows_per_pass, reps=20):
    """The two decode launches alone over the chunk tables align_corpus builds for `vids` (random stitched rows, every row kept):
    per chunk the median device-event time in microseconds, the two kernels alternating."""
    from temporalalignnet_amd import ops
    from temporalalignnet_amd.infer_align import JOINT_MAX_LEN, _chunks
    out = []
    for ch in _chunks(vids, 64, windows_per_pass, None, (JOINT_MAX_LEN[torch.bfloat16] - 64) // 8 * 8, None, ordered=True):
        sim = torch.randn(ch.n_acc, device="cuda") * 5
        rows, order, vtab = ch.rows.cuda(), ch.order.cuda(), ch.vtab.cuda()
        bias = torch.cat([sim[ch.a_off[i]:ch.a_off[i + 1]].view(-1, it["vlen"]).max(-1).values for i, it in enumerate(ch.items)]) - 1.0
        bp = torch.empty(2 * ch.n_acc, dtype=torch.int32, device="cuda")
        run, path = torch.empty(int(ch.v_off[-1]), device="cuda"), torch.empty(len(ch.items), device="cuda")
        ts, seg = (torch.empty(s, dtype=torch.int32, device="cuda") for s in ((ch.n_rows,), (ch.n_rows, 2)))
        fns = {"monotonic": lambda: ops.monotonic_decode(sim, rows, order, vtab, None, bp[:ch.n_acc], run, ts, path),
               "segments": lambda: ops.segment_decode(sim, rows, order, vtab, None, bias, bp, run, seg, path)}
        us = {k: [] for k in fns}
        for r in range(reps + 2):              # the first two rounds warm up
            for k in sorted(fns, reverse=bool(r % 2)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fns[k]()
                e1.record()
                e1.synchronize()
                if r >= 2:
                    us[k].append(e0.elapsed_time(e1) * 1e3)
        out.append({"videos": len(ch.items), "sentences": ch.n_rows, "longest_vlen": int(max(it["vlen"] for it in ch.items)),
                    **{k: round(float(np.median(v)), 1) for k, v in us.items()}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=256)
    ap.add_argument("--reps", type=int, default=2, help="ABBA blocks")
    ap.add_argument("--windows-per-pass", type=int, default=256)
    ap.add_argument("--only", choices=("corpus",), default=None)
    ap.add_argument("--decode", choices=("argmax", "monotonic", "segments"), default="argmax")
    a = ap.parse_args()
    decode = None if a.decode == "argmax" else a.decode
    torch.manual_seed(0)
    model = build_model(default_args(model="init", num_encoder_layers=6, num_decoder_layers=6, use_alignability_head=1),
                        compute_dtype="bf16", random_pos_start=0).cuda().eval()
    vids = corpus(a.videos)
    names = {s: j for j, s in enumerate(s for v in vids for s in v["str"])}
    table = torch.randn(len(names), 512, device="cuda")
    embed = lambda strs: table[torch.tensor([names[s] for s in strs], device="cuda")]      # noqa: E731
    n_win = sum(len(plan_windows(v["start"], v["end"], len(v["video"]))) for v in vids)

    def run_corpus():
        for _ in align_corpus(model, vids, embed, windows_per_pass=a.windows_per_pass, decode=decode):
            pass

    def run_argmax():
        for _ in align_corpus(model, vids, embed, windows_per_pass=a.windows_per_pass):
            pass

    def run_per_video():
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            test_alignment_htm(None, vids, return_per_video=True, batched_sim=make_batched_sim_fn(model, embed))

    def run_monotonic():
        for _ in align_corpus(model, vids, embed, windows_per_pass=a.windows_per_pass, decode="monotonic"):
            pass

    other = "per_video" if decode is None else "argmax"             # what `corpus` is measured against
    paths = {"corpus": run_corpus} if a.only else {"corpus": run_corpus, other: run_per_video if decode is None else run_argmax}
    order = ["corpus"] if a.only else ["corpus", other, other, "corpus"]
    if decode == "segments" and not a.only:    # both yardsticks in the same run
        paths["monotonic"] = run_monotonic
        order = ["argmax", "monotonic", "corpus", "corpus", "monotonic", "argmax"]
    for f in paths.values():                   # warm-up: code objects, workspaces of every pass shape
        f()
    times = {k: [] for k in paths}
    for _ in range(a.reps):
        for k in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            paths[k]()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    out = {"videos": len(vids), "windows": n_win, "sentences": len(names), "windows_per_pass": a.windows_per_pass,
           "model": "E6D6 bf16 head", "decode": a.decode, "gpu": torch.cuda.get_device_name(0)}
    for k, ts in times.items():
        best, med = min(ts), float(np.median(ts))
        out[k] = {"s": [round(t, 4) for t in ts], "videos_per_s": round(len(vids) / med, 2), "windows_per_s": round(n_win / med, 1)}
    if "per_video" in out:
        out["speedup_median"] = round(float(np.median(times["per_video"]) / np.median(times["corpus"])), 2)
    if "argmax" in out:
        out["decode_cost_median"] = round(float(np.median(times["corpus"]) / np.median(times["argmax"])), 4)
    if "monotonic" in out:
        out["monotonic_cost_median"] = round(float(np.median(times["monotonic"]) / np.median(times["argmax"])), 4)
    if decode == "segments" and not a.only:    # (a run to trace holds align_corpus's own launches only)
        per_chunk = decode_launch_us(vids, a.windows_per_pass)
        tot = {k: sum(c[k] for c in per_chunk) for k in ("monotonic", "segments")}
        out["decode_launch_us_per_chunk"] = per_chunk
        out["segments_over_monotonic_launch"] = round(tot["segments"] / tot["monotonic"], 3)
        if "argmax" in out:                    # the launch against everything the plain path does for the same chunks, host time included
            out["segments_launch_share_of_plain_wall"] = round(tot["segments"] * 1e-6 / float(np.median(times["argmax"])), 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
