"""Step time of the headline configuration (E6D6, len 64, bf16, B = 128, stage 1) with per-parameter gradient clipping:
    fused  clip_grad = 3.0, TAN_CLIP_FUSED=1   two launches per group over the flat gradient, early optimizer launches kept
    loop   clip_grad = 3.0, TAN_CLIP_FUSED=0   the torch rule, tensor by tensor (what the step did before csrc/tan_clip.hip)
    none   clip_grad = 0
Every measurement is a FRESH child process (the tools/fresh_steps.py idiom: step-boundary events on the main stream, no host
synchronisation inside the loop), the arms interleaved fused-loop-none-none-loop-fused per round, each child under its own time limit.

    python tools/clip_step_time.py [--rounds 2] [--steps 60] [--warmup 20] [--clip 3.0] [--timeout 240]

Prints one JSON line: per arm the children's median step times [ms] (GPU events; wall = timed window / steps, which is what a
host-bound step costs), their median and spread (max - min over children), and the two ratios the fused clip is judged by."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = {"fused": ("1", None), "loop": ("0", None), "none": ("1", 0.0)}


def child(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from temporalalignnet_amd import synth
    from temporalalignnet_amd.train import Trainer, build_model, default_args, to_device_batch
    dev = torch.device("cuda", 0)
    args_ns = default_args(model="init", num_encoder_layers=6, num_decoder_layers=6, loss_threshold=0.0, seq_len=64, clip_grad=a.clip)
    torch.manual_seed(888)
    model = build_model(args_ns, compute_dtype="bf16", language_model=None).to(dev)
    model.random_pos_start = 1
    tr = Trainer(model, args_ns, iter_per_epoch=2890, warmup=1000)
    tr.batches_seen = tr.iteration = 1000
    batch = to_device_batch(synth.make_batch(888, B=128, T=64, n_min=4, n_max=16), device=dev)
    for _ in range(a.warmup):
        tr.step(batch)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    t0 = time.perf_counter()
    for i in range(a.steps):
        ev[i].record()
        tr.step(batch)
    ev[a.steps].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / a.steps
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(a.steps)]
    out = {"gpu_ms": round(float(np.median(ms)), 4), "wall_ms": round(wall, 4), "chains": bool(tr._last_step_chains)}
    norms = tr.last_grad_norms()
    if norms is not None:                            # how many tensors the last step clipped
        v = torch.stack(list(norms.values()))
        out["clipped"], out["tensors"] = int((v > a.clip).sum()), v.numel()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--clip", type=float, default=3.0)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = {k: [] for k in ARMS}
    for _ in range(a.rounds):
        for arm in ("fused", "loop", "none", "none", "loop", "fused"):
            fused, clip = ARMS[arm]
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup),
                   "--clip", str(a.clip if clip is None else clip)]
            r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TAN_CLIP_FUSED=fused), timeout=a.timeout)
            line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
            if r.returncode != 0 or line is None:            # (a failed child ends the measurement: nothing more is started)
                sys.stderr.write(r.stderr[-3000:])
                raise SystemExit(f"{arm}: child failed with code {r.returncode}")
            runs[arm].append(json.loads(line[7:]))
            print(arm, runs[arm][-1], flush=True)
    out = {"config": "E6D6 len64 bf16 B128 stage1", "clip_grad": a.clip, "steps": a.steps, "warmup": a.warmup}
    for arm, rs in runs.items():
        out[arm] = {}
        for key in ("gpu_ms", "wall_ms"):
            v = sorted(r[key] for r in rs)
            out[arm][key] = {"runs": v, "median": round((v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, 4), "spread": round(v[-1] - v[0], 4)}
        out[arm]["chains"] = all(r["chains"] for r in rs)
        if "clipped" in rs[-1]:
            out[arm]["clipped_tensors"] = [rs[-1]["clipped"], rs[-1]["tensors"]]
    med = lambda arm: out[arm]["wall_ms"]["median"]              # noqa: E731
    out["fused_over_loop"] = round(med("fused") / med("loop"), 4)
    out["fused_over_none"] = round(med("fused") / med("none"), 4)
    out["loop_minus_fused_ms"] = round(med("loop") - med("fused"), 4)
    out["spread_ms"] = max(out[arm]["wall_ms"]["spread"] for arm in ARMS)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
