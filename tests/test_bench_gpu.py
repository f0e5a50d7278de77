"""bench.py's plain run: the headline line without anything `--full` measures, and `--dump-outputs` -- what the last timed step computed,
the same from run to run with the same arguments: the step runs at learning rate 0, so every step computes from the same parameters
and batch, and two runs differ only by the rounding of one step's f32 gradient atomics (parameters bit-identical, the loss to 1e-5, the
gradients within bf16 rounding)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _bench(out_dir, *extra):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("TAN_DDP_MODE", "TAN_FORCE_DIST", "RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out_dir), *extra], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    names = sorted(os.listdir(out_dir))
    return json.loads(lines[0]), {n: np.load(os.path.join(out_dir, n)) for n in names}


def test_plain_run_line_and_dumped_outputs(tmp_path):
    d, a = _bench(tmp_path / "bf16")
    assert d["steps"] == 3 and d["warmup"] == 2 and d["settle_steps"] == 0 and d["n_gpus"] == 1
    assert d["unit"] == "video-seq/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["metric"].startswith("video-seq/sec") and d["value"] > 0
    assert abs(d["value"] - 128 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    assert d["roofline"] is None and "extra" not in d and "cpu_baseline" not in d and "comm" not in d
    assert {"loss.npy", "loss-dual.npy", "loss-joint.npy", "params_sample.npy", "grads_sample.npy"} <= set(a), sorted(a)
    assert sum(os.path.getsize(tmp_path / "bf16" / n) for n in a) <= 64 << 20
    for n, v in a.items():
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all(), n
    assert abs(float(a["loss.npy"]) - d["config"]["final_loss"]) <= 1e-3 * max(1.0, abs(d["config"]["final_loss"]))
    assert a["params_sample.npy"].size > 1_000_000 and np.abs(a["grads_sample.npy"]).max() > 0


def test_same_arguments_dump_the_same_outputs(tmp_path):
    _, a = _bench(tmp_path / "a", "--steps", "12")
    _, b = _bench(tmp_path / "b", "--steps", "12")
    assert sorted(a) == sorted(b)
    for n in a:
        assert a[n].shape == b[n].shape, n
        if not n.endswith("_sample.npy"):
            assert np.allclose(a[n], b[n], rtol=1e-5, atol=1e-6), (n, a[n], b[n])
    assert np.array_equal(a["params_sample.npy"], b["params_sample.npy"])          # (lr = 0: the parameters never move)
    ga, gb = a["grads_sample.npy"].astype(np.float64), b["grads_sample.npy"].astype(np.float64)
    # the gradients pass through bf16 activation gradients: a different f32 atomics order moves some of those by one bf16 ulp, so the
    # bound is the bf16 unit roundoff, 2^-8, norm-relative (measured: 6e-4)
    assert np.linalg.norm(ga - gb) <= 2.0 ** -8 * np.linalg.norm(ga), np.linalg.norm(ga - gb) / np.linalg.norm(ga)
