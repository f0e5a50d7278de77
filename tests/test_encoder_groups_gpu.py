"""tan_encoder_fwd in two video groups (tan_encoder_desc.fwd_group_stream / fwd_group_videos, csrc/tan_encoder.hip): videos [0, g) on
the call's stream, videos [g, B) -- the same launches with every per-row / per-video pointer advanced -- on a second stream, forked
from and joined to the call's stream inside the call.  The stack's forward is row-local per video (one attention workgroup per video,
one MLP workgroup per 64-row panel), so the grouped call is compared BIT FOR BIT with the ungrouped call of the same build: every
block's x_out, the post-LN output and every saved tensor.  There is no tolerance in this file except the whole step's gradients,
whose f32 atomics land in another order from run to run (the bound of test_train_options_gpu's two-chain test).

The stack is tests/test_encoder_stack_gpu.py's: 2 layers, C = 512, H = 8, bf16, seeded, NaN-filled outputs, padded keys in both groups.
Shapes of 8 ... 15 row panels are inside the split-hidden range of the defaults; the grouped cases pass no split scratch, which selects
the whole-panel launches (what a stack of more than 48 panels runs).

  B, L, g      rows per group   what
  8, 64, 4     256 / 256        attnblk<4>, equal groups
  8, 80, 4     320 / 320        attnblk<5>, five panels per group
  12, 80, 4    320 / 640        unequal groups
  8, 64, 4     no_save          outputs equal, the backward-only buffers keep their fill
  fall back:   6, 80, 3 (240 rows: not whole panels); g = 0; g = B; 2, 256, 1 (streamed attention); 8, 64, 4 with the split scratch
  8, 64, 4     20 calls back to back, two inputs in turn, no host synchronisation: the fork and the join order the groups
  whole step   Trainer.step, stage 1, B = 8, T = 64, N = 16: `fwd_groups` True against False
"""
import ctypes as C

import numpy as np
import pytest
import torch

from temporalalignnet_amd import _lib, synth
from test_encoder_stack_gpu import BF16, bits, make_run

pytestmark = pytest.mark.gpu

SAVED = ("xn1", "mean1", "rstd1", "qkv", "attn_o", "lse", "x_mid", "xn2", "mean2", "rstd2", "h_pre", "h_act", "x_out")
BACKWARD_ONLY = ("xn2", "mean2", "rstd2", "h_pre", "h_act", "qkv", "attn_o", "lse")       # what no_save leaves unwritten on this path


def _mask(B, L):
    """padded keys in the first and the last video: one in each group"""
    m = torch.zeros(B, L, dtype=torch.uint8, device="cuda")
    m[0, L - 5:] = 1
    m[B - 1, L - max(1, L // 4):] = 1
    return m


def _run(B, L, split_scratch=False, no_save=False):
    run = make_run(B, L, 2, BF16, None)
    run.set_mask(_mask(B, L))
    if not split_scratch:           # the whole-panel launches, as for a stack past the split-hidden range
        run.split_part = None
        run.d.split_part = None
    run.d.no_save = 1 if no_save else 0
    return run


def _group(run, g, stream):
    run.d.fwd_group_stream, run.d.fwd_group_videos = C.c_void_p(stream.cuda_stream), g
    return run


def _tensors(run):
    out = {f"{i}.{k}": run.buf[i][k] for i in range(run.S) for k in SAVED}
    out |= {"post_out": run.post_out, "post_mean": run.post_mean, "post_rstd": run.post_rstd}
    return out


def _assert_same(got, want):
    """every output and saved tensor, bit for bit (NaN fill included)"""
    got = _tensors(got)
    for k, w in _tensors(want).items():
        assert torch.equal(bits(got[k]), bits(w)), k


PROF_PANEL, PROF_ATTNBLK, PROF_NKINDS = 11, 12, 13          # include/tan_hip.h


def _counted_fwd(run):
    """run.fwd() under the library's launch counter: (row-panel MLP launches, fused attention-branch launches) of the call"""
    L = _lib.lib()
    _lib.check(L.tan_prof_enable(1, 64), "tan_prof_enable")
    try:
        run.fwd()
        torch.cuda.synchronize()
        work, cnt = (C.c_double * PROF_NKINDS)(), (C.c_long * PROF_NKINDS)()
        L.tan_prof_collect_all(work, cnt, PROF_NKINDS)
    finally:
        L.tan_prof_enable(0, 0)
    return cnt[PROF_PANEL], cnt[PROF_ATTNBLK]


def _pair(B, L, g, **kw):
    """(ungrouped run, grouped run) after their forward, synchronised, and each call's launch counts"""
    side = torch.cuda.Stream()
    base = _run(B, L, **kw)
    n_base = _counted_fwd(base)
    run = _group(_run(B, L, **kw), g, side)
    n_run = _counted_fwd(run)
    return base, run, n_base, n_run


@pytest.mark.parametrize("B,L,g", [(8, 64, 4), (8, 80, 4), (12, 80, 4)])
def test_grouped_forward_is_bitwise_the_ungrouped_forward(B, L, g):
    base, run, n_base, n_run = _pair(B, L, g)
    # the grouped call really ran in two groups: every launch of the two layers twice
    assert n_base == (2, 2) and n_run == (4, 4), (n_base, n_run)
    _assert_same(run, base)
    # everything a backward reads was written, in both groups' rows (block 0's ln_1 output included: no xn1_ready here)
    for k, t in _tensors(run).items():
        assert torch.isfinite(t.float()).all(), k


def test_grouped_no_save_forward_leaves_the_backward_only_buffers_alone():
    base, run, n_base, n_run = _pair(8, 64, 4, no_save=True)
    assert n_base == (2, 2) and n_run == (4, 4), (n_base, n_run)
    _assert_same(run, base)
    for i in range(run.S):
        for k in BACKWARD_ONLY:
            assert torch.isnan(run.buf[i][k].float()).all(), (i, k)          # the sentinel fill
        for k in ("x_mid", "x_out"):
            assert torch.isfinite(run.buf[i][k].float()).all(), (i, k)
    saving = _run(8, 64)
    saving.fwd()
    torch.cuda.synchronize()
    for i in range(run.S):
        assert torch.equal(bits(run.buf[i]["x_out"]), bits(saving.buf[i]["x_out"])), i
    assert torch.equal(bits(run.post_out), bits(saving.post_out))


FALLBACK = {  # name -> (B, L, g, run keywords)
    "rows_not_whole_panels": (6, 80, 3, {}),
    "g_zero": (8, 64, 0, {}),
    "g_all": (8, 64, 8, {}),
    "streamed_attention_L256": (2, 256, 1, {}),
    "split_hidden": (8, 64, 4, {"split_scratch": True}),
}


@pytest.mark.parametrize("name", list(FALLBACK))
def test_ineligible_shapes_take_the_ungrouped_path(name):
    B, L, g, kw = FALLBACK[name]
    side = torch.cuda.Stream()
    base = _run(B, L, **kw)
    n_base = _counted_fwd(base)
    run = _group(_run(B, L, **kw), g, side)
    before = side.record_event()
    run.fwd()
    assert before.query()               # complete as soon as the call returns ...
    assert side.query()                 # ... and nothing was queued behind it: the second stream received no work
    torch.cuda.synchronize()
    _assert_same(run, base)
    assert _counted_fwd(run) == n_base  # launch for launch the ungrouped call
    _assert_same(run, base)


def test_fork_and_join_order_back_to_back_calls():
    """20 calls on one descriptor, two inputs in turn: each input is written on the call's stream right before the call and the
    outputs are copied out on it right after, with no host synchronisation in between.  A missing fork wait lets group 1 read the
    previous input (or overwrite rows the previous copy still reads); a missing join lets the copy read group 1's rows too early."""
    B, L, g = 8, 64, 4
    inputs, want = [], []
    for seed in (1, 2):
        base = _run(B, L)
        gen = torch.Generator(device="cuda").manual_seed(seed)
        base.x0.copy_(torch.randn(B * L, 512, generator=gen, device="cuda").to(BF16))
        base.fwd()
        torch.cuda.synchronize()
        inputs.append(base.x0.clone())
        want.append((base.post_out.clone(), base.buf[1]["x_out"].clone(), base.buf[0]["qkv"].clone()))
    side = torch.cuda.Stream()
    run = _group(_run(B, L), g, side)
    got = []
    for n in range(20):
        run.x0.copy_(inputs[n & 1])
        run.fwd()
        got.append((run.post_out.clone(), run.buf[1]["x_out"].clone(), run.buf[0]["qkv"].clone()))
    torch.cuda.synchronize()
    assert not torch.equal(bits(want[0][0]), bits(want[1][0]))
    for n, outs in enumerate(got):
        for j, (a, b) in enumerate(zip(outs, want[n & 1])):
            assert torch.equal(bits(a), bits(b)), (n, j)


def test_whole_step_with_grouped_forwards_matches_the_ungrouped_step(monkeypatch):
    """`Trainer.step`, stage 1, bf16, B = 8, T = 64, N = 16 (joint L = 80), three steps on three batches with `fwd_groups` True
    against False.  The split-hidden range is switched off for both (no split scratch: the whole-panel launches, the only ones that
    run in groups).  Learning rate 0, as in bench.py's result dumps: the parameters stay what they are, so every step's forward sees
    the same bits in both runs and the loss dictionaries are equal bit for bit on all three steps; the backward is unchanged, and
    its gradients differ by the order of their f32 atomics (test_train_options_gpu.test_two_chain_step_matches_the_autograd_step's
    bound: 2e-3 of the norm over all gradients, 2e-2 per parameter)."""
    from temporalalignnet_amd import workspace
    from temporalalignnet_amd.train import Trainer, build_model, default_args, to_device_batch
    monkeypatch.setattr(workspace, "SPLIT_PANELS", 0)
    # 9 ... 16 sentences per video: `Trainer.step` pads the sentence slots to N = 16 (8 * (64 + N) rows in whole panels), joint L = 80
    batches = [to_device_batch(synth.make_batch(90 + i, B=8, T=64, n_min=9, n_max=16)) for i in range(3)]
    assert all(Trainer._pad_sentence_slots(b)["text_embed"].shape[1] == 16 for b in batches)
    outs = {}
    for on in (False, True):
        args = default_args(model="init", num_encoder_layers=2, num_decoder_layers=3, lr=0.0, wd=1e-2)
        torch.manual_seed(11)
        model = build_model(args, compute_dtype="bf16", random_pos_start=0).cuda()
        tr = Trainer(model, args, iter_per_epoch=50, warmup=5)
        tr.online.fwd_groups = on
        assert tr.online._fwd_group_videos(8, 64) == (4 if on else 0) and tr.online._fwd_group_videos(8, 80) == (4 if on else 0)
        assert tr._will_chain(batches[0])
        np.random.seed(3)
        steps = []
        for b in batches:
            ld = tr.step(b)
            torch.cuda.synchronize()
            steps.append(({k: torch.as_tensor(v).detach().clone() for k, v in ld.items()}, tr.online.flat_grad().clone()))
        outs[on] = (steps, tr.online._flat)
    f = outs[True][1]
    for n, ((l0, g0), (l1, g1)) in enumerate(zip(outs[False][0], outs[True][0])):
        assert l0.keys() == l1.keys()
        for k in l0:
            assert torch.isfinite(l0[k]).all() and torch.equal(l0[k], l1[k]), (n, k, l0[k], l1[k])
        assert torch.isfinite(g1).all() and g0.abs().max() > 0
        assert (g1 - g0).norm() <= 2e-3 * g0.norm(), (n, float((g1 - g0).norm() / g0.norm()))
        for name in f.names:
            o, k, _ = f.off[name]
            a, c = g1[o:o + k], g0[o:o + k]
            assert (a - c).norm() <= 2e-2 * c.norm() + 1e-7, (n, name, float((a - c).norm()), float(c.norm()))
