"""The train-loop options of train/main.py:112-139,330-356 that the goldens do not exercise: per-parameter gradient clipping
(utils/train_utils.py:3-13), the 'bce' optimisation policy, gradient accumulation (backprop_freq)."""
import numpy as np
import pytest
import torch

from temporalalignnet_amd import synth

pytestmark = pytest.mark.gpu


def _trainer(seed=0, dtype="fp32", **akw):
    from temporalalignnet_amd.train import Trainer, build_model, default_args
    args = default_args(num_encoder_layers=2, num_decoder_layers=3, lr=1e-3, wd=1e-2, **akw)
    torch.manual_seed(seed)
    m = build_model(args, compute_dtype=dtype, random_pos_start=0).cuda()
    return Trainer(m, args, iter_per_epoch=50, warmup=5), args


def _batch(seed, B=4, T=16):
    from temporalalignnet_amd.train import to_device_batch
    return to_device_batch(synth.make_batch(seed, B=B, T=T, n_min=2, n_max=5))


def test_per_parameter_gradient_clipping_matches_the_reference_rule():
    tr, args = _trainer(model="init", clip_grad=0.05)
    tr.iteration = 7
    tr.zero_grad()
    tr.forward_backward(_batch(1))
    named = [(n, p) for n, p in tr.online.named_parameters() if p.grad is not None and p.grad.abs().max() > 0]
    before = {n: (p.detach().clone(), p.grad.detach().clone()) for n, p in named}
    assert any(g.norm() > 0.05 for _, g in before.values()) and any(g.norm() < 0.05 for _, g in before.values())
    tr.optimizer_step()
    lr = tr.current_lr()
    for n, p in named:
        w, g = before[n]
        coef = 0.05 / (g.norm(2) + 1e-6)
        g = g * coef if coef < 1 else g                                   # clip_gradients()
        wd = 0.0 if any(t in n for t in (".ln_", ".bias")) else args.wd   # optim_policy()
        ref = w.clone().requires_grad_(True)
        ref.grad = g
        opt = torch.optim.AdamW([ref], lr=lr, weight_decay=wd)
        opt.state[ref] = {"step": torch.tensor(7.0), "exp_avg": torch.zeros_like(w), "exp_avg_sq": torch.zeros_like(w)}
        opt.step()
        torch.testing.assert_close(p.detach(), ref.detach(), rtol=1e-5, atol=1e-7, msg=n)


def test_bce_policy_trains_the_alignability_head_only():
    tr, args = _trainer(model="cotrain", optim_policy="bce", loss_threshold=0.5)
    tr.iteration = 10                                   # past the warm-up: non-zero learning rate
    before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
    for s in range(2):
        tr.step(_batch(10 + s, B=6))
    # the ONLINE parameters outside the head are frozen bit for bit; the EMA twin of a frozen tensor is t*m + o*(1 - m) with t == o
    # (tan_model.py:339-344): like the reference's, separately rounded products -- it may move in the last bit, not more
    changed = {n for n, p in tr.model.named_parameters()
               if not (torch.equal(p.detach(), before[n]) if n.startswith("online.") else
                       torch.allclose(p.detach(), before[n], rtol=3e-7, atol=1e-12))}
    assert changed and all("binary_head" in n for n in changed), sorted(changed)[:5]      # online head + its EMA copy


def test_gradient_accumulation_follows_the_reference_loop():
    """backprop_freq = 2 over batches 0,1,2: step on batch 0 alone, then ONE step on the summed gradients of batches 1 and 2, with
    the learning rate of the third iteration (the schedule advances per batch, the Adam step count per optimizer step)."""
    batches = [_batch(20 + i) for i in range(3)]
    ta, _ = _trainer(model="init", backprop_freq=2)
    for i, b in enumerate(batches):
        ta.train_iteration(b, i)
    tb, _ = _trainer(model="init", backprop_freq=1)
    tb.zero_grad(); tb.forward_backward(batches[0]); tb._lr_iter = 0; tb.optimizer_step()
    tb.zero_grad(); tb.forward_backward(batches[1]); tb.forward_backward(batches[2]); tb._lr_iter = 2; tb.optimizer_step()
    assert ta.iteration == tb.iteration == 2 and ta.batches_seen == 3
    # Same arithmetic, different order of the f32 atomics that gather bias / LayerNorm gradients: Adam turns that noise, on
    # parameters whose gradient is ~0, into a fraction of one lr-sized (2e-4) update for a handful of elements -- bounded per
    # element by half an update, and invisible on average.
    diff = (ta.online.flat_parameters() - tb.online.flat_parameters()).abs()
    assert diff.max().item() <= 1e-4, diff.max().item()
    assert diff.mean().item() <= 2e-7 and (diff > 2e-5).float().mean().item() < 1e-4, (diff.mean().item(), (diff > 2e-5).float().mean().item())
    # and it differs from stepping three times
    tc, _ = _trainer(model="init", backprop_freq=1)
    for b in batches:
        tc.step(b)
    d3 = (tc.online.flat_parameters() - ta.online.flat_parameters()).abs()
    assert d3.max() > 1e-4 and d3.mean().item() > 50 * max(diff.mean().item(), 1e-9)


@pytest.mark.parametrize("model_kind", ["init", "cotrain"])
def test_step_boundary_options_do_not_change_the_arithmetic(monkeypatch, model_kind):
    """`Trainer.step` with the weight images written by the optimizer launch itself (TAN_OPT_IMAGES, default) and the fused input
    embeddings (TAN_EMBED_FUSED, default) runs the same arithmetic as AdamW + image rebuilds on the side stream / the unfused
    front-end launches: after three steps in bf16 the parameters agree up to bf16 rounding of the embeddings and the order of the
    f32 gradient atomics."""
    kw = dict(model=model_kind, **({"loss_threshold": 0.5} if model_kind == "cotrain" else {}))
    batches = [_batch(40 + i, B=8, T=64) for i in range(3)]
    flats = {}
    # (stage 1 additionally: the two-chain step with the video stack's AdamW issued under the joint stack's backward -- the defaults)
    for tag, env in (("plain", {"TAN_OPT_IMAGES": "0", "TAN_EMBED_FUSED": "0", "TAN_STEP_CHAINS": "0", "TAN_OPT_EARLY": "0"}),
                     ("images", {"TAN_OPT_IMAGES": "1", "TAN_EMBED_FUSED": "0", "TAN_STEP_CHAINS": "0", "TAN_OPT_EARLY": "0"}),
                     ("chains", {"TAN_OPT_IMAGES": "1", "TAN_EMBED_FUSED": "1", "TAN_STEP_CHAINS": "1", "TAN_OPT_EARLY": "0"}),
                     ("fused", {"TAN_OPT_IMAGES": "1", "TAN_EMBED_FUSED": "1", "TAN_STEP_CHAINS": "1", "TAN_OPT_EARLY": "1"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        tr, _ = _trainer(seed=3, dtype="bf16", **kw)
        if model_kind == "cotrain":
            tr.model._copy_param()
        tr.iteration = tr.batches_seen = 10
        for b in batches:
            tr.step(b)
        torch.cuda.synchronize()
        flats[tag] = (tr.online.flat_parameters().clone(), tr.model.target.flat_parameters().clone() if model_kind == "cotrain" else None)
    ref = flats["plain"]
    assert torch.isfinite(ref[0]).all()
    for tag in ("images", "chains", "fused"):
        d = (flats[tag][0] - ref[0]).abs()
        # Adam turns atomics-order noise on ~zero gradients into lr-sized (1e-3) updates of a few elements: a sign flip is 2 lr per step
        # (the fused front-end adds the position rows in f32 instead of bf16: rounding-level input differences on top of the atomics)
        assert d.max().item() <= 6.5e-3 and d.mean().item() <= (5e-6 if tag == "images" else 3e-5), (tag, d.max().item(), d.mean().item())
        if ref[1] is not None:
            assert (flats[tag][1] - ref[1]).abs().max().item() <= 3.5e-3, tag
    moved = (ref[0] - _trainer(seed=3, dtype="bf16", **kw)[0].online.flat_parameters()).abs().max().item()
    assert moved > 1e-3                       # (the three steps did something)


@pytest.mark.parametrize("random_pos", [0, 1])
def test_two_chain_step_matches_the_autograd_step(monkeypatch, random_pos):
    """Stage 1 in bf16: `Trainer.forward_backward` as two chains that never wait for each other (video stack + dual NCE, joint stack + joint
    NCE, each forward AND backward on its own stream: `_run_chains`) against forward -> get_loss -> loss.backward() under autograd
    (TAN_STEP_CHAINS=0): same kernels on the same values -- loss scalars equal, every parameter gradient equal up to the order of the
    f32 atomics."""
    import numpy as np
    outs = {}
    for tag, env in (("autograd", "0"), ("chains", "1")):
        monkeypatch.setenv("TAN_STEP_CHAINS", env)
        tr, _ = _trainer(seed=5, dtype="bf16", model="init")
        tr.online.random_pos_start = random_pos
        b = _batch(77, B=8, T=64)
        b["padding_mask"][2, -6:] = True
        assert tr._chains_eligible(b, tr.fused_loss) == (env == "1")
        np.random.seed(3)
        tr.zero_grad()
        ld = tr.forward_backward(b)
        torch.cuda.synchronize()
        outs[tag] = ({k: float(ld[k]) for k in ("loss", "loss-dual", "loss-joint")}, tr.online.flat_grad().clone(), tr.online._flat)
    (l0, g0, f), (l1, g1, _) = outs["autograd"], outs["chains"]
    for k in l0:
        assert abs(l0[k] - l1[k]) <= 1e-5 * max(1.0, abs(l0[k])), (k, l0[k], l1[k])
    assert torch.isfinite(g1).all() and g0.abs().max() > 0
    assert (g1 - g0).norm() <= 2e-3 * g0.norm()
    for n in f.names:
        o, k, _ = f.off[n]
        a, c = g1[o:o + k], g0[o:o + k]
        assert (a - c).norm() <= 2e-2 * c.norm() + 1e-7, (n, float((a - c).norm()), float(c.norm()))


def test_small_batch_pads_sentence_slots_to_whole_row_panels():
    """B = 16 with N = 15 sentences per video: 16 * (64 + 15) rows are not whole 64-row panels; the two-chain step adds ONE padded
    sentence slot per video (masked as a key, dropped from the loss) so that the joint stack runs the row-panel kernels -- loss and
    gradients equal the unpadded step's (the fallback launches) up to bf16 rounding of another kernel path."""
    import numpy as np
    from temporalalignnet_amd import synth
    from temporalalignnet_amd.train import Trainer, to_device_batch
    b_np = synth.make_batch(61, B=16, T=64, n_min=4, n_max=15)
    assert b_np["text_embed"].shape[1] == 15
    b = to_device_batch(b_np)
    padded = Trainer._pad_sentence_slots(b)
    assert padded["text_embed"].shape[1] == 16 and padded["_tgt_raw"].shape[1] == 16 and bool(padded["text_padding_mask"][:, 15].all())
    assert Trainer._pad_sentence_slots(padded) is padded
    outs = []
    for pad in (True, False):
        tr, _ = _trainer(seed=9, dtype="bf16", model="init")
        if not pad:
            tr._pad_sentence_slots = lambda batch: batch
        assert tr._chains_eligible(b, tr.fused_loss)
        np.random.seed(1)
        tr.zero_grad()
        ld = tr.forward_backward(b)
        torch.cuda.synchronize()
        outs.append((float(ld["loss"]), tr.online.flat_grad().clone()))
    (l1, g1), (l0, g0) = outs
    assert abs(l1 - l0) <= 2e-3 * abs(l0), (l1, l0)
    assert (g1 - g0).norm() <= 3e-2 * g0.norm(), float((g1 - g0).norm() / g0.norm())


def test_reads_after_a_pipelined_step_wait_for_its_optimizer_launches():
    """`Trainer.step` (stage 1) returns with the optimizer launches of the stacks' matrices still running on the trainer's role streams
    (DESIGN.md section 3.7).  Whatever reads parameters through this package afterwards -- a forward, `state_dict()`,
    `flat_parameters()` -- must see the STEPPED parameters without the caller synchronising: compared with the same read after a
    device-wide synchronisation."""
    tr, _ = _trainer(seed=11, dtype="bf16", model="init")
    assert tr.pipeline
    b = _batch(91, B=16, T=64)
    for _ in range(2):
        tr.step(b)
    assert tr.online._flat.pending                                # (events of the last step are waiting)
    m = tr.online
    with torch.no_grad():
        feat_now = m.get_visual_feature(b["video"], b["padding_mask"]).clone()        # no synchronisation in between
    assert not m._flat.pending
    flat_now = m.flat_parameters().clone()
    torch.cuda.synchronize()
    with torch.no_grad():
        feat_sync = m.get_visual_feature(b["video"], b["padding_mask"])
    assert torch.equal(feat_now, feat_sync) and torch.equal(flat_now, m.flat_parameters())
    tr.step(b)
    sd = {k: v.clone() for k, v in tr.model.state_dict().items()}                     # state_dict(): the same rule
    torch.cuda.synchronize()
    for k, v in tr.model.state_dict().items():
        assert torch.equal(sd[k], v), k


def test_padded_sentence_slots_do_not_change_stage2():
    """The same padding in the co-training step (EMA forward, self-labelling, thresholds, alignability head with abs_text_pos): every
    entry of the loss dict equal to the unpadded step's up to the bf16 rounding of another kernel path."""
    from temporalalignnet_amd import synth
    from temporalalignnet_amd.train import Trainer, to_device_batch
    b = to_device_batch(synth.make_batch(63, B=16, T=64, n_min=4, n_max=15))
    assert b["text_embed"].shape[1] == 15
    outs = []
    for pad in (True, False):
        tr, _ = _trainer(seed=13, dtype="bf16", model="cotrain", loss_threshold=0.5)
        tr.model._copy_param()
        if not pad:
            tr._pad_sentence_slots = lambda batch: batch
        tr.zero_grad()
        ld = tr.forward_backward(b)
        torch.cuda.synchronize()
        outs.append(({k: float(v) for k, v in ld.items()}, tr.online.flat_grad().clone()))
    (l1, g1), (l0, g0) = outs
    assert set(l1) == set(l0)
    for k in l0:
        # (fractions of the ~160 real sentences -- confidence-ratio, alignability_top1 -- move in steps of 1 / 160: a borderline sentence
        #  may fall the other way when another kernel path rounds its bf16 features differently)
        tol = 2.0 / 160 if k in ("confidence-ratio", "alignability_top1") else 5e-3 * max(1.0, abs(l0[k]))
        assert abs(l1[k] - l0[k]) <= tol, (k, l1[k], l0[k])
    assert (g1 - g0).norm() <= 5e-2 * g0.norm(), float((g1 - g0).norm() / g0.norm())


@pytest.mark.parametrize("E,D,B,T", [(1, 1, 32, 16), (1, 2, 8, 64), (3, 1, 8, 64)])
def test_pipelined_chain_steps_on_shallow_and_uneven_stacks(monkeypatch, E, D, B, T):
    """BASELINE configs[0]'s shape (E1D1, len = 16, 32 videos) and uneven stacks through the pipelined two-chain step: stacks shallower
    than the dW tails (the joint chain moves its last TWO blocks' weight gradients off the chain), early optimizer launches of unequal
    unit ranges, alternating workspaces -- five steps against the same five under autograd with one optimizer launch."""
    from temporalalignnet_amd.train import Trainer, build_model, default_args
    batches = [_batch(70 + i, B=B, T=T) for i in range(5)]
    flats = {}
    for tag, env in (("plain", "0"), ("bench", "1")):
        for k in ("TAN_STEP_CHAINS", "TAN_OPT_EARLY", "TAN_OPT_IMAGES", "TAN_STEP_PIPELINE"):
            monkeypatch.setenv(k, env)
        args = default_args(model="init", num_encoder_layers=E, num_decoder_layers=D, lr=1e-3, wd=1e-2)
        torch.manual_seed(17)
        tr = Trainer(build_model(args, compute_dtype="bf16", random_pos_start=0).cuda(), args, iter_per_epoch=50, warmup=5)
        tr.iteration = tr.batches_seen = 10
        assert tr.pipeline == (env == "1")
        for b in batches:
            assert tr._chains_eligible(tr._pad_sentence_slots(b), tr.fused_loss) == (env == "1")
            ld = tr.step(b)
        flats[tag] = tr.online.flat_parameters().clone()
        assert torch.isfinite(ld["loss"]).item() and torch.isfinite(flats[tag]).all()
    d = (flats["bench"] - flats["plain"]).abs()
    # (Adam turns atomics-order noise on ~zero gradients into lr-sized updates of a few elements: the bound of the B = 8 test, five steps)
    assert d.max().item() <= 1.1e-2 and d.mean().item() <= 5e-5, (d.max().item(), d.mean().item())


_SPLIT_AB = r"""
import sys, torch
sys.path.insert(0, {root!r})
from temporalalignnet_amd import synth
from temporalalignnet_amd.train import Trainer, build_model, default_args, to_device_batch
stage = {stage!r}
kw = dict(model="cotrain", loss_threshold=0.5) if stage == "cotrain" else dict(model="init")
args = default_args(num_encoder_layers=6, num_decoder_layers=6, lr=1e-3, wd=1e-5, **kw)
torch.manual_seed(3)
model = build_model(args, compute_dtype="bf16", random_pos_start=0, language_model=None)
head = stage == "cotrain"
sd = {{("online." if head else "") + k: torch.from_numpy(v) for k, v in synth.make_params(7, 6, 6, head).items()}}
if head:
    sd.update({{"target." + k: torch.from_numpy(v) for k, v in synth.make_params(8, 6, 6, head).items()}})
model.load_state_dict(sd)
model.cuda()
tr = Trainer(model, args)
batches = [to_device_batch(synth.make_batch(40 + i, B=16, T=64, n_min=4, n_max=16)) for i in range(3)]
tr.zero_grad()
tr.keep_aux = stage == "cotrain"
tr.forward_backward(batches[0])
tr.keep_aux = False
grad0 = tr.online.flat_grad().clone()
dec = {{}}
if stage == "cotrain":      # what the step decided without gradient: agreement targets, kept sentences, alignability labels
    aux = tr.last_aux
    dec = {{"tgt": (aux["agreement_tgt"] != 0).cpu(), "th": aux["t_th_mask"].cpu(), "lab": torch.nan_to_num(aux["t_align_th_mask"], nan=-1.0).cpu()}}
losses = []
for rep in range(4):                       # 12 pipelined steps: scratch sets, the two activation workspaces and every role stream get reused
    for b in batches:
        losses.append(tr.step(b)["loss"])
flat = [tr.online.flat_parameters().clone()] + ([model.target.flat_parameters().clone()] if head else [])
torch.cuda.synchronize()
assert tr._last_step_chains
torch.save({{"flat": torch.cat(flat).cpu(), "grad": grad0.cpu(), "dec": dec, "loss": torch.stack([l.detach().float().cpu() for l in losses])}}, {out!r})
"""


@pytest.mark.parametrize("stage", ["init", "cotrain"])
def test_small_batch_split_launches_match_the_whole_panel_launches(stage, tmp_path):
    """B_local = 16 (SURVEY 8(d) config 3's second reporting point: 16 / 20 row panels per stack): twelve pipelined two-chain steps of
    E6D6 with the split-hidden MLP launches, the head-pair-split attention branch and every block's weight gradients off the chains
    (TAN_SPLIT_PANELS = 48, the default) against the same steps on the whole-panel launches (TAN_SPLIT_PANELS = 0) -- the variable is read
    once per process, so each side is a process of its own.  Same arithmetic per element up to the order of f32 additions (eight hidden
    chunks, four head pairs) and the bf16 roundings that order flips (1-2 % of x_out's entries by one ulp, tests/test_panel_gpu.py):
    the first step's gradient norm-relative 5e-3 (the bf16 step against the fp32 oracle reads 1.2e-2; a corrupted panel reads > 0.1), the
    losses of the first steps, and the parameters after twelve AdamW steps at lr 1e-3 (an element whose tiny gradient flips sign every
    step moves 1.2e-2 apart; measured max 1.2e-2, mean 4.5e-5)."""
    import os
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    res = {}
    for sp in ("48", "0"):
        out = str(tmp_path / f"split_{sp}.pt")
        env = dict(os.environ, TAN_SPLIT_PANELS=sp)
        r = subprocess.run([sys.executable, "-c", _SPLIT_AB.format(root=root, stage=stage, out=out)], capture_output=True, text=True, env=env,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res[sp] = torch.load(out)
    a, b = res["48"], res["0"]
    assert torch.isfinite(a["flat"]).all() and torch.isfinite(a["loss"]).all()
    rel = ((a["grad"] - b["grad"]).norm() / b["grad"].norm()).item()
    flips = {k: int((a["dec"][k] != b["dec"][k]).sum()) for k in a["dec"]}
    print("first step's gradient, split vs whole-panel launches, norm-relative:", stage, rel, "decisions that differ:", flips)
    # (stage 2: a sentence whose maximum sits at a batch median / quantile changes sides with the last bf16 bit of a logit, and at 16
    #  videos -- ~160 sentences -- one flipped label moves the BCE gradient by percents: the tight bound holds when no decision differs)
    assert rel <= (5e-3 if not any(flips.values()) else 0.25), (rel, flips)
    d = (a["flat"] - b["flat"]).abs()
    # (stage 2 in bf16 is not decision-exact between two kernel paths -- 20 of 16 384 target entries differ on step 1 here -- and
    #  twelve steps amplify that: measured mean 5.6e-4, losses within 4 %; stage 1 has no decisions: mean 4.4e-5)
    tol_mean, tol_loss = (1.5e-4, 2e-2) if stage == "init" else (1.5e-3, 8e-2)
    print("split vs whole-panel launches, 12 steps at B = 16:", stage, "max", d.max().item(), "mean", d.mean().item(),
          "losses", a["loss"][-3:].tolist(), b["loss"][-3:].tolist())
    assert d.max().item() <= 2.5e-2 and d.mean().item() <= tol_mean, (d.max().item(), d.mean().item())
    assert (a["loss"][:3] - b["loss"][:3]).abs().max().item() <= tol_loss * b["loss"][:3].abs().max().item()


@pytest.mark.parametrize("switches", [{}, {"TAN_STEP_PIPELINE": "0"}, {"TAN_OPT_EARLY": "0"}, {"TAN_OPT_IMAGES": "0"},
                                      {"TAN_STEP_PIPELINE": "0", "TAN_OPT_EARLY": "0", "TAN_OPT_IMAGES": "0"}])
def test_stage2_chain_step_matches_the_autograd_step_under_every_schedule_switch(monkeypatch, switches):
    """Stage 2 ('cotrain': EMA forward, self-labelling, threshold 0.5, alignability head + BCE) in bf16 at B = 8: `Trainer.step` as two
    chains with two meeting points (`chain_step.Stage2Step`) against forward -> EMA forward -> get_loss -> loss.backward() under
    autograd (TAN_STAGE2_CHAINS=0), with the step pipelined or joined, the stacks' optimizer launches early or at the end, the weight
    images from the optimizer launch or rebuilt: every entry of the first step's loss dict, and the online AND EMA parameters after three
    steps (same kernels on the same values up to the order of f32 atomics; a batch this small has no sentence near a threshold).
    train/main.py:89-98,112-122; train/loss.py:88-229,277-373."""
    from temporalalignnet_amd import synth
    from temporalalignnet_amd.train import to_device_batch
    batches = [to_device_batch(synth.make_batch(310 + i, B=8, T=64, n_min=4, n_max=12)) for i in range(3)]
    res = {}
    for tag, chains in (("autograd", "0"), ("chains", "1")):
        monkeypatch.setenv("TAN_STAGE2_CHAINS", chains)
        for k in ("TAN_STEP_PIPELINE", "TAN_OPT_EARLY", "TAN_OPT_IMAGES"):
            monkeypatch.delenv(k, raising=False)
        if chains == "1":
            for k, v in switches.items():
                monkeypatch.setenv(k, v)
        tr, _ = _trainer(seed=21, dtype="bf16", model="cotrain", loss_threshold=0.5)
        tr.model._copy_param()
        lds = [tr.step(b) for b in batches]
        assert bool(tr.__dict__.get("_last_step_chains")) == (chains == "1")
        flat = torch.cat([tr.online.flat_parameters().clone(), tr.model.target.flat_parameters().clone()])
        torch.cuda.synchronize()
        res[tag] = ({k: float(v) for k, v in lds[0].items()}, flat)
    (l0, p0), (l1, p1) = res["autograd"], res["chains"]
    assert set(l0) == set(l1), (sorted(l0), sorted(l1))
    for k in l0:
        assert abs(l0[k] - l1[k]) <= 2e-3 * max(1.0, abs(l0[k])), (k, l0[k], l1[k])
    d = (p1 - p0).abs()
    assert torch.isfinite(p1).all() and d.max().item() <= 6.5e-3 and d.mean().item() <= 6e-5, (d.max().item(), d.mean().item())
