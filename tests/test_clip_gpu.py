"""Per-parameter gradient clipping on the device (csrc/tan_clip.hip: tan_clip_sumsq + tan_clip_apply; utils/train_utils.py:3-13, called
at train/main.py:115-116): the two launches against the fp64 rule of tests/test_clip_cpu.py on a synthetic flat buffer, and `Trainer`
with the fused clip against the tensor-by-tensor torch rule (TAN_CLIP_FUSED=0), in fp32 on one shared gradient and in bf16 through the
pipelined two-chain step with early optimizer launches.

Error bound of the norm, from the summation as built (u = 2^-24, every term non-negative, so a sum's relative error is at most u per
rounding on the longest path): a thread adds at most CHUNK / (256 threads x 4 components) = 8 squares per float4 component by fma
(8 roundings), one more for a scalar head / tail element, combines its four components in 2 levels, the wave tree is 6 levels, the four
waves 2 levels: 19 roundings on the chunk's sum of squares.  The partials are summed in double (nothing at this scale).  The square
root halves the relative error (9.5 u); rounding it to f32 and the product with grad_scale add one u each: 11.5 u = 6.9e-7 on the norm.
A clipped element adds the sum norm + 1e-6, the division and the product: 3 u more."""
import numpy as np
import pytest
import torch

from temporalalignnet_amd import ops, synth
from test_clip_cpu import clip_rule_fp64

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NORM_REL = 11.5 * U          # 6.9e-7: see the module docstring
ELEM_REL = NORM_REL + 3 * U  # a clipped element: + (norm + 1e-6), clip / that, g * coef; the test adds one ulp of the expected value


# ------------------------------------------------------------------------------------------------------------------- kernel level
def _synthetic(shift):
    """Segments of 1, 7, 8, 513, CHUNK - 1, CHUNK, CHUNK + 1, 3 CHUNK + 5 elements and one of zeros, at 8-aligned offsets with at least
    eight padding elements (1e30) on either side of each; three groups of three segments; norms on both sides of clip = 1 in every
    group.  shift = 1: the buffer starts one element past an allocation, so no chunk starts on a 16-byte boundary."""
    CH = ops.clip_chunk()
    sizes = [1, 7, 8, 513, CH - 1, CH, CH + 1, 3 * CH + 5, 100]
    norms = [20.0, 0.5, 30.0, 0.3, 12.0, 0.6, 16.0, 0.2, 0.0]
    rng = np.random.default_rng(11)
    offs, pos = [], 8
    for k in sizes:
        offs.append(pos)
        pos = (pos + k + 7) // 8 * 8 + 8
    total = pos
    g = np.full(total, 1e30, dtype=np.float32)
    for o, k, nrm in zip(offs, sizes, norms):
        x = rng.standard_normal(k)
        g[o:o + k] = (x / np.sqrt(np.sum(x * x)) * nrm).astype(np.float32)
    chunks, segs = [], []
    for s, (o, k) in enumerate(zip(offs, sizes)):
        segs.append((len(chunks), (k + CH - 1) // CH))
        chunks += [(o + i, min(CH, k - i), s, 0) for i in range(0, k, CH)]
    seg_bounds = (0, 3, 6, 9)
    chunk_bounds = tuple(segs[s][0] if s < len(segs) else len(chunks) for s in seg_bounds)
    base = torch.full((total + shift,), 1e30, dtype=torch.float32, device="cuda")
    dev_g = base[shift:]
    dev_g.copy_(torch.from_numpy(g))
    tabs = (torch.tensor(chunks, dtype=torch.int32, device="cuda"), torch.tensor(segs, dtype=torch.int32, device="cuda"))
    return g, dev_g, tabs, offs, sizes, chunk_bounds, seg_bounds, len(chunks)


def _run(g, tabs, chunks, segs, n_chunks, n_segs, clip, gs, norms=None):
    partials = torch.full((n_chunks,), float("nan"), device="cuda")
    norms = torch.full((n_segs,), -7.0, device="cuda") if norms is None else norms
    ops.clip_sumsq(g, tabs[0], tabs[1], chunks, segs, partials)
    ops.clip_apply(g, tabs[0], tabs[1], chunks, segs, partials, clip, gs, norms)
    return norms


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_clip_kernels_against_the_fp64_rule(grad_scale, shift):
    g0, dev_g, tabs, offs, sizes, cb, sb, n_chunks = _synthetic(shift)
    assert dev_g.data_ptr() % 16 == 4 * shift
    keep = dev_g.clone()
    norms = _run(dev_g, tabs, (0, n_chunks), (0, 9), n_chunks, 9, 1.0, grad_scale).cpu().numpy()
    got = dev_g.cpu().numpy()
    pad = np.ones(g0.size, dtype=bool)
    kinds = []
    for s, (o, k) in enumerate(zip(offs, sizes)):
        pad[o:o + k] = False
        norm64, want64, clipped = clip_rule_fp64(g0[o:o + k], 1.0, grad_scale)
        kinds.append(clipped)
        print(f"segment {s} ({k} elements): norm {norms[s]:.9g} fp64 {norm64:.9g} rel {abs(norms[s] - norm64) / max(norm64, 1e-30):.3g}")
        assert abs(norms[s] - norm64) <= NORM_REL * norm64, (s, k, norms[s], norm64)          # 6.9e-7 relative; the zero segment: exactly 0
        if clipped:
            want = want64.astype(np.float32)
            err = np.abs(got[o:o + k].astype(np.float64) - want)
            print(f"   clipped: max error / |expected| {np.max(err / np.maximum(np.abs(want), 1e-30)):.3g}")
            assert (err <= ELEM_REL * np.abs(want64) + np.spacing(np.abs(want))).all(), (s, k)
        else:
            assert np.array_equal(got[o:o + k].view(np.uint32), g0[o:o + k].view(np.uint32)), (s, k)      # bit for bit: nothing stored
    assert sum(kinds) == 4 and not kinds[8] and all(any(kinds[a:b]) and not all(kinds[a:b]) for a, b in zip(sb, sb[1:]))
    assert pad.sum() >= 8 * 10 and (got[pad] == np.float32(1e30)).all()                            # every padding sentinel
    full = dev_g.clone()
    # the same input again: the same bits (no atomics, one fixed order of summation)
    dev_g.copy_(keep)
    norms2 = _run(dev_g, tabs, (0, n_chunks), (0, 9), n_chunks, 9, 1.0, grad_scale)
    assert torch.equal(dev_g, full) and np.array_equal(norms2.cpu().numpy().view(np.uint32), norms.view(np.uint32))
    # the middle group alone: the other groups' gradients and norms are not touched, the middle group's are those of the full call
    dev_g.copy_(keep)
    norms3 = _run(dev_g, tabs, (cb[1], cb[2]), (sb[1], sb[2]), n_chunks, 9, 1.0, grad_scale).cpu().numpy()
    lo, hi = offs[3], offs[6] - 8
    assert torch.equal(dev_g[:lo], keep[:lo]) and torch.equal(dev_g[hi:], keep[hi:]) and torch.equal(dev_g[lo:hi], full[lo:hi])
    assert not torch.equal(dev_g[lo:hi], keep[lo:hi])
    assert (norms3[:3] == -7.0).all() and (norms3[6:] == -7.0).all() and np.array_equal(norms3[3:6], norms[3:6])


def test_clip_launches_reject_ranges_outside_their_tables():
    from temporalalignnet_amd import _lib
    _, dev_g, tabs, _, _, _, _, n_chunks = _synthetic(0)
    partials, norms = torch.zeros(n_chunks, device="cuda"), torch.zeros(9, device="cuda")
    keep = dev_g.clone()
    for chunks, segs, p, nr in (((0, n_chunks + 1), (0, 9), partials, norms), ((0, n_chunks), (0, 10), partials, norms),
                                ((0, n_chunks), (0, 9), partials[:-1], norms), ((0, n_chunks), (0, 9), partials, norms[:-1]),
                                ((2, 1), (0, 9), partials, norms)):
        with pytest.raises(_lib.TanHipError):
            ops.clip_apply(dev_g, tabs[0], tabs[1], chunks, segs, p, 1.0, 1.0, nr)
    with pytest.raises(_lib.TanHipError):
        ops.clip_sumsq(dev_g, tabs[0], tabs[1], (0, n_chunks + 1), (0, 9), partials)
    # a segment range that does not hold the chunk range's segments: those chunks are skipped, nothing is written
    ops.clip_sumsq(dev_g, tabs[0], tabs[1], (0, n_chunks), (0, 9), partials)
    ops.clip_apply(dev_g, tabs[0], tabs[1], (0, n_chunks), (0, 0), partials, 1.0, 1.0, norms)
    assert torch.equal(dev_g, keep) and (norms == 0).all()


# ------------------------------------------------------------------------------------------------------------------ trainer level
def _trainer(seed, dtype, E, D, **akw):
    from temporalalignnet_amd.train import Trainer, build_model, default_args
    args = default_args(num_encoder_layers=E, num_decoder_layers=D, lr=1e-3, wd=1e-2, **akw)
    torch.manual_seed(seed)
    m = build_model(args, compute_dtype=dtype, random_pos_start=0).cuda()
    return Trainer(m, args, iter_per_epoch=50, warmup=5)


def test_fused_clip_steps_like_the_torch_rule_on_one_gradient(monkeypatch):
    """fp32, E2D3, B = 4, T = 16: two trainers from one seed, ONE gradient (A's, copied into B: the order of the backward's atomics
    stays out of the comparison); A clips with the two launches, B with the torch rule, tensor by tensor."""
    from temporalalignnet_amd.train import to_device_batch
    batch = to_device_batch(synth.make_batch(1, B=4, T=16, n_min=2, n_max=5))
    ta, tb = (_trainer(0, "fp32", 2, 3, model="init", clip_grad=1.0) for _ in range(2))
    assert torch.equal(ta.online.flat_parameters(), tb.online.flat_parameters())
    for tr in (ta, tb):
        tr.iteration = 7
        tr.zero_grad()
    assert ta.last_grad_norms() is None                                        # nothing has been clipped yet
    ta.forward_backward(batch)
    tb.online.flat_grad().copy_(ta.online.flat_grad())
    before = {n: p.grad.double().norm().item() for n, p in ta.online.named_parameters() if p.grad is not None}
    live = sorted(v for v in before.values() if v > 0)
    clip = live[len(live) // 2] * 1.0001                                       # between two tensors' norms: some above, some below
    assert live[0] < clip < live[-1] and sum(v > clip for v in live) >= 5 and sum(v < clip for v in live) >= 5
    ta.args.clip_grad = tb.args.clip_grad = clip
    monkeypatch.setenv("TAN_CLIP_FUSED", "1")
    ta.optimizer_step()
    norms = ta.last_grad_norms()
    monkeypatch.setenv("TAN_CLIP_FUSED", "0")
    tb.optimizer_step()
    assert tb.last_grad_norms() is None
    torch.testing.assert_close(ta.online.flat_parameters(), tb.online.flat_parameters(), rtol=1e-5, atol=1e-7)
    assert (ta.online.flat_parameters() - _trainer(0, "fp32", 2, 3, model="init").online.flat_parameters()).abs().max() > 1e-5
    # the norms of the clip, by parameter name, against the gradient taken beforehand (fp64)
    assert set(before) <= set(norms) == set(ta.online._flat.names) and all(v.dim() == 0 and v.is_cuda for v in norms.values())
    for n, want in before.items():
        assert abs(norms[n].item() - want) <= NORM_REL * want, (n, norms[n].item(), want)
    # and the gradient buffer afterwards holds the clipped gradients: no tensor above the threshold
    after = {n: p.grad.double().norm().item() for n, p in ta.online.named_parameters() if p.grad is not None}
    for n, want in before.items():                     # (every element within ELEM_REL of its fp64 value: so is the norm; unclipped: equal)
        exp = min(want, clip * want / (want + 1e-6))
        assert abs(after[n] - exp) <= ELEM_REL * exp, (n, after[n], want, clip)
    # clip_grad == 0: no norms
    ta.args.clip_grad = 0.0
    monkeypatch.setenv("TAN_CLIP_FUSED", "1")
    assert ta.last_grad_norms() is None


@pytest.mark.parametrize("kind,E,D", [("init", 1, 2), ("cotrain", 1, 3), ("cotrain", 2, 3)])
def test_clipped_chain_steps_take_the_early_update_schedule(monkeypatch, kind, E, D):
    """bf16, B = 8, T = 64.  Stage 1 at E1D2, the smallest shape the pipelined chains with early optimizer launches run at.  Stage 2
    ('cotrain', loss_threshold 0.5) needs three joint layers -- 'cotrain' always carries the alignability head (train/main.py:361-363),
    whose loss reads the joint stack's stage index 2 (loss.py:341), so a two-layer joint stack has no stage-2 loss, here or in the
    reference -- and is run at E1D3, the smallest stage-2 shape, and at E2D3, the shape of the existing stage-2 chain tests.  With
    clip_grad > 0 the early launches are allowed, each behind the clip of its stack's matrices.  Three steps against the same three
    with the optimizer launches at the end of the step (TAN_OPT_EARLY=0) and against the torch rule (TAN_CLIP_FUSED=0).  Same arithmetic
    up to the order of the f32 gradient atomics: Adam turns that noise, on ~zero gradients, into lr-sized (1e-3) updates of a few
    elements -- the bound of test_pipelined_chain_steps_on_shallow_and_uneven_stacks (five steps there): max 1.1e-2, mean 5e-5."""
    from temporalalignnet_amd.train import to_device_batch
    kw = dict(model=kind, **({"loss_threshold": 0.5} if kind == "cotrain" else {}))
    # (the batches the existing two-chain tests of each stage run at this size)
    mk = (lambda i: synth.make_batch(70 + i, B=8, T=64, n_min=2, n_max=5)) if kind == "init" else \
         (lambda i: synth.make_batch(310 + i, B=8, T=64, n_min=4, n_max=12))
    batches = [to_device_batch(mk(i)) for i in range(3)]

    def fresh(clip):
        tr = _trainer(3, "bf16", E, D, clip_grad=clip, **kw)
        if kind == "cotrain":
            tr.model._copy_param()
        tr.iteration = tr.batches_seen = 10
        return tr

    def grad_norms(tr):
        f = tr.online._ensure_flat()
        return np.asarray([f.view(f.grad, n).double().norm().item() for n in f.names])

    for k in ("TAN_OPT_EARLY", "TAN_CLIP_FUSED", "TAN_STEP_CHAINS", "TAN_STEP_PIPELINE", "TAN_OPT_IMAGES", "TAN_STAGE2_CHAINS"):
        monkeypatch.delenv(k, raising=False)
    probe = fresh(0.0)                                   # the threshold: the median of the first batch's gradient norms
    probe.zero_grad()
    probe.forward_backward(batches[0])
    live = np.sort(grad_norms(probe)[grad_norms(probe) > 0])
    clip = float(live[len(live) // 2])
    assert live[0] < clip < live[-1]
    res = {}
    for tag, env, c in (("early", {}, clip), ("late", {"TAN_OPT_EARLY": "0"}, clip), ("torch", {"TAN_CLIP_FUSED": "0"}, clip),
                        ("noclip", {}, 0.0)):
        for k in ("TAN_OPT_EARLY", "TAN_CLIP_FUSED"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        tr = fresh(c)
        assert tr._early_ok() == (tag != "torch")                 # with clip_grad > 0: only the fused clip keeps the early launches
        calls, orig = [], tr.early_update
        tr.early_update = lambda which, gs: (calls.append(which), orig(which, gs))[1]
        for b in batches:
            ld = tr.step(b)
        chains = bool(tr._last_step_chains)
        assert chains                                             # stage 1 and stage 2: the two-chain step
        assert sorted(calls) == (["joint"] * 3 + ["video"] * 3 if chains and tag in ("early", "noclip") else []), (tag, calls)
        norms = tr.last_grad_norms()
        assert (norms is None) == (tag in ("torch", "noclip"))
        flat = [tr.online.flat_parameters().clone()] + ([tr.model.target.flat_parameters().clone()] if kind == "cotrain" else [])
        res[tag] = (torch.cat(flat), grad_norms(tr), None if norms is None else np.asarray([norms[n].item() for n in tr.online._flat.names]))
        assert torch.isfinite(ld["loss"]).item() and torch.isfinite(res[tag][0]).all()
    n_online = res["early"][0].numel() // (2 if kind == "cotrain" else 1)
    for tag in ("late", "torch"):
        d = (res["early"][0] - res[tag][0]).abs()
        print(kind, E, D, "early vs", tag, "online max", d[:n_online].max().item(), "mean", d[:n_online].mean().item(),
              "twin max", d[n_online:].max().item() if kind == "cotrain" else None)
        for part in ((d[:n_online], d[n_online:]) if kind == "cotrain" else (d,)):
            assert part.max().item() <= 1.1e-2 and part.mean().item() <= 5e-5, (tag, part.max().item(), part.mean().item())
    # the clip acted: the last step's gradient norms were above the threshold for some tensors (what tan_clip_apply reported), the
    # gradient buffer it left holds none above it, the unclipped run's does -- and the parameters moved differently
    for tag in ("early", "late"):
        _, after, seen = res[tag]
        assert (seen > clip).sum() >= 3 and (seen < clip).sum() >= 3, (tag, clip, np.sort(seen)[[0, -1]])
        assert (after <= clip * (1 + 1e-5)).all(), (tag, after.max(), clip)
        assert np.allclose(after, np.minimum(seen, clip * seen / (seen + 1e-6)), rtol=1e-5, atol=0)
    assert (res["torch"][1] <= clip * (1 + 1e-5)).all() and (res["noclip"][1] > clip).sum() >= 3
    d0 = (res["early"][0] - res["noclip"][0]).abs()
    print(kind, E, D, "clipped vs unclipped: max", d0.max().item(), "mean", d0.mean().item())
    assert d0.max().item() > 0
