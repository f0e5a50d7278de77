"""tests/w2v_cases.py on the CPU: the fp32-mode reference is oracle.w2v_ref.forward in float64 (values and gradients) and reproduces
the reference-generated golden G8; the first-index pooling rule gives the expected index on hand-made ties; the bf16 mode reads rounded
operands and pools the rounded h; the exact expectations of the gather / pool kernels are what a plain loop gives; and a pooling that
breaks ties the other way, or a backward without the `pooled > 0` gate, is told apart."""
import numpy as np
import pytest
import torch

import w2v_cases as wc
from oracle import w2v_ref
from temporalalignnet_amd import synth

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
V = 500


def _params():
    return {k: torch.from_numpy(v) for k, v in synth.w2v_params(31, V).items()}


def _fp(g):
    g = g.detach().double().flatten().cpu()
    idx = torch.linspace(0, g.numel() - 1, 16).long()
    return np.concatenate([[g.sum().item(), g.norm().item()], g[idx].numpy()])


@pytest.mark.parametrize("masked", [True, False])
def test_fp32_mode_is_the_oracle_in_float64(masked):
    ids, mask = (torch.from_numpy(a) for a in synth.w2v_tokens(32, 9, V))
    am = mask if masked else None
    w = torch.from_numpy(synth.normal(33, "w", (9, 512)))
    out, grads = wc.forward_backward(_params(), ids, am, w)
    p = {k: v.double().requires_grad_(k != "word_embd.weight") for k, v in _params().items()}
    want = w2v_ref.forward(p, ids, am)
    (want["pooler_output"] * w.double()).sum().backward()
    for k in ("pooler_output", "last_hidden_state"):
        assert float((out[k] - want[k].detach()).abs().max()) <= 1e-12, k
    for k in wc.GRAD_KEYS:                     # (a tie moves the gradient between identical rows of x: the weight gradient is the same)
        assert float((grads[k] - p[k].grad).abs().max()) <= 1e-12 * max(1.0, float(p[k].grad.abs().max())), k


def test_fp32_mode_reproduces_the_reference_golden(golden):
    g = golden("g8_word2vec")
    ids, mask = (torch.from_numpy(a) for a in synth.w2v_tokens(32, 9, V))
    w = torch.from_numpy(synth.normal(33, "w", (9, 512)))
    out, grads = wc.forward_backward(_params(), ids, mask, w)
    np.testing.assert_allclose(out["pooler_output"].numpy(), g["pooler_output"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out["last_hidden_state"].numpy(), g["last_hidden_state"], rtol=1e-5, atol=1e-6)
    nomask = wc.forward(wc.operands(_params(), False), ids)["pooler_output"].detach()
    np.testing.assert_allclose(nomask.numpy(), g["pooler_nomask"], rtol=1e-5, atol=1e-6)
    for k in wc.GRAD_KEYS:
        np.testing.assert_allclose(_fp(grads[k]), g["grad/" + k], rtol=1e-4, atol=1e-6, err_msg=k)


def test_first_index_rule_on_hand_made_ties():
    """h [2, 5, 4]; channel 0: the maximum twice (words 1 and 3); channel 1: every word 0; channel 2: the maximum on the last word only;
    channel 3: 1 + 2^-9 and 1 + 2^-10 differ in f32 and both round to 1 in bf16"""
    h = torch.zeros(2, 5, 4)
    h[0, :, 0] = torch.tensor([0.5, 2.0, 1.0, 2.0, 0.0])
    h[0, :, 2] = torch.tensor([0.0, 0.25, 0.25, 0.0, 0.75])
    h[0, :, 3] = torch.tensor([0.5, 1 + 2.0 ** -10, 0.0, 1 + 2.0 ** -9, 0.0])
    h[1] = h[0].flip(0)
    pooled, first = wc.first_max(h)
    assert first.tolist() == [[1, 0, 4, 3], [1, 0, 0, 1]]
    assert pooled.tolist() == [[2.0, 0.0, 0.75, 1 + 2.0 ** -9]] * 2
    assert wc.last_max(h)[1].tolist() == [[3, 4, 4, 3], [3, 4, 0, 1]]
    pooled, first = wc.first_max(h.to(BF16))                   # the tie that exists only after rounding
    assert first.tolist() == [[1, 0, 4, 1], [1, 0, 0, 1]] and pooled[:, 3].tolist() == [1.0, 1.0]
    # masks: word 1 masked -> the other maximum; every word masked -> the fill, index 0; a masked word ties with an unmasked -6e4
    keep = torch.ones(2, 5, dtype=torch.uint8)
    keep[0, 1] = 0
    keep[1] = 0
    pooled, first = wc.first_max(h, keep)
    assert first[0].tolist() == [3, 0, 4, 3] and first[1].tolist() == [0, 0, 0, 0] and bool((pooled[1] == wc.FILL).all())
    h2 = torch.full((1, 3, 1), wc.FILL)
    assert wc.first_max(h2, torch.tensor([[0, 1, 1]]))[1].item() == 0
    assert wc.first_max(h2.to(BF16), torch.tensor([[0, 1, 1]]))[1].item() == 1        # -59904 > -6e4: no tie in bf16
    p, a = wc.wordpool_expected(h2.to(BF16), torch.tensor([[0, 0, 0]]), BF16)
    assert p.item() == -59904.0 and a.item() == 0 and a.dtype == torch.int32


def test_duplicated_ids_and_dead_channels_tie_in_the_model_reference():
    """without a mask the trailing id-0 words are the same row: wherever one of them is the maximum the rule picks the first of them;
    a channel no word fires in is 0 for every word and picks word 0"""
    ids = torch.tensor([[7, 0, 9, 0, 0, 0], [0, 0, 0, 0, 0, 0]])
    out = wc.forward(wc.operands(_params(), False), ids)
    h, first = out["h"].detach(), out["first"]
    assert bool((h[0, 1] == h[0, 3]).all()) and bool((h[1] == h[1, :1]).all())
    assert not bool(((first[0] == 3) | (first[0] == 4) | (first[0] == 5)).any()) and bool((first[0] == 1).any())
    assert bool((first[1] == 0).all())
    dead = h[0].amax(0) == 0
    assert bool(dead.any()) and bool((first[0][dead] == 0).all())


def test_bf16_mode_reads_rounded_operands_and_pools_the_rounded_h():
    ids, mask = wc.tokens(5, 6, 9, V)
    p = _params()
    q = wc.operands(p, True)
    for k in ("word_embd.weight", "fc1.weight", "fc2.weight"):
        assert torch.equal(q[k].detach(), p[k].bfloat16().double()) and not torch.equal(q[k].detach(), p[k].double())
    for k in ("fc1.bias", "fc2.bias"):
        assert torch.equal(q[k].detach(), p[k].double())
    assert not q["word_embd.weight"].requires_grad and q["fc1.weight"].requires_grad
    out = wc.forward(q, ids, mask, bf16=True)
    h = out["h"].detach()
    assert torch.equal(h, h.bfloat16().double())                       # the stored values
    pooled, first = wc.first_max(h, wc.keep_mask(mask))
    assert torch.equal(first, out["first"])
    # the straight-through term: the gradient is that of the unrounded chain at the same selection
    w = torch.randn(6, 512, generator=torch.Generator().manual_seed(1), dtype=F64)
    (out["pooler_output"] * w).sum().backward()
    q2 = wc.operands(p, True)
    x = q2["word_embd.weight"][ids]
    h2 = torch.relu(x @ q2["fc1.weight"].t() + q2["fc1.bias"])
    sel = h2.gather(1, first[:, None, :])[:, 0]
    ((sel @ q2["fc2.weight"].t() + q2["fc2.bias"]) * w).sum().backward()
    gate = (pooled > 0)
    assert bool(gate.any()) and not bool(gate.all())
    for k in ("fc1.weight", "fc1.bias"):
        assert float((q[k].grad - q2[k].grad).abs().max()) <= 1e-12, k
    assert float((q["fc2.bias"].grad - q2["fc2.bias"].grad).abs().max()) == 0


def test_exact_params_make_h_exact_in_f32_and_tie_between_different_words():
    p = wc.exact_params(_params())
    wc.assert_h_exact(p)
    with pytest.raises(AssertionError):
        wc.assert_h_exact(_params())
    assert torch.equal(p["fc2.weight"], _params()["fc2.weight"]) and not torch.equal(p["fc1.weight"], _params()["fc1.weight"])
    ids, mask = wc.tokens(9, 40, 8, V)
    x = p["word_embd.weight"][ids].view(-1, 300)
    h64 = x.double() @ p["fc1.weight"].double().t() + p["fc1.bias"].double()
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(0))
    for h32 in (x @ p["fc1.weight"].t() + p["fc1.bias"], x[:, perm] @ p["fc1.weight"][:, perm].t() + p["fc1.bias"]):
        assert h32.dtype == F32 and torch.equal(h32.double(), h64)               # any order of accumulation
    for bf16 in (False, True):                                                   # nothing to round in the operands of fc1
        q = wc.operands(p, bf16)
        assert all(torch.equal(q[k].detach(), p[k].double()) for k in ("word_embd.weight", "fc1.weight", "fc1.bias"))
    # under the mask the tied words are different words: the index decides where the gradient goes
    out = wc.forward(wc.operands(p, False), ids, mask)
    hd = out["h"].detach().masked_fill(~wc.keep_mask(mask)[:, :, None], wc.FILL)
    tied = (hd == hd.amax(1, keepdim=True)) & (hd > 0)
    assert bool((tied.sum(1) > 1).any())
    w = torch.randn(40, 512, generator=torch.Generator().manual_seed(3), dtype=F64)
    _, g_first = wc.forward_backward(p, ids, mask, w)
    _, g_last = wc.forward_backward(p, ids, mask, w, pool=wc.last_max)
    assert wc.rel_err(g_last["fc1.weight"], g_first["fc1.weight"]) > 1e-3        # (the fp32 cap of the model test is 1e-5)


def test_out_of_range_ids_read_row_zero():
    ids, mask = wc.tokens(6, 4, 7, V)
    bad = ids.clone()
    bad[0, 0], bad[1, 1], bad[3, 2] = -1, V, V + 7
    fixed = bad.clone()
    fixed[0, 0] = fixed[1, 1] = fixed[3, 2] = 0
    q = wc.operands(_params(), False)
    a, b = wc.forward(q, bad, mask), wc.forward(q, fixed, mask)
    assert torch.equal(a["pooler_output"], b["pooler_output"]) and torch.equal(a["last_hidden_state"], b["last_hidden_state"])


def test_tokens_and_masks_hold_what_they_promise():
    ids, mask = wc.tokens(3, 9, 32, V)
    assert ids.dtype == torch.int64 and mask.dtype == torch.uint8 and int(ids.max()) < V and int(ids.min()) == 0
    assert bool((ids[2] == 0).all()) and int(ids[1, 2]) == 0 and int(ids[1, 3]) != 0 and bool((ids[:, 0][[0, 1, 3]] != 0).all())
    ids, mask = wc.tokens(3, 1, 32, V)
    assert ids.shape == (1, 32) and int(mask.sum()) >= 1
    k = wc.masks(7, 9, 0)
    assert k[0].tolist() == [1, 1, 1, 0, 0, 0, 1, 1, 1] and k[1].tolist() == [0] + [1] * 8 and int(k[2].sum()) == 0 and int(k[3].sum()) == 9
    assert wc.masks(3, 1, 0).tolist() == [[0], [0], [0]]
    for dtype in (F32, BF16):
        m = wc.masks(7, 9, 1)
        h = wc.tied_h(7, 9, 64, dtype, m, 2)
        hd = h.double().masked_fill(~m.bool()[:, :, None], wc.FILL)
        ties = (hd == hd.amax(1, keepdim=True)).sum(1)
        assert bool((ties > 1).any()) and bool((ties == 1).any())
        assert bool((h[:, :, 0::8] == 0).all())
        _, first = wc.first_max(h, m)
        assert int(first[6, 1]) == (0 if dtype == F32 else 1)              # sentence 6: word 0 masked, the others at -6e4 unmasked


def test_kernel_expectations_are_what_a_loop_gives():
    g = torch.Generator().manual_seed(4)
    table = torch.randn(6, 5, generator=g)
    ids = torch.tensor([0, 5, -1, 6, 13, 2])
    for dtype in (F32, BF16):
        out = wc.gather_expected(table, ids, 6, 5, 8, dtype)
        for r, i in enumerate([0, 5, 0, 0, 0, 2]):
            assert torch.equal(out[r, :5], table[i].to(dtype)) and bool((out[r, 5:] == 0).all())
        assert torch.equal(wc.gather_expected(table, None, 4, 5, 8, dtype)[:, :5], table[:4].to(dtype))
    M, W, H = 3, 4, 8
    m = torch.tensor([[1, 0, 1, 1], [0, 0, 0, 0], [1, 1, 1, 1]], dtype=torch.uint8)
    h = wc.tied_h(M, W, H, F32, m, 5)
    pooled, arg = wc.wordpool_expected(h, m, F32)
    for mm in range(M):
        for j in range(H):
            best, bi = -float("inf"), 0
            for w in range(W):
                v = float(h[mm, w, j]) if m[mm, w] else wc.FILL
                if v > best:
                    best, bi = v, w
            assert float(pooled[mm, j]) == best and int(arg[mm, j]) == bi
    dp = torch.randn(M, H, generator=g)
    dh, gated = wc.wordpool_bwd_expected(dp, pooled, arg, W)
    for mm in range(M):
        for w in range(W):
            for j in range(H):
                want = float(dp[mm, j]) if (int(arg[mm, j]) == w and float(pooled[mm, j]) > 0) else 0.0
                assert float(dh[mm, w, j]) == want
    assert bool((pooled <= 0).any()) and bool((gated[pooled <= 0] == 0).all())


def test_a_wrong_tie_rule_or_a_missing_gate_is_told_apart():
    """Duplicated ids tie between equal rows of x, so either index gives the same weight gradient; the kernel-level test compares the
    index itself.  Ties after bf16 rounding are between different words: there the last index among equal maxima moves fc1's
    gradient by more than the bf16 cap of the model test (0.016)."""
    ids, mask = wc.tokens(8, 12, 9, V)
    w = torch.randn(12, 512, generator=torch.Generator().manual_seed(2), dtype=F64)
    _, g_first = wc.forward_backward(_params(), ids, mask, w, bf16=True)
    _, g_last = wc.forward_backward(_params(), ids, mask, w, bf16=True, pool=wc.last_max)
    assert wc.rel_err(g_last["fc1.weight"], g_first["fc1.weight"]) > 0.016
    # no gate: d_pooled reaches dh where pooled <= 0
    M, W, H = 4, 3, 16
    h = wc.tied_h(M, W, H, F32, None, 6)
    pooled, arg = wc.wordpool_expected(h, None, F32)
    dp = torch.ones(M, H)
    dh, _ = wc.wordpool_bwd_expected(dp, pooled, arg, W)
    ungated = torch.zeros(M, W, H).scatter_(1, arg.long()[:, None, :], dp[:, None, :])
    assert not torch.equal(dh, ungated) and float(dh.sum()) == float((pooled > 0).sum())
