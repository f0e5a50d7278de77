"""tests/attnblk_cases.py on the CPU: the exact cases are exact (every input, q, k, v, o and x_mid representable where the GPU test
says so, the score gap at attn_cases' margin, an f32 softmax of the built scores equal to the closed form bit for bit), their closed
forms are what an fp64 evaluation of the module's own stage references gives, the padding sets hold what they promise, and the stage
bounds hold for a plain f32 / bf16 evaluation and fail for a slightly wrong one."""
import math

import pytest
import torch

import attn_cases as ac
import attnblk_cases as bc

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
H, C = bc.H, bc.C


def test_template_of():
    for L in (49, 64):
        assert bc.template_of(L) == dict(nrb16=4, nkb=2, LP=64, XROWS=64, NIDLE=4, NKV=8)
    for L in (65, 80):
        assert bc.template_of(L) == dict(nrb16=5, nkb=3, LP=96, XROWS=80, NIDLE=2, NKV=24)
    assert all(bc.template_of(L)["LP"] - L <= 47 for L in range(49, 81)) and bc.template_of(49)["LP"] - 49 == 15
    assert bc.path_of(64)["Lp"] == 64 and bc.path_of(65)["Lp"] == 96 and bc.path_of(80)["nch"] == 1
    assert bc.LENGTHS == [49, 56, 63, 64, 65, 72, 79, 80]


def test_keypad_sets():
    for L in bc.LENGTHS:
        want = {"none", "tail", "scatter", "lead32", "butlast"} | ({"mid32"} if L > 64 else set())
        s1 = bc.keypad_sets(1, L)
        assert s1[0][1] is None and {n for names, _ in s1 for n in names} == want
        s3 = bc.keypad_sets(3, L)
        assert s3[0][1] is None and {n for names, _ in s3 for n in names} == want | {"all"}
        dead = [kp.bool().all(1) for _, kp in s3[1:]]
        assert any(bool(d[1]) for d in dead), "every key of the middle video"
        assert all(not bool(d.all()) for d in dead), "next to live videos"
        for names, kp in s3[1:]:
            assert len(set(names)) == 3 and kp.shape == (3, L) and kp.dtype == torch.uint8
        kp = bc.cycle_keypad(260, L)
        names = [n for n in ac.PATTERNS if ac.pad_pattern(n, L, 0) is not None]
        assert len(names) == len(want) + 1 and torch.equal(kp[len(names) + 1], ac.pad_pattern(names[1], L, 0))
        assert bool(kp.bool().all(1).any()) and not bool(kp[:256].bool().all(1)[-1]) and bool(kp[256:].any())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", bc.LENGTHS)
def test_exact_case_is_exact(L, B):
    for i, (names, keypad) in enumerate(bc.keypad_sets(B, L)):
        c = bc.exact_case(B, L, 100 * L + 10 * B + i, keypad)
        bc.assert_exact_conditions(c)
        live, alive = c["live"], c["live"].any(1)
        # the closed-form q | k | v is the GEMM of the inputs, in f32 as in fp64
        ref, _, _ = bc.qkv_stage(c["xn1"], c["w_in"], c["b_in"])
        assert torch.equal(ref, c["qkv"].double()), names
        assert torch.equal(c["xn1"] @ c["w_in"].T + c["b_in"], c["qkv"])
        v = ac.split_qkv(c["qkv"], B, L, H)[2]
        assert float(v.abs().max()) <= 10 and v[0, 0].unique(dim=0).shape[0] == L and not torch.equal(v[0, 0], v[0, 1])
        # an f32 softmax of the scores equals the closed-form P bit for bit
        q, k, _ = ac.split_qkv(c["qkv"], B, L, H)
        s = ((q * 0.125) @ k.transpose(-1, -2)).masked_fill(~live[:, None, None, :], -math.inf)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        p = e / e.sum(-1, keepdim=True)
        assert torch.equal(p[alive].double(), c["P"][alive]), names
        assert bool((c["P"][~alive] == 0).all()) and bool(torch.isinf(c["lse"][~alive]).all()) and bool((c["o"].view(B, L, C)[~alive] == 0).all())
        assert bool((c["P"].sum(-1)[alive] == 1).all())
        # q of a head meets only the k of the same head at 504: the signed permutations differ
        cross = (q[:, 0] * 0.125) @ k[:, 1].transpose(-1, -2)
        assert float(cross.max()) < ac.SCORE_HOT
        # heads of a pair have different targets; the last row's pair is targeted where it is live
        if "butlast" not in names:                                                      # (one live key: every head targets it)
            assert not torch.equal(c["P"][:, 0], c["P"][:, 1])
        for b in range(B):
            if bool(live[b, L - 1]):
                assert float(c["P"][b, 0, 0, L - 1]) > 0 and float(c["P"][b, 1, L - 1, L - 1]) > 0
        # the closed forms against the fp64 stage references of the module
        m, _, _ = bc.attn_stage(c["qkv"], keypad, B, L)
        assert float((m["P"] - c["P"]).abs().max()) < 1e-30 and float((m["o"] - ac.split_rows(c["o"], B, L, H)).abs().max()) < 1e-28
        fin = ~torch.isinf(c["lse"])
        assert torch.equal(torch.isinf(m["lse"]), ~fin) and float((m["lse"][fin] - c["lse"][fin]).abs().max()) < 1e-12
        for split in (False, True):
            xr, _ = bc.xmid_stage(c["o"], c["x_in"], c["w_out"], c["b_out"], split)
            assert torch.equal(xr, c["x_mid"])
        xc, _ = bc.chained_xmid(c, keypad, False)
        assert float((xc - c["x_mid"]).abs().max()) < 1e-26
        # some x_mid need more than 8 bits (the kernel must round them to nearest even), most do not
        inexact = c["x_mid"].bfloat16().double() != c["x_mid"]
        assert float(inexact.double().mean()) < 0.5
        assert bool(inexact.any()) or names == ("butlast",)                          # (P = 1: o, and so x_mid, are integers up to 256)
        assert torch.equal(c["x_mid"].view(B, L, C)[~alive], (c["x_in"] + c["b_out"]).double().view(B, L, C)[~alive])


def test_exact_case_on_a_large_batch():
    B, L = 260, 64
    c = bc.exact_case(B, L, 5, bc.cycle_keypad(B, L))
    bc.assert_exact_conditions(c)
    assert torch.equal(c["xn1"] @ c["w_in"].T + c["b_in"], c["qkv"])


def bf16_eval(I, keypad, dup_last=0.0, planes=4):
    """the branch in plain f32 torch, rounded to bf16 where the kernels round (qkv, P as an operand, o); dup_last: the last key counted
    (1 + dup_last) times; planes: head pairs that reach x_mid"""
    B, L = I["B"], I["L"]
    qkv = (I["xn1"].float() @ I["w_in"].float().T + I["b_in"]).to(BF16)
    q, k, v = ac.split_qkv(qkv.float(), B, L, H)
    live = ac.live_mask(keypad, B, L, "cpu")
    s = ((q @ k.transpose(-1, -2)) * 0.125).masked_fill(~live[:, None, None, :], -math.inf)
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    e[..., L - 1] *= 1 + dup_last
    l = e.sum(-1, keepdim=True)
    o = ac.merge_rows((e / l).to(BF16).float() @ v).to(BF16)
    wo = I["w_out"].float().clone()
    wo[:, 128 * planes:] = 0
    x_mid = (I["x_in"].float() + o.float() @ wo.T + I["b_out"]).to(BF16)
    return qkv, o, (mx + l.log())[..., 0], x_mid


@pytest.mark.parametrize("L,sname", [(49, "ordinary"), (80, "ordinary"), (65, "large")])
def test_stage_bounds_hold_for_a_plain_evaluation_and_catch_a_slip(L, sname):
    B = 3
    names, keypad = bc.keypad_sets(B, L)[1]
    assert "all" not in names
    I = bc.random_case(B, L, 7 + L, sname)
    qkv, o, lse, x_mid = bf16_eval(I, keypad)
    ref, b, _ = bc.qkv_stage(I["xn1"], I["w_in"], I["b_in"])
    rs = [bc.worst_ratio(qkv, ref, b)]
    m, b_o, b_lse = bc.attn_stage(qkv, keypad, B, L)
    rs += [bc.worst_ratio(ac.split_rows(o, B, L, H), m["o"], b_o), bc.worst_ratio(lse, m["lse"], b_lse)]
    for split in (False, True):
        xr, bx = bc.xmid_stage(o, I["x_in"], I["w_out"], I["b_out"], split)
        rs.append(bc.worst_ratio(x_mid, xr, bx))
    if sname == "ordinary":
        xr, bx = bc.chained_xmid(I, keypad, False)
        rs.append(bc.worst_ratio(x_mid, xr, bx))
    assert max(rs) <= 1.0 and min(rs) > 0.0, rs
    assert rs[0] > 0.3 and rs[1] > 0.3 and rs[3] > 0.3, rs         # bf16 outputs: the bounds are little more than the stores' half ulp
    # the last key double-counted by 3 %: the softmax stage sees it
    _, o2, lse2, _ = bf16_eval(I, keypad, dup_last=0.03)
    live_last = ac.live_mask(keypad, B, L, "cpu")[:, L - 1]
    assert bool(live_last.any())
    assert bc.worst_ratio(ac.split_rows(o2, B, L, H), m["o"], b_o) > 1.0 and bc.worst_ratio(lse2, m["lse"], b_lse) > 1.0
    # a head pair's plane missing: the out-projection stage sees it
    x3 = bf16_eval(I, keypad, planes=3)[3]
    xr, bx = bc.xmid_stage(o, I["x_in"], I["w_out"], I["b_out"], True)
    assert bc.worst_ratio(x3, xr, bx) > 1.0
