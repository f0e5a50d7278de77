"""tests/attn_cases.py on the CPU: the two-hot construction is exact in f32, its closed form is what fp64 autograd gives, the fp64
reference by hand equals autograd on random data, the padding sets hold what they promise, and the error bounds hold for a plain
f32 evaluation and fail for a slightly wrong one."""
import math

import pytest
import torch

import attn_cases as ac

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def test_codes():
    c = ac.codes(512)
    assert c.shape == (512, 64) and bool((c[:, 63] == 0).all()) and bool((c[:, :63].abs() == 1).all())
    d = c @ c.t()
    assert bool((d.diagonal() == 63).all())
    off = d - 63 * torch.eye(512)
    assert float(off.max()) == 63 - 14                     # two codes differ in at least one bit = 7 dimensions
    assert 64 * 63 / 8 == ac.SCORE_HOT and 64 * (63 - 14) / 8 == ac.SCORE_NEXT


@pytest.mark.parametrize("L,onehot", [(L, False) for L in (1, 17, 100, 289, 513)] + [(L, True) for L in (1, 17, 100, 289)])
def test_twohot_is_exact_in_f32(L, onehot):
    """every value is exact in bf16; the f32 softmax of the built scores (f32 exp) equals the closed-form P bit for bit; targets are
    live keys; a padded partner makes a row one-hot; all-padded videos have P = 0, lse = -inf.  (One-hot: one code per key, so at most
    512 keys.)"""
    B, H = 3, 3
    for names, keypad in ac.keypad_sets(B, L):
        c = ac.twohot_case(B, L, H, 7 + L, keypad, onehot=onehot)
        qkv = c["qkv"]
        assert torch.equal(qkv.to(BF16).float(), qkv) and torch.equal(c["d_o"].to(BF16).float(), c["d_o"])
        q, k, v = ac.split_qkv(qkv, B, L, H)
        s = (q * 0.125) @ k.transpose(-1, -2)
        assert torch.equal(s, s.round()) and float(s.max()) == ac.SCORE_HOT
        live = ac.live_mask(keypad, B, L, "cpu")
        sm = s.masked_fill(~live[:, None, None, :], -math.inf)
        mx = sm.amax(-1, keepdim=True)
        e = torch.exp(sm - mx)
        p = e / e.sum(-1, keepdim=True)
        alive = live.any(1)
        assert torch.equal(p[alive].double(), c["P"][alive]), names
        assert bool((mx[alive] == ac.SCORE_HOT).all())
        assert bool((c["P"][~alive] == 0).all()) and bool(torch.isinf(c["lse"][~alive]).all())
        cnt = c["cnt"][alive]
        assert int(cnt.min()) >= 1 and int(cnt.max()) <= (1 if onehot else 2)
        assert torch.equal(c["lse"][alive], ac.SCORE_HOT + cnt.double().log())
        assert bool((c["P"].sum(-1)[alive] == 1).all())
        if keypad is not None:
            assert bool((c["P"][:, :, :, :][(~live)[:, None, None, :].expand_as(c["P"])] == 0).all())
        ac.assert_exact_conditions(ac.manual(qkv, keypad, c["d_o"], B, L, H, P=c["P"], lse=c["lse"]))


@pytest.mark.parametrize("L", [17, 100, 289])
def test_closed_form_is_what_fp64_autograd_gives(L):
    """exp(-112) is not 0 in fp64, so torch.softmax is not exactly two-hot; the closed form is within 1e-30 of it everywhere"""
    B, H = 3, 2
    for names, keypad in ac.keypad_sets(B, L)[:3]:
        c = ac.twohot_case(B, L, H, 11 + L, keypad)
        m = ac.manual(c["qkv"], keypad, c["d_o"], B, L, H, P=c["P"], lse=c["lse"])
        o, lse, g = ac.ref_autograd(c["qkv"], keypad, c["d_o"], B, L, H)
        assert float((ac.merge_rows(m["o"]) - o).abs().max()) < 1e-30, names
        assert float((ac.merge_qkv(m["dq"], m["dk"], m["dv"]) - g).abs().max()) < 1e-30, names
        fin = ~torch.isinf(lse)
        assert torch.equal(torch.isinf(m["lse"]), torch.isinf(lse)) and float((m["lse"][fin] - lse[fin]).abs().max()) < 1e-12


def rand_case(B, L, H, seed, scale, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * L, 3 * H * 64, generator=g)
    qkv[:, :2 * H * 64] *= scale
    return qkv.to(dtype).float(), torch.randn(B * L, H * 64, generator=g).to(dtype).float()


@pytest.mark.parametrize("L,scale", [(33, 1.5), (200, 1.5), (200, 10.0)])
def test_manual_equals_autograd(L, scale):
    B, H = 3, 2
    for names, keypad in ac.keypad_sets(B, L):
        qkv, d_o = rand_case(B, L, H, L, scale)
        m = ac.manual(qkv, keypad, d_o, B, L, H)
        o, lse, g = ac.ref_autograd(qkv, keypad, d_o, B, L, H)
        tol = lambda r: 1e-12 * (1 + float(r.abs().max()))                                       # noqa: E731
        assert float((ac.merge_rows(m["o"]) - o).abs().max()) < tol(o), names
        assert float((ac.merge_qkv(m["dq"], m["dk"], m["dv"]) - g).abs().max()) < tol(g), names
        fin = ~torch.isinf(lse)
        assert torch.equal(torch.isinf(m["lse"]), torch.isinf(lse)) and float((m["lse"][fin] - lse[fin]).abs().max()) < 1e-10
        dead = ~ac.live_mask(keypad, B, L, "cpu").any(1)
        assert bool((m["dq"][dead] == 0).all()) and bool((m["dv"][dead] == 0).all()) and bool((m["o"][dead] == 0).all())


def test_keypad_sets():
    for B in (1, 3):
        for L in (1, 17, 64, 97, 200, 289, 513):
            sets = ac.keypad_sets(B, L)
            assert sets[0][1] is None
            seen = set()
            for names, kp in sets[1:]:
                assert kp.shape == (B, L) and kp.dtype == torch.uint8
                seen |= set(names)
                for n, row in zip(names, kp):
                    assert torch.equal(row, ac.pad_pattern(n, L, 0)) or n == "scatter"
                if B > 1:
                    assert not bool(kp.bool().all())             # "all" stands next to live videos
            fit = {n for n in ac.PATTERNS if ac.pad_pattern(n, L, 0) is not None} - ({"all"} if B == 1 else set())
            assert fit - {"none"} <= seen, (B, L, fit - seen)
    assert int((ac.pad_pattern("butlast", 200, 0) == 0).sum()) == 1
    assert bool(ac.pad_pattern("lead96", 200, 0)[:96].all()) and not bool(ac.pad_pattern("lead96", 200, 0)[96:].any())
    assert bool(ac.pad_pattern("mid128", 289, 0)[128:256].all()) and int(ac.pad_pattern("mid128", 289, 0).sum()) == 128
    assert ac.pad_pattern("lead128", 128, 0) is None and ac.pad_pattern("mid96", 192, 0) is None


def test_path_of():
    names = {(True, 1): "short", (True, 128): "short", (True, 129): "mid", (True, 288): "mid", (True, 289): "long", (False, 64): "f32"}
    for (bf, L), n in names.items():
        assert ac.path_of(bf, L)["name"] == n
    assert [ac.path_of(True, L)["nkb"] for L in (32, 33, 96, 97, 160, 161, 257, 288)] == [1, 2, 3, 4, 5, 6, 9, 9]
    assert [ac.path_of(True, L)["nch"] for L in (129, 192, 193, 288, 289, 384, 385, 513)] == [2, 2, 3, 3, 3, 3, 4, 5]
    assert ac.path_of(False, 449)["Lp"] == 512 and ac.path_of(True, 513)["Lp"] == 640


def f32_eval(qkv, keypad, d_o, B, L, H, drop_key=None, half_delta=False):
    """the attention forward and backward in plain f32 torch (the order of operations of the f32 kernels, not their tiling)"""
    q, k, v = ac.split_qkv(qkv.float(), B, L, H)
    do = ac.split_rows(d_o.float(), B, L, H)
    live = ac.live_mask(keypad, B, L, "cpu")[:, None, None, :]
    s = ((q * 0.125) @ k.transpose(-1, -2)).masked_fill(~live, -math.inf)
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    p = e / l
    if drop_key is not None:
        p = p.clone()
        p[..., drop_key] = 0
    o, lse = p @ v, (mx + l.log())[..., 0]
    delta = (do * o)[..., :32 if half_delta else 64].sum(-1, keepdim=True)
    pb = torch.exp(s - lse[..., None])
    ds = pb * (do @ v.transpose(-1, -2) - delta)
    return o, lse, (ds @ k) * 0.125, (ds.transpose(-1, -2) @ q) * 0.125, pb.transpose(-1, -2) @ do


def worst(got, ref, bound):
    return float(((got.double() - ref).abs() / bound).max())


@pytest.mark.parametrize("L,scale", [(40, 1.5), (130, 1.5), (130, 10.0)])
def test_bounds_hold_for_f32_and_catch_a_slip(L, scale):
    """a plain f32 evaluation stays inside the f32 bounds (forward; backward fed its own o and lse); dropping one key from P v, or
    half of delta's sum, does not"""
    B, H = 2, 2
    keypad = torch.stack([ac.pad_pattern("tail", L, 0), ac.pad_pattern("lead32", L, 0)])
    qkv, d_o = rand_case(B, L, H, 5 + L, scale, F32)
    m = ac.manual(qkv, keypad, d_o, B, L, H)
    pc = ac.path_of(False, L)
    b_o, b_lse = ac.fwd_bounds(m, pc)
    bq, bk, bv = ac.bwd_bounds(m, pc, b_o, b_lse)
    o, lse, dq, dk, dv = f32_eval(qkv, keypad, d_o, B, L, H)
    rs = [worst(o, m["o"], b_o), worst(lse, m["lse"], b_lse), worst(dq, m["dq"], bq), worst(dk, m["dk"], bk), worst(dv, m["dv"], bv)]
    assert max(rs) <= 1.0, rs
    o2 = f32_eval(qkv, keypad, d_o, B, L, H, drop_key=L // 2)[0]
    assert worst(o2, m["o"], b_o) > 1.0
    dq2 = f32_eval(qkv, keypad, d_o, B, L, H, half_delta=True)[2]
    assert worst(dq2, m["dq"], bq) > 1.0
