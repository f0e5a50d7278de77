"""tests/panel_cases.py on the CPU: the packer's index map is a bijection and agrees with the slot test_panel_gpu.py pins; the selector
scrambles cover every chunk, block and k step; the exact inputs are exact and their closed forms are what f32 and fp64 give; the
section C bounds hold for a plain f32 evaluation with the kernel's rounding points and fail for slightly wrong ones."""
import pytest
import torch

import panel_cases as pc

F32, F64, BF16 = pc.F32, pc.F64, pc.BF16


# ---- A
@pytest.mark.parametrize("N,K,qkv16", pc.PACK_MATRICES)
def test_pack_index_map_is_a_bijection_and_holds_the_pinned_slot(N, K, qkv16):
    TN, TK = pc.tile_format(N, K, qkv16)
    idx = pc.pack_index_map(N, K, TN, TK)
    assert idx.numel() == N * K and torch.equal(torch.sort(idx)[0], torch.arange(N * K))
    assert bool((idx.view(-1, 8)[:, 1:] - idx.view(-1, 8)[:, :-1] == 1).all())            # 16-byte runs along k
    if qkv16:       # fragment p = 23 of tile (3, 15): v (which = 2), odd head of pair 3, feature block 3; lane 45: row 13, k = 8 * 2
        t = idx.view(N // 384, K // 32, 24, 64, 8)
        assert t[3, 15, 23, 45, 0].item() == (2 * 512 + 7 * 64 + 3 * 16 + 13) * K + 15 * 32 + 16
        return
    W = pc.WAVES
    KS, RB = TK // 16, TN // (32 * W)
    tiles = idx.view(N // TN, K // TK, W, RB, KS, 64, 8)
    nb, kb, wv, rb, ks, lane = 0, (K // TK) - 1, W - 1, RB - 1, KS - 1, 45                # test_panel_gpu.py's slot
    rho = lane & 31
    row = nb * TN + wv * (TN // W) + rb * 32 + (rho & 3) + 4 * (rho >> 3) + 16 * ((rho >> 2) & 1)
    k = kb * TK + ks * 16 + 8 * (lane >> 5)
    assert torch.equal(tiles[nb, kb, wv, rb, ks, lane], row * K + k + torch.arange(8))


def test_frag_row_is_the_accumulator_layout():
    """f maps the MFMA rows a lane's 16 registers hold, (r & 3) + 8 (r >> 2) + 4 hi, onto the consecutive features 16 hi + r"""
    for hi in range(2):
        for r in range(16):
            assert pc.frag_row(torch.tensor((r & 3) + 8 * (r >> 2) + 4 * hi)).item() == 16 * hi + r


# ---- B
def test_selector_scrambles_cover_every_chunk_block_and_k_step():
    assert len(pc.SCRAMBLES) >= 3
    seen = {k: set() for k in ("fc", "proj", "out", "projT", "fcT", "outT", "inT")}
    for s in pc.SCRAMBLES:
        sel = pc.selector_weights(s)
        for name, (N, K) in (("fc", (2048, 512)), ("projT", (2048, 512))):         # c_fc phase: hidden chunk x k step of 16
            assert sel[name].shape == (N,) and int(sel[name].max()) < K
            cells = set(zip((torch.arange(N) // 256).tolist(), (sel[name] // 16).tolist()))
            assert len(cells) == 8 * 32, name                                        # every scramble alone
            seen[name] |= cells
        for name, K in (("proj", 2048), ("fcT", 2048), ("out", 512), ("outT", 512), ("inT", 1536)):     # c_proj-like: 32-feature block, k step
            assert sel[name].shape == (512,) and int(sel[name].max()) < K
            assert set((sel[name] // 16).tolist()) == set(range(K // 16)), name      # every k step (chunk x step of the c_proj phase)
            seen[name] |= set(zip((torch.arange(512) // 32).tolist(), (sel[name] // 16).tolist()))
        for name in ("out", "outT"):
            assert torch.equal(torch.sort(sel[name])[0], torch.arange(512))
    for name in ("proj", "fcT", "out", "outT", "inT"):
        assert {b for b, _ in seen[name]} == set(range(16)), name
    a, b = pc.selector_weights(0), pc.selector_weights(1)
    assert all(not torch.equal(a[k], b[k]) for k in a)
    W = pc.selector_matrix(a["fc"], 512)
    assert bool((W.float().sum(1) == 1).all()) and bool(((W == 0) | (W == 1)).all())
    assert torch.equal(W.float().argmax(1), a["fc"])


@pytest.mark.parametrize("seed,head", [(0, False), (1, True), (2, True)])
def test_exact_forward_inputs_are_exact_and_the_closed_forms_hold_in_f32_and_fp64(seed, head):
    I = pc.exact_fwd_inputs(64, seed, head=head)
    x = I["x_mid"].float()
    assert torch.equal(x.mean(1), I["c"]) and bool(((x - I["c"][:, None]).abs() == 1).all())
    assert torch.equal(x.double().mean(1), I["c"].double()) and bool(((x.double() - I["c"].double()[:, None]).square().mean(1) == 1).all())
    xn2 = pc.exact_xn2(I)
    exact = (x.double() - I["c"].double()[:, None]) * I["ln_g"].double() + I["ln_b"].double()
    assert torch.equal(xn2.double(), exact) and bool((xn2.float().abs() >= 0.5).all())
    if head:
        assert torch.equal(pc.exact_head_closed(I), I["x_mid"])
        assert torch.equal(I["x_in"].double(), I["c"].double()[:, None] - I["b_out"].double())     # c - b_out is exact in bf16
    o = pc.fwd_f32(I)                      # a plain f32 evaluation (rsqrt(1) = 1, sigmoid(>= 13.75 * 1.702) = 1)
    assert torch.equal(o["x_mid"], I["x_mid"]) and torch.equal(o["mean2"], I["c"]) and bool((o["rstd2"] == 1).all())
    assert torch.equal(o["xn2"], xn2)
    h_pre, x_out = pc.exact_fwd_closed(I, o["xn2"], o["h_act"], o["x_mid"])
    assert torch.equal(o["h_pre"], h_pre) and torch.equal(o["h_act"], h_pre) and torch.equal(o["x_out"], x_out)
    # every addition of the closed forms is exact in f32 (so fused and separate multiply-adds agree), and fp64 gives the same
    sig, tau = I["sel"]["fc"], I["sel"]["proj"]
    p64 = xn2.double()[:, sig] * 1.0 + I["b_fc"].double()
    assert torch.equal(p64, (xn2.float()[:, sig] + I["b_fc"]).double()) and torch.equal(p64.to(BF16), h_pre)
    assert bool((p64 >= 13.75).all()) and bool((1 + torch.exp2(-1.702 * 1.4426950408889634 * p64.float()) == 1).all())
    y64 = h_pre.double()[:, tau] + I["b_proj"].double()
    v64 = y64 + x.double()
    assert torch.equal(y64, (h_pre.float()[:, tau] + I["b_proj"]).double())
    assert torch.equal(v64, ((h_pre.float()[:, tau] + I["b_proj"]) + x).double()) and torch.equal(v64.to(BF16), x_out)
    ref = pc.fwd_reference(I)              # ... and the section C reference agrees with the closed forms within its (tiny) bounds
    for k in ("h_pre", "h_act", "x_out"):
        assert pc.worst_ratio(o[k], *ref[k]) <= 1.0, k


@pytest.mark.parametrize("form", ["dx", "ln1", "inp"])
def test_exact_backward_inputs_give_the_closed_forms(form):
    I = pc.bwd_inputs(64, 3, "exact", form)
    o = pc.bwd_f32(I, tail=True)
    dxp = I["dx"] if form == "dx" else o["dx_out"]
    assert torch.equal(o["dh"], dxp[:, I["sel"]["projT"]])                       # quickgelu'(16) = 1 in f32
    assert torch.equal(o["d_o"], o["dx2"][:, I["sel"]["outT"]])
    if form == "dx":
        assert torch.equal(o["g_b_fc"] - I["g0"]["g_b_fc"], I["dx"].float()[:, I["sel"]["projT"]].sum(0))
        assert bool((I["dx"].float() == I["dx"].float().round()).all())
    if form == "inp":
        dxn1 = I["dqkv"].float()[:, I["sel"]["inT"]] + I["dstage"].float()
        assert torch.equal(o["g_ln1_b"] - I["g0"]["g_ln1_b"], dxn1.sum(0)) and torch.equal(dxn1.to(BF16).float(), dxn1)
    x = torch.tensor(16.0)
    s = 1 / (1 + torch.exp2(-1.702 * 1.4426950408889634 * x))
    assert s.item() == 1.0 and ((x * 1.702) * s * (1 - s) + s).item() == 1.0


# ---- C
def test_half_ulp_and_store_bound():
    y = torch.tensor([0.0, 1.0, 1.5, 1.999, 2.0, 0.75, 3e-3], dtype=F64)
    want = torch.tensor([0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -17], dtype=F64)
    assert torch.equal(pc.half_ulp_bf16(y), want)
    v = torch.randn(100000, dtype=F64, generator=torch.Generator().manual_seed(0))
    r = pc.worst_ratio(v.float().to(BF16), v, pc.store(v, pc.U * v.abs()))
    assert 0.9 < r <= 1.0                                                          # tight: a rounding that flips the wrong way shows


FWD = [("init", False, 1e-5), ("init", True, 1e-3), ("large", False, 1e-5), ("sel", False, 1e-3), ("sel", True, 1e-5)]


@pytest.mark.parametrize("kind,head,eps", FWD)
def test_forward_bounds_hold_for_an_f32_evaluation(kind, head, eps):
    I = pc.fwd_inputs(64, 5, kind, head=head, eps=eps)
    o = pc.fwd_f32(I)
    for tag, ref in (("chained", pc.fwd_reference(I)), ("fed", pc.fwd_reference(I, o))):
        for k, (r, b) in ref.items():
            if k == "x_mid" and not head:
                continue
            assert pc.worst_ratio(o[k], r, b) <= 1.0, (tag, k, pc.worst_ratio(o[k], r, b))
    if kind == "large":
        assert o["h_pre"].float().abs().max().item() > 25


def test_forward_bounds_fail_for_slightly_wrong_evaluations():
    I = pc.fwd_inputs(64, 5, "sel", eps=1e-3)
    good = pc.fwd_f32(I)

    def worst(o, k):
        return pc.worst_ratio(o[k], *pc.fwd_reference(I, o)[k])
    assert worst(pc.fwd_f32(I, k=1.7), "h_act") > 1.0 and worst(good, "h_act") <= 1.0                 # 1.702 -> 1.7
    assert worst(pc.fwd_f32(I, drop_eps=True), "nrstd") > 1.0 and worst(good, "nrstd") <= 1.0          # eps ignored
    bad = pc.fwd_f32(I, ln_from_unrounded=True)                                                        # LN of the unrounded x_out
    assert worst(bad, "nmean") > 1.0 and worst(bad, "xn_next") > 1.0 and worst(good, "xn_next") <= 1.0
    J = dict(I)
    J["b_fc"] = I["b_fc"].clone()
    J["b_fc"][8:16] += 2.0 ** -6                                                                       # a wrong bias on 8 features
    assert pc.worst_ratio(pc.fwd_f32(J)["h_pre"], *pc.fwd_reference(I, good)["h_pre"]) > 1.0
    # (chained bounds carry every upstream bf16 rounding through K = 512 and K = 2048 as if all of them lined up: they are wide by
    # nature, which is why every case is ALSO checked stage by stage from the stored values)


BWD = [("init", "dx", True, True, 1.0), ("init", "ln1", True, True, 10.0), ("init", "inp", True, True, 1.0), ("init", "inp", False, False, 1.0),
       ("sel", "dx", True, True, 1.0), ("sel", "inp", True, False, 1.0), ("exact", "ln1", True, True, 1.0)]


@pytest.mark.parametrize("kind,form,dstage,res,hscale", BWD)
def test_backward_bounds_hold_for_an_f32_evaluation(kind, form, dstage, res, hscale):
    I = pc.bwd_inputs(64, 9, kind, form, dstage=dstage, res=res, hscale=hscale)
    o = pc.bwd_f32(I, tail=True)
    for tag, ref in (("chained", pc.bwd_reference(I, tail=True)), ("fed", pc.bwd_reference(I, o, tail=True)),
                     ("split", pc.bwd_reference(I, o, split=True))):
        assert set(ref) <= set(o)
        for k, (r, b) in ref.items():
            assert pc.worst_ratio(o[k], r, b) <= 1.0, (tag, k, pc.worst_ratio(o[k], r, b))


def test_backward_bounds_fail_for_slightly_wrong_evaluations():
    I = pc.bwd_inputs(64, 9, "sel", "inp", dstage=True, res=True)
    good = pc.bwd_f32(I)

    def worst(o, k):
        return pc.worst_ratio(o[k], *pc.bwd_reference(I, o)[k])
    assert worst(pc.bwd_f32(I, k=1.7), "dh") > 1.0 and worst(good, "dh") <= 1.0                        # 1.702 -> 1.7
    assert worst(pc.bwd_f32(I, m2_div=511.0), "dx2") > 1.0 and worst(good, "dx2") <= 1.0                # 1 / 512 -> 1 / 511
    bad = pc.bwd_f32(I, drop_row=True)                                                                 # one of 64 rows lost
    for k in ("g_b_fc", "g_ln_g", "g_ln_b", "g_b_out", "g_ln1_g", "g_ln1_b", "g_dx_colsum"):
        assert worst(bad, k) > 1.0 and worst(good, k) <= 1.0, k
    assert worst(pc.bwd_f32(I, db_times_g=True), "g_ln1_b") > 1.0
    assert worst(pc.bwd_f32(I, colsum_rounded=True), "g_b_out") > 1.0                                  # column sums of the ROUNDED dx2
    I2 = pc.bwd_inputs(64, 9, "init", "dx")
    bad = pc.bwd_f32(I2, drop_row=True)
    assert pc.worst_ratio(bad["g_b_fc"], *pc.bwd_reference(I2)["g_b_fc"]) > 1.0                        # ... chained, dense weights
    fed = pc.bwd_reference(I2, bad)
    for k in ("g_b_fc", "g_ln_g", "g_ln_b", "g_b_out"):
        assert pc.worst_ratio(bad[k], *fed[k]) > 1.0, k                                                # ... fed, dense weights
