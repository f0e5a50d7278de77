"""The loss kernels (tan_loss.hip, tan_simnce.hip) one by one, through their loss.py wrappers, against plain float64 PyTorch
references (oracle/loss_ref.py where it states the operation), at the tile boundaries and capacity limits of each kernel.
Every reference reads the values the kernel read (bf16 inputs are upcast, never regenerated).  Integer and boolean outputs are
compared exactly; each floating-point tolerance carries its reason."""
import ctypes as C
import math
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import loss_ref
from temporalalignnet_amd import _lib, loss as L

pytestmark = pytest.mark.gpu

TAU, FILL = loss_ref.TEMPERATURE, loss_ref.FILL
F64 = torch.float64
# the empty-positive-set fill of an NCE term is -6e4 + log(count) in f32: two f32 ulps at 6e4
FILL_TOL = 2 * 2.0 ** -8


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _cuda(*xs):
    return [x.cuda() for x in xs]


def _u8(x):
    return x.to(torch.uint8).contiguous().cuda()


# ------------------------------------------------------------------------------------------------------------------------------
# 1. materialised NCE: tan_nce_fwd / tan_nce_bwd through _NCEFn

nce_ref = loss_ref.nce_ref          # (the fp64 terms of loss_ref.nce over the real sentences, leaked frames filled: stated in the oracle)


def _fill_rows(tgt, tpad, row_leak, S):
    """[S,R] bool: rows whose positive set is empty (no positive among the real sentences, or a leaked frame)."""
    B, T, N = tgt.shape
    has = ((tgt != 0) & ~tpad.bool()[:, None, :]).any(-1).view(-1)
    if row_leak is not None:
        has = has & (row_leak.view(-1) == 0)
    return (~has)[None].expand(S, -1)


def _fill_cols(tgt, row_leak, S):
    B, T, N = tgt.shape
    pos = tgt != 0
    if row_leak is not None:
        pos = pos & (row_leak.view(B, T, 1) == 0)
    return (~pos.any(1)).view(-1)[None].expand(S, -1)


def check_terms(v, t, v_ref, t_ref_valid, tgt, tpad, row_leak, col_of=None, atol=2e-4):
    """Kernel terms against the fp64 reference.  v [S,R]; t [S,Mc] in the kernel's column order (col_of[j] = padded column of
    t[:, j], identity when None).  Terms with an empty positive set (no positive, or a leaked frame: those stay in the loss when
    the self-labelling marked them positive) are checked against the reference's fill -6e4 + log(#real sentences or #rows)."""
    S, R = v.shape
    B, T, N = tgt.shape
    keep = ~tpad.bool().view(-1)
    fr = _fill_rows(tgt, tpad, row_leak, S)
    dv = (v.double() - v_ref).abs()
    if (~fr).any():
        assert dv[~fr].max().item() <= atol, dv[~fr].max().item()
    if fr.any():
        assert dv[fr].max().item() <= FILL_TOL, dv[fr].max().item()
        assert (v[fr] > 5e4).all()
    # columns: back to the padded order, real sentences only
    t_full = torch.full((S, B * N), float("nan"), dtype=F64, device=v.device)
    t_full[:, keep] = t_ref_valid
    if col_of is None:
        col_of = torch.arange(t.shape[1], device=v.device)
    ref_c = t_full[:, col_of]
    real = keep[col_of]
    fc = _fill_cols(tgt, row_leak, S)[:, col_of] & real[None]
    dt = (t.double() - ref_c).abs()
    ok = real[None] & ~fc
    if ok.any():
        assert dt[ok].max().item() <= atol, dt[ok].max().item()
    if fc.any():
        assert dt[fc].max().item() <= FILL_TOL, dt[fc].max().item()


def _nce_case(S, B, T, N, seed, leak, pad, neg_rows=True):
    g = _gen(seed)
    R, Mp = B * T, B * N
    lg = torch.rand(S, R, Mp, generator=g) * 2 - 1
    tgt = (torch.rand(B, T, N, generator=g) < 0.2).float()
    tpad = torch.zeros(B, N, dtype=torch.bool)
    if pad and N > 1:
        for b in range(B):
            tpad[b, torch.randint(1, N + 1, (1,), generator=g).item():] = True
        tpad[B - 1, 1:] = True                                   # a video whose sentences are all padded except one
    tgt = tgt * (~tpad)[:, None, :].float()
    tgt[:, :, N // 2] = 0                                        # a sentence column without a positive
    tgt[:, T // 3, :] = 0                                        # frames without a positive
    if neg_rows:
        lg[:, torch.arange(0, R, 7)] = -1.0                      # rows at logit -1 throughout
        lg[:, -2] = -1.0                                         # (the last row stays random: a chunk that re-read it would show)
    row_leak = None
    if leak:
        row_leak = torch.zeros(R, dtype=torch.uint8)
        row_leak[T - 2:T] = 1
        row_leak[R - 3:] = 1
        row_leak[R // 2] = 1
    return lg, tgt, tpad, row_leak


def _ctx():
    return types.SimpleNamespace()


@pytest.mark.parametrize("S,B,T,N,leak,pad", [
    (1, 1, 9, 5, False, False),          # R < 16: one partial wave
    (6, 3, 37, 7, True, True),           # R = 111: last 64-row chunk 47 rows, its third wave 15
    (2, 5, 100, 9, False, True),
    (1, 4, 23, 31, True, True),
    (2, 64, 3, 256, True, False),        # Mp = 16384 (the LDS column accumulators' limit); S*R*Mp = 6.3 M: 3 grid-stride passes
])
def test_materialised_nce_matches_fp64(S, B, T, N, leak, pad):
    lg, tgt, tpad, row_leak = _nce_case(S, B, T, N, 100 + S * 7 + N, leak, pad)
    R, Mp = B * T, B * N
    g = _gen(7 + N)
    g_v = torch.randn(S, R, generator=g)
    g_t = torch.randn(S, Mp, generator=g) * (~tpad).view(1, -1).float()       # padded columns are not terms of the loss
    lg, tgt, g_v, g_t = _cuda(lg, tgt, g_v, g_t)
    tp = tpad.cuda()
    ci = _u8(tpad.view(-1))
    rl = _u8(row_leak) if leak else None
    # the wrapper's forward / backward, driven by hand to reach the saved sums (for the bf16 d-logits launch below)
    ctx = _ctx()
    v, t = L._NCEFn.forward(ctx, lg, tgt, ci, rl, B, T, N)
    dl = L._NCEFn.backward(ctx, g_v, g_t)[0]
    lg64 = lg.double().requires_grad_(True)
    v_ref, t_ref = nce_ref(lg64, tgt, tp, rl)
    check_terms(v, t, v_ref.detach(), t_ref.detach(), tgt, tp, rl)
    # d logits: fp64 autograd of sum(g_v v) + sum(g_t t) through the same (leaked) reference; rows / columns with an empty
    # positive set have a constant positive term there, and the kernel's gradient of it is zero as well
    keep = ~tp.view(-1)
    (v_ref * g_v.double()).sum().add((t_ref * g_t.double()[:, keep]).sum()).backward()
    want = lg64.grad
    scale = want.abs().max().item()
    # f32 exp of arguments up to 2/0.07 (~2e-6 relative) and sums of <= 16384 of them: 1e-4 relative per element
    err = (dl.double() - want).abs()
    assert (err <= 1e-4 * want.abs() + 1e-6 * scale).all(), (err / (want.abs() + 1e-6 * scale)).max().item()
    # out_dtype = TAN_BF16 (the fused path's d-logits format): the same values at bf16 rounding (half an ulp: <= 2^-8 relative)
    lg_s, tgt_s, ci_s, rl_s, rowsum, colsum, possum_v, possum_t = ctx.saved
    dl16 = torch.empty(S, R, Mp, dtype=torch.bfloat16, device="cuda")
    _lib.check(_lib.lib().tan_nce_bwd(L._p(lg), L._p(tgt), L._p(ci), L._p(rl), L._p(rowsum), L._p(colsum), L._p(possum_v),
                                      L._p(possum_t), L._p(g_v), L._p(g_t), L._p(dl16), _lib.TAN_BF16, C.c_int(S), C.c_int(B),
                                      C.c_int(T), C.c_int(N), L.ops._stream()), "tan_nce_bwd")
    err16 = (dl16.double() - want).abs()
    assert (err16 <= (2.0 ** -8 + 1e-4) * want.abs() + 1e-6 * scale).all(), (err16 / (want.abs() + 1e-6 * scale)).max().item()


def test_materialised_nce_rejects_more_columns_than_its_lds_holds():
    B, T, N = 1, 2, 16385
    lg = torch.zeros(1, B * T, B * N, device="cuda")
    tgt = torch.zeros(B, T, N, device="cuda")
    ci = torch.zeros(B * N, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.TanHipError):
        L._NCEFn.forward(_ctx(), lg, tgt, ci, None, B, T, N)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. fused similarity + NCE: _FusedNCEFn (tan_simnce_fwd, tan_simnce_bwd with and without e_keep / d_vn + the d-feature GEMMs)

class _NoKeep:
    """The library with tan_simnce_keeps() answering 0: the forward keeps no exponentials, the backward recomputes them."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, k):
        return (lambda *a: 0) if k == "tan_simnce_keeps" else getattr(self._lib, k)


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("S,B,T,N,shared,compact,leak", [
    # (Cw = 512 always takes the resident sweep, res_enabled(); the 2048-column simnce_kernel of other channel counts is not reached)
    (2, 5, 27, 7, False, False, True),       # Mc = 35 (not a multiple of 8: d-logits pass + GEMM); R = 135
    (1, 64, 3, 32, True, False, False),      # Mc = 2048, N = 32: one-pass backward
    (1, 257, 2, 8, False, False, True),      # Mc = 2056: more columns than the non-resident sweep's 2048; R = 514
    (1, 256, 2, 32, True, False, False),     # Mc = 8192 = S_MAXCOLS_RES, the resident sweep's limit
    (2, 12, 20, 32, False, True, True),      # N = 32, compacted
    (2, 12, 20, 33, True, True, False),      # N = 33: past the one-pass backward's limit, compacted
    (1, 264, 2, 33, False, True, False),     # 8712 padded columns compacted to Mc = 8192
])
def test_fused_nce_matches_fp64(S, B, T, N, shared, compact, leak, keep):
    R, Mp, Cw = B * T, B * N, 512
    lim = _lib.lib().tan_simnce_max_cols()
    g = _gen(2000 + S * 31 + B + N)
    tpad = torch.zeros(B, N, dtype=torch.bool)
    if compact:
        if Mp > 4096:
            tpad[:, N - 2:] = True                               # 8712 - 528 real sentences: Mc = 8192
        else:
            tpad[::3, 1:] = True                                 # every third video keeps one sentence
            tpad[1, N - 3:] = True
    n_valid = int((~tpad).sum())
    prep = L.compaction_prep(_u8(tpad.view(-1)), n_valid) if compact else None
    Mc = prep[0].shape[0] if prep is not None else Mp
    if compact:
        assert Mc < Mp
    assert Mc <= lim == 8192                                     # (resident sweep at Cw = 512)
    vn = F.normalize(torch.randn(S, R, Cw, generator=g), dim=-1).bfloat16()
    tn = F.normalize(torch.randn(1 if shared else S, Mp, Cw, generator=g), dim=-1).bfloat16()
    tgt = (torch.rand(B, T, N, generator=g) < 0.15).float() * (~tpad)[:, None, :].float()
    tgt[:, :, 0] = 0
    row_leak = None
    if leak:
        row_leak = torch.zeros(R, dtype=torch.uint8)
        row_leak[T - 2:T] = 1
        row_leak[R - 3:] = 1
    g_v = torch.randn(S, R, generator=g)
    g_t = torch.randn(S, Mp, generator=g) * (~tpad).view(1, -1).float()
    vn, tn, tgt, g_v, g_t = _cuda(vn, tn, tgt, g_v, g_t)
    tp = tpad.cuda()
    ci = _u8(tpad.view(-1))
    rl = _u8(row_leak) if leak else None
    col_of = prep[0] if prep is not None else None
    g_t_run = g_t[:, col_of] if col_of is not None else g_t

    real = _lib.lib
    if not keep:
        proxy = _NoKeep(real())
        _lib.lib = lambda: proxy
    try:
        v = vn.clone().requires_grad_(True)
        t = tn.clone().requires_grad_(True)
        v_terms, t_terms = L._FusedNCEFn.apply(v, t, tgt, ci, rl, B, T, N, prep)
        assert t_terms.shape == (S, Mc)
        (v_terms * g_v).sum().add((t_terms * g_t_run).sum()).backward()
    finally:
        _lib.lib = real

    vn64 = vn.double().requires_grad_(True)
    tn64 = tn.double().requires_grad_(True)
    lg64 = torch.einsum("src,smc->srm", vn64, tn64.expand(S, -1, -1))
    v_ref, t_ref = nce_ref(lg64, tgt, tp, rl)
    # logits: f32 MFMA sums of 512 bf16 products (<= 512 * 2^-24 of a cosine) scaled by 1/0.07
    check_terms(v_terms.detach(), t_terms.detach(), v_ref.detach(), t_ref.detach(), tgt, tp, rl, col_of=col_of, atol=1e-3)
    keepc = ~tp.view(-1)
    (v_ref * g_v.double()).sum().add((t_ref * g_t.double()[:, keepc]).sum()).backward()
    # d logits are bf16 (2^-9), so are the kept exponentials and the returned feature gradients: three 2^-9 roundings
    bound = 3 * 2.0 ** -9
    for got, want in ((v.grad, vn64.grad), (t.grad, tn64.grad)):
        assert torch.isfinite(got).all()
        rel = (got.double() - want).norm().item() / want.norm().item()
        assert rel <= bound, rel
    if compact:                                  # dropped (padded) sentences take part in nothing: exactly zero gradient
        assert (t.grad[:, tp.view(-1)] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. self-labelling: tan_selflabel, tan_diag_max

def selflabel_ref(z, vpad, tpad, dur):
    """fp64 loss_ref.self_label of the raw same-video cosines z [B,T,N]."""
    bank = loss_ref.window_bank(dur.to(F64), z.shape[1])
    return loss_ref.self_label((z.to(F64) / TAU)[:, None], vpad.bool(), tpad.bool(), bank), bank


def check_selflabel(got, ref, bank, z, vpad, tpad):
    B, N, T = ref["scan"].shape
    scan = ref["scan"]
    top2 = scan.topk(min(2, T), dim=-1).values
    top1 = top2[..., 0]
    # p1 = softmax over texts carries ~2e-6 relative f32 error; /0.07 makes that ~3e-5 absolute in the exponent of the time
    # softmax, so the scan is good to ~1e-4 of its maximum
    margin = 1e-4 * top1.abs().clamp(min=1e-30)
    pos = got["max_pos"].long()
    sep = (top2[..., 0] - top2[..., -1] > margin) if T > 1 else torch.ones_like(top1, dtype=torch.bool)
    assert torch.equal(pos[sep], ref["max_pos"][sep]), (pos[sep] != ref["max_pos"][sep]).nonzero()[:8]
    picked = scan.gather(-1, pos[..., None])[..., 0]
    assert (picked >= top1 - margin).all()
    assert (pos >= 0).all() and (pos < T).all()
    # the window of the kernel's own pick
    w = bank.gather(2, pos[:, :, None, None].expand(-1, -1, 1, T))[:, :, 0]                  # [B,N,T]
    assert torch.equal(got["tgt"].bool(), w > 0)
    assert ((got["max_prob"].double() - picked).abs() <= margin).all()
    zm = (z.to(F64) / TAU).masked_fill(vpad.bool()[:, :, None], FILL).masked_fill(tpad.bool()[:, None, :], FILL)
    ml = (zm.permute(0, 2, 1) * w).sum(-1)
    # a window mean of <= T f32 terms of magnitude <= 6e4 (padded frames) or 1/0.07
    wabs = (zm.abs().permute(0, 2, 1) * w).sum(-1)
    assert ((got["max_logit"].double() - ml).abs() <= 3e-5 * wabs + 1e-6).all()


def _sl_case(B, T, N, seed):
    g = _gen(seed)
    z = torch.rand(B, T, N, generator=g) * 2 - 1
    dur = torch.randint(1, T + 1, (B, N), generator=g).float()
    specials = [1.0, 2.0, float(T - 1), float(T)]
    for k in range(min(N, 4)):
        dur[0, k] = max(specials[k], 1.0)
    tpad = torch.rand(B, N, generator=g) < 0.2
    tpad[0, :min(N, 4)] = False
    if B > 1:
        tpad[B - 1] = True                                # a video with every sentence padded
    if N > 1:
        tpad[0, N - 1] = True
    dur = dur.masked_fill(tpad, 0.0)
    vpad = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        vpad[b, T - (b * 5) % max(T // 2, 1):] = b > 0    # video-padding tails
    return z, vpad, tpad, dur


@pytest.mark.parametrize("B,T,N", [(2, 256, 32), (2, 64, 128), (3, 37, 1), (2, 300, 5), (4, 100, 9)])
def test_selflabel_matches_fp64_on_compact_blocks(B, T, N):
    z, vpad, tpad, dur = _cuda(*_sl_case(B, T, N, 300 + T + N))
    got = L._selflabel(L._Blocks.of_diag(z), _u8(vpad), _u8(tpad), dur, B, T, N)
    ref, bank = selflabel_ref(z, vpad, tpad, dur)
    check_selflabel(got, ref, bank, z, vpad, tpad)


@pytest.mark.parametrize("S,B,T,N", [(3, 3, 70, 6), (2, 2, 130, 17)])
def test_selflabel_and_diag_max_read_the_last_stage_of_stage_major_logits(S, B, T, N):
    """_Blocks.of_logits: the last stage's same-video blocks of a [S, R, Mp] tensor (block stride T*Mp + N, row stride Mp)."""
    z, vpad, tpad, dur = _sl_case(B, T, N, 400 + T)
    g = _gen(5)
    lg = torch.rand(S, B * T, B * N, generator=g) * 2 - 1
    for b in range(B):
        lg[S - 1, b * T:(b + 1) * T, b * N:(b + 1) * N] = z[b]
    lg, z, vpad, tpad, dur = _cuda(lg, z, vpad, tpad, dur)
    blk = L._Blocks.of_logits(lg, B, T, N)
    got = L._selflabel(blk, _u8(vpad), _u8(tpad), dur, B, T, N)
    ref, bank = selflabel_ref(z, vpad, tpad, dur)
    check_selflabel(got, ref, bank, z, vpad, tpad)
    for leak in (None, _u8(vpad.view(-1))):
        md = L._diag_max(blk, leak, B, T, N).view(B, N)
        x = z.to(F64) / TAU
        if leak is not None:
            x = x.masked_fill(vpad[:, :, None], FILL)
        want = x.max(1).values
        assert ((md.double() - want).abs() <= 2.0 ** -23 * want.abs()).all()   # one f32 division, correctly rounded


@pytest.mark.parametrize("B,T,N", [(2, 256, 32), (3, 37, 1)])
def test_diag_max_matches_fp64_on_compact_blocks(B, T, N):
    z, vpad, tpad, dur = _cuda(*_sl_case(B, T, N, 500 + T))
    for leak in (None, _u8(vpad.view(-1))):
        md = L._diag_max(L._Blocks.of_diag(z), leak, B, T, N).view(B, N)
        x = z.to(F64) / TAU
        if leak is not None:
            x = x.masked_fill(vpad[:, :, None], FILL)
        want = x.max(1).values
        assert ((md.double() - want).abs() <= 2.0 ** -23 * want.abs()).all()   # one f32 division, correctly rounded


def test_selflabel_exact_ties_go_to_the_first_window():
    """Scan values that tie exactly in f32 and in fp64: a plateau of identical frames read through windows of 1 or 2 members (each a
    power of two, so the window mean of equal values is exact).  Tied starts 5, 69 and 133 sit in the same lane of the wave's
    64-way stride; the first maximal start, 5, must win (torch.max's first index)."""
    B, T, N = 1, 200, 2
    z = torch.full((B, T, N), 0.0)
    high = torch.zeros(T, dtype=torch.bool)
    for a, b in ((5, 11), (69, 75), (133, 141)):
        high[a:b] = True
    z[0, :, 0] = torch.where(high, torch.tensor(0.9), torch.tensor(0.2))
    z[0, :, 1] = torch.where(high, torch.tensor(-0.9), torch.tensor(0.1))      # text 1 peaks on the low frames
    dur = torch.tensor([[2.0, 1.0]])
    vpad = torch.zeros(B, T, dtype=torch.bool)
    tpad = torch.zeros(B, N, dtype=torch.bool)
    z, dur, vpad, tpad = _cuda(z, dur, vpad, tpad)
    got = L._selflabel(L._Blocks.of_diag(z), _u8(vpad), _u8(tpad), dur, B, T, N)
    ref, bank = selflabel_ref(z, vpad, tpad, dur)
    scan = ref["scan"][0, 0]
    assert ref["max_pos"][0, 0].item() == 5 and scan[5] == scan[69] == scan[133] == scan.max()
    assert got["max_pos"][0, 0].item() == 5
    # text 1 (one-frame windows): ties on every low frame; the first, 1, shares lane 1 with the tied starts 65 and 129
    assert ref["max_pos"][0, 1].item() == 1
    assert ref["scan"][0, 1, 1] == ref["scan"][0, 1, 65] == ref["scan"][0, 1, 129] == ref["scan"][0, 1].max()
    assert got["max_pos"][0, 1].item() == 1
    check_selflabel(got, ref, bank, z, vpad, tpad)


def test_selflabel_rejects_blocks_larger_than_its_lds():
    B, T, N = 1, 2731, 3                                   # T*N = 8193: two f32 [T,N] planes are 64 KiB + 24 B
    z = torch.zeros(B, T, N, device="cuda")
    dur = torch.ones(B, N, device="cuda")
    with pytest.raises(_lib.TanHipError):
        L._selflabel(L._Blocks.of_diag(z), _u8(torch.zeros(B, T)), _u8(torch.zeros(B, N)), dur, B, T, N)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. agreement, masked quantile, stage-2 statistics

def _agreement(jt, dt, yt, ml_j, ml_d, q_j, q_d, kind, B, T, N):
    tgt = torch.empty(B, T, N, device="cuda")
    iou = torch.empty(B, N, device="cuda")
    conf = torch.empty(B, N, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().tan_agreement(L._p(jt), L._p(dt), L._p(yt), L._p(ml_j), L._p(ml_d), L._p(q_j), L._p(q_d),
                                        C.c_int(L._KIND[kind]), L._p(tgt), L._p(iou), L._p(conf), C.c_int(B), C.c_int(T),
                                        C.c_int(N), L.ops._stream()), "tan_agreement")
    return tgt, iou, conf


def _windows(g, B, N, T):
    start = torch.randint(0, T, (B, N), generator=g)
    length = torch.randint(1, max(2, T // 4), (B, N), generator=g)
    t = torch.arange(T)
    return (t >= start[..., None]) & (t < (start + length)[..., None]), start, length


@pytest.mark.parametrize("kind", ["i", "u", "keep", "keep-joint"])
@pytest.mark.parametrize("B,T,N", [(3, 512, 64), (4, 77, 9)])
def test_agreement_matches_the_reference_exactly(kind, B, T, N):
    g = _gen(600 + T + N)
    jt, js, jl = _windows(g, B, N, T)
    dt, _, _ = _windows(g, B, N, T)
    yt, _, _ = _windows(g, B, N, T)
    t = torch.arange(T)
    # IoU exactly 0.5 (the dual window is the first half of an even-length joint window), exactly 1, and 0
    for n in range(0, N, 3):
        ln = 2 * max(1, (jl[0, n].item() + 1) // 2)
        s0 = min(js[0, n].item(), T - ln)
        jt[0, n] = (t >= s0) & (t < s0 + ln)
        dt[0, n] = (t >= s0) & (t < s0 + ln // 2)
    dt[1, :N // 2] = jt[1, :N // 2]
    # a later sentence whose whole agreed window an earlier one covers: de-duplicated away, it falls back to the YouTube target
    jt[2 % B, 1] = jt[2 % B, 0]
    dt[2 % B, 1] = dt[2 % B, 0]
    # frames where no sentence agrees: the last video's second half
    jt[B - 1, :, T // 2:] = False
    dt[B - 1, :, T // 2:] = False
    tpad = torch.zeros(B, N, dtype=torch.bool)
    tpad[B - 1, N - 2:] = True
    for x in (jt, dt, yt):
        x[tpad] = False
    ml_j = torch.randn(B, N, generator=g)
    ml_d = torch.randn(B, N, generator=g)
    q_j, q_d = torch.tensor([0.1]), torch.tensor([-0.2])
    ml_j[0, :4] = q_j                                       # at the quantile: confident (>=)
    ml_d[0, 2:6] = q_d
    jt, dt, yt, ml_j, ml_d, q_j, q_d = _cuda(jt, dt, yt, ml_j, ml_d, q_j, q_d)
    got_tgt, got_iou, got_conf = _agreement(_u8(jt), _u8(dt), _u8(yt), ml_j, ml_d, q_j, q_d, kind, B, T, N)
    dedup, iou, conf = loss_ref.agreement(jt, dt, yt, ml_d >= q_d, ml_j >= q_j, kind)
    assert (iou == 0.5).any() and (iou == 1).any()
    assert torch.equal(got_iou, iou)
    assert torch.equal(got_conf.bool(), conf)
    assert torch.equal(got_tgt, dedup.permute(0, 2, 1))
    if kind in ("keep", "keep-joint"):
        assert (dedup[2 % B, 1] == yt[2 % B, 1].float()).all() and yt[2 % B, 1].any()


def test_agreement_rejects_more_than_64_sentences():
    B, T, N = 1, 8, 65
    u = torch.zeros(B, N, T, dtype=torch.uint8, device="cuda")
    f = torch.zeros(B, N, device="cuda")
    q = torch.zeros(1, device="cuda")
    with pytest.raises(_lib.TanHipError):
        _agreement(u, u, u, f, f, q, q, "keep", B, T, N)


def quantile_f32(x, q):
    """torch.quantile(x, q) ('linear') of f32 values, spelled out in f32 with at::lerp's two-sided formula and no fused
    multiply-add (what the kernels compute; torch's own lerp may contract to an fma and differ in the last bit)."""
    v = x.float().sort().values
    m = v.numel()
    if m == 0:
        return torch.tensor(float("nan"))
    rank = torch.tensor(q, dtype=torch.float32) * torch.tensor(float(m - 1), dtype=torch.float32)
    lo = torch.floor(rank)
    il = int(lo.item())
    ih = min(il + 1, m - 1)
    w = rank - lo
    a, b = v[il], v[ih]
    return a + w * (b - a) if w.item() < 0.5 else b - (b - a) * (1 - w)


def _same(a, b):
    """NaN-aware equality of two f32 scalars."""
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or a == b


def _check_quantile(got, x_valid, q):
    want = quantile_f32(x_valid, q)
    assert _same(got, want), (got, want.item())
    tq = torch.quantile(x_valid.float(), q).item() if x_valid.numel() else float("nan")
    assert _same(got, tq) or abs(got - tq) <= 2.0 ** -23 * abs(tq), (got, tq)     # torch's lerp: at most an fma apart


@pytest.mark.parametrize("n", [4095, 4096, 8192])
def test_masked_quantile_matches_torch_at_its_sort_limits(n):
    g = _gen(700 + n)
    cases = []
    cases.append((torch.randn(n, generator=g), torch.rand(n, generator=g) < 0.3))
    ties = torch.tensor([-1.0, -0.0, 0.0, 0.0, 1.0, 2.5])[torch.randint(0, 6, (n,), generator=g)]
    cases.append((ties, torch.rand(n, generator=g) < 0.1))                    # heavy ties, +-0.0
    one = torch.ones(n, dtype=torch.bool)
    one[n // 2] = False
    cases.append((torch.randn(n, generator=g), one))                          # a single valid entry
    cases.append((torch.randn(n, generator=g), torch.ones(n, dtype=torch.bool)))   # nothing valid: NaN
    cases.append((torch.randn(n, generator=g), torch.zeros(n, dtype=torch.bool)))
    for x, inv in cases:
        xc, ic = x.cuda(), _u8(inv)
        for q in (0.0, 0.3, 0.5, 0.77, 1.0):
            got = L._quantile(xc, ic, q).item()
            _check_quantile(got, x[~inv], q)


def test_masked_quantile_rejects_more_than_8192_entries():
    x = torch.zeros(8193, device="cuda")
    with pytest.raises(_lib.TanHipError):
        L._quantile(x, _u8(torch.zeros(8193)), 0.5)


def _s2_inputs(B, T, N, seed):
    g = _gen(seed)
    Mp = B * N
    vals = torch.tensor([-3.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0])
    md = torch.where(torch.rand(Mp, generator=g) < 0.6, vals[torch.randint(0, 7, (Mp,), generator=g)], torch.randn(Mp, generator=g))
    mj = torch.where(torch.rand(Mp, generator=g) < 0.6, vals[torch.randint(0, 7, (Mp,), generator=g)], torch.randn(Mp, generator=g) * 3)
    tpad = torch.rand(B, N, generator=g) < 0.15
    if Mp <= 2:
        tpad[:] = False
    tgt = (torch.rand(B, T, N, generator=g) < 0.3).float()
    pos = (torch.randint(0, 65, (B, N, 2), generator=g).float() / 64).sort(-1).values    # on a 1/64 grid: exact centres
    conf = (torch.rand(B, N, generator=g) < 0.5).to(torch.uint8)
    return md, mj, tpad, tgt, pos, conf


@pytest.mark.filterwarnings("ignore:std\\(\\). degrees of freedom")  # one real sentence: 0/0, as in the reference
@pytest.mark.parametrize("use_align,with_pos", [(True, True), (True, False), (False, False)])
@pytest.mark.parametrize("B,T,N", [(64, 2, 128), (1, 3, 1), (1, 4, 2), (2, 5, 1)])
def test_stage2_masks_match_fp64(B, T, N, use_align, with_pos):
    Mp = B * N
    md, mj, tpad, tgt, pos, conf = _s2_inputs(B, T, N, 800 + Mp)
    q_th = 0.5
    md, mj, tgt, pos, conf = _cuda(md, mj, tgt, pos, conf)
    tp = tpad.cuda()
    s2 = L.stage2_masks(md, mj, _u8(tpad), tgt, pos if with_pos else None, conf, q_th, use_align, B, T, N)
    scal = s2["scal"].cpu()
    valid = ~tp.view(-1)
    M = int(valid.sum())
    # the radix select: threshold and medians are the quantiles of the kernel's own metric / of md, mj (NaN-aware: with one real
    # sentence the standard deviation is 0/0, as in the reference)
    _check_quantile(scal[5].item(), s2["metric"][valid].cpu(), q_th)
    if use_align:
        _check_quantile(scal[6].item(), md[valid].cpu(), 0.5)
        _check_quantile(scal[7].item(), mj[valid].cpu(), 0.5)
    # metric: fp64 z-scores over the real sentences (f32 sums over <= 8192 sentences: ~1e-5 relative)
    md64, mj64 = md.double(), mj.double()
    metric = loss_ref.threshold_metric(md64[valid], mj64[valid])
    got_metric = s2["metric"][valid].double()
    if M > 1:
        assert ((got_metric - metric).abs() <= 1e-5 * (1 + metric.abs())).all()
    else:
        assert torch.isnan(got_metric).all() and torch.isnan(metric).all()
    th = torch.quantile(metric, q_th) if M > 1 else torch.tensor(float("nan"), dtype=F64)
    thm = s2["th_mask"].view(-1)
    assert not thm[~valid].any()
    # ties included: the kept mask is `metric <= threshold` over the kernel's own metric and (exact) threshold
    assert torch.equal(thm, (s2["metric"] <= scal[5].item()) & valid)
    ref_mask = metric <= th
    clear = (metric - th).abs() > 1e-5 * (1 + th.abs())                  # not within rounding of the threshold
    assert torch.equal(thm[valid][clear], ref_mask[clear])
    assert torch.equal(s2["th_f"], thm.float())
    rows = ((tgt * valid.view(B, 1, N).float() * s2["th_f"].view(B, 1, N)).sum(-1) > 0).view(-1).float()
    assert torch.equal(s2["rows"], rows)
    assert abs(scal[3].item() - (conf.view(-1).double()[valid].sum() / M).item()) <= 2.0 ** -23
    assert scal[4].item() == M
    if not use_align:
        return
    # labels: the reference decisions wherever md, mj are not within f32 rounding of their medians
    med_d = torch.quantile(md64[valid], 0.5)
    med_j = torch.quantile(mj64[valid], 0.5)
    centre = pos.double().view(Mp, 2).mean(-1)[valid] if with_pos else None
    lab_ref = loss_ref.alignability_labels(md64[valid], mj64[valid], med_d, med_j, centre)
    lab = s2["lab"]
    assert torch.isnan(lab[~valid]).all()
    # ties included: strict comparisons with the kernel's (exact) medians, and the centre test in f32
    md_k, mj_k = md[valid], mj[valid]
    if M > 2:
        assert ((md_k == scal[6].item()) | (mj_k == scal[7].item())).any()    # the heavy ties do sit on the medians
    centre_k = ((pos[..., 0] + pos[..., 1]) / 2).view(Mp)[valid] if with_pos else None
    lab_k = loss_ref.alignability_labels(md_k, mj_k, md_k.new_tensor(scal[6].item()), mj_k.new_tensor(scal[7].item()), centre_k)
    assert torch.equal(lab[valid], lab_k)
    near = ((md64[valid] - med_d).abs() <= 2.0 ** -22 * med_d.abs()) | ((mj64[valid] - med_j).abs() <= 2.0 ** -22 * med_j.abs())
    if with_pos:
        near &= (centre >= 0.2) & (centre <= 0.8)
    assert torch.equal(lab[valid][~near].double(), lab_ref[~near])
    sel = ((lab != 2) & valid).float()
    assert torch.equal(s2["sel"], sel) and torch.equal(s2["y"], torch.nan_to_num(lab) * sel)
    n_sel, n_pos = sel.double().sum().item(), (torch.nan_to_num(lab) * sel).double().sum().item()
    assert scal[0].item() == n_sel and scal[1].item() == n_pos
    pw = n_sel / n_pos - 1.0 if n_pos else (float("inf") if n_sel else float("nan"))
    assert _same(scal[2].item(), pw) or abs(scal[2].item() - pw) <= 2.0 ** -22 * abs(pw)   # one f32 division and subtraction


# ------------------------------------------------------------------------------------------------------------------------------
# 5. NCE tail, positive masks, alignability BCE

def _tail_ref(v_d, t_d, v_j, t_j, rm, cm, counts=None):
    nr, nc = (rm.sum(), cm.sum()) if counts is None else (counts[0], counts[1])
    Sd, Sj = v_d.shape[0], v_j.shape[0]
    ld = ((v_d * rm).sum() / (Sd * nr) + (t_d * cm).sum() / (Sd * nc)) / 2
    lj = ((v_j * rm).sum() / (Sj * nr) + (t_j * cm).sum() / (Sj * nc)) / 2
    return ld, lj, (ld + lj) / 2


@pytest.mark.parametrize("R,M,Sd,Sj", [(1, 1, 1, 1), (1023, 4097, 6, 3), (8192, 8193, 2, 2), (8193, 8192, 3, 6),
                                       (3 * 8192 + 5, 7, 2, 1)])
@pytest.mark.parametrize("global_counts", [False, True])
def test_nce_tail_matches_fp64(R, M, Sd, Sj, global_counts):
    g = _gen(900 + R + M)
    v_d, v_j = torch.rand(Sd, R, generator=g) * 10, torch.rand(Sj, R, generator=g) * 10
    t_d, t_j = torch.rand(Sd, M, generator=g) * 10, torch.rand(Sj, M, generator=g) * 10
    rm = (torch.rand(R, generator=g) < 0.6).float()
    cm = (torch.rand(M, generator=g) < 0.6).float()
    rm[-1] = 1.0; cm[-1] = 1.0                                   # the last row / column (past 8192: a second unrolled pass)
    if R > 8192:
        rm[8192] = 1.0
    v_d, v_j, t_d, t_j, rm, cm = _cuda(v_d, v_j, t_d, t_j, rm, cm)
    counts = torch.stack([rm.sum() + 5, cm.sum() + 3]) if global_counts else None
    ins = [x.clone().requires_grad_(True) for x in (v_d, t_d, v_j, t_j)]
    out = L._NCETail.apply(*ins, rm, cm, counts)
    ref_ins = [x.double().requires_grad_(True) for x in (v_d, t_d, v_j, t_j)]
    ref = _tail_ref(*ref_ins, rm.double(), cm.double(), None if counts is None else counts.double())
    # f32 sums of <= 150 k positive terms (per-thread partials, then a 1024-way tree): ~1e-6 relative
    for a, b in zip(out, ref):
        assert abs(a.item() - b.item()) <= 1e-5 * abs(b.item()), (a.item(), b.item())
    gs = torch.randn(3, generator=g)
    sum(o * gi.item() for o, gi in zip(out, gs)).backward()
    sum(o * gi.item() for o, gi in zip(ref, gs)).backward()
    for a, b in zip(ins, ref_ins):                              # a few f32 products and quotients per element
        assert ((a.grad.double() - b.grad).abs() <= 1e-6 * b.grad.abs().max()).all()
    # nce_term_grads: the gradient of the mean alone, from the masks
    gvd, gtd, gvj, gtj, cnt = L.nce_term_grads(rm, cm, Sd, Sj)
    for x in ref_ins:
        x.grad = None
    _tail_ref(*ref_ins, rm.double(), cm.double())[2].backward()          # (local counts: what nce_term_grads divides by)
    for a, b in zip((gvd, gtd, gvj, gtj), ref_ins):
        assert ((a.double() - b.grad).abs() <= 1e-6 * b.grad.abs().max()).all()
    assert torch.equal(cnt, torch.stack([rm.sum(), cm.sum()]))


def test_nce_tail_of_empty_masks_is_nan():
    """Masked means over nothing: 0/0 = NaN, like the reference's empty .mean()."""
    Sd, Sj, R, M = 2, 3, 100, 40
    v_d, v_j = torch.rand(Sd, R, device="cuda"), torch.rand(Sj, R, device="cuda")
    t_d, t_j = torch.rand(Sd, M, device="cuda"), torch.rand(Sj, M, device="cuda")
    for rm, cm in ((torch.zeros(R), torch.ones(M)), (torch.ones(R), torch.zeros(M))):
        rm, cm = rm.cuda(), cm.cuda()
        out = L._NCETail.apply(v_d, t_d, v_j, t_j, rm, cm, None)
        ref = (v_d[:, rm.bool()].mean() + t_d[:, cm.bool()].mean()) / 2
        assert torch.isnan(ref) and all(torch.isnan(o).item() for o in out)


@pytest.mark.parametrize("B,T,N", [(1, 1, 1), (3, 300, 260), (5, 17, 9)])
def test_pos_masks_match_the_torch_statement(B, T, N):
    g = _gen(1000 + T)
    tgt = (torch.rand(B, T, N, generator=g) < 0.02).float()
    tgt[0, :, 0] = 1.0
    tpad = torch.rand(B, N, generator=g) < 0.3
    tgt, tpad = _cuda(tgt, tpad)
    rows, cols = L._pos_masks(tgt, _u8(tpad), B, T, N)
    assert torch.equal(rows, ((tgt != 0) & ~tpad[:, None, :]).any(-1).view(-1).float())
    assert torch.equal(cols, ((tgt != 0).any(1) & ~tpad).view(-1).float())


@pytest.mark.parametrize("n", [1, 1023, 1025, 8192])
def test_bce_sel_matches_fp64(n):
    g = _gen(1100 + n)
    x = torch.randn(n, generator=g) * 4
    sat = torch.tensor([30.0, -30.0, 80.0, -80.0])
    k = min(n, 64)
    x[:k] = sat[torch.arange(k) % 4]
    y = (torch.rand(n, generator=g) < 0.4).float()
    y[:k] = ((torch.arange(k) // 4) % 2).float()                # both labels at every saturated logit
    sel = (torch.rand(n, generator=g) < 0.8).float()
    sel[:k] = 1.0
    if n == 1:
        y[0] = 1.0
    n_sel, n_pos = (sel.sum(), (y * sel).sum())
    scal = torch.zeros(8)
    scal[0], scal[1] = n_sel, n_pos
    scal[2] = n_sel / n_pos - 1.0
    x, y, sel, scal = _cuda(x, y, sel, scal)
    xg = x.clone().requires_grad_(True)
    out = L._BCESelFn.apply(xg, y, sel, scal)
    s = sel.bool()
    x64 = x.double().requires_grad_(True)
    pw = scal[2].double()
    bce = F.binary_cross_entropy_with_logits(x64[s], y.double()[s], pos_weight=pw.expand(int(s.sum())), reduction="sum") / scal[0].double()
    top1 = (((x[s] > 0).float() == y[s]).double().sum() / scal[0].double()).item()
    # f32 log1p(exp(-|x|)) terms (~2 ulp each) summed over <= 8192 entries
    assert abs(out[0].item() - bce.item()) <= 1e-5 * abs(bce.item()), (out[0].item(), bce.item())
    assert abs(out[1].item() - top1) <= 2.0 ** -23 * top1
    gv = torch.tensor([1.7, -0.4], device="cuda")
    (out * gv).sum().backward()
    (bce * 1.7).backward()
    want = x64.grad
    # f32 sigmoid: 1 - sigmoid(x) is lost below 2^-24 (|x| >~ 17), an absolute error of ~1e-7 of the largest gradient
    assert ((xg.grad.double() - want).abs() <= 1e-5 * want.abs() + 1e-7 * want.abs().max()).all()
    assert (xg.grad[~s] == 0).all()
