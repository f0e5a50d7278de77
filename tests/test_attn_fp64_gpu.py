"""The attention core (csrc/tan_attn.hip + tan_attn_img.h) on every length branch, through ops.attn_fwd / ops.attn_bwd with and
without g_b_qkv (and tan_attn_fwd directly where its error code is wanted).  Inputs, closed forms, references and bounds live in
tests/attn_cases.py (checked on the CPU by test_attn_cases_cpu.py).  Two kinds of test:

A. Exact structure tests.  One-hot / two-hot softmaxes: key j carries the +-1 code of its pair, query i is 64 x the code of its
   target pair, so scores are integers, 504 on the target and <= 392 elsewhere: exp(s - max) is exactly 0 off the target and P is
   exactly 1/2, 1/2 or 1 (partner padded, or a singleton).  v, d_o are integers in [-6, 6].  Asserted with torch.equal:
     forward   o = the mean of the target v rows; every-key-padded videos give o = 0, lse = -inf; lse against 504 + log(count)
               within u |lse| + 4 u (the final addition; logf(2) to 2 ulp, logf(1) = 0)
     backward  fed the closed-form o and lse (rounded to the storage type): dk, dv rows of keys nobody targets and of padded keys
               are 0; dq rows of one-hot queries are 0; bf16: dv = the scatter-add of P d_o, rounded to bf16 where a key collects
               more than 8 bits.  NOT exact, and held to the section B bound against the closed form instead: dq of two-hot rows,
               dk of targeted keys (the backward's P is rebuilt from the f32 lse = 504.69.., so it is 1/2 (1 +- |lse| u) before
               it is rounded, and P (dP - delta) keeps that error), and the f32 dv (its P is never rounded to bf16).
     one-hot   (every key a singleton, one L per NKB of the short and mid kernels): dq = dk = 0, dv integers, and with an integer
               g0 the fused bias gradient is g0 + the column sums exactly; dqkv is bit-equal with and without g_b_qkv.
     guards    o, lse, dqkv, g live inside larger buffers filled with -77 (64 elements in front and behind: 128 / 256 bytes, so
               the 16-byte accesses stay aligned); the guards are intact after every launch, and the outputs start as NaN.
B. fp64 numerics on random data (scores of standard deviation 2.25, and "large": 100, |score| up to ~450).  The reference is
   float64 PyTorch (the model's formula, autograd, logsumexp) of the values the kernel read.  Per element, u = 2^-24:
     forward P   the max cancels, so per key: e_S = 64 u sum_d |q k| / 8 (score accumulation) + 2 u |S - max| (subtraction, exp's
                 argument; the alphas of an online softmax split the same total) + (2 + 3 chunks) u; the row sum: the P-weighted
                 mean of that + (Lp / 2 + 6) u
     o           sum_j |P v| (rel P + 2^-8 for the bf16 operand) + (Lp + 2) u sum_j |P v|, then the store (2^-8 |o| or u |o|)
     lse         P-weighted (e_S + 2 u |S - max|) + (Lp / 2 + 3 chunks + 8) u + 2 u |log l| + u |lse|
     backward P  e_S + e_lse (u |lse| fed / the forward bound chained) + u |S| + 2 u |S - lse| + 2 u
     delta       short: sum_j P (|dP| pi + 64 u sum_d |dO v|) + (Lp / 2 + 2) u sum_j P |dP|; mid, long, f32: sum_d |dO| e_o + 64 u
                 sum_d |dO o| with e_o = the rounding of the o that was fed (or the forward bound)
     dS          |dS| pi + P (e_dP + e_delta) + 2 u P (|dP| + |delta|), + 2^-8 as a bf16 operand
     dq, dk, dv  the operand errors through the magnitudes of the contraction + (Lp + 2) u of them, then the store
     g_b_qkv     (chain) u (sum_rows |dqkv stored| + |g0|): chain = 32 + B NKB + 1 fused, B L + 1 through tan_colsum_acc
   A bound is a worst case and an error is not, so ratios far below 1 are expected; section A catches the structural slips.
   Two kinds of case per branch: the backward fed the reference's o and lse rounded to the storage type (a forward error cannot
   hide in it or cancel), and chained cases fed the forward kernel's own o and lse.

Shapes (B in {1, 3}, H in {1, 3, 8}; BH below) and the kernel each enters:
  attn_fwd_short_kernel / attn_bwd_short_kernel<1..4>   bf16 L = 1, 17, 32 | 33, 64 | 65, 80, 96 | 97, 128
      staggered start (gridDim.x >= 1024)                test_staggered_start: B = 128, H = 8, L = 64 (<2>: four phases), 80 (<3>: two)
  attn_fwd_mid_kernel / attn_bwd_mid_kernel<5..9>        bf16 L = 129, 160 | 161, 192 | 200, 224 | 225, 256 | 257, 272, 288
  attn_fwd_long_kernel, attn_bwd_dq_long_kernel,
  attn_bwd_dkv_long_kernel                               bf16 L = 289, 384, 385, 513 (3, 3, 4, 5 blocks of 128)
  attn_fwd_kernel<float>, attn_bwd_dq_kernel<float>,
  attn_bwd_dkv_kernel<float>                             f32 L = 1, 63, 64, 65, 200, 448; L = 449: TAN_ERR_BAD_ARG (test_f32_forward_449)
  every one of them: test_exact_twohot, test_fp64_fed, test_fp64_chained; fused gbias: those and test_exact_onehot_fused_bias
Padding (attn_cases.keypad_sets: a different pattern per video, every pattern that fits L): none (null pointer), ragged tail,
scattered keys, the whole leading 32 / 96 / 128 keys (a wave's block, the mid forward's first chunk: m = -inf carries over, the
long kernels' first block), the whole second 32 / 96 / 128, every key but the last, every key (next to live videos).
NOT covered: attn_fwd_kernel<bf16_t>, attn_bwd_dq_kernel<bf16_t>, attn_bwd_dkv_kernel<bf16_t> -- long_path() is constant true, so no
call reaches them.  tan_attnblk.hip has its own files (test_attnblk_fp64_gpu.py, test_attnblk_gpu.py).

Measured on an MI355X (worst observed / bound over every case; test_report_worst_ratios prints them):
                     f32      short    mid      long
  fwd      o         0.039    0.809    0.697    0.636
  fwd      lse       0.082    0.029    0.032    0.034
  fed      dq        0.075    0.827    0.477    0.471
  fed      dk        0.066    0.780    0.508    0.490
  fed      dv        0.079    0.783    0.819    0.780
  fed      g_b_qkv   0.441    0.103    0.100    0.009
  chained  dq        0.009    0.769    0.204    0.186
  chained  dk        0.011    0.747    0.266    0.262
  chained  dv        0.038    0.823    0.731    0.680
  chained  g_b_qkv   0.387    0.071    0.122    0.010
  exact    lse       0.047    0.047    0.047    0.047
  exact    dq        0.000    0.484    0.000    0.000
  exact    dk        0.001    0.606    0.320    0.366
  exact    dv        0.001    0.000    0.000    0.000
  exact    g_b_qkv   0.017    0.048    0.000    0.000
A bf16 output sits at 0.5 - 0.8 because its bound is little more than the half ulp of the store and of the bf16 operands; the f32
kernels sit below 0.1 because their chains are counted at full length.  "exact" rows: the two-hot cases against the closed form --
the mid and long kernels take delta from the (here exact) o and the bf16 rounding of dS gives back the exact quarter-integers, so
their dq is exact; the short kernel's delta = sum P~ dP carries the error of P~.  The chained bounds are wider than the fed ones
(the forward's bounds stand in for the inputs' errors), hence the lower ratios.

Mutants of tan_attn.hip / tan_attn_img.h this file was run against once each (none is kept): the first assertion that failed in
the whole file, and in section B alone (test_fp64_fed, test_fp64_chained; ratio = observed / bound).  L = 1 / 17 / 129 / 289 are
the first cases of the short / mid / long branches in collection order.
  alpha = 1 in attn_fwd_mid_kernel                  exact_twohot[bf16-129] unpadded: o != mean of target v (5456 values) | mid fwd/o 881
  alpha = 1 in attn_fwd_long_kernel                 exact_twohot[bf16-289] unpadded: o != mean of target v (52495)       | long fwd/o 668
  my_bias dropped, phase B of the short backward    exact_twohot[bf16-1]: g_b_qkv 1.4e7 (keys past L are counted)        | short fed/g_b_qkv 1.4e7
  img_swz(row + 8) -> img_swz(row) in img_frag_tr   exact_twohot[bf16-17]: o != mean of target v (2062)                  | short fwd/o 1374
  0.125f -> 0.25f in the short backward's dk        exact_twohot[bf16-17]: short exact/dk 85                             | short fed/dk 126
  long_delta summed over half of d                  exact_twohot[bf16-289]: dq of a one-hot row is not 0                 | long fed/dq 79
  last wave left out of the short fused gbias       exact_twohot[bf16-1]: g_b_qkv 4.7e5                                  | short fed/g_b_qkv 4.7e5
  last wave left out of the mid fused gbias         exact_twohot[bf16-129]: g_b_qkv 6267                                 | mid fed/g_b_qkv 9335
  dead = false in attn_fwd_long_kernel              exact_twohot[bf16-289] pad (lead32, lead96, lead128): o (55488)      | long fwd/o NaN, same pad
  dead = false in attn_fwd_mid_kernel               exact_twohot[bf16-129] pad (lead32, lead96, lead128): o (49536)      | mid fwd/o NaN, same pad
  no max subtraction in attn_fwd_short_kernel       exact_twohot[bf16-1]: o != mean of target v (1536)                   | short fwd/lse 9.5e4
  lse = -inf not turned into +inf in long_lse       exact_twohot[bf16-289] pad (butlast, all, none): dk / dv of a padded key | long fed/dq NaN, same pad
  the lane ^ 32 exchange of bm left out (mid fwd)   exact_twohot[bf16-129] unpadded: o != mean of target v (51432)       | mid fwd/o 978
"""
import math

import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
TAG = {F32: "f32", BF16: "bf16"}
U = ac.U
SENT, LEAD = -77.0, 64
WORST = {}

L_SHORT = [1, 17, 32, 33, 64, 65, 80, 96, 97, 128]
L_MID = [129, 160, 161, 192, 200, 224, 225, 256, 257, 272, 288]
L_LONG = [289, 384, 385, 513]
L_F32 = [1, 63, 64, 65, 200, 448]
BH = {BF16: {1: (3, 8), 17: (1, 3), 32: (3, 1), 33: (3, 3), 64: (3, 8), 65: (1, 8), 80: (3, 8), 96: (3, 1), 97: (1, 3), 128: (3, 8),
             129: (3, 3), 160: (1, 8), 161: (3, 1), 192: (3, 8), 200: (1, 3), 224: (3, 3), 225: (3, 1), 256: (3, 8), 257: (1, 1),
             272: (3, 8), 288: (3, 3), 289: (3, 3), 384: (1, 8), 385: (3, 1), 513: (3, 3)},
      F32: {1: (3, 3), 63: (1, 8), 64: (3, 1), 65: (3, 8), 200: (3, 3), 448: (3, 1)}}
CASES = [(BF16, L) for L in L_SHORT + L_MID + L_LONG] + [(F32, L) for L in L_F32]
IDS = [f"{TAG[d]}-{L}" for d, L in CASES]
ONEHOT_L = [17, 64, 80, 128, 160, 192, 224, 256, 288]          # NKB = 1 .. 9


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def guarded(shape, dtype, fill=float("nan")):
    """a tensor of `shape` inside a larger buffer of SENT (16-byte aligned), filled with `fill`"""
    n = math.prod(shape)
    buf = torch.full((LEAD + n + LEAD,), SENT, dtype=dtype, device=DEV)
    v = buf[LEAD:LEAD + n].view(shape)
    v.copy_(fill) if torch.is_tensor(fill) else v.fill_(fill)
    assert v.data_ptr() % 16 == 0
    return buf, v


def intact(buf):
    return bool((buf[:LEAD] == SENT).all()) and bool((buf[-LEAD:] == SENT).all())


def fwd(qkv, keypad, B, L, H):
    from temporalalignnet_amd import ops
    ob, o = guarded((B * L, H * 64), qkv.dtype)
    lb, lse = guarded((B, H, L), F32)
    ops.attn_fwd(qkv, keypad, o, lse, B, L, H)
    assert intact(ob) and intact(lb), "attn_fwd wrote outside o / lse"
    return o, lse


def bwd(qkv, keypad, o, lse, d_o, B, L, H, g0=None):
    from temporalalignnet_amd import ops
    db, dqkv = guarded(tuple(qkv.shape), qkv.dtype)
    gb, g = guarded(tuple(g0.shape), F32, g0) if g0 is not None else (None, None)
    ops.attn_bwd(qkv, keypad, o, lse, d_o, dqkv, B, L, H, g_b_qkv=g)
    assert intact(db) and (gb is None or intact(gb)), "attn_bwd wrote outside dqkv / g_b_qkv"
    return dqkv, g


def ratio(key, case, got, ref, bound):
    """observed / bound, worst element, recorded per key; where the bound is 0 the result must be exact.  NaN fails."""
    err = (got.double() - ref).abs()
    bound = bound.expand_as(err)
    pos = bound > 0
    assert bool((err[~pos] == 0).all()), (key, case, "inexact where the bound is 0")
    r = (err[pos] / bound[pos]).max().item() if bool(pos.any()) else 0.0
    assert math.isfinite(r), (key, case, r)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1.0, (key, case, f"observed / bound = {r:.4g}")
    return r


def check_lse(key, case, lse, ref, bound):
    dead = torch.isinf(ref)
    assert torch.equal(torch.isinf(lse), dead) and bool((lse[dead] < 0).all()), (key, case, "lse = -inf exactly for all-padded videos")
    zero = torch.zeros((), device=DEV)
    ratio(key, case, torch.where(dead, zero, lse), torch.where(dead, zero.double(), ref), bound)


def check_bwd(tag, case, dqkv, m, bounds, B, L, H):
    dq, dk, dv = ac.split_qkv(dqkv, B, L, H)
    for n, got, b in zip(("dq", "dk", "dv"), (dq, dk, dv), bounds):
        ratio(f"{tag}/{n}", case, got, m[n], b)


def check_gbias(tag, case, g, g0, dqkv, dqkv_plain, pc, B, L):
    """the entry with g_b_qkv: the same dqkv bit for bit, and g = g0 + the column sums of the STORED dqkv within the chain bound"""
    assert torch.equal(bits(dqkv), bits(dqkv_plain)), (tag, case, "dqkv differs with g_b_qkv")
    d = dqkv.double()
    ratio(f"{tag}/g_b_qkv", case, g, g0.double() + d.sum(0), ac.gbias_chain(pc, B, L) * U * (d.abs().sum(0) + g0.double().abs()))


# ======================================================================================================================
# A. exact structure tests
# ======================================================================================================================
def exact_case(dtype, B, L, H, seed, names, keypad, onehot=False, bounds=True):
    case = f"{TAG[dtype]} B={B} L={L} H={H} pad={names} onehot={onehot}"
    keypad = None if keypad is None else keypad.to(DEV)
    c = ac.twohot_case(B, L, H, seed, keypad, onehot=onehot, device=DEV)
    qkv, d_o = c["qkv"].to(dtype), c["d_o"].to(dtype)
    assert torch.equal(qkv.float(), c["qkv"]) and torch.equal(d_o.float(), c["d_o"])
    m = ac.manual(c["qkv"], keypad, c["d_o"], B, L, H, P=c["P"], lse=c["lse"])
    ac.assert_exact_conditions(m)
    pc = ac.path_of(dtype == BF16, L)
    tag = f"{pc['name']} exact"
    # ---- forward
    o, lse = fwd(qkv, keypad, B, L, H)
    o_want = ac.merge_rows(m["o"]).to(dtype)
    assert torch.equal(o_want.double(), ac.merge_rows(m["o"]))                      # the expectation itself is exact in the type
    assert torch.equal(o, o_want), (case, "o != mean of the target v rows", int((o != o_want).sum()))
    lse_f = torch.where(torch.isinf(c["lse"]), torch.zeros_like(c["lse"]), c["lse"])
    check_lse(f"{tag}/lse", case, lse, c["lse"], torch.where(torch.isinf(c["lse"]), torch.zeros_like(lse_f), U * lse_f.abs() + 4 * U))
    # ---- backward, fed the closed form
    lse_fed = c["lse"].float()
    dqkv, _ = bwd(qkv, keypad, o_want, lse_fed, d_o, B, L, H)
    dq, dk, dv = ac.split_qkv(dqkv, B, L, H)
    untargeted = c["P"].sum(2) == 0
    assert bool(untargeted.any()) or L < 33
    assert bool((dk[untargeted] == 0).all()) and bool((dv[untargeted] == 0).all()), (case, "dk / dv of an untargeted or padded key")
    assert bool((dq[c["cnt"] <= 1] == 0).all()), (case, "dq of a one-hot row")
    if dtype == BF16:
        assert torch.equal(dv, m["dv"].to(dtype)), (case, "dv != scatter-add of P d_o", int((dv != m["dv"].to(dtype)).sum()))
    if onehot:
        assert bool((dq == 0).all()) and bool((dk == 0).all()), (case, "one-hot: dq = dk = 0")
    if bounds:
        check_bwd(tag, case, dqkv, m, ac.bwd_bounds(m, pc, *ac.fed_errors(m, pc)), B, L, H)
    # ---- the entry with the bias gradient
    g0 = torch.randint(-50, 51, (3 * H * 64,), generator=torch.Generator().manual_seed(seed + 1)).float().to(DEV)
    dqkv2, g = bwd(qkv, keypad, o_want, lse_fed, d_o, B, L, H, g0)
    check_gbias(tag, case, g, g0, dqkv2, dqkv, pc, B, L)
    if onehot:
        assert float(dqkv.double().abs().sum(0).max()) + 50 < 2 ** 24
        assert torch.equal(g.double(), g0.double() + dqkv.double().sum(0)), (case, "g != g0 + column sums")


@pytest.mark.parametrize("dtype,L", CASES, ids=IDS)
def test_exact_twohot(dtype, L):
    """section A on every branch and every padding set (see the module docstring)"""
    B, H = BH[dtype][L]
    for i, (names, keypad) in enumerate(ac.keypad_sets(B, L)):
        exact_case(dtype, B, L, H, 1000 + 10 * L + i, names, keypad)


@pytest.mark.parametrize("L", ONEHOT_L)
def test_exact_onehot_fused_bias(L):
    """every key a singleton: P = 1 exactly, dq = dk = 0, dv integers, g = g0 + column sums exactly (fused: short and mid bf16)"""
    for i, (names, keypad) in enumerate(ac.keypad_sets(3, L)[:3]):
        exact_case(BF16, 3, L, 8, 2000 + 10 * L + i, names, keypad, onehot=True, bounds=False)


@pytest.mark.parametrize("L", [64, 80])
def test_staggered_start(L):
    """B H = 1024 workgroups: the short backward's staggered start (L = 64: NKB = 2, phases 0..3; L = 80: NKB = 3, phases 0, 1)"""
    names = [n for n in ac.PATTERNS if ac.pad_pattern(n, L, 0) is not None]           # L = 64: six patterns, L = 80: seven
    kp = torch.stack([ac.pad_pattern(names[b % len(names)], L, b) for b in range(128)])
    exact_case(BF16, 128, L, 8, 3000 + L, "every pattern in turn", kp, bounds=False)


def test_f32_forward_449():
    """the f32 forward keeps a [64][Lpad + 1] score panel in LDS: Lpad = 512 does not fit, and the call must say so
    (TAN_ERR_BAD_ARG, TanHipError through ops) before anything is launched: o and lse keep their fill"""
    from temporalalignnet_amd import _lib, ops
    B, L, H = 1, 449, 1
    qkv = torch.randn(B * L, 3 * H * 64, device=DEV)
    ob, o = guarded((B * L, H * 64), F32, SENT)
    lb, lse = guarded((B, H, L), F32, SENT)
    rc = _lib.lib().tan_attn_fwd(ops._ptr(qkv), None, ops._ptr(o), ops._f32(lse), B, L, H, _lib.TAN_F32, ops._stream())
    assert rc == -1                                                                 # TAN_ERR_BAD_ARG
    with pytest.raises(_lib.TanHipError):
        ops.attn_fwd(qkv, None, o, lse, B, L, H)
    torch.cuda.synchronize()
    assert bool((ob == SENT).all()) and bool((lb == SENT).all())
    o448, _ = fwd(qkv[:448].contiguous(), None, 1, 448, 1)                          # one row fewer fits
    assert bool(torch.isfinite(o448).all())


# ======================================================================================================================
# B. fp64 numerics
# ======================================================================================================================
SCALES = {"ordinary": 1.5, "large": 10.0}


def rand_inputs(B, L, H, dtype, seed, scale):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    qkv = torch.randn(B * L, 3 * H * 64, generator=g, device=DEV)
    qkv[:, :2 * H * 64] *= scale
    return qkv.to(dtype), torch.randn(B * L, H * 64, generator=g, device=DEV).to(dtype)


def reference(qkv, keypad, d_o, B, L, H):
    """fp64 autograd (the values the assertions compare with) and the by-hand quantities (the magnitudes the bounds need)"""
    o, lse, g = ac.ref_autograd(qkv, keypad, d_o, B, L, H)
    m = ac.manual(qkv, keypad, d_o, B, L, H)
    m["dq"], m["dk"], m["dv"] = ac.split_qkv(g, B, L, H)
    m["o"], m["lse"] = ac.split_rows(o, B, L, H), lse
    return m


def fp64_case(dtype, B, L, H, seed, sname, names, keypad, chained):
    case = f"{TAG[dtype]} B={B} L={L} H={H} {sname} pad={names}"
    keypad = None if keypad is None else keypad.to(DEV)
    qkv, d_o = rand_inputs(B, L, H, dtype, seed, SCALES[sname])
    m = reference(qkv, keypad, d_o, B, L, H)
    pc = ac.path_of(dtype == BF16, L)
    b_o, b_lse = ac.fwd_bounds(m, pc)
    o, lse = fwd(qkv, keypad, B, L, H)
    if chained:
        tag = f"{pc['name']} chained"
        e_o, e_lse = b_o, b_lse
    else:
        tag = f"{pc['name']} fed"
        ratio(f"{pc['name']} fwd/o", case, ac.split_rows(o, B, L, H), m["o"], b_o)
        check_lse(f"{pc['name']} fwd/lse", case, lse, m["lse"], b_lse)
        o, lse = ac.merge_rows(m["o"]).to(dtype), m["lse"].float()
        e_o, e_lse = ac.fed_errors(m, pc)
    dqkv, _ = bwd(qkv, keypad, o, lse, d_o, B, L, H)
    check_bwd(tag, case, dqkv, m, ac.bwd_bounds(m, pc, e_o, e_lse), B, L, H)
    dead = ~m["live"].any(1)
    assert bool((dqkv.view(B, L, -1)[dead] == 0).all()), (case, "dqkv of an all-padded video")
    g0 = torch.randn(3 * H * 64, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
    dqkv2, g = bwd(qkv, keypad, o, lse, d_o, B, L, H, g0)
    check_gbias(tag, case, g, g0, dqkv2, dqkv, pc, B, L)


@pytest.mark.parametrize("dtype,L", CASES, ids=IDS)
def test_fp64_fed(dtype, L):
    """forward against fp64; backward fed the reference's o and lse rounded to the storage type; both score scales, every padding set"""
    B, H = BH[dtype][L]
    for s, sname in enumerate(SCALES):
        for i, (names, keypad) in enumerate(ac.keypad_sets(B, L)):
            fp64_case(dtype, B, L, H, 4000 + 100 * L + 10 * s + i, sname, names, keypad, chained=False)


@pytest.mark.parametrize("dtype,L", CASES, ids=IDS)
def test_fp64_chained(dtype, L):
    """backward fed the forward kernel's own o and lse (bounds: the forward's bounds as the inputs' errors); both score scales, the
    unpadded set and the last padding set"""
    B, H = BH[dtype][L]
    sets = ac.keypad_sets(B, L)
    for s, sname in enumerate(SCALES):
        for i in sorted({0, len(sets) - 1}):
            fp64_case(dtype, B, L, H, 5000 + 100 * L + 10 * s + i, sname, sets[i][0], sets[i][1], chained=True)


def test_report_worst_ratios():
    for k in sorted(WORST):
        print(f"WORST {k}: {WORST[k]:.4f}")
