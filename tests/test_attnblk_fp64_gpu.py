"""The fused attention branch (csrc/tan_attnblk.hip: in_proj GEMM, eight heads of attention, out_proj, bias and residual in one launch)
through the C ABI, at every length class of both templates.  Inputs, closed forms, references and bounds live in
tests/attnblk_cases.py (checked on the CPU by test_attnblk_cases_cpu.py).  EVERY case of this file goes through `run_all`: four
launches -- tan_attnblk_fwd and tan_attnblk_fwd_split, each saving qkv / attn_o / lse and each with the three pointers null -- with
  guards     qkv, attn_o, lse, x_mid and the split scratch `part` live inside larger allocations of -77: 48 rows of the tensor in front
             and behind (LP - L <= 47 rows is the furthest a store without its `row < L` guard could reach), 64 floats for lse; all
             16-byte aligned.  The bands are intact after every launch; the outputs and `part` start as NaN and end finite (lse: or
             -inf).  The inputs (xn1, x_in, keypad, both packed weights, both biases) sit inside larger allocations of finite filler.
  no-save    the launch with null pointers leaves three buffers of -77 in the places of qkv, attn_o and lse untouched, and its x_mid
             is bit-equal to the saving launch's, whole and split
  split      qkv, attn_o and lse of the split launch are bit-equal to the whole launch's (the same instructions); x_mid differs only
             by the order of f32 additions -- and not at all in section A, where the sums are exact

A. Exact structure (test_exact, test_exact_large_batch; torch.equal).  A two-hot softmax built through xn1 and w_in: xn1 carries the
   +-1 code of the row's own pair and the codes of two target pairs, w_q[h] is 64 x and w_k[h] 1 x a signed permutation (one per
   head) of the code channels, w_v[h] picks +- two integer channels, w_out has four small integers per row, biases and x_in are
   integers.  Scores are 504 on the target pair and <= 392 elsewhere, P is exactly 1/2 or 1, every GEMM sum is exact in any order.
     qkv     = the closed-form q | k | v                       attn_o = the mean of the target v rows (padded query rows too); 0 for a
     x_mid   = bf16(x_in + o w_out^T + b_out), exact value,             video with every key padded
               rounded to nearest even where it needs > 8 bits  lse    = 504 + log(count) within u |lse| + 4 u; -inf for such a video
   Row 0 targets the pair of the last row (which the panel repeats up to LP) wherever that key is live, so a repeated row that is
   visible as a key doubles a count.  Even and odd heads have different targets; every head its own permutation, signs and v.
B. fp64 numerics on random bf16 data (test_fp64_stages, test_fp64_chained): w_q, w_k scaled for scores of standard deviation 2.25
   ("ordinary") and 100 ("large", |score| up to ~450).  float64 PyTorch on the device, of the values the kernel read, stage by stage
   so that an error cannot hide behind a bf16 rounding flip upstream.  Per element, u = 2^-24, r = 2^-8 (half an ulp of bf16):
     qkv     against fp64 of xn1 and w_in:           e = 512 u (sum_k |x w| + |b|),  bound e + r (|ref| + e)
     attn_o  against fp64 attention of the kernel's own saved qkv: attn_cases.fwd_bounds of the short branch, Lp = LP:
             per key  rho = 64 u sum_d |q k| / 8 + 2 u |S - max| + 5 u;  rel P = rho + P-mean(rho) + (LP / 2 + 6) u, + r (P as a bf16
             operand);  o: sum_j |P v| rel P + (LP + 2) u sum_j |P v|, then the store r (|o| + e)
     lse     the same reference:  P-mean(64 u sum_d |q k| / 8 + 2 u |S - max|) + (LP / 2 + 11) u + 2 u |log l| + u |lse|
     x_mid   against fp64 of the kernel's own saved attn_o, M = sum_k |o w| + |b_out| + |x_in|:
             whole (one accumulator, K = 512, + bias, + residual)  e = 514 u M;   split (planes of K = 128, three additions of the
             four planes, + bias, + residual)  e = 133 u M;   bound e + r (|ref| + e)
     chained x_mid from the raw inputs (ordinary scale): the qkv bound pushed through the scores (D = the largest score change of a
             row), the softmax (|P~ - P| <= P expm1(2 D)), P v and the out-projection, plus the stages' own bounds
             (attnblk_cases.chained_xmid).  Wide by construction; it ties the stages together.
   A bound is a worst case and an error is not, so ratios below 1 are expected; section A catches the structural slips.
C. Argument checks (test_supported, test_bad_arguments): tan_attnblk_supported at L = 48, 49, 80, 81, C != 512, H != 8, f32; both
   entry points return TAN_ERR_BAD_ARG for a partly null save triple, a null `part`, B = 0, L = 48 and L = 81, and touch no output.

Lengths, and what each enters (B in {1, 3}; a different padding pattern per video at B = 3):
  L = 49, 56, 63, 64   attnblk_fwd_kernel<4> / <4, true>: NKB = 2, LP = 64, XROWS = 64, four idle waves copy k and v out (8 pieces each);
                       15, 8, 1, 0 repeated panel rows
  L = 65, 72, 79, 80   attnblk_fwd_kernel<5> / <5, true>: NKB = 3, LP = 96, XROWS = 80, image rows 80..95 zeroed, two idle waves (24 pieces
                       each); 15, 8, 1, 0 repeated panel rows
  B = 260, L = 64, 80  test_exact_large_batch: more than 256 workgroups (1040 in the split launch), every padding pattern in turn
  attnblk_split_finish_kernel: every split launch
Padding (attn_cases.PATTERNS that fit): none (null pointer), ragged tail, scattered keys, the whole leading 32 keys (a wave's key
block), the whole second 32 (L > 64), every key but the last, every key of a video (first at L > 64, last at L <= 64, and the
middle one in an extra set at every L; always next to live videos).

Measured on an MI355X (worst observed / bound over every case; test_report_worst_ratios prints them):
                       whole    split
  stage    qkv         0.962    (bit-equal)
  stage    attn_o      0.862    (bit-equal)
  stage    lse         0.027    (bit-equal)
  stage    x_mid       0.988    0.994
  chained  x_mid       0.988    0.994
  exact    lse         0.047    0.047
The bf16 outputs sit near 1 because their bounds are little more than the half ulp of the store (qkv, x_mid: e is 512 u of magnitudes,
2^-15 of them, next to r = 2^-8) and a few of some 10^7 elements come that close to a rounding boundary; attn_o adds the half ulp of P as
an operand.  The chained figure is that of the all-padded videos, where x_mid = x_in + b_out and the bound is the store's alone;
everywhere else the chained bound is several times the error.

Mutants of tan_attnblk.hip this file was run against once each (none is kept): the first assertion that failed in the whole file,
and in section B alone.
  `j >= L ||` dropped from the key bias             test_exact[49-1] unpadded: attn_o != mean of target v (1454 values)   | stage/attn_o 674
  img_swz dropped in the GEMM-a epilogue            test_exact[49-1] unpadded: q != closed form (11154)                   | stage/qkv 7697
  head h ^ 1 in the lse store                       test_exact[49-1] unpadded: exact whole/lse 2.3e4                      | stage/lse 7.2e4
  plane 3 left out of attnblk_split_finish_kernel   test_exact[49-1] unpadded: split x_mid != closed form (23155)         | stage split/x_mid 1.0e4
  k and v swapped in the idle waves' copy-out       test_exact[49-1] unpadded: k != closed form (22683)                   | stage/qkv 1.0e4
  GEMM-b reads ring slot (KB + 1) % 4               test_exact[49-1] unpadded: qkv: split != whole (the next GEMM-a's     | the same assertion
                                                    weights are loaded into the wrong slot)                              |
  score scale 0.125f -> 0.126f                      test_exact[49-1] unpadded: exact whole/lse 1.3e5                      | stage/attn_o 4.1
  heads of a pair swapped in the attn_o copy-out    test_exact[49-1] unpadded: attn_o != mean of target v (24012)         | stage/attn_o 4264
  row0 = (blockIdx.x & 255) * L                     test_exact_large_batch[64]: x_mid of video 256.. still NaN            | survives (B <= 3): structural
(L = 49, B = 1, unpadded is the first case in collection order.  Mutants that drop a `row < L` store guard or a min(m, L - 1) clamp
can write or read outside the allocations and were not run.)
"""
import ctypes as C
import math

import pytest
import torch

import attn_cases as ac
import attnblk_cases as bc
from test_attnblk_gpu import pack

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U, H, CH = bc.U, bc.H, bc.C
SENT, BAND_ROWS, BAND_LSE = -77.0, 48, 64
BAD_ARG = -1
WORST = {}


def _api():
    from temporalalignnet_amd import _lib, ops
    return _lib, ops


def guarded(rows, width, dtype, fill=float("nan"), band=None):
    """[rows, width] inside a larger buffer of SENT (BAND_ROWS rows in front and behind, or `band` elements), filled with `fill`"""
    lead, n = band if band is not None else BAND_ROWS * width, rows * width
    buf = torch.full((lead + n + lead,), SENT, dtype=dtype, device=DEV)
    v = buf[lead:lead + n].view(rows, width)
    v.copy_(fill) if torch.is_tensor(fill) else v.fill_(fill)
    assert v.data_ptr() % 16 == 0 and (lead * buf.element_size()) % 16 == 0
    return buf, v, lead


def intact(g):
    buf, _, lead = g
    return bool((buf[:lead] == SENT).all()) and bool((buf[-lead:] == SENT).all())


def housed(t, filler, lead=None):
    """an input inside a larger allocation of finite filler"""
    t = t.contiguous()
    lead = lead or 48 * (t.shape[-1] if t.dim() > 1 else 16)
    buf = torch.full((lead + t.numel() + lead,), filler, dtype=t.dtype, device=DEV)
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 0
    return v


def prepare(I, keypad):
    """the inputs of a case on the device, in the kernel's types, packed and housed"""
    xn1, x_in, w_in, w_out = (I[n].to(DEV).to(BF16) for n in ("xn1", "x_in", "w_in", "w_out"))
    pw_qkv, pw_out = pack([(w_in, 384, 32), (w_out, 512, 16)])
    P = dict(xn1=housed(xn1, 3.0), x_in=housed(x_in, 5.0), pw_qkv=housed(pw_qkv, 0.5, 4096), pw_out=housed(pw_out, 0.5, 4096),
             b_in=housed(I["b_in"].to(DEV).float(), 7.0, 64), b_out=housed(I["b_out"].to(DEV).float(), 7.0, 64),
             keypad=None if keypad is None else housed(keypad.to(DEV), 0, 4096), B=I["B"], L=I["L"])
    P.update(w_in=w_in, w_out=w_out)
    return P


def desc(P, L=None, B=None):
    _lib, _ = _api()
    d = _lib.AttnBlkDesc()
    d.B, d.L, d.C, d.H = P["B"] if B is None else B, P["L"] if L is None else L, CH, H
    d.xn1, d.x_in = P["xn1"].data_ptr(), P["x_in"].data_ptr()
    d.key_padding_mask = P["keypad"].data_ptr() if P["keypad"] is not None else None
    d.pw_qkv, d.pw_out, d.b_qkv, d.b_out = P["pw_qkv"].data_ptr(), P["pw_out"].data_ptr(), P["b_in"].data_ptr(), P["b_out"].data_ptr()
    return d


def buffers(B, L, save, split, fill=float("nan")):
    R = B * L
    side = fill if save else SENT
    return dict(qkv=guarded(R, 3 * CH, BF16, side), attn_o=guarded(R, CH, BF16, side), lse=guarded(B * H, L, F32, side, BAND_LSE),
                x_mid=guarded(R, CH, BF16, fill), part=guarded(4 * R, CH, F32, fill) if split else None)


def call(d, G, save, split, part_null=False, keep=("qkv", "attn_o", "lse")):
    """the entry point's return code; save: the pointers of `keep` are passed, the others null"""
    _lib, ops = _api()
    for n in ("qkv", "attn_o", "lse"):
        setattr(d, n, G[n][1].data_ptr() if save and n in keep else None)
    d.x_mid = G["x_mid"][1].data_ptr()
    if split:
        return _lib.lib().tan_attnblk_fwd_split(C.byref(d), None if part_null else C.c_void_p(G["part"][1].data_ptr()), ops._stream())
    return _lib.lib().tan_attnblk_fwd(C.byref(d), ops._stream())


def launch(P, save, split, case):
    """one launch; the guard, sentinel and finiteness assertions; -> {name: tensor}"""
    B, L = P["B"], P["L"]
    G = buffers(B, L, save, split)
    rc = call(desc(P), G, save, split)
    torch.cuda.synchronize()
    what = (case, "split" if split else "whole", "save" if save else "no-save")
    assert rc == 0, (what, rc)
    for n, g in G.items():
        assert g is None or intact(g), (what, f"wrote outside {n}")
    out = {n: g[1] for n, g in G.items() if g is not None}
    assert bool(torch.isfinite(out["x_mid"]).all()), (what, "x_mid not finite everywhere")
    if split:
        assert bool(torch.isfinite(out["part"]).all()), (what, "part not finite everywhere")
    if save:
        assert bool(torch.isfinite(out["qkv"]).all()) and bool(torch.isfinite(out["attn_o"]).all()), (what, "qkv / attn_o not finite")
        assert not bool(torch.isnan(out["lse"]).any()) and not bool((out["lse"] == math.inf).any()), (what, "lse NaN or +inf")
    else:
        for n in ("qkv", "attn_o", "lse"):
            assert bool((G[n][0] == SENT).all()), (what, f"a no-save launch wrote {n}")
    out["lse"] = out["lse"].view(B, H, L)
    return out


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def run_all(P, case):
    """whole and split, saving and not: -> (whole, split) of the saving launches"""
    w, s = launch(P, True, False, case), launch(P, True, True, case)
    for n in ("qkv", "attn_o", "lse"):
        assert torch.equal(bits(s[n]), bits(w[n])), (case, f"{n}: split != whole")
    for split, ref in ((False, w), (True, s)):
        o = launch(P, False, split, case)
        assert torch.equal(bits(o["x_mid"]), bits(ref["x_mid"])), (case, "split" if split else "whole", "x_mid: no-save != save")
    return w, s


def ratio(key, case, got, ref, bound):
    r = bc.worst_ratio(got, ref, bound)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1.0, (key, case, f"observed / bound = {r:.4g}")


def check_lse(key, case, lse, ref, bound):
    dead = torch.isinf(ref)
    assert torch.equal(torch.isinf(lse), dead) and bool((lse[dead] < 0).all()), (key, case, "lse = -inf exactly for all-padded videos")
    zero = torch.zeros((), device=DEV)
    ratio(key, case, torch.where(dead, zero, lse), torch.where(dead, zero.double(), ref), torch.where(dead, zero.double(), bound))


# ======================================================================================================================
# A. exact structure
# ======================================================================================================================
def exact_case(B, L, seed, names, keypad):
    case = f"exact B={B} L={L} pad={names}"
    c = bc.exact_case(B, L, seed, keypad, device=DEV)
    if B <= 3:
        bc.assert_exact_conditions(c)
    P = prepare(c, keypad)
    for n in ("xn1", "x_in"):
        assert torch.equal(P[n].float(), c[n]), n
    assert torch.equal(P["w_in"].float(), c["w_in"]) and torch.equal(P["w_out"].float(), c["w_out"])
    w, s = run_all(P, case)
    qkv, o, x_mid = c["qkv"].to(BF16), c["o"].to(BF16), c["x_mid"].to(BF16)
    assert torch.equal(qkv.float(), c["qkv"]) and torch.equal(o.double(), c["o"])                 # the expectations are exact in bf16
    assert torch.equal(x_mid.double(), c["x_mid"].float().to(BF16).double())
    for tag, out in (("whole", w), ("split", s)):
        for third, n in enumerate("qkv"):
            sl = slice(third * CH, (third + 1) * CH)
            assert torch.equal(out["qkv"][:, sl], qkv[:, sl]), (case, tag, f"{n} != closed form", int((out["qkv"][:, sl] != qkv[:, sl]).sum()))
        assert torch.equal(out["attn_o"], o), (case, tag, "attn_o != mean of the target v rows", int((out["attn_o"] != o).sum()))
        assert torch.equal(out["x_mid"], x_mid), (case, tag, "x_mid != bf16(x_in + o w_out^T + b_out)", int((out["x_mid"] != x_mid).sum()))
        fin = ~torch.isinf(c["lse"])
        lse_f = torch.where(fin, c["lse"], torch.zeros_like(c["lse"]))
        check_lse(f"exact {tag}/lse", case, out["lse"], c["lse"], U * lse_f.abs() + 4 * U)
    assert torch.equal(bits(s["x_mid"]), bits(w["x_mid"])), (case, "x_mid: split != whole")
    dead = ~c["live"].any(1)
    if bool(dead.any()):
        assert bool((w["attn_o"].view(B, L, CH)[dead] == 0).all()) and bool((w["lse"][dead] == -math.inf).all()), (case, "all-padded video")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", bc.LENGTHS)
def test_exact(L, B):
    """section A at every length and every padding set (see the module docstring)"""
    for i, (names, keypad) in enumerate(bc.keypad_sets(B, L)):
        exact_case(B, L, 1000 + 100 * L + 10 * B + i, names, keypad)


@pytest.mark.parametrize("L", [64, 80])
def test_exact_large_batch(L):
    """B = 260: more workgroups than one round of 256 (row0 = blockIdx.x L, keypad + blockIdx.x L, lse[(b H + h) L + ...]), every
    padding pattern in turn"""
    exact_case(260, L, 2000 + L, "every pattern in turn", bc.cycle_keypad(260, L))


# ======================================================================================================================
# B. fp64 numerics
# ======================================================================================================================
def fp64_case(B, L, seed, sname, names, keypad, chained):
    case = f"{sname} B={B} L={L} pad={names}"
    I = bc.random_case(B, L, seed, sname, device=DEV)
    kp = None if keypad is None else keypad.to(DEV)
    P = prepare(I, kp)
    w, s = run_all(P, case)
    if chained:
        for tag, out, split in (("whole", w, False), ("split", s, True)):
            ref, bound = bc.chained_xmid(I, kp, split)
            ratio(f"chained {tag}/x_mid", case, out["x_mid"], ref, bound)
        return
    ref, bound, _ = bc.qkv_stage(I["xn1"], I["w_in"], I["b_in"])
    ratio("stage/qkv", case, w["qkv"], ref, bound)
    m, b_o, b_lse = bc.attn_stage(w["qkv"], kp, B, L)
    ratio("stage/attn_o", case, ac.split_rows(w["attn_o"], B, L, H), m["o"], b_o)
    check_lse("stage/lse", case, w["lse"], m["lse"], b_lse)
    for tag, out, split in (("whole", w, False), ("split", s, True)):
        ref, bound = bc.xmid_stage(out["attn_o"], I["x_in"], I["w_out"], I["b_out"], split)
        ratio(f"stage {tag}/x_mid", case, out["x_mid"], ref, bound)
    dead = ~m["live"].any(1)
    if bool(dead.any()):
        want = (I["x_in"].float() + I["b_out"]).to(BF16).view(B, L, CH)[dead]
        assert bool((w["attn_o"].view(B, L, CH)[dead] == 0).all()), (case, "attn_o of an all-padded video")
        assert torch.equal(w["x_mid"].view(B, L, CH)[dead], want) and torch.equal(s["x_mid"].view(B, L, CH)[dead], want), (case, "x_mid of an all-padded video")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", bc.LENGTHS)
def test_fp64_stages(L, B):
    """every stage against fp64 of what the stage read; both score scales, every padding set"""
    for si, sname in enumerate(bc.SCALES):
        for i, (names, keypad) in enumerate(bc.keypad_sets(B, L)):
            fp64_case(B, L, 4000 + 100 * L + 20 * si + 10 * (B // 3) + i, sname, names, keypad, chained=False)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", bc.LENGTHS)
def test_fp64_chained(L, B):
    """x_mid from the raw inputs, whole and split; the unpadded set and the last padding set"""
    sets = bc.keypad_sets(B, L)
    for i in sorted({0, len(sets) - 1}):
        fp64_case(B, L, 5000 + 100 * L + 10 * B + i, "ordinary", sets[i][0], sets[i][1], chained=True)


# ======================================================================================================================
# C. argument checks
# ======================================================================================================================
def test_supported():
    _lib, _ = _api()
    sup = _lib.lib().tan_attnblk_supported
    assert [sup(L, 512, 8, _lib.TAN_BF16) for L in (48, 49, 80, 81)] == [0, 1, 1, 0]
    assert sup(64, 256, 8, _lib.TAN_BF16) == 0 and sup(64, 1024, 8, _lib.TAN_BF16) == 0
    assert sup(64, 512, 4, _lib.TAN_BF16) == 0 and sup(64, 512, 16, _lib.TAN_BF16) == 0
    assert sup(64, 512, 8, _lib.TAN_F32) == 0 and sup(80, 512, 8, _lib.TAN_F32) == 0


@pytest.mark.parametrize("split", [False, True], ids=["whole", "split"])
def test_bad_arguments(split):
    """TAN_ERR_BAD_ARG, and nothing launched: every output buffer, bands and all, keeps its fill.  The buffers are sized for L = 81
    so that the unsupported lengths have room, whatever a launch would do."""
    B, L = 2, 64
    I = bc.random_case(B, 81, 1, "ordinary", device=DEV)
    I["L"] = L
    P = prepare(I, torch.zeros(B, 81, dtype=torch.uint8))
    G = buffers(B, 81, True, True, fill=SENT)

    def untouched(what):
        torch.cuda.synchronize()
        for n, g in G.items():
            assert bool((g[0] == SENT).all()), (what, f"{n} was written")

    for Lbad in (48, 81):
        assert call(desc(P, L=Lbad), G, True, split) == BAD_ARG, Lbad
        assert call(desc(P, L=Lbad), G, False, split) == BAD_ARG, Lbad
        untouched(f"L = {Lbad}")
    assert call(desc(P, B=0), G, True, split) == BAD_ARG
    untouched("B = 0")
    if split:
        assert call(desc(P), G, True, True, part_null=True) == BAD_ARG and call(desc(P), G, False, True, part_null=True) == BAD_ARG
        untouched("part = NULL")
    for keep in (("qkv",), ("attn_o",), ("lse",), ("qkv", "attn_o"), ("qkv", "lse"), ("attn_o", "lse")):
        assert call(desc(P), G, True, split, keep=keep) == BAD_ARG, keep
        untouched(f"save triple with only {keep}")


def test_report_worst_ratios():
    for k in sorted(WORST):
        print(f"WORST {k}: {WORST[k]:.4f}")
