"""Inputs, closed-form expectations, fp64 references and per-element error bounds for the fused attention branch
(csrc/tan_attnblk.hip: x_mid = x_in + out_proj(MHA(xn1)) in one launch, C = 512, H = 8, 48 < L <= 80), in plain torch on any device.
tests/test_attnblk_fp64_gpu.py runs the kernels against them; tests/test_attnblk_cases_cpu.py checks this file.  The padding patterns,
the +-1 codes, the fp64 attention by hand and the softmax bounds are those of tests/attn_cases.py.

Layout (as the kernels): xn1, x_in, attn_o, x_mid [B * L, 512]; qkv [B * L, 1536] = q | k | v, heads contiguous inside each third;
lse [B, 8, L]; keypad [B, L] uint8 (1 = padded key); w_in [1536, 512], w_out [512, 512] (nn.Linear: y = x w^T + b).

Exact cases (`exact_case`).  The kernel computes q, k and v itself, so the two-hot softmax of attn_cases is built through xn1 and w_in:
  xn1 channels   0 ..  63   the +-1 code of the row's own pair as a KEY (pairs: a random pairing of the rows of a video; the last
                            pair is a singleton when L is odd)
                64 .. 127   the code of the pair the row targets as a QUERY in the even heads (a random LIVE key's pair)
               128 .. 191   the same for the odd heads (another random live key's pair)
               192 .. 511   integers in [-4, 4]
  w_q[h]   64 x a signed permutation (one per head) of the target code's channels;  w_k[h]  the same signed permutation of the key
           code's channels, unscaled: q = 64 code(target), k = code(own pair), both permuted and signed per head, so q . k / 8 is 504 on
           the target pair and at most 392 anywhere else -- but only between the q and the k of the SAME head
  w_v[h]   each feature +- one integer channel +- another;  b_q = b_k = 0, b_v integers in [-2, 2]:  |v| <= 10, distinct per row and head
  w_out    one entry of +-1 .. +-3 per output feature and head pair (four per row);  b_out in [-8, 8], x_in in [-200, 200] (8 bits)
Every term of every GEMM is an integer or a half, every partial sum stays far below 2^24 of them, so the f32 sums are exact in any
order; exp(s - max) is exactly 0 off the target (e^-112 is below the smallest f32 denormal), P is exactly 1/2 or 1 and o = the mean of
the target v rows is exact in bf16.  x_mid = x_in + o w_out^T + b_out is an exact f32 half-integer of up to ~300: those below 128 need no
more than 8 bits, the rest must be stored ROUNDED to nearest even, which is what `.to(bfloat16)` of the exact value gives.  Row 0 of every
video targets the pair of the LAST row in the even heads and the last row targets its own pair in the odd heads (where that key is
live): the panel rows past L repeat the last row, so a kernel that let them through as keys would count that pair 1 + (LP - L) times.

fp64 stages (`qkv_stage`, `attn_stage`, `xmid_stage`, `chained_xmid`) and their bounds: see each docstring.  u = 2^-24."""
import math

import torch

import attn_cases as ac

U, TINY, F64 = ac.U, ac.TINY, ac.F64
RND = 2.0 ** -8             # half an ulp of bf16, relative
C, H, DH = 512, 8, 64
LENGTHS = [49, 56, 63, 64, 65, 72, 79, 80]
N_INT = C - 192             # integer channels of xn1 in an exact case


def template_of(L):
    """what tan_attnblk_fwd instantiates for L: NRB16 16-row blocks of GEMM-a, NKB 32-key blocks, LP image rows, XROWS panel rows,
    NIDLE waves without an attention unit and the NKV 8-row pieces of k and v each of them copies out per head pair"""
    assert 48 < L <= 80
    nrb16 = 4 if L <= 64 else 5
    nkb = (nrb16 + 1) // 2
    lp = 32 * nkb
    nidle = 8 - 2 * nkb
    return dict(nrb16=nrb16, nkb=nkb, LP=lp, XROWS=16 * nrb16, NIDLE=nidle, NKV=4 * (lp // 8) // nidle)


def path_of(L):
    """the attention unit is attn_fwd_short_kernel's: attn_cases' bounds of the short bf16 branch, with the same padded extent"""
    pc = ac.path_of(True, L)
    assert pc["name"] == "short" and pc["Lp"] == template_of(L)["LP"]
    return pc


def keypad_sets(B, L):
    """attn_cases.keypad_sets, and for B = 3 one more set with every key of the MIDDLE video padded (the sets of attn_cases put such a
    video first at L > 64 and last at L <= 64)"""
    sets = ac.keypad_sets(B, L)
    if B == 3:
        names = ("scatter", "all", "butlast")
        sets.append((names, torch.stack([ac.pad_pattern(n, L, 900 + i) for i, n in enumerate(names)])))
    return sets


def cycle_keypad(B, L):
    """[B, L]: every pattern that fits L in turn, video by video (the large batches)"""
    names = [n for n in ac.PATTERNS if ac.pad_pattern(n, L, 0) is not None]
    return torch.stack([ac.pad_pattern(names[b % len(names)], L, b) for b in range(B)])


# ----------------------------------------------------------------------------------------------------------------------
# exact cases
# ----------------------------------------------------------------------------------------------------------------------
def exact_case(B, L, seed, keypad=None, device="cpu"):
    """dict of inputs (f32, every value exact in bf16; biases f32), of the closed forms qkv [B L, 1536] f32, P [B, 8, L, L] f64,
    cnt [B, 8, L], lse [B, 8, L] f64 (504 + log cnt; -inf in a video with every key padded), o [B L, 512] f64 (P v; 0 there) and
    x_mid [B L, 512] f64 (exact, not yet rounded), and of what built them (pair_of_key [B, L], tgt [B, 2, L])."""
    g = torch.Generator().manual_seed(seed)
    R = B * L
    code = ac.codes((L + 1) // 2)
    perm = torch.rand(B, L, generator=g).argsort(-1)
    pair_of_key = torch.empty(B, L, dtype=torch.long)
    pair_of_key.scatter_(1, perm, (torch.arange(L) // 2).expand(B, L).contiguous())
    live = ac.live_mask(keypad, B, L, "cpu")
    w = live.float()
    w[~live.any(1)] = 1.0                                  # a video without a live key: the targets do not matter
    tkey = torch.multinomial(w, 2 * L, replacement=True, generator=g).view(B, 2, L)
    last = live[:, L - 1]
    tkey[last, 0, 0] = L - 1                               # the pair of the last row, which the panel repeats up to LP
    tkey[last, 1, L - 1] = L - 1
    tgt = pair_of_key[:, None, :].expand(B, 2, L).gather(2, tkey)
    xn1 = torch.zeros(B, L, C)
    xn1[:, :, 0:64] = code[pair_of_key]
    xn1[:, :, 64:128] = code[tgt[:, 0]]
    xn1[:, :, 128:192] = code[tgt[:, 1]]
    xn1[:, :, 192:] = torch.randint(-4, 5, (B, L, N_INT), generator=g).float()
    xn1 = xn1.view(R, C)
    # weights
    w_in, b_in = torch.zeros(3 * C, C), torch.zeros(3 * C)
    hperm = torch.stack([torch.randperm(DH, generator=g) for _ in range(H)])            # [H, 64]
    hsign = torch.randint(0, 2, (H, DH), generator=g).float() * 2 - 1
    feat = torch.arange(C)
    hd, dd = feat // DH, feat % DH
    w_in[feat, 64 + 64 * (hd % 2) + hperm[hd, dd]] = 64.0 * hsign[hd, dd]
    w_in[C + feat, hperm[hd, dd]] = hsign[hd, dd]
    c1 = torch.randint(0, N_INT, (C,), generator=g)
    c2 = (c1 + 1 + torch.randint(0, N_INT - 1, (C,), generator=g)) % N_INT               # != c1
    s1, s2 = (torch.randint(0, 2, (C,), generator=g).float() * 2 - 1 for _ in range(2))
    w_in[2 * C + feat, 192 + c1] = s1
    w_in[2 * C + feat, 192 + c2] = s2
    b_in[2 * C:] = torch.randint(-2, 3, (C,), generator=g).float()
    w_out = torch.zeros(C, C)
    for hp in range(4):
        kcol = 128 * hp + torch.randint(0, 128, (C,), generator=g)
        w_out[feat, kcol] = (torch.randint(1, 4, (C,), generator=g) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)).float()
    b_out = torch.randint(-8, 9, (C,), generator=g).float()
    x_in = torch.randint(-200, 201, (R, C), generator=g).float()
    I = dict(xn1=xn1, x_in=x_in, w_in=w_in, b_in=b_in, w_out=w_out, b_out=b_out, pair_of_key=pair_of_key, tgt=tgt, live=live)
    I = {k: v.to(device) for k, v in I.items()}
    # closed forms
    xv = I["xn1"].view(B, L, C)
    hperm, hsign = hperm.to(device), hsign.to(device)
    cd = code.to(device)
    tg = I["tgt"][:, torch.arange(H, device=device) % 2]                                   # [B, H, L]
    q = 64.0 * hsign[None, :, None, :] * cd[tg].gather(3, hperm[None, :, None, :].expand(B, H, L, DH))
    k = hsign[None, :, None, :] * cd[I["pair_of_key"]][:, None].expand(B, H, L, DH).gather(3, hperm[None, :, None, :].expand(B, H, L, DH))
    xi = xv.reshape(R, C)[:, 192:]
    v = ac.split_rows(s1.to(device) * xi[:, c1.to(device)] + s2.to(device) * xi[:, c2.to(device)] + I["b_in"][2 * C:], B, L, H)
    hot = (I["pair_of_key"][:, None, None, :] == tg[:, :, :, None]) & I["live"][:, None, None, :]
    cnt = hot.sum(-1)
    P = hot.to(F64) / cnt.clamp(min=1).to(F64)[..., None]
    lse = torch.where(cnt > 0, ac.SCORE_HOT + cnt.clamp(min=1).to(F64).log(), torch.full((), -math.inf, dtype=F64, device=device))
    o = ac.merge_rows(P @ v.double())
    x_mid = I["x_in"].double() + o @ I["w_out"].double().T + I["b_out"].double()
    I.update(qkv=ac.merge_qkv(q, k, v), P=P, cnt=cnt, lse=lse, o=o, x_mid=x_mid, B=B, L=L,
             keypad=None if keypad is None else keypad.to(device))
    return I


def assert_exact_conditions(c):
    """What keeps an exact case exact, from the data: every input is a bf16 value; every f32 accumulator's terms add up to less than
    2^24 in magnitude, in units of the smallest step that occurs (1 in GEMM-a and the scores, 1/2 in P v, GEMM-b and the epilogue);
    q, k, v and o have at most 8 significant bits; a non-target live key is at least SCORE_HOT - SCORE_NEXT = 112 below the target
    (the margin at which f32 exp returns exactly 0), and so is the all-zero k of an image row the kernel zeroes (score 0)."""
    B, L = c["B"], c["L"]
    for n in ("xn1", "x_in", "w_in", "w_out"):
        assert torch.equal(c[n].bfloat16().float(), c[n]), n
    for n in ("b_in", "b_out"):
        assert torch.equal(c[n], c[n].round()), n
    assert float((c["xn1"].abs() @ c["w_in"].abs().T + c["b_in"].abs()).max()) < 2 ** 24
    qkv = c["qkv"]
    assert torch.equal(qkv.bfloat16().float(), qkv) and torch.equal(qkv, qkv.round())
    q, k, v = ac.split_qkv(qkv, B, L, H)
    S = (q @ k.transpose(-1, -2)) * 0.125
    assert float((q.abs() @ k.abs().transpose(-1, -2)).max()) < 2 ** 24
    hot = c["P"] > 0
    alive = c["live"].any(1)
    assert bool((S[hot] == ac.SCORE_HOT).all())
    other = (~hot) & c["live"][:, None, None, :]
    assert float(S.masked_fill(~other, -math.inf).max()) <= ac.SCORE_NEXT and ac.SCORE_HOT - ac.SCORE_NEXT >= 112 and math.exp(-112) < 2.0 ** -149
    assert int(c["cnt"][alive].min()) >= 1 and int(c["cnt"].max()) <= 2 and bool((c["cnt"][~alive] == 0).all())
    assert float((2 * c["P"] @ v.abs().double()).max()) < 2 ** 24
    o2 = 2 * c["o"]
    assert torch.equal(o2, o2.round()) and float(o2.abs().max()) <= 256
    assert torch.equal(c["o"].bfloat16().double(), c["o"])
    assert float((o2.abs() @ c["w_out"].abs().double().T + 2 * c["b_out"].abs() + 2 * c["x_in"].abs()).max()) < 2 ** 24
    x2 = 2 * c["x_mid"]
    assert torch.equal(x2, x2.round()) and torch.equal(c["x_mid"].float().double(), c["x_mid"])


# ----------------------------------------------------------------------------------------------------------------------
# random cases
# ----------------------------------------------------------------------------------------------------------------------
SCALES = {"ordinary": 1.5, "large": 10.0}        # standard deviation of q and k: scores of 2.25, and of 100 (|score| up to ~450)


def random_case(B, L, seed, sname, device="cpu"):
    """bf16 xn1 ~ N(0, 1), x_in ~ 1.5 N(0, 1); w_q, w_k ~ scale / sqrt(512), w_v, w_out ~ 1 / sqrt(512); f32 biases ~ 0.1 N(0, 1)"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)                          # noqa: E731
    R, sc = B * L, SCALES[sname]
    w_in = rn(3 * C, C) * C ** -0.5
    w_in[:2 * C] *= sc
    BF = torch.bfloat16
    return dict(xn1=rn(R, C).to(BF), x_in=(rn(R, C) * 1.5).to(BF), w_in=w_in.to(BF), b_in=rn(3 * C) * 0.1,
                w_out=(rn(C, C) * C ** -0.5).to(BF), b_out=rn(C) * 0.1, B=B, L=L)


# ----------------------------------------------------------------------------------------------------------------------
# fp64 stages: the reference of one stage from the values the kernel read, and the bound of the kernel's output against it
# ----------------------------------------------------------------------------------------------------------------------
def _d(x):
    return x.to(F64)


def _store(ref, e):
    """a value within e of ref, stored as bf16"""
    return e + RND * (ref.abs() + e) + TINY


def qkv_stage(xn1, w_in, b_in):
    """qkv = xn1 w_in^T + b_in.  The accumulator starts from the f32 bias and takes K = 512 products of two bf16 values (each exact in
    f32) in 16 MFMA steps: whatever the order, at most 512 additions deep:  e = 512 u (sum_k |x w| + |b|), then the bf16 store.
    Returns ref, bound, e (the bound before the store)."""
    ref = _d(xn1) @ _d(w_in).T + _d(b_in)
    e = 512 * U * (_d(xn1).abs() @ _d(w_in).abs().T + _d(b_in).abs())
    return ref, _store(ref, e), e


def attn_stage(qkv, keypad, B, L):
    """fp64 attention of the qkv handed in (the kernel's own saved rows) by attn_cases.manual, with attn_cases.fwd_bounds of the short
    bf16 branch: scores of K = 64, softmax terms, P rounded to bf16, the O chain over LP keys, the bf16 store of O; lse in f32.
    Returns m (o [B, 8, L, 64], lse [B, 8, L], ...), b_o, b_lse."""
    m = ac.manual(_d(qkv), keypad, torch.zeros(B * L, C, dtype=F64, device=qkv.device), B, L, H)
    b_o, b_lse = ac.fwd_bounds(m, path_of(L))
    return m, b_o, b_lse


def xmid_stage(attn_o, x_in, w_out, b_out, split, e_o=None):
    """x_mid = x_in + attn_o w_out^T + b_out from the attn_o handed in (the kernel's own saved rows; or a reference within e_o).
      whole launch   one f32 accumulator over the four head pairs: K = 512 products, then + b_out, + x_in:  514 u M
      split launch   a plane per head pair (K = 128), the four planes added in order (3 additions), + b_out, + x_in:  133 u M
    with M = sum_k |o w| + |b_out| + |x_in|; then the bf16 store.  Returns ref, bound."""
    o, w = _d(attn_o), _d(w_out)
    ref = _d(x_in) + o @ w.T + _d(b_out)
    mag = o.abs() @ w.abs().T + _d(b_out).abs() + _d(x_in).abs()
    e = ((128 + 3 + 2) if split else (512 + 2)) * U * mag
    if e_o is not None:
        e = e + e_o @ w.abs().T + ((128 + 3 + 2) if split else (512 + 2)) * U * (e_o @ w.abs().T)
    return ref, _store(ref, e)


def chained_xmid(I, keypad, split):
    """x_mid from the raw inputs, fp64 all the way, and its bound: the stages' bounds pushed through the stages.
      qkv~   within b = qkv_stage's bound of qkv (e_q, e_k, e_v per element)
      S~     |dS_ij| <= (sum_d |q_i| e_k_j + e_q_i |k_j| + e_q_i e_k_j) / 8;  D_i = its largest over the live keys j
      P      P_j = exp(S_j) / sum exp(S): every term moves by a factor within exp(+-D_i), so |P~_j - P_j| <= P_j expm1(2 D_i)
      o      |P~ v~ - P v| <= expm1(2 D) P (|v| + e_v) + P e_v, plus the attention's own bound (attn_cases.fwd_bounds at the reference,
             magnitudes grown by (1 + expm1(2 D)) (1 + 2^-7)): e_o
      x_mid  xmid_stage's bound with o within e_o.
    The bound is wide (D is a worst case over 64 half-ulp errors of the same sign): this check ties the stages together, the
    per-stage checks are the sharp ones.  Returns ref, bound."""
    B, L = I["B"], I["L"]
    qkv, b_qkv, _ = qkv_stage(I["xn1"], I["w_in"], I["b_in"])
    m = ac.manual(qkv, keypad, torch.zeros(B * L, C, dtype=F64, device=qkv.device), B, L, H)
    eq, ek, ev = ac.split_qkv(b_qkv, B, L, H)
    aq, ak = m["q"].abs(), m["k"].abs()
    dS = (aq @ ek.transpose(-1, -2) + eq @ ak.transpose(-1, -2) + eq @ ek.transpose(-1, -2)) * 0.125
    D = dS.masked_fill(~m["live"][:, None, None, :], 0.0).amax(-1, keepdim=True)
    grow = torch.expm1(2 * D)
    P = m["P"]
    e_in = grow * (P @ (m["v"].abs() + ev)) + P @ ev
    b_o, _ = ac.fwd_bounds(m, path_of(L))
    e_o = ac.merge_rows(e_in + b_o * (1 + grow) * (1 + 2 * RND))
    return xmid_stage(ac.merge_rows(m["o"]), I["x_in"], I["w_out"], I["b_out"], split, e_o=e_o)


def worst_ratio(got, ref, bound):
    """observed / bound over the elements with a positive bound (the others must be exact: returns inf if not)"""
    err = (_d(got) - ref).abs()
    bound = bound.expand_as(err)
    pos = bound > 0
    if not bool((err[~pos] == 0).all()):
        return math.inf
    r = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    return r if math.isfinite(r) else math.inf
