"""Inputs, closed-form expectations, fp64 references and per-element error bounds for the attention core (csrc/tan_attn.hip), in plain
torch on any device.  tests/test_attn_fp64_gpu.py runs the kernels against them; tests/test_attn_cases_cpu.py checks this file.

Layout (as the kernels): qkv [B * L, 3 C] = q | k | v with heads contiguous inside each third, o / d_o [B * L, C], row = b * L + t,
lse [B, H, L], keypad [B, L] uint8 (1 = padded key).  Inside this file everything is [B, H, L, 64].

One-hot / two-hot cases (`twohot_case`): key j carries the +-1 code of its pair index (9 bits, each repeated 7 times, dimension 63
zero), query i is 64 x the code of its target pair.  Scores are integers: 504 on the target pair, at most 392 anywhere else, so
exp(s - max) is exactly 0 off the target in f32 (e^-112 is below the smallest denormal) and P is exactly 1/2, 1/2 or 1.  v and d_o
are small integers.  Everything the kernels then compute in the forward is exact, and so is most of the backward.

Error bounds (`fwd_bounds`, `bwd_bounds`), u = 2^-24, derived from what the kernels do; see the docstring of each."""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -120          # absolute floor: f32 flushes below 2^-126 (a P or a product that small counts as 0)
DH = 64
F64 = torch.float64


# ----------------------------------------------------------------------------------------------------------------------
# layout
# ----------------------------------------------------------------------------------------------------------------------
def split_qkv(qkv, B, L, H):
    """[B * L, 3 C] -> q, k, v as [B, H, L, 64]"""
    q, k, v = qkv.view(B, L, 3, H, DH).permute(2, 0, 3, 1, 4)
    return q, k, v


def split_rows(x, B, L, H):
    """[B * L, C] -> [B, H, L, 64]"""
    return x.view(B, L, H, DH).permute(0, 2, 1, 3)


def merge_rows(x):
    """[B, H, L, 64] -> [B * L, C]"""
    B, H, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, H * DH)


def merge_qkv(q, k, v):
    return torch.cat([merge_rows(q), merge_rows(k), merge_rows(v)], 1)


def live_mask(keypad, B, L, device):
    if keypad is None:
        return torch.ones(B, L, dtype=torch.bool, device=device)
    return keypad.to(device) == 0


# ----------------------------------------------------------------------------------------------------------------------
# which kernel a call enters, and the lengths of its addition chains
# ----------------------------------------------------------------------------------------------------------------------
def path_of(bf16, L):
    """name: the dispatch branch of tan_attn_fwd / _bwd; Lp: the key (and query) extent the kernels walk, padded; nch: the number of
    online-softmax chunks (1: the softmax sees the whole row at once); rnd: half an ulp of the stored type; prnd: the rounding of
    P and dS to the MFMA operand type; nkb: 32-row blocks (the template argument of the short and mid kernels)."""
    nkb = (L + 31) // 32
    if not bf16:
        return dict(name="f32", Lp=(L + 63) // 64 * 64, nch=1, rnd=U, prnd=0.0, nkb=nkb)
    if L <= 128:
        return dict(name="short", Lp=32 * nkb, nch=1, rnd=2.0 ** -8, prnd=2.0 ** -8, nkb=nkb)
    if L <= 288:
        return dict(name="mid", Lp=32 * nkb, nch=(nkb + 2) // 3, rnd=2.0 ** -8, prnd=2.0 ** -8, nkb=nkb)
    nb = (L + 127) // 128
    return dict(name="long", Lp=128 * nb, nch=nb, rnd=2.0 ** -8, prnd=2.0 ** -8, nkb=nkb)


# ----------------------------------------------------------------------------------------------------------------------
# key padding patterns
# ----------------------------------------------------------------------------------------------------------------------
def pad_pattern(name, L, seed):
    """[L] uint8, or None where the pattern does not fit the length.  lead<n> / mid<n>: the whole first n keys / the whole second
    run of n keys (n = 32: a wave's key block, 96: a chunk of the mid forward, 128: a block of the long kernels)."""
    p = torch.zeros(L, dtype=torch.uint8)
    if name == "none":
        return p
    if name == "tail":
        if L < 2:
            return None
        p[L - max(1, L // 5):] = 1
    elif name == "scatter":
        if L < 3:
            return None
        g = torch.Generator().manual_seed(seed)
        p[torch.randperm(L, generator=g)[:max(1, L // 7)]] = 1
    elif name.startswith("lead"):
        n = int(name[4:])
        if L <= n:
            return None
        p[:n] = 1
    elif name.startswith("mid"):
        n = int(name[3:])
        if L <= 2 * n:
            return None
        p[n:2 * n] = 1
    elif name == "butlast":
        if L < 2:
            return None
        p[:L - 1] = 1
    elif name == "all":
        p[:] = 1
    else:
        raise ValueError(name)
    return p


PATTERNS = ["none", "tail", "scatter", "lead32", "lead96", "lead128", "mid32", "mid96", "mid128", "butlast", "all"]


def keypad_sets(B, L):
    """A list of (names, keypad [B, L] uint8 or None): every pattern that fits L, B at a time, a different one per video; "all" only
    next to live videos (B > 1).  The first set of a B = 1 list is unpadded (keypad None: the kernels' null-pointer branch)."""
    fit = [n for n in PATTERNS if pad_pattern(n, L, 0) is not None and not (B == 1 and n == "all")]
    sets = [(("none",) * B, None)]
    rest = fit[1:] if B == 1 else fit
    for s in range(0, len(rest), B):
        names = [rest[(s + i) % len(rest)] for i in range(B)]
        if B > 1 and all(n == "all" for n in names):
            names[0] = "none"
        sets.append((tuple(names), torch.stack([pad_pattern(n, L, 17 * s + i) for i, n in enumerate(names)])))
    return sets


# ----------------------------------------------------------------------------------------------------------------------
# one-hot / two-hot cases
# ----------------------------------------------------------------------------------------------------------------------
def codes(n, device="cpu"):
    """[n, 64] f32: the 9 bits of the index as +-1, each 7 times, dimension 63 zero"""
    assert n <= 512
    idx = torch.arange(n, device=device)
    bits = ((idx[:, None] >> torch.arange(9, device=device)) & 1) * 2 - 1
    return torch.cat([bits.repeat_interleave(7, dim=1), torch.zeros(n, 1, dtype=bits.dtype, device=device)], 1).float()


SCORE_HOT, SCORE_NEXT = 504.0, 392.0


def twohot_case(B, L, H, seed, keypad=None, onehot=False, vmax=6, device="cpu"):
    """dict: qkv [B * L, 3 C] f32 and d_o [B * L, C] f32 (every value exact in bf16), keypad, P [B, H, L, L] f64 (closed form: 1 / count
    on the live keys of the query's target pair; 0 in a video with every key padded), lse [B, H, L] f64 (504 + log count, -inf)."""
    g = torch.Generator().manual_seed(seed)
    per = 1 if onehot else 2
    code = codes((L + per - 1) // per, device)
    perm = torch.rand(B, H, L, generator=g).argsort(-1)
    pair_of_key = torch.empty(B, H, L, dtype=torch.long)
    pair_of_key.scatter_(2, perm, (torch.arange(L) // per).expand(B, H, L).contiguous())
    live = live_mask(keypad, B, L, "cpu")
    w = live.float()
    w[~live.any(1)] = 1.0                                  # a video without a live key: the targets do not matter
    tkey = torch.multinomial(w, H * L, replacement=True, generator=g).view(B, H, L)
    tgt = pair_of_key.gather(2, tkey)
    v = torch.randint(-vmax, vmax + 1, (B, H, L, DH), generator=g).float().to(device)
    d_o = torch.randint(-vmax, vmax + 1, (B, H, L, DH), generator=g).float().to(device)
    pair_of_key, tgt, live = pair_of_key.to(device), tgt.to(device), live.to(device)
    k, q = code[pair_of_key], 64.0 * code[tgt]
    hot = (pair_of_key[:, :, None, :] == tgt[:, :, :, None]) & live[:, None, None, :]
    cnt = hot.sum(-1)
    P = hot.to(F64) / cnt.clamp(min=1).to(F64)[..., None]
    lse = torch.where(cnt > 0, SCORE_HOT + cnt.clamp(min=1).to(F64).log(), torch.full((), -math.inf, dtype=F64, device=device))
    return dict(qkv=merge_qkv(q, k, v), d_o=merge_rows(d_o), keypad=None if keypad is None else keypad.to(device), P=P, lse=lse,
                cnt=cnt, B=B, L=L, H=H)


def assert_exact_conditions(m):
    """What keeps a two-hot case exact, from the data (m = manual(..., P = closed form)): every f32 accumulator's terms add up to
    less than 2^24 in magnitude, in units of the smallest step that occurs (1/2 for P v and P^T dO: twice the sum is an integer), and
    every o a kernel stores as bf16 has at most 8 significant bits (halves, so |2 o| <= 256).  dv is a sum over the queries that
    target a key -- every query of the video where one key is live -- so its exact f32 value can need more bits: the kernels must
    then store that value ROUNDED to nearest even, which is what `.to(bfloat16)` of the exact value gives."""
    aq, ak, av, ado = (m[n].abs() for n in ("q", "k", "v", "do"))
    assert float((aq @ ak.transpose(-1, -2)).max()) < 2 ** 24                       # scores (before the exact 1/8)
    assert float((ado @ av.transpose(-1, -2)).max()) < 2 ** 24                      # dP
    assert float((2 * m["P"] @ av).max()) < 2 ** 24 and float((2 * m["P"].transpose(-1, -2) @ ado).max()) < 2 ** 24
    for x in (m["o"], m["dv"]):
        assert bool((2 * x == (2 * x).round()).all())
    assert float((2 * m["o"]).abs().max()) <= 256


# ----------------------------------------------------------------------------------------------------------------------
# fp64: every quantity of the forward and the backward, by hand (P given: the closed form of a two-hot case)
# ----------------------------------------------------------------------------------------------------------------------
def manual(qkv, keypad, d_o, B, L, H, P=None, lse=None):
    """o = P v, dP = dO v^T, delta = rowsum(P dP), dS = P (dP - delta), dq = dS k / 8, dk = dS^T q / 8, dv = P^T dO with
    P = softmax(q k^T / 8 + key padding) and lse its log-sum-exp -- or the P / lse handed in.  A video whose keys are all padded
    has P = 0 and lse = -inf (what the kernels define; torch gives NaN there)."""
    q, k, v = (t.to(F64) for t in split_qkv(qkv, B, L, H))
    do = split_rows(d_o.to(F64), B, L, H)
    live = live_mask(keypad, B, L, qkv.device)
    mask = live[:, None, None, :]
    S = (q @ k.transpose(-1, -2)) * 0.125
    dead = (~live.any(1))[:, None, None, None]
    Sm = S.masked_fill(~mask, -math.inf)
    mrow = torch.where(dead, torch.zeros((), dtype=F64, device=S.device), Sm.amax(-1, keepdim=True))
    if P is None:
        E = (Sm - mrow).exp()
        lsum = E.sum(-1, keepdim=True)
        P = torch.where(dead, torch.zeros_like(E), E / lsum)
        lse = torch.where(dead, torch.full_like(lsum, -math.inf), mrow + lsum.log())[..., 0]
    o = P @ v
    dP = do @ v.transpose(-1, -2)
    delta = (P * dP).sum(-1)
    dS = P * (dP - delta[..., None])
    dq, dk, dv = (dS @ k) * 0.125, (dS.transpose(-1, -2) @ q) * 0.125, P.transpose(-1, -2) @ do
    return dict(q=q, k=k, v=v, do=do, S=S, mrow=mrow[..., 0], P=P, lse=lse, o=o, dP=dP, delta=delta, dS=dS, dq=dq, dk=dk, dv=dv,
                live=live, B=B, L=L, H=H)


def attn_ref(qkv, keypad, B, L, H):
    """the formula of the model (tests/test_kernels_gpu.py:_attn_ref) and logsumexp of the same scores, in the dtype of qkv"""
    q, k, v = split_qkv(qkv, B, L, H)
    s = (q * 0.125) @ k.transpose(-1, -2)
    if keypad is not None:
        s = s.masked_fill(keypad.bool()[:, None, None, :], -math.inf)
    return merge_rows(torch.softmax(s, -1) @ v), torch.logsumexp(s, -1)


def ref_autograd(qkv, keypad, d_o, B, L, H):
    """o [B * L, C], lse [B, H, L], dqkv [B * L, 3 C] in fp64 from attn_ref + autograd.  A video with every key padded is computed
    unpadded (videos do not interact) and then set to what the kernels define: o = 0, lse = -inf, dqkv = 0."""
    kp, deadv = keypad, None
    if keypad is not None:
        deadv = keypad.bool().all(1)
        kp = keypad.clone()
        kp[deadv] = 0
    x = qkv.to(F64).detach().clone().requires_grad_(True)
    o, lse = attn_ref(x, kp, B, L, H)
    o.backward(d_o.to(F64))
    o, lse, g = o.detach().clone(), lse.detach().clone(), x.grad
    if deadv is not None and bool(deadv.any()):
        o.view(B, L, -1)[deadv] = 0
        g.view(B, L, -1)[deadv] = 0
        lse[deadv] = -math.inf
    return o, lse, g


# ----------------------------------------------------------------------------------------------------------------------
# error bounds
# ----------------------------------------------------------------------------------------------------------------------
def _common(m, pc):
    """e_S: a score is an f32 sum of 64 exact products (bf16 x bf16, or the f32 fma chain), times the exact 1/8, plus the exact
    0 / -inf of the padding: 64 u sum_d |q k| / 8.  chain_l: the additions a row's sum of exponentials goes through -- at most
    half the padded row per lane (16 per 32-key block in the bf16 kernels, a quarter of the row in the f32 one) plus the lane
    exchanges and the chunks' running sum."""
    aq, ak = m["q"].abs(), m["k"].abs()
    eS = 64 * U * (aq @ ak.transpose(-1, -2)) * 0.125
    lse_f = torch.where(torch.isinf(m["lse"]), torch.zeros_like(m["lse"]), m["lse"])
    return eS, lse_f, pc["Lp"] / 2 + 4


def fwd_bounds(m, pc):
    """Per-element bounds of o [B, H, L, 64] and lse [B, H, L] (entries of an all-padded video: bound 0 for lse, TINY for o).
    The computed P_j is exp(S^_j - m^) / sum_k exp(S^_k - m^): the max m^ cancels, so what remains per key is
      rho_j = e_S(j)  +  2 u |S_j - m|  (the subtraction, and the product with log2 e inside __expf / expf; with an online softmax
              the same total, split between exp(S_j - m_chunk) and the alphas exp(m_chunk - m))  +  (2 + 3 nch) u  (exp itself
              1 ulp, and per chunk: alpha's ulp, its product with l and with o),
    and the sum's own error: the P-weighted mean of rho plus chain_l u, and 2 u for 1 / l and the product.
      o   = sum_j P_j v_j:  sum |P v| (relP + prnd: P rounded to bf16 as an MFMA operand) + (Lp + 2) u sum |P v| (one addition per
            key at most, + scale), then the store.
      lse = m + log l:  P-weighted (e_S + 2 u |S - m|)  +  (chain_l + 3 nch + 4) u (the sum's chain, the alphas, exp's ulp: relative
            errors of l, absolute ones of log l)  +  2 u |log l| (logf to 2 ulp)  +  u |lse| (the final addition)."""
    eS, lse_f, chain_l = _common(m, pc)
    P, S = m["P"], m["S"]
    gap = torch.where(P > 0, (m["mrow"][..., None] - S).abs(), torch.zeros_like(S))
    rho = eS + 2 * U * gap + (2 + 3 * pc["nch"]) * U
    rhobar = (P * rho).sum(-1, keepdim=True)
    relP = rho + rhobar + (chain_l + 2) * U
    relPr = relP + pc["prnd"] + relP * pc["prnd"]
    av = m["v"].abs()
    eP = P * relPr + TINY
    e_o = eP @ av + (pc["Lp"] + 2) * U * (P @ av)
    b_o = e_o + pc["rnd"] * (m["o"].abs() + e_o) + TINY
    b_lse = (P * (eS + 2 * U * gap)).sum(-1) + (chain_l + 3 * pc["nch"] + 4) * U + 2 * U * (lse_f - m["mrow"]).abs() + U * lse_f.abs()
    b_lse = torch.where(torch.isinf(m["lse"]), torch.zeros_like(b_lse), b_lse)
    return b_o, b_lse


def bwd_bounds(m, pc, e_o, e_lse):
    """Per-element bounds of dq, dk, dv [B, H, L, 64] for a backward fed an o that is within e_o [B, H, L, 64] and an lse within
    e_lse [B, H, L] of the reference's (fed the rounded reference: 2^-8 |o| or u |o|, and u |lse|; fed the forward kernel's own: its
    bounds).
      P~ = exp(S^ - lse~):  relative  pi = e_S + e_lse + u |S| + 2 u |S - lse| + 2 u   (the two additions of the argument, the product
           with log2 e, exp 1 ulp);  + prnd where P is rounded to bf16 as the operand of dv
      dP = dO v^T:  64 u sum_d |dO v|
      delta:  short bf16 kernel  sum_j P~ dP^  -> sum_j P (|dP| pi + e_dP) + (Lp / 2 + 2) u sum_j P |dP|
              every other kernel rowsum(dO o~)  -> sum_d |dO| e_o + 64 u sum_d |dO o|
      dS = P~ (dP^ - delta^):  |dS| pi + P (e_dP + e_delta) + 2 u P (|dP| + |delta|) (the subtraction and the product); + prnd (bf16
           operand of dq and dk)
      dq = dS k / 8, dk = dS^T q / 8, dv = P~^T dO:  the operand's error through the magnitudes + (Lp + 2) u sum of magnitudes;
           the 1/8 is exact; then the store."""
    eS, lse_f, _ = _common(m, pc)
    P, S, dP, dS, do = m["P"], m["S"], m["dP"], m["dS"], m["do"]
    x = torch.where(P > 0, (S - lse_f[..., None]).abs(), torch.zeros_like(S))
    pi = eS + e_lse[..., None] + U * S.abs() + 2 * U * x + 2 * U
    e_dP = 64 * U * (do.abs() @ m["v"].abs().transpose(-1, -2))
    if pc["name"] == "short":
        e_delta = (P * (dP.abs() * pi + e_dP)).sum(-1) + (pc["Lp"] / 2 + 2) * U * (P * dP.abs()).sum(-1)
    else:
        e_delta = (do.abs() * e_o).sum(-1) + 64 * U * (do * m["o"]).abs().sum(-1)
    mag = dP.abs() + m["delta"].abs()[..., None]
    e_dS = dS.abs() * pi + P * (e_dP + e_delta[..., None]) + 2 * U * P * mag + TINY * mag
    e_dS = e_dS + pc["prnd"] * (dS.abs() + e_dS)
    ch = (pc["Lp"] + 2) * U
    e_dq = ((e_dS + ch * dS.abs()) @ m["k"].abs()) * 0.125
    e_dk = ((e_dS + ch * dS.abs()).transpose(-1, -2) @ m["q"].abs()) * 0.125
    piP = pi + pc["prnd"] + pi * pc["prnd"]
    e_dv = (P * piP + TINY + ch * P).transpose(-1, -2) @ do.abs()
    return tuple(e + pc["rnd"] * (r.abs() + e) + TINY for e, r in ((e_dq, m["dq"]), (e_dk, m["dk"]), (e_dv, m["dv"])))


def fed_errors(m, pc):
    """e_o, e_lse of a backward that is fed the reference's o and lse rounded to the storage types"""
    lse_f = torch.where(torch.isinf(m["lse"]), torch.zeros_like(m["lse"]), m["lse"])
    return pc["rnd"] * m["o"].abs(), U * lse_f.abs()


def gbias_chain(pc, B, L):
    """the longest chain of f32 additions behind an entry of g_b_qkv: fused (short, mid) the 32 rows a wave parked, then one atomic
    per (video, wave) onto the starting value; otherwise tan_colsum_acc over B L rows, in whatever order (any order of n additions
    is at most n - 1 deep)"""
    return 32 + B * pc["nkb"] + 1 if pc["name"] in ("short", "mid") else B * L + 1
