"""Inputs, closed forms, fp64 references and per-element bounds for the row-panel MLP kernels (csrc/tan_panel.hip).  Pure torch,
device-agnostic; checked on the CPU by test_panel_cases_cpu.py, used on the GPU by test_panel_fp64_gpu.py.

A. pack_index_map: the whole element index map of tan_pack_weights for the three tile formats.
B. selector weights (one 1.0 per output row) and inputs on dyadic grids: every MFMA sum is a single non-zero product, every
   addition is exact in f32, so the kernel's outputs have closed forms that hold bit for bit.
C. fwd_reference / bwd_reference: float64 evaluations of the model's formulas, stage by stage, each with the bound of the kernel's
   f32 / bf16 evaluation of that stage.  A stage takes its input either from what the kernel STORED for the stage before it
   ("fed": the input is exact, an upstream error cannot hide or cancel) or from the reference with its bound ("chained").

Error model (u = 2^-24, the unit roundoff of f32; every bound keeps its second-order terms, no factor is fitted):
  an f32 operation    fl(a op b) = (a op b)(1 + d), |d| <= u.  A fused multiply-add rounds once where the separate operations round
                      twice, so counting them separately covers both.
  a sum of m terms    in ANY order or tree: <= gamma(m - 1) sum |terms|, gamma(n) = n u / (1 - n u).  Adding an exact zero does not
                      round, so m counts the non-zero products of a dot product (+ 1 when the accumulator starts from the bias):
                      m = K for dense weights, 1 for a selector.  The same bound covers the whole-panel kernels (K = 2048 in
                      sequence) and the split ones (eight planes of K = 256, added in chunk order): both are trees over the same terms.
  a reduction         of `depth` successive roundings per path (lane-local additions, then the cross-lane / cross-wave levels):
                      <= gamma(depth) sum |terms|
  v_exp_f32, v_rcp_f32, v_rsq_f32 (exp2, rcp, rsqrtf)   1 ulp, i.e. a relative error of at most 2 u each
  a bf16 store        half an ulp of the binade of the f32 value that is rounded: hu(|ref| + e), hu(y) = 2^(floor(log2 y) - 8)
                      (<= 2^-8 |y|); e is the bound of the f32 value.  An exact zero stays exact.
"""
import math

import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U = 2.0 ** -24
C, FF, QKV = 512, 2048, 1536
WAVES = 8
HW_U = 2.0                        # v_exp_f32 / v_rcp_f32 / v_rsq_f32: 1 ulp <= 2 u relative
# reduction depths (successive f32 roundings on the longest path), read off the kernels
D_LN_ROW = 13                     # LN prologue / ln_1 backward prologue / split finish: 7 lane-local additions + 6 wave_sum levels
D_LN_PANEL = 39                   # whole-panel epilogues: 31 lane-local + pn_half_sum + 7 over the eight waves (>= the split finish's 13)
D_COL_PROLOGUE = 14               # ln_1 prologue column sums: 7 over a wave's 8 rows + 7 over the eight waves
D_COL_PANEL = 6                   # panel column sums: the two row blocks, then 5 levels over 32 lanes (= split finish: 3 + 3)


def gamma(n):
    n = torch.as_tensor(n, dtype=F64)
    return n * U / (1 - n * U)


# ======================================================================================================================
# A. the packer
# ======================================================================================================================
def frag_row(rho):
    """feature of a 32-feature block that MFMA row rho carries (tan_panel.hip: f)"""
    return (rho & 3) + 4 * (rho >> 3) + 16 * ((rho >> 2) & 1)


def pack_index_map(N, K, TN, TK, waves=WAVES):
    """idx with packed.flatten()[d] == w.flatten()[idx[d]] for the row-major [N][K] matrix w"""
    e = torch.arange(8)
    if TN == 384:                 # "qkv16": tile (head pair nb, k step kt of 32) = 24 fragments [16 features][32 k], lane: row l & 15, k = 8 (l >> 4)
        assert N == QKV and K % 32 == 0 and TK == 32
        tk = K // 32
        nb = torch.arange(N // 384).view(-1, 1, 1, 1, 1)
        kt = torch.arange(tk).view(1, -1, 1, 1, 1)
        p = torch.arange(24).view(1, 1, -1, 1, 1)
        lane = torch.arange(64).view(1, 1, 1, -1, 1)
        which, j, fblk = (p >> 2) % 3, p // 12, p & 3
        row = which * 512 + (2 * nb + j) * 64 + fblk * 16 + (lane & 15)
        k = kt * 32 + 8 * (lane >> 4) + e.view(1, 1, 1, 1, -1)
        return (row * K + k).reshape(-1)
    assert N % TN == 0 and K % TK == 0 and TN % (32 * waves) == 0 and TK % 16 == 0
    KS, RB = TK // 16, TN // (32 * waves)
    nb = torch.arange(N // TN).view(-1, 1, 1, 1, 1, 1, 1)
    kt = torch.arange(K // TK).view(1, -1, 1, 1, 1, 1, 1)
    w = torch.arange(waves).view(1, 1, -1, 1, 1, 1, 1)
    rb = torch.arange(RB).view(1, 1, 1, -1, 1, 1, 1)
    ks = torch.arange(KS).view(1, 1, 1, 1, -1, 1, 1)
    lane = torch.arange(64).view(1, 1, 1, 1, 1, -1, 1)
    row = nb * TN + w * (TN // waves) + rb * 32 + frag_row(lane & 31)
    k = kt * TK + ks * 16 + 8 * (lane >> 5) + e.view(1, 1, 1, 1, 1, 1, -1)
    return (row * K + k).reshape(-1)


def tile_format(N, K, qkv16=False):
    """the format flat_params.py packs an [N][K] matrix in"""
    return (384, 32) if qkv16 else ((512, 16) if N == 512 else (256, 32))


PACK_MATRICES = [(2048, 512, False), (512, 2048, False), (512, 512, False), (512, 1536, False), (1536, 512, False), (1536, 512, True)]


# ======================================================================================================================
# B. selector weights and exact inputs
# ======================================================================================================================
def selector_map(N, K, seed):
    """sel[n] = the one column of row n that holds 1.0.  Every run of K / 16 consecutive rows visits every k step of 16 once (in a
    random order, at a random place inside the step), so every 32-feature block of every wave meets K steps all over the contraction."""
    g = torch.Generator().manual_seed(1000 + seed)
    steps = K // 16
    ks = torch.cat([torch.randperm(steps, generator=g) for _ in range(-(-N // steps))])[:N]
    return ks * 16 + torch.randint(0, 16, (N,), generator=g)


def selector_perm(N, seed):
    return torch.randperm(N, generator=torch.Generator().manual_seed(2000 + seed))


def selector_matrix(sel, K):
    W = torch.zeros(sel.numel(), K, dtype=BF16)
    W[torch.arange(sel.numel()), sel] = 1.0
    return W


def selector_weights(seed):
    """the selector maps of one scramble: forward W_fc [2048][512], W_proj [512][2048], W_out [512][512]; backward (the TRANSPOSED
    matrices are what the kernel multiplies by) W_proj^T [2048][512], W_fc^T [512][2048], W_out^T [512][512], W_in^T [512][1536]"""
    return {"fc": selector_map(FF, C, 10 * seed), "proj": selector_map(C, FF, 10 * seed + 1), "out": selector_perm(C, 10 * seed + 2),
            "projT": selector_map(FF, C, 10 * seed + 3), "fcT": selector_map(C, FF, 10 * seed + 4), "outT": selector_perm(C, 10 * seed + 5),
            "inT": selector_map(C, QKV, 10 * seed + 6)}


SCRAMBLES = (0, 1, 2)


def _grid(g, lo, hi, step, n):
    """n values of the grid {lo, lo + step, .., hi}"""
    return lo + step * torch.randint(0, int(round((hi - lo) / step)) + 1, (n,), generator=g).to(F32)


def exact_fwd_inputs(R, seed, head=False, eps=0.0):
    """x_mid rows in {c - 1, c + 1}, half each: mean = c, variance = 1 exactly; ln_2 on a dyadic grid with |g| - |b| >= 1/2 (xn2 has at
    most 5 significant bits and |xn2| >= 1/2); b_fc in [16, 24] (steps of 1/8): the pre-activation is >= 13.75, 1 + exp2(-1.702 log2e x)
    is 1 in f32 and QuickGELU is the identity.  With the head: attn_o = (x_mid - c)[:, pi^-1] in {-1, 1} and x_in = c - b_out, so that
    (attn_o[:, pi] + b_out) + x_in is x_mid again."""
    g = torch.Generator().manual_seed(seed)
    sel = selector_weights(seed % 3)
    c = torch.randint(-24, 25, (R, 1), generator=g).to(F32)
    sgn = torch.where(torch.rand(R, C, generator=g).argsort(1) < C // 2, 1.0, -1.0)
    I = {"kind": "exact", "R": R, "eps": eps, "sel": sel, "c": c[:, 0].clone()}
    I["x_mid"] = (c + sgn).to(BF16)
    I["ln_g"], I["ln_b"] = _grid(g, 1.0, 1.75, 0.25, C), _grid(g, -0.5, 0.5, 0.125, C)
    I["b_fc"], I["b_proj"] = _grid(g, 16.0, 24.0, 0.125, FF), _grid(g, -2.0, 2.0, 0.125, C)
    I["nln_g"], I["nln_b"] = _grid(g, 0.75, 1.25, 0.0625, C), _grid(g, -0.5, 0.5, 0.125, C)
    I["w_fc"], I["w_proj"] = selector_matrix(sel["fc"], C), selector_matrix(sel["proj"], FF)
    if head:
        I["w_out"] = selector_matrix(sel["out"], C)
        I["b_out"] = _grid(g, -1.0, 1.0, 0.25, C)
        inv = torch.empty(C, dtype=torch.long)
        inv[sel["out"]] = torch.arange(C)
        I["attn_o"] = sgn[:, inv].to(BF16)                # attn_o[:, pi[n]] = sgn[:, n]
        I["x_in"] = (c - I["b_out"]).to(BF16)
    return I


def exact_xn2(I):
    """LN2 of the exact rows with rstd = 1: (+-1) g + b, exact in bf16 (and what any rstd within a few ulp of 1 rounds to)"""
    x = I["x_mid"].float()
    return ((x - I["c"].to(x.device)[:, None]) * I["ln_g"] + I["ln_b"]).to(BF16)


def exact_fwd_closed(I, xn2, h_act, x_mid):
    """h_pre = bf16(xn2[:, sigma] + b_fc) = h_act, x_out = bf16((h_act[:, tau] + b_proj) + x_mid): the kernel's order of additions (the
    accumulator starts from b_fc; the epilogue computes acc + bias + res from the left), from the kernel's own stored xn2 / h_act"""
    sig, tau = I["sel"]["fc"].to(xn2.device), I["sel"]["proj"].to(xn2.device)
    h_pre = (xn2.float()[:, sig] + I["b_fc"]).to(BF16)
    x_out = ((h_act.float()[:, tau] + I["b_proj"]) + x_mid.float()).to(BF16)
    return h_pre, x_out


def exact_head_closed(I):
    pi = I["sel"]["out"].to(I["attn_o"].device)
    return ((I["attn_o"].float()[:, pi] + I["b_out"]) + I["x_in"].float()).to(BF16)


def _ln_stats_f32(x, eps):
    x = x.float()
    mean = x.mean(1)
    return mean.contiguous(), ((x - mean[:, None]).square().mean(1) + eps).rsqrt().contiguous()


def bwd_inputs(R, seed, kind, form, dstage=True, res=True, hscale=1.0):
    """kind: "init" (weights at their initialisation scale), "sel" (selector weights, random data: the MFMA sums are single products,
    which leaves the pointwise arithmetic alone under a bound of a few u) or "exact" (selector weights, h_pre = 16 so that quickgelu'
    is 1, integer gradients).  form: "dx" (plain), "ln1" (the ln_1 backward prologue) or "inp" (the in_proj head in front of it)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    sel = selector_weights(seed % 3)
    I = {"kind": kind, "form": form, "R": R, "sel": sel}
    I["x_mid"] = (rn(R, C) * 1.5).to(BF16)
    I["mean2"], I["rstd2"] = _ln_stats_f32(I["x_mid"], 1e-5)
    I["ln_g"] = 1 + 0.1 * rn(C)
    if kind == "init":
        I["wt_proj"] = (rn(C, FF) * 0.03).to(BF16).T.contiguous()          # W_proj^T [2048][512]
        I["wt_fc"] = (rn(FF, C) * 1024 ** -0.5).to(BF16).T.contiguous()     # W_fc^T [512][2048]
        I["wt_out"] = (rn(C, C) * 512 ** -0.5).to(BF16).T.contiguous()
        I["wt_in"] = (rn(QKV, C) * 512 ** -0.5).to(BF16).T.contiguous()     # W_in^T [512][1536]
    else:
        I["wt_proj"], I["wt_fc"] = selector_matrix(sel["projT"], C), selector_matrix(sel["fcT"], FF)
        I["wt_out"], I["wt_in"] = selector_matrix(sel["outT"], C), selector_matrix(sel["inT"], QKV)
    if kind == "exact":
        I["h_pre"] = torch.full((R, FF), 16.0).to(BF16)
        ints = lambda n, a: torch.randint(-a, a + 1, (R, n), generator=g).to(BF16)
        I["g0"] = {"g_b_fc": 3.0, "g_ln_g": -2.0, "g_ln_b": 5.0, "g_b_out": 1.0, "g_ln1_g": 4.0, "g_ln1_b": -3.0, "g_dx_colsum": 2.0}
    else:
        I["h_pre"] = (rn(R, FF) * hscale).to(BF16)
        ints = lambda n, a: (rn(R, n) * 0.02).to(BF16)
        I["g0"] = {"g_b_fc": 0.5, "g_ln_g": 0.25, "g_ln_b": -0.5, "g_b_out": 1.0, "g_ln1_g": -0.25, "g_ln1_b": 0.5, "g_dx_colsum": -1.0}
    if form == "dx":
        I["dx"] = ints(C, 8)
    else:
        I["ln1_x"] = (rn(R, C) * 2).to(BF16)
        I["ln1_mean"], I["ln1_rstd"] = _ln_stats_f32(I["ln1_x"], 1e-5)
        I["ln1_g"] = 1 + 0.1 * rn(C)
        I["res"] = ints(C, 8) if res else None
        if form == "ln1":
            I["ln1_dxn"] = ints(C, 8)
        else:
            I["dqkv"] = ints(QKV, 4)
            I["dstage"] = ints(C, 4) if dstage else None
    return I


def fwd_inputs(R, seed, kind, head=False, eps=1e-5):
    """kind: "init" (test_panel_gpu.py's inputs: x_mid ~ 1.5 N(0, 1), weights at their initialisation scale), "large" (b_fc ~ 10 N(0, 1):
    |h_pre| reaches about 30, both tails of the sigmoid) or "sel" (selector weights, random data)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    sel = selector_weights(seed % 3)
    I = {"kind": kind, "R": R, "eps": eps, "sel": sel}
    if kind == "sel":
        I["w_fc"], I["w_proj"] = selector_matrix(sel["fc"], C), selector_matrix(sel["proj"], FF)
    else:
        I["w_fc"], I["w_proj"] = (rn(FF, C) * 1024 ** -0.5).to(BF16), (rn(C, FF) * 0.03).to(BF16)
    I["b_fc"], I["b_proj"] = rn(FF) * (10.0 if kind == "large" else (1.0 if kind == "sel" else 0.1)), rn(C) * 0.1
    I["ln_g"], I["ln_b"] = 1 + 0.1 * rn(C), 0.1 * rn(C)
    I["nln_g"], I["nln_b"] = 1 + 0.1 * rn(C), 0.1 * rn(C)
    if head:
        I["x_in"], I["attn_o"] = (rn(R, C) * 1.5).to(BF16), rn(R, C).to(BF16)
        I["w_out"] = selector_matrix(sel["out"], C) if kind == "sel" else (rn(C, C) * 512 ** -0.5).to(BF16)
        I["b_out"] = rn(C) * 0.1
    else:
        I["x_mid"] = (rn(R, C) * 1.5).to(BF16)
    return I


def to_device(I, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in I.items()}


# ======================================================================================================================
# C. references and bounds.  A value travels as (v, e): the float64 reference and the bound of the kernel's f32 value against it.
# ======================================================================================================================
def _z(v):
    return torch.zeros((), dtype=F64, device=v.device)


def f_mul(a, ea, b, eb):
    v = a * b
    e = a.abs() * eb + b.abs() * ea + ea * eb
    return v, e + U * (v.abs() + e)


def f_add(a, ea, b, eb):
    v = a + b
    e = ea + eb
    return v, e + U * (v.abs() + e)


def half_ulp_bf16(y):
    _, ex = torch.frexp(y)                                    # y = m 2^ex, 1/2 <= m < 1: binade floor(log2 y) = ex - 1
    return torch.where(y > 0, torch.ldexp(torch.ones_like(y), ex - 9), torch.zeros_like(y))


def store(v, e):
    """the bound of the bf16 value that is stored for an f32 value within e of v"""
    return e + half_ulp_bf16(v.abs() + e)


def gemm(x, ex, W, bias=None):
    """x W^T (+ bias, from which the accumulator starts) for a bf16 matrix W [N][K]: gamma(m - 1) sum |terms| over the m non-zero terms"""
    Wd = W.double()
    v, mag = x @ Wd.T, (x.abs() + ex) @ Wd.abs().T
    m = (W != 0).sum(1).double()
    e = (ex @ Wd.abs().T) if torch.is_tensor(ex) and ex.dim() == 2 else torch.zeros_like(v)
    if bias is not None:
        v, mag, m = v + bias.double(), mag + bias.double().abs(), m + 1
    return v, e + gamma((m - 1).clamp_min(0)) * mag


def reduce_sum(t, et, dim, depth):
    """an f32 reduction of `depth` successive roundings: (sum, sum of the terms' bounds + gamma(depth) sum |terms|)"""
    return t.sum(dim), et.sum(dim) + gamma(depth) * (t.abs() + et).sum(dim)


def ln_fwd(x, ex, g, b, eps, depth):
    """LayerNorm as the kernels compute it: mean, then the centred second moment, rsqrtf, (d rstd) g + b.  Returns (mean, rstd, y)
    pairs; y is the f32 value before its bf16 store."""
    s, es = reduce_sum(x, ex, 1, depth)
    mean, emean = s / C, es / C                                # (1 / 512 is a power of two)
    d, ed = f_add(x, ex, -mean[:, None], emean[:, None])
    sq, esq = f_mul(d, ed, d, ed)
    q, eq = reduce_sum(sq, esq, 1, depth)
    v, ev = f_add(q / C, eq / C, torch.tensor(float(torch.tensor(eps, dtype=F32)), dtype=F64, device=x.device), _z(x))
    rstd = v.rsqrt()
    tiny = torch.finfo(F32).tiny
    er = torch.maximum((v - ev).clamp_min(tiny).rsqrt() - rstd, rstd - (v + ev).rsqrt())
    er = er + HW_U * U * (rstd + er)
    t, et = f_mul(d, ed, rstd[:, None], er[:, None])
    t, et = f_mul(t, et, g.double(), _z(x))
    y, ey = f_add(t, et, b.double(), _z(x))
    return (mean, emean), (rstd, er), (y, ey)


def sigmoid_1702(p, ep):
    """s = rcp(1 + exp2(c p)), c = f32(-1.702f * 1.4426950f), against sigmoid(1.702 p): the argument carries 4 u (1.702f, log2e, their
    product, the multiplication by p) and 1.702 ep; exp2 and rcp 2 u each; 1 + E rounds once.  Returns (s, es, 1 - s)."""
    a = 1.702 * p
    ea = 1.702 * ep + 4 * U * a.abs()                            # in nats: d(exp2(a log2e)) / exp2 = d a
    s, oms = torch.sigmoid(a), torch.sigmoid(-a)                 # E = exp(-a): E / (1 + E) = 1 - s
    rE = torch.expm1(ea) + HW_U * U * torch.exp(ea)
    rt = oms * rE + U * (1 + oms * rE)                           # relative error of t = fl(1 + E)
    rr = rt / (1 - rt) + HW_U * U * (1 + rt / (1 - rt))
    return s, s * rr, oms


def quickgelu(p, ep):
    s, es, _ = sigmoid_1702(p, ep)
    return f_mul(p, ep, s, es)


def quickgelu_grad(x):
    """s + (1.702f x) s (1 - s) from the exact bf16 pre-activation x, in the kernel's order: t = (x * 1.702f) * s; t * (1 - s) + s"""
    zero = _z(x)
    s, es, oms = sigmoid_1702(x, zero)
    kx, ekx = f_mul(x, zero, torch.full_like(x, 1.702), U * 1.702)
    t, et = f_mul(kx, ekx, s, es)
    om, eom = oms, es + U * (oms + es)
    w, ew = f_mul(t, et, om, eom)
    return f_add(w, ew, s, es)


def _src(stored, name, pair, fed):
    """the next stage's input: what the kernel stored (exact) where there is such a tensor and the case is fed, else the reference"""
    if fed and stored is not None and stored.get(name) is not None:
        return stored[name].double(), torch.zeros_like(pair[0])
    return pair[0], store(*pair)


def fwd_reference(I, O=None):
    """name -> (float64 reference, bound) for every output of tan_mlp_fwd / tan_mlp_fwd_split.  O: the kernel's stored outputs (fed:
    xn2 -> h_pre, h_act; h_act -> x_out; x_out -> xn_next, nmean, nrstd; with the head x_mid -> LN2 and the residual) or None (chained)."""
    fed, out = O is not None, {}
    zero = torch.zeros((), dtype=F64, device=I["b_fc"].device)
    if "attn_o" in I:
        y, ey = gemm(I["attn_o"].double(), zero, I["w_out"])
        y, ey = f_add(y, ey, I["b_out"].double(), zero)
        xm = f_add(y, ey, I["x_in"].double(), zero)
        out["x_mid"] = (xm[0], store(*xm))
        x, ex = _src(O, "x_mid", xm, fed)
    else:
        x, ex = I["x_mid"].double(), torch.zeros(I["x_mid"].shape, dtype=F64, device=zero.device)
    mean, rstd, xn = ln_fwd(x, ex, I["ln_g"], I["ln_b"], I["eps"], D_LN_ROW)
    out["mean2"], out["rstd2"], out["xn2"] = mean, rstd, (xn[0], store(*xn))
    xs, exs = _src(O, "xn2", xn, fed)
    p, ep = gemm(xs, exs, I["w_fc"], I["b_fc"])
    out["h_pre"] = (p, store(p, ep))
    act = quickgelu(p, ep)                                      # from the f32 pre-activation: h_act is NOT a function of the stored h_pre
    out["h_act"] = (act[0], store(*act))
    hs, ehs = _src(O, "h_act", act, fed)
    y, ey = gemm(hs, ehs, I["w_proj"])
    y, ey = f_add(y, ey, I["b_proj"].double(), zero)
    xo = f_add(y, ey, x, ex)
    out["x_out"] = (xo[0], store(*xo))
    xos, exos = _src(O, "x_out", xo, fed)
    nmean, nrstd, xnn = ln_fwd(xos, exos, I["nln_g"], I["nln_b"], I["eps"], D_LN_PANEL)
    out["nmean"], out["nrstd"], out["xn_next"] = nmean, nrstd, (xnn[0], store(*xnn))
    return out


def colsum(t, et, g0, depth, atomics):
    """g0 + the column sums over the rows: `depth` roundings inside a workgroup, then one f32 atomic per workgroup in any order"""
    v, e = reduce_sum(t, et, 0, depth + atomics)
    return g0 + v, e + gamma(depth + atomics) * abs(g0)


def ln_bwd(d, ed, x, mean, rstd, gam, res, eres, depth):
    """o = rstd (d g - m1 - xh m2) + res with m1 = mean(d g), m2 = mean(d g xh), xh = (x - mean) rstd: returns (o, eo) before the bf16
    store and the terms of the parameter gradients, (d xh, e), (d, e)"""
    zero = _z(d)
    xm, exm = f_add(x, zero, -mean[:, None], zero)
    xh, exh = f_mul(xm, exm, rstd[:, None], zero)
    dg, edg = f_mul(d, ed, gam, zero)
    s1, es1 = reduce_sum(dg, edg, 1, depth)
    pr, epr = f_mul(dg, edg, xh, exh)
    s2, es2 = reduce_sum(pr, epr, 1, depth)
    m1, em1, m2, em2 = s1 / C, es1 / C, s2 / C, es2 / C
    t, et = f_mul(xh, exh, m2[:, None], em2[:, None])
    a, ea = f_add(dg, edg, -m1[:, None], em1[:, None])
    a, ea = f_add(a, ea, -t, et)
    o, eo = f_mul(a, ea, rstd[:, None], zero)
    if res is not None:
        o, eo = f_add(o, eo, res, eres)
    return (o, eo), f_mul(d, ed, xh, exh), (d, ed + torch.zeros_like(d))


def bwd_reference(I, O=None, split=False, tail=False):
    """name -> (float64 reference, bound) for every output of tan_mlp_bwd / tan_mlp_bwd_split.  O: the kernel's stored outputs (fed:
    dx_out -> dh; dh -> dx2 and its column sums; dx2 -> d_o) or None (chained).  The in_proj head's dxn1 never leaves the LDS: dx_out
    is always chained through it."""
    fed, out, R = O is not None, {}, I["R"]
    dev = I["h_pre"].device
    zero = torch.zeros((), dtype=F64, device=dev)
    g0, nat = I["g0"], (R // 16 if split else R // 64)
    D = lambda k: I[k].double()
    if I["form"] == "dx":
        dx, edx = D("dx"), torch.zeros(R, C, dtype=F64, device=dev)
    else:
        if I["form"] == "inp":
            d, ed = gemm(D("dqkv"), zero, I["wt_in"])
            if I["dstage"] is not None:
                d, ed = f_add(d, ed, D("dstage"), zero)
            d, ed = d, store(d, ed)                                # dxn1 is rounded to bf16 once, into the LDS panel
        else:
            d, ed = D("ln1_dxn"), torch.zeros(R, C, dtype=F64, device=dev)
        res = None if I["res"] is None else D("res")
        o, t_g, t_b = ln_bwd(d, ed, D("ln1_x"), D("ln1_mean"), D("ln1_rstd"), D("ln1_g"), res, zero, D_LN_ROW)
        out["dx_out"] = (o[0], store(*o))
        out["g_ln1_g"] = colsum(*t_g, g0["g_ln1_g"], D_COL_PROLOGUE, R // 64)
        out["g_ln1_b"] = colsum(*t_b, g0["g_ln1_b"], D_COL_PROLOGUE, R // 64)
        out["g_dx_colsum"] = colsum(*o, g0["g_dx_colsum"], D_COL_PROLOGUE, R // 64)      # of the UNROUNDED dx
        dx, edx = _src(O, "dx_out", o, fed)
    av, eav = gemm(dx, edx, I["wt_proj"])
    z, ez = quickgelu_grad(D("h_pre"))
    dd = f_mul(av, eav, z, ez)
    out["dh"] = (dd[0], store(*dd))
    out["g_b_fc"] = colsum(*dd, g0["g_b_fc"], D_COL_PANEL, R // 64)                      # (split: the chunk kernel's own atomics)
    dhs, edhs = _src(O, "dh", dd, fed)
    dy, edy = gemm(dhs, edhs, I["wt_fc"])
    o, t_g, t_b = ln_bwd(dy, edy, D("x_mid"), D("mean2"), D("rstd2"), D("ln_g"), dx, edx, D_LN_PANEL)
    out["dx2"] = (o[0], store(*o))
    out["g_ln_g"] = colsum(*t_g, g0["g_ln_g"], D_COL_PANEL, nat)
    out["g_ln_b"] = colsum(*t_b, g0["g_ln_b"], D_COL_PANEL, nat)
    out["g_b_out"] = colsum(*o, g0["g_b_out"], D_COL_PANEL, nat)                         # of the UNROUNDED dx2
    if tail:
        xs, exs = _src(O, "dx2", o, fed)
        v, e = gemm(xs, exs, I["wt_out"])
        out["d_o"] = (v, store(v, e))
    return out


# ---- plain f32 evaluations with the kernel's rounding points (the CPU test holds the bounds against these, and against slightly
# ---- wrong ones)
def fwd_f32(I, k=1.702, drop_eps=False, ln_from_unrounded=False):
    f = lambda t: t.float()
    if "attn_o" in I:
        x_mid = ((f(I["attn_o"]) @ f(I["w_out"]).T + I["b_out"]) + f(I["x_in"])).to(BF16)
    else:
        x_mid = I["x_mid"]
    x = f(x_mid)

    def ln(x, g, b, eps):
        mean = x.mean(1)
        d = x - mean[:, None]
        rstd = (d.square().mean(1) + eps).rsqrt()
        return mean, rstd, (d * rstd[:, None] * g + b).to(BF16)
    mean2, rstd2, xn2 = ln(x, I["ln_g"], I["ln_b"], I["eps"])
    pre = f(xn2) @ f(I["w_fc"]).T + I["b_fc"]
    act = pre * torch.sigmoid(k * pre)
    v = (f(act.to(BF16)) @ f(I["w_proj"]).T + I["b_proj"]) + x
    x_out = v.to(BF16)
    nmean, nrstd, xn_next = ln(v if ln_from_unrounded else f(x_out), I["nln_g"], I["nln_b"], 0.0 if drop_eps else I["eps"])
    return {"x_mid": x_mid, "mean2": mean2, "rstd2": rstd2, "xn2": xn2, "h_pre": pre.to(BF16), "h_act": act.to(BF16), "x_out": x_out,
            "nmean": nmean, "nrstd": nrstd, "xn_next": xn_next}


def bwd_f32(I, tail=False, k=1.702, m2_div=512.0, drop_row=False, db_times_g=False, colsum_rounded=False):
    f = lambda t: t.float()
    out, g0 = {}, I["g0"]

    def lnb(d, x, mean, rstd, gam, res):
        xh = (x - mean[:, None]) * rstd[:, None]
        dg = d * gam
        m1, m2 = dg.sum(1) / 512.0, (dg * xh).sum(1) / m2_div
        o = rstd[:, None] * (dg - m1[:, None] - xh * m2[:, None])
        return (o if res is None else o + res), d * xh, d

    def cs(t, g):
        return (t[1:] if drop_row else t).sum(0) + g
    if I["form"] == "dx":
        dx = I["dx"]
    else:
        if I["form"] == "inp":
            d = f(I["dqkv"]) @ f(I["wt_in"]).T
            d = f((d if I["dstage"] is None else d + f(I["dstage"])).to(BF16))
        else:
            d = f(I["ln1_dxn"])
        o, tg, tb = lnb(d, f(I["ln1_x"]), I["ln1_mean"], I["ln1_rstd"], I["ln1_g"], None if I["res"] is None else f(I["res"]))
        dx = o.to(BF16)
        out["dx_out"] = dx
        out["g_ln1_g"], out["g_dx_colsum"] = cs(tg, g0["g_ln1_g"]), cs(o, g0["g_dx_colsum"])
        out["g_ln1_b"] = cs(tb * I["ln1_g"] if db_times_g else tb, g0["g_ln1_b"])
    x = f(I["h_pre"])
    s = torch.sigmoid(1.702 * x)
    dd = (f(dx) @ f(I["wt_proj"]).T) * ((x * k) * s * (1 - s) + s)
    out["dh"], out["g_b_fc"] = dd.to(BF16), cs(dd, g0["g_b_fc"])
    dy = f(out["dh"]) @ f(I["wt_fc"]).T
    o, tg, tb = lnb(dy, f(I["x_mid"]), I["mean2"], I["rstd2"], I["ln_g"], f(dx))
    out["dx2"] = o.to(BF16)
    out["g_ln_g"], out["g_ln_b"] = cs(tg, g0["g_ln_g"]), cs(tb, g0["g_ln_b"])
    out["g_b_out"] = cs(f(out["dx2"]) if colsum_rounded else o, g0["g_b_out"])
    if tail:
        out["d_o"] = (f(out["dx2"]) @ f(I["wt_out"]).T).to(BF16)
    return out


def worst_ratio(got, ref, bound):
    """max over ALL elements of |got - ref| / bound; where the bound is 0 the value must be exact (else inf).  NaN gives inf."""
    err = (got.double() - ref).abs()
    bound = bound.expand_as(err)
    pos = bound > 0
    if not bool((err[~pos] == 0).all()) or not bool(torch.isfinite(err).all()):
        return math.inf
    return (err[pos] / bound[pos]).max().item() if bool(pos.any()) else 0.0
