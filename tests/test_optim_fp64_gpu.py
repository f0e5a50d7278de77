"""The optimizer family of csrc/tan_optim.hip -- tan_adamw_step, tan_ema_update, tan_adamw_step_images -- called directly through
ctypes on tensors built here (no Trainer, no model), against references that share no code with the kernels:

  ref64   torch.optim.AdamW's single-tensor formulas in float64 from the f32 inputs upcast, scalar prefactors in Python floats.
          Bounds from the rounding model of the documented operation order (u = 2^-24, constants doubled):
            v    |v - v64| <= 8u v64
            m    |m - m64| <= 8u (|g grad_scale| + |m_old|)
            p    |p - p64| <= 4u |p64| + 16u |upd64| + step_size bound_m / denom64
            ema  |e - e64| <= 6u (|e_old m| + |p_new (1 - m)|), p_new the kernel's own f32 result
          Elements whose g*g (or a product of it) is a positive f32 denormal are exempt from the relative v bound, elements whose g*g
          overflows f32 (v = inf in f32, finite in f64) from the v and p bounds: ref32 and explicit statements cover them.
  ref32   the f32 restatement of adamw_elem / ema_elem on the CPU, one torch operation per rounded operation, prefactors rounded to
          f32 as the host code rounds them: p, m, v, ema must be BIT-equal, the bf16 shadows equal tensor.bfloat16() of them.
  images  an index-level oracle of the four weight images written from include/tan_hip.h and the comments of tan_panel.hip /
          tan_attnblk.hip (`pack_index`), over all elements; tan_pack_weights and tan_transpose_batch are checked against it first.

Every pure output starts as a sentinel (a NaN bit pattern), every buffer carries a guard region behind n that must come back
bit-unchanged.  tests/test_optim_cpu.py checks the bounds themselves without a GPU (ref32 and torch.optim.AdamW inside them).

Measured on an MI355X (worst ratio to each bound over every case of a section; `test_report_worst_ratios` prints them):
  section (tests)                          m      v      p      ema
  sizes   (test_adamw_step_sizes)          0.12   0.41   0.53   0.33
  hyper   (test_adamw_step_hyperparam.)    0.11   0.35   0.50   0.32
  modes   (test_adamw_step_modes)          0.11   0.32   0.47   0.32
  images  (test_adamw_images_*)            0.12   0.40   0.55   0.33
  tan_ema_update                           -      -      -      0.33
  trajectory, 25 calls, (p, m, v):  kernel (1.0361e-06, 5.597e-08, 2.2892e-07)   torch.optim.AdamW (1.0351e-06, 5.708e-08, 2.2869e-07)
ref32 held bit for bit in every case: sqrtf and both divisions are correctly rounded on gfx950, f32 denormals are kept, and nothing
is contracted into an FMA.  (The first version of ref32 used torch's CPU sqrt and differed in 0.8 % of the parameters: the CPU side
was the one off by an ulp, see ref32.)
"""
import ctypes as C
import math

import pytest
import torch

from temporalalignnet_amd import _lib

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U = 2.0 ** -24
FMIN, FMAX = 2.0 ** -126, 3.4028234663852886e38
GUARD = 512
S32 = 0x7FC5A5A5            # f32 sentinel: a quiet NaN with a payload
S16 = 0x7FA5                # bf16 sentinel: a NaN with a payload
N_LIST = (1, 255, 256, 257, 8192 * 256 + 257, 5_000_003)
WORST = {}                  # "section/tensor" -> worst measured ratio to its bound


class HP:
    def __init__(self, lr=1e-3, wd=1e-2, betas=(0.9, 0.999), eps=1e-8, step=1, grad_scale=1.0):
        self.lr, self.wd, self.beta1, self.beta2, self.eps, self.step, self.grad_scale = lr, wd, betas[0], betas[1], eps, step, grad_scale

    @property
    def gs32(self):                                   # the f32 value the entry point receives, as a Python float
        return torch.tensor(self.grad_scale, dtype=F32).item()


def prefactors(hp):
    """torch.optim's scalar prefactors in Python floats (double)"""
    bc1, bc2 = 1.0 - hp.beta1 ** hp.step, 1.0 - hp.beta2 ** hp.step
    return dict(decay=1.0 - hp.lr * hp.wd, w1=1.0 - hp.beta1, beta2=hp.beta2, w2=1.0 - hp.beta2, eps=hp.eps,
                step_size=hp.lr / bc1, bc2_sqrt=math.sqrt(bc2))


def _mode_or_ones(mode, like):
    return torch.ones(like.numel(), dtype=torch.uint8, device=like.device) if mode is None else mode.to(like.device)


def ref64(p, g, m, v, mode, hp):
    """fp64 AdamW (torch.optim.AdamW single-tensor formulas) + the bounds of the header; any device."""
    c = prefactors(hp)
    mode = _mode_or_ones(mode, p)
    P, G, M, V = (x.double() for x in (p, g, m, v))
    act = mode < 2
    G = G * hp.gs32
    Pd = torch.where(mode == 1, P * c["decay"], P)
    M1 = M + (G - M) * c["w1"]
    GG = G * G
    V1 = V * c["beta2"] + c["w2"] * GG
    denom = V1.sqrt() / c["bc2_sqrt"] + c["eps"]
    upd = c["step_size"] * M1 / denom
    P1 = Pd - upd
    bm = 8 * U * (G.abs() + M.abs())
    bv = 8 * U * V1
    bp = 4 * U * P1.abs() + 16 * U * upd.abs() + c["step_size"] * bm / denom
    zero = torch.zeros_like(P)

    def sub(x):
        return (x > 0) & (x < FMIN)
    denorm = (sub(GG) | sub(GG * c["w2"]) | sub(V * c["beta2"])) & act
    over = (GG > FMAX) & act
    return dict(p=torch.where(act, P1, P), m=torch.where(act, M1, M), v=torch.where(act, V1, V),
                bp=torch.where(act, bp, zero), bm=torch.where(act, bm, zero), bv=torch.where(act, bv, zero),
                skip_v=denorm | over, skip_p=over)


def ema_ref64(e, p_new, ema_m):
    mm = torch.tensor(ema_m, dtype=F32).item()
    a, b = e.double() * mm, p_new.double() * (1.0 - mm)
    return a + b, 6 * U * (a.abs() + b.abs())


def ref32(p, g, m, v, mode, hp):
    """adamw_elem's sequence on the CPU in f32, one torch operation per rounded operation."""
    assert p.device.type == "cpu" and p.dtype == F32
    c = {k: torch.tensor(x, dtype=F32) for k, x in prefactors(hp).items()}
    mode = _mode_or_ones(mode, p)
    gi = g * torch.tensor(hp.grad_scale, dtype=F32)
    pd = torch.where(mode == 1, p * c["decay"], p)
    d1 = (gi - m) * c["w1"]
    m1 = m + d1
    a = v * c["beta2"]
    b = (gi * gi) * c["w2"]
    v1 = a + b
    # sqrtf is correctly rounded on the device; torch's CPU sqrt of a contiguous f32 tensor is a vector-library call that is not
    # (0.7 % of random inputs are one ulp off).  The square root in double, rounded once to f32, is: 53 >= 2 * 24 + 2 bits.
    denom = v1.double().sqrt().float() / c["bc2_sqrt"] + c["eps"]
    upd = c["step_size"] * (m1 / denom)
    p1 = pd - upd
    act = mode < 2
    return dict(p=torch.where(act, p1, p), m=torch.where(act, m1, m), v=torch.where(act, v1, v))


def ema_ref32(e, p_new, ema_m):
    mm = torch.tensor(ema_m, dtype=F32)
    a = e * mm
    b = p_new * (torch.tensor(1.0, dtype=F32) - mm)
    return a + b


def ratio(got, want, bound, skip=None):
    """worst |got - want| / bound over the elements not in `skip`; a zero bound demands equality.  NaN or inf in `got` fails."""
    got = got.double()
    keep = torch.ones_like(got, dtype=torch.bool) if skip is None else ~skip
    if not keep.any():
        return 0.0
    d = (got - want).abs()[keep]
    b = bound[keep]
    assert torch.isfinite(got[keep]).all()
    exact = b == 0
    assert (d[exact] == 0).all()
    if exact.all():
        return 0.0
    return (d[~exact] / b[~exact]).max().item()


def record(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


def check64(section, got, p, g, m, v, mode, hp, sel=None):
    """`got` (dict p, m, v; same device as the inputs) inside ref64's bounds, on the elements of `sel` (default: all)."""
    r = ref64(p, g, m, v, mode, hp)
    none = torch.zeros(p.numel(), dtype=torch.bool, device=p.device)
    out = sel.logical_not() if sel is not None else none
    rs = {}
    for k, b, skip in (("m", "bm", none), ("v", "bv", r["skip_v"]), ("p", "bp", r["skip_p"])):
        rs[k] = record(f"{section}/{k}", ratio(got[k], r[k], r[b], skip | out))
        assert rs[k] <= 1.0, (section, k, rs[k])
    return rs


def check_ema64(section, e_got, e_old, p_new, ema_m, sel=None):
    want, bound = ema_ref64(e_old, p_new, ema_m)
    r = record(f"{section}/ema", ratio(e_got, want, bound, None if sel is None else ~sel))
    assert r <= 1.0, (section, "ema", r)
    return r


def bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16) if t.dtype in (F32, BF16) else t


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def make_inputs(n, seed):
    """p, g, m, v, ema on the CPU: normal gradients at scales 1e-6 / 1 / 1e3 in runs of 16, and in every 16 elements
    k = 0: g = 0 on zero state; 1: g = 0 on non-zero state; 2: g = 1e-20 on zero state (square denormal); 3: g = 1e19 (square finite);
    4: g = 3e19 (square overflows); 5: g = -3e19 on zero state.  n = 1 is a normal element."""
    gen = torch.Generator().manual_seed(seed)
    i = torch.arange(n)
    scale = torch.tensor([1e-6, 1.0, 1e3])[(i // 16) % 3]
    p = torch.randn(n, generator=gen) * 0.05
    g = torch.randn(n, generator=gen) * scale
    m = torch.randn(n, generator=gen) * scale * 0.1
    v = (torch.randn(n, generator=gen) * scale) ** 2 * 0.01 + scale * scale * 1e-4
    e = p + torch.randn(n, generator=gen) * 0.01
    k = (i + 9) % 16
    zs = (k == 0) | (k == 2) | (k == 5)
    m[zs] = 0.0
    v[zs] = 0.0
    g[(k == 0) | (k == 1)] = 0.0
    g[k == 2] = 1e-20
    g[k == 3] = 1e19
    g[k == 4] = 3e19
    g[k == 5] = -3e19
    return dict(p=p, g=g, m=m, v=v, e=e, k=k)


def check_statements(inp, out, mode, hp):
    """What must hold whatever the references say: p stays finite; g = 0 on zero state is exactly the decay (0 / eps); a gradient
    whose square overflows gives v = inf, denom = inf, update 0."""
    mode = _mode_or_ones(mode, inp["p"])
    assert torch.isfinite(out["p"]).all()
    pd = torch.where(mode == 1, inp["p"] * torch.tensor(prefactors(hp)["decay"], dtype=F32), inp["p"])
    act = mode < 2
    z = (inp["k"] == 0) & act
    assert bits_equal(out["p"][z], pd[z]) and (out["m"][z] == 0).all() and (out["v"][z] == 0).all()
    gi = (inp["g"] * torch.tensor(hp.grad_scale, dtype=F32)).double()
    ov = (gi * gi > 3.5e38) & act
    assert torch.isinf(out["v"][ov]).all() and (out["p"][ov] == pd[ov]).all()


# ------------------------------------------------------------------------------------------------------------------------------
# device buffers with sentinels and guards

def _stream():
    from temporalalignnet_amd import ops
    return ops._stream()


def guarded(x):
    """CPU tensor of n elements -> device buffer of n + GUARD, the guard filled with the sentinel of its type"""
    n = x.numel()
    buf = torch.empty(n + GUARD, dtype=x.dtype)
    if x.dtype == F32:
        buf.view(torch.int32)[n:] = S32
    elif x.dtype == BF16:
        buf.view(torch.int16)[n:] = S16
    else:
        buf[n:] = 0xA5 if x.dtype == torch.uint8 else -7
    buf[:n] = x
    return buf.cuda()


def sentinel16(n):
    return torch.full((n + GUARD,), S16, dtype=torch.int16).view(BF16).cuda()


def guard_ok(buf, n):
    want = S32 if buf.dtype == F32 else S16 if buf.dtype == BF16 else (0xA5 if buf.dtype == torch.uint8 else -7)
    return bool((bits(buf)[n:] == want).all())


def is_sentinel(t):
    return bits(t) == (S32 if t.dtype == F32 else S16)


def run_adamw(inp, mode, hp, ema_m=None, want_p16=True, want_e16=True):
    """tan_adamw_step on CPU inputs -> CPU outputs (n elements each); guards and read-only inputs checked here."""
    n = inp["p"].numel()
    P, G, M, V = (guarded(inp[k]) for k in "pgmv")
    md = guarded(mode) if mode is not None else None
    p16 = sentinel16(n) if want_p16 else None
    E = guarded(inp["e"]) if ema_m is not None else None
    e16 = sentinel16(n) if (ema_m is not None and want_e16) else None

    def ptr(t):
        return None if t is None else t.data_ptr()
    _lib.check(_lib.lib().tan_adamw_step(ptr(P), ptr(G), ptr(M), ptr(V), ptr(md), n, hp.lr, hp.beta1, hp.beta2, hp.eps, hp.wd, hp.step,
                                         hp.grad_scale, ptr(p16), ptr(E), 0.0 if ema_m is None else ema_m, ptr(e16), _stream()),
               "tan_adamw_step")
    torch.cuda.synchronize()
    for t in (P, G, M, V, md, p16, E, e16):
        assert t is None or guard_ok(t, n)
    assert bits_equal(G[:n].cpu(), inp["g"]) and (md is None or torch.equal(md[:n].cpu(), mode))
    out = dict(p=P[:n].cpu(), m=M[:n].cpu(), v=V[:n].cpu())
    for k, t in (("p16", p16), ("e", E), ("e16", e16)):
        if t is not None:
            out[k] = t[:n].cpu()
    return out


def check_adamw(section, inp, mode, hp, ema_m=0.999):
    """one tan_adamw_step call against ref32 (bits), ref64 (bounds), the bf16 rounding and the explicit statements"""
    out = run_adamw(inp, mode, hp, ema_m)
    r = ref32(inp["p"], inp["g"], inp["m"], inp["v"], mode, hp)
    for k in "pmv":
        assert bits_equal(out[k], r[k]), (section, k, int((bits(out[k]) != bits(r[k])).sum()))
    e_ref = ema_ref32(inp["e"], r["p"], ema_m)
    assert bits_equal(out["e"], e_ref), (section, "ema")
    md = _mode_or_ones(mode, inp["p"])
    act = md < 2
    assert bits_equal(out["p16"][act], out["p"][act].bfloat16()) and is_sentinel(out["p16"][~act]).all()
    assert bits_equal(out["e16"], out["e"].bfloat16())
    check64(section, out, inp["p"], inp["g"], inp["m"], inp["v"], mode, hp)
    check_ema64(section, out["e"], inp["e"], out["p"], ema_m)
    check_statements(inp, out, mode, hp)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# 1 + 2. tan_adamw_step and tan_ema_update

@pytest.mark.parametrize("n", N_LIST)
def test_adamw_step_sizes(n):
    inp = make_inputs(n, seed=n % 1000)
    mode = (torch.arange(n) % 2).to(torch.uint8)
    check_adamw("sizes", inp, mode, HP(step=3, grad_scale=0.5))


@pytest.mark.parametrize("lr,wd", [(1e-3, 1e-2), (1e-4, 0.0), (0.0, 0.1)])
@pytest.mark.parametrize("step", [1, 2, 1000, 200000])
def test_adamw_step_hyperparameters(step, lr, wd):
    n = 2048 + 257
    inp = make_inputs(n, seed=step % 97 + 1)
    mode = ((torch.arange(n) // 3) % 2).to(torch.uint8)
    for eps in (1e-8, 1e-6):
        for gs in (1.0, 0.5, 0.125, 1.0 / 3.0):
            for betas in ((0.9, 0.999), (0.9, 0.98)):
                check_adamw("hyper", inp, mode, HP(lr=lr, wd=wd, betas=betas, eps=eps, step=step, grad_scale=gs))
    if step == 200000:                                          # both bias corrections have reached 1 in double
        c = prefactors(HP(lr=lr, wd=wd, step=step))
        assert c["bc2_sqrt"] == 1.0 and c["step_size"] == lr


def test_adamw_step_modes():
    n = 4096 + 257
    inp = make_inputs(n, seed=5)
    i = torch.arange(n)
    hp = HP(step=7, grad_scale=0.5)
    # NULL = all decay, bit for bit
    a = run_adamw(inp, None, hp, 0.999)
    b = run_adamw(inp, torch.ones(n, dtype=torch.uint8), hp, 0.999)
    for k in a:
        assert bits_equal(a[k], b[k]), k
    for mode in ((i % 4).to(torch.uint8), ((i // 64) % 4).to(torch.uint8), torch.full((n,), 2, dtype=torch.uint8),
                 torch.full((n,), 3, dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8)):
        out = check_adamw("modes", inp, mode, hp)
        fr = mode >= 2                     # skipped / frozen: p, m, v, shadow untouched, the EMA twin still moves from the old p
        for k in "pmv":
            assert bits_equal(out[k][fr], inp[k][fr]), k
        assert is_sentinel(out["p16"][fr]).all()
        assert bits_equal(out["e"][fr], ema_ref32(inp["e"], inp["p"], 0.999)[fr])
        assert bits_equal(out["e16"][fr], out["e"][fr].bfloat16())
        if fr.any():
            assert (out["e"][fr] != inp["e"][fr]).any()
    # mode 0 differs from mode 1 by exactly the decay factor: the moments do not see it, and with a gradient and state of zero
    # (update 0 / eps = 0) mode 0 leaves p alone where mode 1 gives p * decay
    zero = torch.zeros(n)
    flat = dict(inp, g=zero, m=zero.clone(), v=zero.clone())
    o0 = run_adamw(flat, torch.zeros(n, dtype=torch.uint8), hp)
    o1 = run_adamw(flat, torch.ones(n, dtype=torch.uint8), hp)
    assert bits_equal(o0["p"], inp["p"]) and bits_equal(o1["p"], inp["p"] * torch.tensor(1.0 - 1e-3 * 1e-2, dtype=F32))
    o0 = run_adamw(inp, torch.zeros(n, dtype=torch.uint8), hp)
    o1 = run_adamw(inp, torch.ones(n, dtype=torch.uint8), hp)
    assert bits_equal(o0["m"], o1["m"]) and bits_equal(o0["v"], o1["v"])
    upd = inp["p"] - o0["p"]                                   # (what mode 0 subtracted, to within one rounding of p)
    decayed = inp["p"] * torch.tensor(1.0 - 1e-3 * 1e-2, dtype=F32)
    assert ((o1["p"].double() - (decayed.double() - upd.double())).abs() <= 4 * U * (inp["p"].abs() + upd.abs()).double()).all()


def test_adamw_step_optional_outputs():
    n = 1000
    inp = make_inputs(n, seed=11)
    mode = (torch.arange(n) % 2).to(torch.uint8)
    hp = HP(step=4)
    full = run_adamw(inp, mode, hp, 0.999)
    a = run_adamw(inp, mode, hp, 0.999, want_p16=False)
    b = run_adamw(inp, mode, hp, None)
    c = run_adamw(inp, mode, hp, 0.999, want_e16=False)
    assert set(a) == {"p", "m", "v", "e", "e16"} and set(b) == {"p", "m", "v", "p16"} and set(c) == {"p", "m", "v", "p16", "e"}
    for o in (a, b, c):
        for k in o:
            assert bits_equal(o[k], full[k]), k


def test_bf16_shadow_rounding_edges():
    """lr = 0, wd = 0: the parameter passes through unchanged, so the shadow is the rounding of exactly what is placed in p."""
    pat = [0x00000000, 0x80000000,                              # both zeros
           0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # exact ties, even and odd upper halves, both signs
           0x3F807FFF, 0x3F808001, 0x3F80FFFF,                  # just below / above a tie
           0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x80008000, 0x807FFFFF,   # f32 denormals
           0x00800000, 0x7F7F0000, 0x7F7F7FFF, 0x7F7E8000, 0xFF7F7FFF, 0x7F7F8000]                           # smallest normal, top
    base = torch.tensor([x - (1 << 32) if x >= (1 << 31) else x for x in pat], dtype=torch.int32).view(F32)
    p = base.repeat(23)[:513].contiguous()
    n = p.numel()
    z = torch.zeros(n)
    inp = dict(p=p, g=z.clone(), m=z.clone(), v=z.clone(), e=p.clone())
    out = run_adamw(inp, None, HP(lr=0.0, wd=0.0, step=1), 1.0)
    assert bits_equal(out["p"], p)
    assert bits_equal(out["p16"], p.bfloat16())
    assert (out["e"] == p).all() and bits_equal(out["e16"], out["e"].bfloat16())
    # the rounding itself, stated on bits: round to nearest even of the upper 16
    b = p.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    want = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    got = out["p16"].view(torch.int16).to(torch.int64) & 0xFFFF
    assert torch.equal(got, want)


def run_ema(tgt, src, m, with16):
    n = tgt.numel()
    T, S = guarded(tgt), guarded(src)
    t16 = sentinel16(n) if with16 else None
    _lib.check(_lib.lib().tan_ema_update(T.data_ptr(), S.data_ptr(), n, m, None if t16 is None else t16.data_ptr(), _stream()),
               "tan_ema_update")
    torch.cuda.synchronize()
    assert guard_ok(T, n) and guard_ok(S, n) and (t16 is None or guard_ok(t16, n))
    assert bits_equal(S[:n].cpu(), src)
    return T[:n].cpu(), (None if t16 is None else t16[:n].cpu())


@pytest.mark.parametrize("with16", [True, False])
@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("m", [0.0, 0.999, 1.0])
def test_ema_update(m, n, with16):
    inp = make_inputs(n, seed=3 + n % 100)
    tgt, src = inp["e"], inp["p"]
    if n > 16:
        tgt[3], src[3], tgt[4], src[4], tgt[5] = -0.0, 0.0, 0.0, -0.0, 1e-40
    got, got16 = run_ema(tgt, src, m, with16)
    assert bits_equal(got, ema_ref32(tgt, src, m))
    if with16:
        assert bits_equal(got16, got.bfloat16())
    check_ema64("ema_update", got, tgt, src, m)
    if m == 1.0:
        assert (got == tgt).all()
    if m == 0.0:
        assert (got == src).all()


def trajectory_inputs(n=1 << 16, steps=25, seed=2024):
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen) * 0.05
    signal = torch.randn(n, generator=gen) * 0.1
    gs = []
    for t in range(steps):
        g = signal + torch.randn(n, generator=gen) * 0.05
        if t % 3 == 2:
            g[torch.arange(n) % 7 == 0] = 0.0
        gs.append(g)
    return p0, gs


TRAJ_HP = dict(lr=1e-3, wd=1e-2, betas=(0.9, 0.999), eps=1e-8)


def trajectory_errors(p0, gs, stepper):
    """`stepper(p, g, m, v, step) -> p, m, v` (f32) carried over len(gs) steps against ref64 carrying its own f64 state:
    ||x - x64|| / ||x64 - x_0|| for p, m, v"""
    z = torch.zeros_like(p0)
    p, m, v = p0.clone(), z.clone(), z.clone()
    P, M, V = p0.double(), z.double(), z.double()
    for t, g in enumerate(gs):
        p, m, v = stepper(p, g, m, v, t + 1)
        c = prefactors(HP(step=t + 1, **TRAJ_HP))
        G = g.double()
        P = P * c["decay"]
        M = M + (G - M) * c["w1"]
        V = V * c["beta2"] + c["w2"] * G * G
        P = P - c["step_size"] * M / (V.sqrt() / c["bc2_sqrt"] + c["eps"])
    return tuple(((a.double() - b).norm() / (b - o.double()).norm()).item() for a, b, o in ((p, P, p0), (m, M, z), (v, V, z)))


def torch_adamw_trajectory(p0, gs):
    w = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([w], lr=TRAJ_HP["lr"], betas=TRAJ_HP["betas"], eps=TRAJ_HP["eps"], weight_decay=TRAJ_HP["wd"], foreach=False)

    def stepper(p, g, m, v, step):
        w.grad = g.clone()
        opt.step()
        s = opt.state[w]
        return w.detach().clone(), s["exp_avg"].clone(), s["exp_avg_sq"].clone()
    return trajectory_errors(p0, gs, stepper)


def test_trajectory_of_25_direct_calls():
    """25 calls, state carried by the kernel.  The admissible error is measured, not derived: twice what torch.optim.AdamW
    (foreach=False, f32, CPU) shows on the same sequence with the same metric, computed in this run."""
    p0, gs = trajectory_inputs()
    n = p0.numel()
    z = torch.zeros(n)
    P, M, V = guarded(p0), guarded(z), guarded(z)
    snaps = []

    def stepper(p, g, m, v, step):
        G = guarded(g)
        hp = HP(step=step, **TRAJ_HP)
        _lib.check(_lib.lib().tan_adamw_step(P.data_ptr(), G.data_ptr(), M.data_ptr(), V.data_ptr(), None, n, hp.lr, hp.beta1, hp.beta2,
                                             hp.eps, hp.wd, step, 1.0, None, None, 0.0, None, _stream()), "tan_adamw_step")
        torch.cuda.synchronize()
        assert guard_ok(P, n) and guard_ok(M, n) and guard_ok(V, n) and guard_ok(G, n)
        out = P[:n].cpu(), M[:n].cpu(), V[:n].cpu()
        r = ref32(p, g, m, v, None, hp)                    # (and every step is ref32's step, bit for bit)
        snaps.append(all(bits_equal(o, r[k]) for o, k in zip(out, "pmv")))
        return out
    kern = trajectory_errors(p0, gs, stepper)
    ref = torch_adamw_trajectory(p0, gs)
    print(f"trajectory (p, m, v): kernel {kern}  torch.optim.AdamW {ref}")
    WORST["trajectory/kernel"], WORST["trajectory/torch"] = kern, ref
    assert all(snaps)
    for k, r in zip(kern, ref):
        assert k <= 2.0 * r, (kern, ref)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the weight images

PANEL_WAVES = 8


def pack_index(N, K, TN, TK):
    """Index-level statement of a tan_pack_weights image of a row-major [N][K] matrix in tiles [TN][TK] (include/tan_hip.h):
    int64 [N*K], packed position -> source position n*K + k.
    General format: tiles in (n-block, k-block) order; inside a tile wave w of 8 owns rows w*TN/8.., as fragments [row block of 32]
    [k step of 16] of 1 KiB; lane l's 8 elements are W[row0 + f(l & 31)][k0 + 8 (l >> 5) ..] with the row permutation
    f(rho) = (rho & 3) + 4 (rho >> 3) + 16 ((rho >> 2) & 1).
    "qkv16" (TN = 384, N = 1536): tile (head pair hp, k step of 32) holds 24 fragments of 16 rows x 32 k; fragment p has in_proj rows
    which*512 + (2 hp + j)*64 + fblk*16 .. +15 with which = (p / 4) % 3, j = p / 12, fblk = p % 4; lane l: row l & 15, k = 8 (l >> 4) .."""
    ar = torch.arange
    lane, j = ar(64)[:, None], ar(8)[None, :]
    if TN == 384:
        assert N == 1536 and TK == 32 and K % 32 == 0
        hp, kt, p = ar(N // 384)[:, None, None, None, None], ar(K // 32)[None, :, None, None, None], ar(24)[None, None, :, None, None]
        which, jj, fblk = (p // 4) % 3, p // 12, p % 4
        row = which * 512 + (2 * hp + jj) * 64 + fblk * 16 + (lane & 15)
        k = kt * 32 + 8 * (lane >> 4) + j
        return (row * K + k).reshape(-1)
    assert TN * TK * 2 == 16384 and N % TN == 0 and K % TK == 0
    W, RB, KS = PANEL_WAVES, TN // (32 * PANEL_WAVES), TK // 16
    sh = (N // TN, K // TK, W, RB, KS)
    nb, kb, w, rb, ks = (ar(s).view([-1 if a == i else 1 for a in range(5)] + [1, 1]) for i, s in enumerate(sh))
    rho = lane & 31
    f = (rho & 3) + 4 * (rho >> 3) + 16 * ((rho >> 2) & 1)
    row = nb * TN + w * (TN // W) + rb * 32 + f
    k = kb * TK + ks * 16 + 8 * (lane >> 5) + j
    return (row * K + k).reshape(-1)


def transpose_index(N, K):
    """position in the row-major W^T [K][N] -> source position in W [N][K]"""
    return torch.arange(N * K).view(N, K).t().reshape(-1)


# (N, K, tn_w, tk_w, tn_t, tk_t): the default model's matrices as flat_params.image_table lists them, and entries without packed images
DEFAULT_ENTRIES = [(1536, 512, 384, 32, 512, 16), (512, 512, 512, 16, 512, 16), (2048, 512, 256, 32, 512, 16),
                   (512, 2048, 512, 16, 256, 32), (512, 1024, 512, 16, 0, 0), (512, 768, 512, 16, 0, 0)]
PLAIN_ENTRIES = [(64, 64, 0, 0, 0, 0), (64, 192, 0, 0, 0, 0), (192, 64, 0, 0, 0, 0)]
IMAGES = ("p16", "pt", "pp", "ptp", "e16", "ep")
_index_cache = {}


def entry_maps(ent):
    """image -> int64 [N*K]: position inside the entry's image -> source position inside the matrix (None: no such image)"""
    if ent not in _index_cache:
        N, K, tn_w, tk_w, tn_t, tk_t = ent
        ident, t = torch.arange(N * K), transpose_index(N, K)
        packed = pack_index(N, K, tn_w, tk_w) if tn_w else None
        tpacked = t[pack_index(K, N, tn_t, tk_t)] if tn_t else None
        for x in (packed, tpacked):
            assert x is None or torch.equal(torch.sort(x)[0], ident)
        _index_cache[ent] = dict(p16=ident, pt=t, pp=packed, ptp=tpacked, e16=ident, ep=packed)
    return _index_cache[ent]


class Table:
    """A flat layout the test builds: every matrix at a multiple of 8 elements, behind it a bias-like gap of N + 3 elements that only
    rest_idx owns, then up to 7 elements owned by nobody."""

    def __init__(self, entries, modes=None):
        self.entries, self.offs, self.prefix = list(entries), [], [0]
        off, rest, nobody = 8, [], [torch.arange(8)]
        for (N, K, *_) in self.entries:
            assert off % 8 == 0 and N % 64 == 0 and K % 64 == 0
            self.offs.append(off)
            self.prefix.append(self.prefix[-1] + (N // 64) * (K // 64))
            off += N * K
            rest.append(torch.arange(off, off + N + 3))
            off += N + 3
            pad = -off % 8
            nobody.append(torch.arange(off, off + pad))
            off += pad
        self.n, self.n_units = off, self.prefix[-1]
        self.rest, self.nobody = torch.cat(rest), torch.cat(nobody)
        self.unit_of = torch.full((self.n,), -1, dtype=torch.int64)
        self.src = {k: torch.full((self.n,), -1, dtype=torch.int64) for k in IMAGES}
        self.mode = (torch.arange(self.n) % 2).to(torch.uint8)
        for e, (ent, o) in enumerate(zip(self.entries, self.offs)):
            N, K = ent[:2]
            r, c = torch.arange(N)[:, None], torch.arange(K)[None, :]
            self.unit_of[o:o + N * K] = (self.prefix[e] + (r // 64) * (K // 64) + c // 64).reshape(-1)
            self.mode[o:o + N * K] = (e % 2) if modes is None else modes[e]
            for k, idx in entry_maps(ent).items():
                if idx is not None:
                    self.src[k][o:o + N * K] = idx + o
        self.owned = self.unit_of >= 0
        arr = (_lib.ImageEntry * len(self.entries))(*[_lib.ImageEntry(o, *ent) for o, ent in zip(self.offs, self.entries)])
        self.table_bytes = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.prefix_t = torch.tensor(self.prefix, dtype=torch.int64)

    def inputs(self, seed):
        return make_inputs(self.n, seed)

    def device_state(self, inp):
        st = {k: guarded(inp[k]) for k in "pgmve"}
        st["mode"] = guarded(self.mode)
        for k in IMAGES:
            st[k] = sentinel16(self.n)
        st["table"], st["prefix"] = self.table_bytes.cuda(), self.prefix_t.cuda()
        return st


STATE_KEYS = ("p", "g", "m", "v", "e", "mode") + IMAGES


def snapshot(st):
    return {k: st[k].cpu() for k in STATE_KEYS}


def call_images(tab, st, hp, ema_m, units=(0, 0), rest=None, null=()):
    d = _lib.AdamwImagesDesc()

    def ptr(k):
        return None if k in null else st[k].data_ptr()
    d.p, d.g, d.m, d.v, d.mode, d.n = ptr("p"), ptr("g"), ptr("m"), ptr("v"), ptr("mode"), tab.n
    d.lr, d.beta1, d.beta2, d.eps, d.weight_decay, d.step, d.grad_scale = hp.lr, hp.beta1, hp.beta2, hp.eps, hp.wd, hp.step, hp.grad_scale
    d.p_bf16, d.ema, d.ema_m, d.ema_bf16 = ptr("p16"), ptr("e"), ema_m, ptr("e16")
    d.table, d.unit_prefix, d.n_entries, d.n_units = st["table"].data_ptr(), st["prefix"].data_ptr(), len(tab.entries), tab.n_units
    d.p_packed, d.p_t, d.p_tpacked, d.ema_packed = ptr("pp"), ptr("pt"), ptr("ptp"), ptr("ep")
    keep = None
    if rest is not None and rest.numel():
        keep = rest.to(torch.int32).cuda()
        d.rest_idx, d.n_rest = keep.data_ptr(), keep.numel()
    d.unit_begin, d.unit_end = units
    _lib.check(_lib.lib().tan_adamw_step_images(C.byref(d), _stream()), "tan_adamw_step_images")
    torch.cuda.synchronize()
    del keep


def expected_images_call(tab, before, hp, ema_m, units=(0, 0), rest=None, null=()):
    """What one tan_adamw_step_images call must leave in every buffer, from ref32 and the index oracle; `before` = snapshot."""
    n = tab.n
    u0, u1 = units[0], (units[1] if units[1] > 0 else tab.n_units)
    b = {k: t[:n] for k, t in before.items()}
    r = ref32(b["p"], b["g"], b["m"], b["v"], b["mode"], hp)
    in_win = tab.owned & (tab.unit_of >= u0) & (tab.unit_of < u1)
    in_rest = torch.zeros(n, dtype=torch.bool)
    if rest is not None and rest.numel():
        in_rest[rest.long()] = True
    touched = in_win | in_rest
    want = {k: t.clone() for k, t in before.items()}
    for k in "pmv":
        want[k][:n] = torch.where(touched, r[k], b[k])
    has_ema = "e" not in null
    if has_ema:
        want["e"][:n] = torch.where(touched, ema_ref32(b["e"], want["p"][:n], ema_m), b["e"])
    vals = {"p": bits(want["p"][:n].bfloat16()), "e": bits(want["e"][:n].bfloat16())}
    for k in IMAGES:
        if k in null or (k[0] == "e" and not has_ema):
            continue
        src = tab.src[k]
        s = src.clamp(min=0)
        w = (src >= 0) & in_win[s]
        img = bits(want[k])
        img[:n][w] = vals[k[0]][s][w]
        if k == "p16":                             # the plain kernel's shadows on the rest: only where the parameter is stepped
            w = in_rest & (b["mode"] < 2)
            img[:n][w] = vals["p"][w]
        if k == "e16":
            img[:n][in_rest] = vals["e"][in_rest]
    return want, touched


def assert_state(tag, got, want):
    for k in STATE_KEYS:
        a, b = bits(got[k]), bits(want[k])
        assert torch.equal(a, b), (tag, k, int((a != b).sum()), (a != b).nonzero().flatten()[:4].tolist())


def images_step(tag, tab, st, hp, ema_m, **kw):
    """one call, checked in full against the oracle (guards and sentinels are part of the compared buffers)"""
    before = snapshot(st)
    call_images(tab, st, hp, ema_m, **kw)
    after = snapshot(st)
    want, touched = expected_images_call(tab, before, hp, ema_m, **kw)
    assert_state(tag, after, want)
    return before, after, touched


def test_pack_index_is_what_pack_weights_and_transpose_batch_write():
    assert _lib.lib().tan_panel_waves() == PANEL_WAVES
    gen = torch.Generator().manual_seed(1)
    shapes = []
    for (N, K, tn_w, tk_w, tn_t, tk_t) in DEFAULT_ENTRIES:
        shapes.append((N, K, tn_w, tk_w))
        if tn_t:
            shapes.append((K, N, tn_t, tk_t))
    for (N, K, TN, TK) in shapes:
        n = N * K
        w = torch.randn(n, generator=gen).bfloat16()
        src, dst, dst_t = guarded(w), sentinel16(n), sentinel16(n)
        ent = (_lib.PackEntry * 1)(_lib.PackEntry(0, 0, N, K, TN, TK))
        tab = torch.frombuffer(bytearray(bytes(ent)), dtype=torch.uint8).cuda()
        _lib.check(_lib.lib().tan_pack_weights(src.data_ptr(), dst.data_ptr(), tab.data_ptr(), 1, (N // TN) * (K // TK), _stream()),
                   "tan_pack_weights")
        tt = torch.tensor([[0, N, K]], dtype=torch.int64).cuda()
        _lib.check(_lib.lib().tan_transpose_batch(src.data_ptr(), dst_t.data_ptr(), tt.data_ptr(), 1, N, K, _lib.TAN_BF16, _stream()),
                   "tan_transpose_batch")
        torch.cuda.synchronize()
        assert guard_ok(src, n) and guard_ok(dst, n) and guard_ok(dst_t, n)
        assert bits_equal(dst[:n].cpu(), w[pack_index(N, K, TN, TK)]), (N, K, TN, TK)
        assert bits_equal(dst_t[:n].cpu(), w[transpose_index(N, K)]), (N, K)
        assert bits_equal(dst_t[:n].cpu(), w.view(N, K).t().contiguous().view(-1))


def _bounds_on(section, tab, before, after, touched, hp, ema_m):
    n = tab.n
    b = {k: t[:n].cuda() for k, t in before.items()}
    a = {k: t[:n].cuda() for k, t in after.items()}
    sel = touched.cuda()
    check64(section, a, b["p"], b["g"], b["m"], b["v"], b["mode"], hp, sel)
    check_ema64(section, a["e"], b["e"], a["p"], ema_m, sel)


@pytest.mark.parametrize("which", ["default", "plain"])
def test_adamw_images_whole_call(which):
    tab = Table(DEFAULT_ENTRIES if which == "default" else PLAIN_ENTRIES)
    inp = tab.inputs(seed=21)
    hp = HP(step=5, grad_scale=0.5)
    st = tab.device_state(inp)
    before, after, touched = images_step(which, tab, st, hp, 0.999, rest=tab.rest)
    n = tab.n
    assert torch.equal(touched, ~torch.isin(torch.arange(n), tab.nobody))
    for k in ("p", "m", "v", "e"):                               # nobody's elements: bit-unchanged
        assert bits_equal(after[k][:n][tab.nobody], before[k][:n][tab.nobody])
    _bounds_on("images", tab, before, after, touched, hp, 0.999)
    # p, m, v, ema equal tan_adamw_step on the same inputs bit for bit (on everything the image call owns)
    plain = run_adamw(inp, tab.mode, hp, 0.999)
    for k in ("p", "m", "v", "e"):
        assert bits_equal(after[k][:n][touched], plain[k][touched]), k
    check_statements(inp, {k: torch.where(touched, after[k][:n], plain[k]) for k in "pmv"}, tab.mode, hp)
    if which == "plain":                                         # "0 = none": no packed image is ever written
        for k in ("pp", "ptp", "ep"):
            assert is_sentinel(after[k]).all()


def test_adamw_images_null_pointers():
    tab = Table(DEFAULT_ENTRIES[:2] + PLAIN_ENTRIES[:1] + DEFAULT_ENTRIES[4:5])
    inp = tab.inputs(seed=22)
    hp = HP(step=2)
    st = tab.device_state(inp)
    _, full, _ = images_step("all", tab, st, hp, 0.999, rest=tab.rest)
    for null in (("p16",), ("pt",), ("pp",), ("ptp",), ("e16",), ("ep",), ("e",), ("pp", "pt", "ptp", "ep")):
        st = tab.device_state(inp)
        before, after, _ = images_step(null, tab, st, hp, 0.999, rest=tab.rest, null=null)
        untouched = set(null) | ({"e16", "ep"} if "e" in null else set())
        for k in STATE_KEYS:
            if k in untouched:
                assert bits_equal(after[k], before[k]), (null, k)
            else:
                assert bits_equal(after[k], full[k]), (null, k)


@pytest.mark.parametrize("cuts", ["entries", "inside"])
def test_adamw_images_unit_windows(cuts):
    tab = Table(DEFAULT_ENTRIES[1:3] + PLAIN_ENTRIES[1:] + DEFAULT_ENTRIES[5:])
    inp = tab.inputs(seed=23)
    hp = HP(step=9, grad_scale=0.125)
    st = tab.device_state(inp)
    _, whole, _ = images_step("whole", tab, st, hp, 0.999, rest=tab.rest)
    a, b = (tab.prefix[1], tab.prefix[4]) if cuts == "entries" else (tab.prefix[0] + 37, tab.prefix[2] + 2)
    assert 0 < a < b < tab.n_units
    st = tab.device_state(inp)
    images_step("[0,a)", tab, st, hp, 0.999, units=(0, a))
    images_step("[a,b)", tab, st, hp, 0.999, units=(a, b))
    images_step("[b,n)", tab, st, hp, 0.999, units=(b, 0))
    images_step("rest only", tab, st, hp, 0.999, units=(tab.n_units, tab.n_units), rest=tab.rest)
    assert_state("union", snapshot(st), whole)


def test_adamw_images_per_matrix_modes():
    ents = [DEFAULT_ENTRIES[1], PLAIN_ENTRIES[1], DEFAULT_ENTRIES[1], PLAIN_ENTRIES[2], DEFAULT_ENTRIES[5]]
    modes = [0, 1, 2, 3, 2]
    tab = Table(ents, modes)
    tab.mode[tab.rest] = (torch.arange(tab.rest.numel()) % 4).to(torch.uint8)
    inp = tab.inputs(seed=24)
    hp = HP(step=3)
    st = tab.device_state(inp)
    before, after, touched = images_step("modes", tab, st, hp, 0.999, rest=tab.rest)
    n = tab.n
    _bounds_on("images", tab, before, after, touched, hp, 0.999)
    for o, (N, K, *_), md in zip(tab.offs, ents, modes):
        sl = slice(o, o + N * K)
        same = all(bits_equal(after[k][:n][sl], before[k][:n][sl]) for k in "pmv")
        assert same == (md >= 2)
        # the images are the current values whatever the mode, and the EMA twin moved
        assert bits_equal(after["p16"][:n][sl], after["p"][:n][sl].bfloat16())
        assert bits_equal(after["pt"][:n][sl], after["p"][:n][sl].bfloat16().view(N, K).t().reshape(-1))
        assert bits_equal(after["e"][:n][sl], ema_ref32(before["e"][:n][sl], after["p"][:n][sl], 0.999))
        assert not bits_equal(after["e"][:n][sl], before["e"][:n][sl])
        assert bits_equal(after["e16"][:n][sl], after["e"][:n][sl].bfloat16())


@pytest.mark.parametrize("n_rest", [0, 1, 257, -1])
def test_adamw_images_rest_idx(n_rest):
    tab = Table(PLAIN_ENTRIES + DEFAULT_ENTRIES[1:2])
    tab.mode[tab.rest] = ((torch.arange(tab.rest.numel()) // 5) % 4).to(torch.uint8)
    inp = tab.inputs(seed=25)
    hp = HP(step=6, grad_scale=1.0 / 3.0)
    if n_rest < 0:
        rest = tab.rest
    else:                                                  # ascending, runs and single elements
        i = torch.arange(tab.rest.numel())
        rest = tab.rest[(i % 11 < 6) | (i % 11 == 8)][:n_rest]
    st = tab.device_state(inp)
    before, after, touched = images_step("rest", tab, st, hp, 0.999, units=(tab.n_units, tab.n_units), rest=rest)
    assert int(touched.sum()) == rest.numel() == (tab.rest.numel() if n_rest < 0 else n_rest)
    if rest.numel():
        # equals tan_adamw_step restricted to those indices
        plain = run_adamw(inp, tab.mode, hp, 0.999)
        r = rest.long()
        for k in ("p", "m", "v", "e", "e16"):
            assert bits_equal(after[k][:tab.n][r], plain[k][r]), k
        act = tab.mode[r] < 2
        assert bits_equal(after["p16"][:tab.n][r][act], plain["p16"][r][act])


def test_adamw_images_full_model_table():
    """the matrices of a 6 + 6-layer model (the benchmark's unit count), once"""
    tab = Table(DEFAULT_ENTRIES[:4] * 12 + DEFAULT_ENTRIES[4:])
    assert tab.n_units == 12 * 768 + 224
    inp = tab.inputs(seed=26)
    hp = HP(step=12, grad_scale=0.125)
    st = tab.device_state(inp)
    before, after, touched = images_step("full", tab, st, hp, 0.999, rest=tab.rest)
    _bounds_on("images", tab, before, after, touched, hp, 0.999)


def test_host_tables_partition_the_flat_buffer():
    from temporalalignnet_amd.train import Trainer, build_model, default_args
    torch.manual_seed(0)
    args = default_args(model="init", num_encoder_layers=2, num_decoder_layers=2)
    model = build_model(args, compute_dtype="bf16").cuda()
    tr = Trainer(model, args)
    f, st = tr._ensure_state()
    tab, prefix, n_ent, n_units, ranges = tr._adamw_tables(f, st)
    count = torch.zeros(f.total, dtype=torch.int32)
    for lo, hi in ranges:
        count[lo:hi] += 1
    rest = st["rest_idx"].cpu().long()
    assert (rest[1:] > rest[:-1]).all()
    count[rest] += 1
    assert (count == 1).all()
    prefix = prefix.cpu().tolist()
    assert len(ranges) == n_ent == len(prefix) - 1 and prefix[-1] == n_units
    by_off = {o: n for n, (o, _, _) in f.off.items()}
    names = [by_off[lo] for lo, _ in ranges]
    order = [0 if n.startswith("video_temporal_encoder.") else 1 if ".resblocks." in n else 2 for n in names]
    assert order == sorted(order) and set(order) == {0, 1, 2}
    assert all(n.endswith("_pre_proj.weight") for n, o in zip(names, order) if o == 2)
    assert f.video_units == prefix[order.index(1)] and f.mats_units == prefix[order.index(2)]
    ents = (_lib.ImageEntry * n_ent).from_buffer_copy(bytes(tab.cpu().numpy()))
    for e, n, (lo, hi), u0, u1 in zip(ents, names, ranges, prefix, prefix[1:]):
        assert e.off == lo and e.off % 8 == 0 and e.N * e.K == hi - lo and (e.N // 64) * (e.K // 64) == u1 - u0
        assert (e.N, e.K) == tuple(f.off[n][2]) and e.N % 64 == 0 and e.K % 64 == 0
        md = st["mode"][lo:hi]
        assert bool((md == md[0]).all())                 # the image kernel reads one mode per matrix


def test_report_worst_ratios():
    for k in sorted(WORST):
        print(f"WORST {k}: {WORST[k]}")
