"""The row-panel MLP kernels (csrc/tan_panel.hip) through the C ABI (tan_pack_weights, tan_mlp_fwd, tan_mlp_fwd_split, tan_mlp_bwd,
tan_mlp_bwd_split with _lib.MlpDesc / MlpBwdDesc / PackEntry), exactly where the arithmetic can be made exact and per element against
float64 everywhere else.  Inputs, closed forms, references and bounds live in tests/panel_cases.py (checked on the CPU by
test_panel_cases_cpu.py).  R = 64 (one panel), 192 (three: a row0 slip shows) and 4160 (65 panels: more workgroups than the 64 / 24 the
up-front weight touches are spread over); C = 512, FF = 2048.

A. test_pack_whole_image: the full element index map of the three tile formats ([512][16], [256][32], the [384][32] "qkv16"), six
   matrices in ONE launch with unequal non-zero src_off / dst_off inside a sentinel-filled buffer, with max_tiles below the tile
   count (grid-stride loop) and above it; the WHOLE destination buffer is compared bit for bit.
B. Exact structure tests (torch.equal).  Selector weights (one 1.0 per output row, three scrambles that together visit every hidden
   chunk, 32-feature block and k step of every GEMM phase): every MFMA sum is a single product.
     forward   x_mid rows in {c - 1, c + 1}, eps = 0, dyadic ln_2 / biases, b_fc >= 16 (QuickGELU is the identity in f32):
               mean2 == c, |rstd2 - 1| <= one f32 ulp, xn2 == (+-1) g + b, h_pre == bf16(xn2[:, sigma] + b_fc) == h_act,
               x_out == bf16((h_act[:, tau] + b_proj) + x_mid) (the accumulator starts from b_fc; the epilogue adds acc + bias + res from
               the left), evaluated from the kernel's own stored xn2 / h_act; head: x_mid == bf16((attn_o[:, pi] + b_out) + x_in);
               split: seven of the eight planes are zero, x_out and the side outputs are bit-equal to the whole-panel launch
     backward  h_pre = 16 (quickgelu' == 1): dh == dx[:, tau'] (dx = the input or the stored dx_out), d_o == dx2_stored[:, pi'];
               integer dx / dqkv / dstage and integer g0: g_b_fc - g0 and g_ln1_b - g0 are the column sums exactly (the latter sees
               the in_proj head's dxn1 = dqkv[:, sel] + dstage); everything else is held to the section C bound
     pairs     bit-equal x_out, xn_next, nmean, nrstd (and x_mid, xn2, mean2, rstd2 where bound) between modes 0 / 16, 2048 / 2048|16,
               4096 / 4096|16 in EVERY forward case of B and C; bit-equal dh, dx2, dx_out with and without the d_o tail in every
               whole-panel backward case.  (No difference was seen on the device: the pairs stay at torch.equal.)
C. float64 numerics, per element, NO element excluded (test_fp64_fed / test_fp64_chained, forward and backward).  fed: a stage's
   reference is float64 of what the kernel STORED for the stage before it (xn2 -> h_pre, h_act; h_act -> x_out; x_out -> xn_next,
   nmean, nrstd; dx_out -> dh; dh -> dx2 and its column sums; dx2 -> d_o).  h_act is a function of the f32 pre-activation, not of
   the stored h_pre, so it is fed from xn2; the in_proj head's dxn1 never leaves the LDS, so dx_out is chained through it.  chained:
   float64 from the inputs only, every upstream bound propagated (through K = 512 and K = 2048 as if all roundings lined up: wide).
   Inputs: "init" (test_panel_gpu.py's: x_mid ~ 1.5 N(0, 1), weights at their initialisation scale), "large" (|h_pre| up to ~35,
   both tails of the sigmoid; backward: h_pre ~ 10 N(0, 1)) and "sel" (selector weights under random data: the GEMM bounds
   collapse to a few u, which leaves the pointwise arithmetic -- QuickGELU and its derivative, the LayerNorms, the column sums --
   alone under bounds of half a bf16 ulp + a few u; the dense bounds, gamma(K) sum |terms|, are too wide to see a third digit).
   Bounds, u = 2^-24 (panel_cases.py composes them operation by operation, second-order terms kept):
     any f32 operation u |result| (a fused multiply-add counts as two); a bf16 store hu(|ref| + e) <= 2^-8 |x|, the half ulp of the binade
     LN prologue    mean: gamma(13) mean |x| (7 lane-local additions + 6 wave_sum levels); centred squares the same; rsqrtf 2 u;
                    xn2 = ((d rstd) g + b): three operations, then the store
     c_fc           gamma(m) (sum_k |xn2 w| + |b_fc|), m = non-zero products of the row (512 dense, 1 selector; the accumulator starts
                    from the bias), then the store of h_pre
     QuickGELU      on the f32 pre-activation: the exponent carries 4 u (1.702f, log2e, their product, the multiplication) + 1.702 e_pre,
                    exp2 2 u, 1 + E one rounding, rcp 2 u, x * s one rounding, then the store of h_act
     c_proj         gamma(m - 1) sum_k |h_act w| (m = 2048 dense; any order: the split kernels' eight planes are a tree over the same terms),
                    + b_proj, + x_mid: two roundings, then the store of x_out
     next LN        from the bf16-rounded x_out; depth 39 (31 lane-local + half-wave + 7 over the waves; the split finish has 13)
     dh             gamma(m - 1) sum |dx w| times quickgelu'(h_pre) from the bf16 h_pre: t = (x 1.702f) s, t (1 - s) + s, the product, the store
     LN backward    xh = (x - mean) rstd; m1, m2 at depth 13 (ln_1 prologue, split finish) or 39 (panel epilogue); o = rstd (d g - m1 - xh m2)
                    + res: five operations, then the store (dx_out / dx2)
     in_proj head   gamma(m - 1) sum |dqkv w| (K = 1536) + dstage, rounded to bf16 once; d_o: gamma(m - 1) sum |dx2 w|, the store
     column sums    of the UNROUNDED f32 terms: sum of the terms' bounds + gamma(depth + atomics) (sum_rows |term| + |g0|), depth 6 in a
                    panel (14 in the ln_1 prologue), one atomic per workgroup: R / 64, or R / 16 for the split finish

Cases and the instantiation each enters (every forward case runs with and without side outputs; S = stats (xn2, mean2, rstd2) bound,
N = xn_next bound; every whole-panel backward case runs with and without the pwt_out / d_o tail):
  tan_mlp_fwd        mlp_panel_kernel<0> / <16>        exact 64 (S N), 192 (N); init 64 (S N, eps 1e-5), 192 (eps 1e-3), 4160 (S N, 1e-3);
                                                        large 64 (S N); sel 192 (S N)
                     <2048> / <2048|16> (pw_out head)  exact 192 (S N), 4160 (S); init 64 (S N, 1e-3), 4160 (S, 1e-5); large 192 (N); sel 192 (S N)
  tan_mlp_fwd_split  <4096> / <4096|16> +              exact 64 (S N), 4160 (S N); init 64 (S N, 1e-3), 4160 (N, 1e-5); sel 192 (S N)
                     mlp_split_finish_fwd_kernel       (every split launch runs twice in a row, `part` starts as NaN)
  tan_mlp_bwd        <0>, plain dx                     exact 64, 4160; init 64; sel 192; large 192
                     <0>, ln1_dxn prologue             exact 192 (res aliasing dx2, g_ln1 bound); init 192 (res, g_ln1); sel 4160 (res NULL, g_ln1 NULL)
                     <512>, pwt_in head                exact 4160 (dstage, res, g_ln1), 64 (dstage NULL, res NULL, g_ln1 NULL); init 4160 (dstage,
                                                        res, g_ln1), 64 (NULL, NULL, NULL); sel 192 (dstage, res, g_ln1)
  tan_mlp_bwd_split  <4096> +                          exact 192; init 64, 4160; sel 192
                     mlp_split_finish_bwd_kernel
D. Every output lives inside a buffer of -77 with 64 elements in front and behind (guards checked after every launch), starts as NaN;
   the accumulated gradients start from non-zero g0 and the increment is what is checked; test_rejections: every listed bad
   descriptor returns -1 and leaves the NaN outputs untouched.

Measured on an MI355X (worst observed / bound over every case of the group; test_report_worst_ratios prints them):
                             bwd-dx    bwd-inp    bwd-ln1  bwd-split        fwd   fwd-head  fwd-split
  chained/d_o                 0.787      0.557      0.767
  chained/dh                  1.000      0.909      0.999      1.000
  chained/dx2                 0.915      0.697      0.899      0.938
  chained/dx_out                         0.876      1.000
  chained/g_b_fc              0.044      0.104      0.044      0.038
  chained/g_b_out             0.076      0.037      0.017      0.070
  chained/g_dx_colsum                    0.069      0.023
  chained/g_ln1_b                        0.196      0.010
  chained/g_ln1_g                        0.280      0.031
  chained/g_ln_b              0.233      0.082      0.032      0.201
  chained/g_ln_g              0.262      0.130      0.043      0.292
  chained/h_act                                                           0.999      0.764      0.996
  chained/h_pre                                                           0.999      0.822      0.999
  chained/mean2                                                           0.009      0.100      0.005
  chained/nmean                                                           0.073      0.045      0.069
  chained/nrstd                                                           0.046      0.027      0.072
  chained/rstd2                                                           0.096      0.098      0.093
  chained/x_mid                                                                      1.000
  chained/x_out                                                           0.995      0.939      0.989
  chained/xn2                                                             1.000      0.548      0.999
  chained/xn_next                                                         0.530      0.359      0.624
  exact/d_o                   0.000      0.000      0.000
  exact/dh                    0.000      0.000      0.000      0.000
  exact/dx2                   1.000      1.000      1.000      1.000
  exact/dx_out                           0.868      1.000
  exact/g_b_fc                0.000      0.001      0.001      0.000
  exact/g_b_out               0.013      0.012      0.007      0.009
  exact/g_dx_colsum                      0.000      0.015
  exact/g_ln1_b                          0.000      0.000
  exact/g_ln1_g                          0.000      0.032
  exact/g_ln_b                0.000      0.030      0.008      0.000
  exact/g_ln_g                0.077      0.077      0.048      0.036
  exact/h_act                                                             0.000      0.000      0.000
  exact/h_pre                                                             0.000      0.000      0.000
  exact/mean2                                                             0.000      0.000      0.000
  exact/nmean                                                             0.000      0.000      0.000
  exact/nrstd                                                             0.064      0.081      0.045
  exact/rstd2                                                             0.000      0.000      0.000
  exact/x_mid                                                                        0.000
  exact/x_out                                                             1.000      1.000      1.000
  exact/xn2                                                               0.000      0.000      0.000
  exact/xn_next                                                           0.998      0.999      0.999
  fed/d_o                     0.962      0.972      0.958
  fed/dh                      1.000      1.000      1.000      1.000
  fed/dx2                     1.000      1.000      1.000      1.000
  fed/dx_out                             0.876      1.000
  fed/g_b_fc                  0.044      0.034      0.007      0.038
  fed/g_b_out                 0.025      0.018      0.004      0.034
  fed/g_dx_colsum                        0.069      0.023
  fed/g_ln1_b                            0.196      0.010
  fed/g_ln1_g                            0.280      0.031
  fed/g_ln_b                  0.045      0.034      0.007      0.029
  fed/g_ln_g                  0.062      0.074      0.006      0.074
  fed/h_act                                                               1.000      1.000      1.000
  fed/h_pre                                                               1.000      1.000      1.000
  fed/mean2                                                               0.009      0.015      0.005
  fed/nmean                                                               0.018      0.010      0.012
  fed/nrstd                                                               0.048      0.034      0.045
  fed/rstd2                                                               0.096      0.108      0.093
  fed/x_mid                                                                          1.000
  fed/x_out                                                               1.000      1.000      1.000
  fed/xn2                                                                 1.000      1.000      0.999
  fed/xn_next                                                             0.999      0.999      0.999

A bf16 output sits at 1.000 (0.9995 and up) wherever its input is exact: its bound is the half ulp of the store plus a few u, and among
10^5 .. 10^7 elements some land next to a tie; the exact cases reach the tie itself.  The f32 statistics and the column sums stay
below 0.3 because their reduction chains are counted at full length.  The chained bounds of the dense cases are wider than the fed
ones (every upstream bound is carried through the contractions as if the roundings lined up), hence the lower ratios.

Mutants of tan_panel.hip this file was run against once each (none is kept).  Per mutant: the first assertion that failed in the
whole file | the first in section C alone (test_fp64_*); a number is observed / bound.
   1  pack_tiles_kernel: the fields (rho >> 2) & 1 and rho >> 3 of f exchanged, f = rho (kept inside the 32-row block: exchanging
      the two coefficients as they stand would read rows of the next tile)
          test_pack_whole_image[5]: the image differs | fwd fed/h_pre init-64 9012
   2  1.702f -> 1.7f in mlp_epi_p1 (section B cannot see it: QuickGELU is the identity there)
          fwd fed/h_act init-64 2.61 | the same
   3  1.702f -> 1.7f in mlp_bepi_p3 (section B: quickgelu' is 1)
          bwd-dx fed/dh init-64-dx 207 | the same
   4  a.eps dropped from the next LayerNorm's rsqrtf (section B: eps = 0)
          fwd fed/nrstd init-4160 (eps = 1e-3) 82.2 | the same
   5  the next LayerNorm computed from the unrounded v instead of xr
          fwd exact/nmean exact-64 56.7 | fwd fed/nmean init-64 103
   6  split_sum8 starting at plane 1 (plane 0 lost, plane 1 twice)
          exact-64-split: x_out != the closed form (8192 values) | fwd-split fed/x_out init-64-split 603
   7  1.0f / 511 for m2 in pn_ln_bwd_epilogue
          bwd-dx exact/dx2 exact-64-dx 41.5 | bwd-dx fed/dx2 sel-192-dx 47.7 (the dense cases in front of it pass: gamma(2047)
          sum |dh w| is wider than the slip)
   8  dmul = 0 in the in_proj head
          exact-4160-inp: g_ln1_b - g0 != the column sums of dxn1 | bwd-inp fed/dx_out init-4160-inp 252
   9  rmul = 1 with ln1_res == NULL
          bwd-inp exact/dx_out exact-64-inp 533 | bwd-ln1 fed/dx_out sel-4160-ln1 2.4e8
  10  b_out read at bp + 8 pp for both half-waves in the out-projection head
          exact-192-head: x_mid != the closed form | fwd-head fed/x_mid init-64-head 1060
  11  db.v[j] += d * gm.v[j] in the ln_1 prologue
          bwd-ln1 exact/g_ln1_b exact-192-ln1 5.7e4 | bwd-ln1 fed/g_ln1_b init-192-ln1 4.2e4
  12  ds[j] += the bf16-ROUNDED o in mlp_split_finish_bwd_kernel
          bwd-split exact/g_b_out exact-192-split 134 | bwd-split fed/g_b_out sel-192-split 170.  Caught by the selector cases only:
          there the bound of the unrounded terms is a few u per row, while with dense weights gamma(2047) sum |dh w| per row is wider
          than the half ulps that the rounding adds up (init-64-split and init-4160-split pass with this mutant).
"""
import ctypes as C
import math

import pytest
import torch

import panel_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64, BF16 = pc.F32, pc.F64, pc.BF16
SENT, LEAD = -77.0, 64
WORST = {}
_CACHE = {}


def _lib_ops():
    from temporalalignnet_amd import _lib, ops
    return _lib, ops


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


def ptr(t):
    return None if t is None else t.data_ptr()


def pack_launch(src, dst, entries, max_tiles):
    _lib, ops = _lib_ops()
    arr = (_lib.PackEntry * len(entries))(*[_lib.PackEntry(*e) for e in entries])
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    code = _lib.lib().tan_pack_weights(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), C.c_void_p(tab.data_ptr()), len(entries),
                                       max_tiles, ops._stream())
    torch.cuda.synchronize()
    return code


def packed(I, names):
    """the packed images of I's weight matrices (in flat_params.py's formats), cached on the case"""
    pw = I.setdefault("_pw", {})
    todo = [n for n in names if n not in pw]
    if todo:
        mats = [I[n].contiguous() for n in todo]
        src = torch.cat([m.reshape(-1) for m in mats])
        dst = torch.empty_like(src)
        ents, off, mx = [], 0, 0
        for m in mats:
            N, K = m.shape
            TN, TK = pc.tile_format(N, K)
            ents.append((off, off, N, K, TN, TK))
            mx, off = max(mx, (N // TN) * (K // TK)), off + N * K
        assert pack_launch(src, dst, ents, mx) == 0
        off = 0
        for n, m in zip(todo, mats):
            pw[n] = dst[off:off + m.numel()]
            off += m.numel()
    return [pw[n] for n in names]


def ratio(key, case, got, ref, bound):
    r = pc.worst_ratio(got, ref, bound)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1.0, (key, case, f"observed / bound = {r:.4g}")
    return r


# ======================================================================================================================
# launches
# ======================================================================================================================
def split_twice(run, *args, **kw):
    """a split launch twice in a row on ONE `part` (NaN before the first, the first launch's planes before the second), each into
    fresh NaN outputs and gradients at g0; both are checked for guards and return codes, the second one's outputs are returned"""
    pbuf, part = guarded((8, args[0]["R"], 512), F32)
    run(*args, _part=part, **kw)
    O = run(*args, _part=part, **kw)
    assert intact(pbuf), "a split launch wrote outside `part`"
    return O


def run_fwd(I, side=True, split=False, nxt=True, stats=True, tweak=None, _part=None):
    """one tan_mlp_fwd / tan_mlp_fwd_split launch (the split one twice in a row) into guarded NaN outputs.  tweak(d): a bad descriptor;
    the call must then return -1 and leave everything untouched."""
    if split and _part is None:
        return split_twice(run_fwd, I, side=side, split=True, nxt=nxt, stats=stats, tweak=tweak)
    _lib, ops = _lib_ops()
    R, head = I["R"], "attn_o" in I
    bufs, O = {}, {}

    def out(name, shape, dtype):
        bufs[name], O[name] = guarded(shape, dtype)
        return O[name].data_ptr()
    d = _lib.MlpDesc()
    d.rows, d.C, d.FF, d.eps, d.variant = R, 512, 2048, I["eps"], 0
    pw_fc, pw_pj = packed(I, ["w_fc", "w_proj"])
    d.ln_g, d.ln_b, d.pw_fc, d.pw_proj, d.b_fc, d.b_proj = (ptr(t) for t in (I["ln_g"], I["ln_b"], pw_fc, pw_pj, I["b_fc"], I["b_proj"]))
    if head:
        d.x_mid = out("x_mid", (R, 512), BF16)
        d.attn_o, d.pw_out, d.b_out, d.x_in = ptr(I["attn_o"]), ptr(packed(I, ["w_out"])[0]), ptr(I["b_out"]), ptr(I["x_in"])
    else:
        d.x_mid = ptr(I["x_mid"])
    d.x_out = out("x_out", (R, 512), BF16)
    if side:
        d.h_pre, d.h_act = out("h_pre", (R, 2048), BF16), out("h_act", (R, 2048), BF16)
    if stats:
        d.xn2, d.mean2, d.rstd2 = out("xn2", (R, 512), BF16), out("mean2", (R,), F32), out("rstd2", (R,), F32)
    if nxt:
        d.nln_g, d.nln_b = ptr(I["nln_g"]), ptr(I["nln_b"])
        d.xn_next, d.nmean, d.nrstd = out("xn_next", (R, 512), BF16), out("nmean", (R,), F32), out("nrstd", (R,), F32)
    if tweak is not None:
        tweak(d)
    if split:
        codes = [_lib.lib().tan_mlp_fwd_split(C.byref(d), C.c_void_p(_part.data_ptr()), ops._stream())]
    else:
        codes = [_lib.lib().tan_mlp_fwd(C.byref(d), ops._stream())]
    torch.cuda.synchronize()
    assert all(intact(b) for b in bufs.values()), ("a forward launch wrote outside its outputs", [k for k, b in bufs.items() if not intact(b)])
    if tweak is not None:
        assert codes == [-1] * len(codes), codes
        assert all(bool(torch.isnan(v).all()) for v in O.values()), "a rejected call wrote to its outputs"
        return None
    assert codes == [0] * len(codes), codes
    return O


GRADS = ("g_b_fc", "g_ln_g", "g_ln_b", "g_b_out", "g_ln1_g", "g_ln1_b", "g_dx_colsum")


def run_bwd(I, tail=False, split=False, gl=True, tweak=None, _part=None):
    """one tan_mlp_bwd / tan_mlp_bwd_split launch (the split one twice in a row).  ln1_res aliases dx2 (as in tan_encoder_bwd) where
    the case has a residual gradient, else it is NULL."""
    if split and _part is None:
        return split_twice(run_bwd, I, tail=tail, split=True, gl=gl, tweak=tweak)
    _lib, ops = _lib_ops()
    R, form = I["R"], I["form"]
    bufs, O = {}, {}

    def out(name, shape, dtype, fill=float("nan")):
        bufs[name], O[name] = guarded(shape, dtype, fill)
        return O[name].data_ptr()
    d = _lib.MlpBwdDesc()
    d.rows, d.C, d.FF = R, 512, 2048
    pwt_proj, pwt_fc = packed(I, ["wt_proj", "wt_fc"])
    d.h_pre, d.x_mid, d.mean2, d.rstd2, d.ln_g = (ptr(I[k]) for k in ("h_pre", "x_mid", "mean2", "rstd2", "ln_g"))
    d.pwt_proj, d.pwt_fc = ptr(pwt_proj), ptr(pwt_fc)
    d.dh = out("dh", (R, 2048), BF16)
    res = I.get("res")
    d.dx2 = out("dx2", (R, 512), BF16, res if res is not None else float("nan"))
    for k in GRADS[:4]:
        setattr(d, k, out(k, (2048 if k == "g_b_fc" else 512,), F32, I["g0"][k]))
    if form == "dx":
        d.dx = ptr(I["dx"])
    else:
        d.ln1_x, d.ln1_mean, d.ln1_rstd, d.ln1_g = (ptr(I[k]) for k in ("ln1_x", "ln1_mean", "ln1_rstd", "ln1_g"))
        d.ln1_res = O["dx2"].data_ptr() if res is not None else None
        d.dx_out = out("dx_out", (R, 512), BF16)
        if gl:
            for k in GRADS[4:]:
                setattr(d, k, out(k, (512,), F32, I["g0"][k]))
        if form == "ln1":
            d.ln1_dxn = ptr(I["ln1_dxn"])
        else:
            d.dqkv, d.pwt_in, d.dstage = ptr(I["dqkv"]), ptr(packed(I, ["wt_in"])[0]), ptr(I["dstage"])
    if tail:
        d.pwt_out, d.d_o = ptr(packed(I, ["wt_out"])[0]), out("d_o", (R, 512), BF16)
    if tweak is not None:
        tweak(d)
    if split:
        codes = [_lib.lib().tan_mlp_bwd_split(C.byref(d), C.c_void_p(_part.data_ptr()), ops._stream())]
    else:
        codes = [_lib.lib().tan_mlp_bwd(C.byref(d), ops._stream())]
    torch.cuda.synchronize()
    assert all(intact(b) for b in bufs.values()), ("a backward launch wrote outside its outputs", [k for k, b in bufs.items() if not intact(b)])
    if tweak is not None:
        assert codes == [-1] * len(codes), codes
        for k, v in O.items():
            want = I["g0"][k] if k in GRADS else (res if k == "dx2" and res is not None else None)
            ok = torch.isnan(v).all() if want is None else (v == want).all()
            assert bool(ok), ("a rejected call wrote to", k)
        return None
    assert codes == [0] * len(codes), codes
    return O


# ======================================================================================================================
# A. the packer, whole image
# ======================================================================================================================
@pytest.mark.parametrize("max_tiles", [5, 1 << 20])
def test_pack_whole_image(max_tiles):
    """six matrices (flat_params.py's shapes and formats, in_proj in both of its formats) in one launch; src_off and dst_off are
    non-zero and unequal (the destination order is the reverse of the source order, with guard gaps); max_tiles = 5 makes every
    block of the grid walk up to 26 tiles, the large value gives the 64-block grid two tiles of the 128-tile matrices each."""
    n_tot = sum(N * K for N, K, _ in pc.PACK_MATRICES)
    i = torch.arange(72 + n_tot, device=DEV, dtype=torch.int64)
    src = (((i * 2654435761) >> 13) & 0xFFFF).to(torch.int32).to(torch.int16).view(BF16)       # pseudo-random bit patterns
    gap = 64
    dst = torch.full((gap + n_tot + gap * len(pc.PACK_MATRICES),), SENT, dtype=BF16, device=DEV)
    want = dst.clone()
    ents, soff = [], 72
    doffs, doff = [], gap
    for N, K, _ in reversed(pc.PACK_MATRICES):
        doffs.append(doff)
        doff += N * K + gap
    doffs.reverse()
    for (N, K, q16), doff in zip(pc.PACK_MATRICES, doffs):
        TN, TK = pc.tile_format(N, K, q16)
        ents.append((soff, doff, N, K, TN, TK))
        idx = pc.pack_index_map(N, K, TN, TK).to(DEV)
        want[doff:doff + N * K] = src[soff:soff + N * K][idx]
        assert soff != doff and soff % 8 == 0 and doff % 8 == 0
        soff += N * K
    assert pack_launch(src, dst, ents, max_tiles) == 0
    assert torch.equal(bits(dst), bits(want))


# ======================================================================================================================
# B + C, forward
# ======================================================================================================================
#            id                kind     R     seed head   split  nxt    stats  eps
FWD_CASES = [("exact-64",       "exact", 64,   0,   False, False, True,  True,  0.0),
             ("exact-192",      "exact", 192,  2,   False, False, True,  False, 0.0),
             ("exact-192-head", "exact", 192,  1,   True,  False, True,  True,  0.0),
             ("exact-4160-head", "exact", 4160, 0,  True,  False, False, True,  0.0),
             ("exact-64-split", "exact", 64,   1,   False, True,  True,  True,  0.0),
             ("exact-4160-split", "exact", 4160, 2, False, True,  True,  True,  0.0),
             ("init-64",        "init",  64,   10,  False, False, True,  True,  1e-5),
             ("init-192",       "init",  192,  11,  False, False, False, False, 1e-3),
             ("init-4160",      "init",  4160, 12,  False, False, True,  True,  1e-3),
             ("large-64",       "large", 64,   13,  False, False, True,  True,  1e-5),
             ("sel-192",        "sel",   192,  14,  False, False, True,  True,  1e-3),
             ("init-64-head",   "init",  64,   15,  True,  False, True,  True,  1e-3),
             ("init-4160-head", "init",  4160, 16,  True,  False, False, True,  1e-5),
             ("large-192-head", "large", 192,  17,  True,  False, True,  False, 1e-5),
             ("sel-192-head",   "sel",   192,  18,  True,  False, True,  True,  1e-5),
             ("init-64-split",  "init",  64,   19,  False, True,  True,  True,  1e-3),
             ("init-4160-split", "init", 4160, 20,  False, True,  True,  False, 1e-5),
             ("sel-192-split",  "sel",   192,  21,  False, True,  True,  True,  1e-5)]
FWD_IDS = [c[0] for c in FWD_CASES]


def fwd_group(head, split):
    return "fwd-split" if split else ("fwd-head" if head else "fwd")


def fwd_run(case):
    """inputs and the two launches (with / without side outputs) of a case, once per session"""
    cid, kind, R, seed, head, split, nxt, stats, eps = case
    if ("fwd", cid) not in _CACHE:
        I = pc.exact_fwd_inputs(R, seed, head=head, eps=eps) if kind == "exact" else pc.fwd_inputs(R, seed, kind, head=head, eps=eps)
        I = pc.to_device(I, DEV)
        I["sel"] = pc.to_device(I["sel"], DEV)
        O = run_fwd(I, True, split, nxt, stats)
        O16 = run_fwd(I, False, split, nxt, stats)
        _CACHE["fwd", cid] = (I, O, O16)
    return _CACHE["fwd", cid]


def check_pair(cid, O, O16):
    for k in ("x_mid", "xn2", "mean2", "rstd2", "x_out", "xn_next", "nmean", "nrstd"):
        if k in O:
            assert torch.equal(bits(O[k]), bits(O16[k])), (cid, k, "differs between the instantiations with and without side outputs",
                                                           int((bits(O[k]) != bits(O16[k])).sum()))
    assert "h_pre" not in O16 and "h_act" not in O16


def check_fwd(tag, case, I, O, ref):
    cid, head, split = case[0], case[4], case[5]
    for k, (r, b) in ref.items():
        if k in O:
            ratio(f"{fwd_group(head, split)}/{tag}/{k}", cid, O[k], r, b)


@pytest.mark.parametrize("case", [c for c in FWD_CASES if c[1] == "exact"], ids=[c[0] for c in FWD_CASES if c[1] == "exact"])
def test_exact_forward(case):
    cid, kind, R, seed, head, split, nxt, stats, eps = case
    I, O, O16 = fwd_run(case)
    check_pair(cid, O, O16)
    if head:
        assert torch.equal(O["x_mid"], pc.exact_head_closed(I)) and torch.equal(O["x_mid"], I["x_mid"]), (cid, "x_mid of the pw_out head")
    if stats:
        assert torch.equal(O["mean2"], I["c"]), (cid, "mean2 != c")
        assert bool(((O["rstd2"] - 1).abs() <= 2.0 ** -23).all()), (cid, "rstd2 is not 1 within an ulp")
        xn2 = O["xn2"]
        assert torch.equal(xn2, pc.exact_xn2(I)), (cid, "xn2 != (+-1) g + b", int((xn2 != pc.exact_xn2(I)).sum()))
    else:
        xn2 = pc.exact_xn2(I)
    h_pre, x_out = pc.exact_fwd_closed(I, xn2, O["h_act"], I["x_mid"])
    assert torch.equal(O["h_pre"], h_pre), (cid, "h_pre != bf16(xn2[:, sigma] + b_fc)", int((O["h_pre"] != h_pre).sum()))
    assert torch.equal(O["h_act"], O["h_pre"]), (cid, "QuickGELU is not the identity", int((O["h_act"] != O["h_pre"]).sum()))
    assert torch.equal(O["x_out"], x_out), (cid, "x_out != bf16((h_act[:, tau] + b_proj) + x_mid)", int((O["x_out"] != x_out).sum()))
    if split:       # seven of the eight planes are exactly zero: bit-equal to the whole-panel launch
        W = run_fwd(I, True, False, nxt, stats)
        for k in ("xn2", "mean2", "rstd2", "h_pre", "h_act", "x_out"):
            assert torch.equal(bits(W[k]), bits(O[k])), (cid, k, "split != whole panel")
    check_fwd("exact", case, I, O, pc.fwd_reference(I, O))             # xn_next, nmean, nrstd (and the rest once more) under section C


@pytest.mark.parametrize("case", [c for c in FWD_CASES if c[1] != "exact"], ids=[c[0] for c in FWD_CASES if c[1] != "exact"])
def test_fp64_fed_forward(case):
    I, O, O16 = fwd_run(case)
    check_pair(case[0], O, O16)
    if case[1] == "large":
        assert O["h_pre"].float().max().item() > 25 and O["h_pre"].float().min().item() < -25
    check_fwd("fed", case, I, O, pc.fwd_reference(I, O))


@pytest.mark.parametrize("case", [c for c in FWD_CASES if c[1] != "exact"], ids=[c[0] for c in FWD_CASES if c[1] != "exact"])
def test_fp64_chained_forward(case):
    I, O, O16 = fwd_run(case)
    check_fwd("chained", case, I, O, pc.fwd_reference(I))


# ======================================================================================================================
# B + C, backward
# ======================================================================================================================
#            id                  kind     R     seed form   split  dstage res    gl     hscale
BWD_CASES = [("exact-64-dx",      "exact", 64,   0,   "dx",  False, True,  True,  True,  1.0),
             ("exact-4160-dx",    "exact", 4160, 1,   "dx",  False, True,  True,  True,  1.0),
             ("exact-192-ln1",    "exact", 192,  1,   "ln1", False, True,  True,  True,  1.0),
             ("exact-4160-inp",   "exact", 4160, 2,   "inp", False, True,  True,  True,  1.0),
             ("exact-64-inp",     "exact", 64,   1,   "inp", False, False, False, False, 1.0),
             ("exact-192-split",  "exact", 192,  0,   "dx",  True,  True,  True,  True,  1.0),
             ("init-64-dx",       "init",  64,   30,  "dx",  False, True,  True,  True,  1.0),
             ("large-192-dx",     "init",  192,  31,  "dx",  False, True,  True,  True,  10.0),
             ("sel-192-dx",       "sel",   192,  32,  "dx",  False, True,  True,  True,  1.0),
             ("init-192-ln1",     "init",  192,  33,  "ln1", False, True,  True,  True,  1.0),
             ("sel-4160-ln1",     "sel",   4160, 34,  "ln1", False, True,  False, False, 1.0),
             ("init-4160-inp",    "init",  4160, 35,  "inp", False, True,  True,  True,  1.0),
             ("init-64-inp",      "init",  64,   36,  "inp", False, False, False, False, 1.0),
             ("sel-192-inp",      "sel",   192,  37,  "inp", False, True,  True,  True,  1.0),
             ("init-64-split",    "init",  64,   38,  "dx",  True,  True,  True,  True,  1.0),
             ("sel-192-split",    "sel",   192,  39,  "dx",  True,  True,  True,  True,  1.0),
             ("init-4160-split",  "init",  4160, 40,  "dx",  True,  True,  True,  True,  1.0)]


def bwd_group(form, split):
    return "bwd-split" if split else f"bwd-{form}"


def bwd_run(case):
    cid, kind, R, seed, form, split, dstage, res, gl, hscale = case
    if ("bwd", cid) not in _CACHE:
        I = pc.to_device(pc.bwd_inputs(R, seed, kind, form, dstage=dstage, res=res, hscale=hscale), DEV)
        I["sel"] = pc.to_device(I["sel"], DEV)
        O = run_bwd(I, tail=not split, split=split, gl=gl)
        O0 = None if split else run_bwd(I, tail=False, split=False, gl=gl)
        _CACHE["bwd", cid] = (I, O, O0)
    return _CACHE["bwd", cid]


def check_bwd(tag, case, I, O, ref):
    cid, form, split = case[0], case[4], case[5]
    for k, (r, b) in ref.items():
        if k in O:
            ratio(f"{bwd_group(form, split)}/{tag}/{k}", cid, O[k], r, b)


def check_tail_pair(cid, O, O0):
    if O0 is not None:
        for k in ("dh", "dx2", "dx_out"):
            if k in O:
                assert torch.equal(bits(O[k]), bits(O0[k])), (cid, k, "differs with and without the d_o tail")


def _sel(case, kinds):
    return dict(argvalues=[c for c in case if c[1] in kinds], ids=[c[0] for c in case if c[1] in kinds])


@pytest.mark.parametrize("case", **_sel(BWD_CASES, ("exact",)))
def test_exact_backward(case):
    cid, kind, R, seed, form, split, dstage, res, gl, hscale = case
    I, O, O0 = bwd_run(case)
    check_tail_pair(cid, O, O0)
    dxp = I["dx"] if form == "dx" else O["dx_out"]
    want = dxp[:, I["sel"]["projT"]]
    assert torch.equal(O["dh"], want), (cid, "dh != dx[:, tau']", int((O["dh"] != want).sum()))
    if not split:
        want = O["dx2"][:, I["sel"]["outT"]]
        assert torch.equal(O["d_o"], want), (cid, "d_o != dx2[:, pi']", int((O["d_o"] != want).sum()))
    if form == "dx":
        inc = I["dx"].double()[:, I["sel"]["projT"]].sum(0)
        assert inc.abs().max().item() * 2 < 2 ** 24
        assert torch.equal(O["g_b_fc"].double() - I["g0"]["g_b_fc"], inc), (cid, "g_b_fc - g0 != the column sums of dh")
    if form == "inp" and gl:
        dxn1 = I["dqkv"].double()[:, I["sel"]["inT"]] + (I["dstage"].double() if dstage else 0.0)
        assert torch.equal(O["g_ln1_b"].double() - I["g0"]["g_ln1_b"], dxn1.sum(0)), (cid, "g_ln1_b - g0 != the column sums of dxn1")
    check_bwd("exact", case, I, O, pc.bwd_reference(I, O, split=split, tail=not split))


@pytest.mark.parametrize("case", **_sel(BWD_CASES, ("init", "sel")))
def test_fp64_fed_backward(case):
    I, O, O0 = bwd_run(case)
    check_tail_pair(case[0], O, O0)
    check_bwd("fed", case, I, O, pc.bwd_reference(I, O, split=case[5], tail=not case[5]))


@pytest.mark.parametrize("case", **_sel(BWD_CASES, ("init", "sel")))
def test_fp64_chained_backward(case):
    I, O, O0 = bwd_run(case)
    check_bwd("chained", case, I, O, pc.bwd_reference(I, None, split=case[5], tail=not case[5]))


# ======================================================================================================================
# D. rejections
# ======================================================================================================================
def test_rejections():
    """each bad descriptor returns -1 and leaves the NaN-filled outputs (and the gradients' starting values) untouched"""
    def s(**kw):
        def tweak(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return tweak
    I = pc.to_device(pc.fwd_inputs(64, 50, "init"), DEV)
    H = pc.to_device(pc.fwd_inputs(64, 51, "init", head=True), DEV)
    dummy = torch.zeros(64 * 2048, dtype=BF16, device=DEV)
    for sp in (False, True):
        for tw in (s(rows=100), s(rows=0), s(C=256), s(FF=1024), s(h_act=None), s(rstd2=None), s(nln_g=None), s(nrstd=None)):
            run_fwd(I, split=sp, tweak=tw)
    run_fwd(I, side=False, tweak=s(h_pre=dummy.data_ptr()))                     # h_pre without h_act
    for tw in (s(attn_o=None), s(b_out=None), s(x_in=None)):                    # pw_out without the rest of the head
        run_fwd(H, tweak=tw)
    run_fwd(I, split=True, tweak=s(pw_out=dummy.data_ptr()))                    # the split entry runs the MLP branch only
    B = {f: pc.to_device(pc.bwd_inputs(64, 52, "init", f), DEV) for f in ("dx", "ln1", "inp")}
    for sp in (False, True):
        for tw in (s(rows=100), s(C=256), s(FF=1024)):
            run_bwd(B["dx"], split=sp, tweak=tw)
    run_bwd(B["inp"], tweak=s(dqkv=None))                                       # pwt_in without dqkv
    run_bwd(B["inp"], tweak=s(ln1_dxn=dummy.data_ptr()))                        # pwt_in together with ln1_dxn
    run_bwd(B["ln1"], tweak=s(dx_out=None))                                     # a prologue without dx_out
    run_bwd(B["inp"], tweak=s(dx_out=None))
    run_bwd(B["dx"], tail=True, tweak=s(d_o=None))                              # pwt_out without d_o
    run_bwd(B["dx"], split=True, tweak=s(pwt_in=dummy.data_ptr(), dqkv=dummy.data_ptr()))
    run_bwd(B["dx"], split=True, tweak=s(pwt_out=dummy.data_ptr(), d_o=dummy.data_ptr()))
    run_bwd(B["dx"], split=True, tweak=s(ln1_dxn=dummy.data_ptr()))


def test_report_worst_ratios():
    """prints the table of the module docstring (run the whole file with -s); every group has been entered"""
    groups = sorted({k.split("/")[0] for k in WORST})
    if not WORST:                       # (run alone: nothing to report)
        return
    names = []
    for k in WORST:
        n = k.split("/", 1)[1]
        if n not in names:
            names.append(n)
    print("\n" + " " * 24 + "".join(f"{g:>11}" for g in groups))
    for n in sorted(names, key=lambda n: (n.split("/")[0], n)):
        row = "".join(f"{WORST[g + '/' + n]:11.3f}" if g + "/" + n in WORST else " " * 11 for g in groups)
        print(f"  {n:<22}" + row)
    assert set(groups) == {"fwd", "fwd-head", "fwd-split", "bwd-dx", "bwd-ln1", "bwd-inp", "bwd-split"}
    assert all(v <= 1.0 for v in WORST.values())
