"""Every kernel of csrc/tan_norm.hip at every dispatch branch and edge, through ops.py (and the C ABI directly where ops.py has no
wrapper: tan_rows_gather, tan_quickgelu, tan_transpose_batch).  Two kinds of test:

A. Exact-integer structure tests (torch.equal, no tolerance).  The inputs are small integers, so every f32 sum and product is exact
   and the order of the atomics cannot matter; a dropped, duplicated or misplaced row changes a result by at least 1.  What keeps a
   case exact: every partial sum of an f32 accumulator stays below 2^24 in magnitude (asserted from the data as the sum of the
   magnitudes of the added terms, which bounds every partial sum in every order), and every value stored as bf16 is an integer of
   at most 8 significant bits (|v| <= 256) -- except the LayerNorm dx, which is built to need more and must come back ROUNDED.
     LayerNorm backward: mean = 0, rstd = 1 are fed by hand, so xhat = x.  x, dy in [-3, 3], gamma in [-20, 20], dres in [-250, 250];
     eight channels per row are fixed up (x = 1 / 0, gamma = 1, |dy| <= C / 8 <= 128) so that sum(g) and sum(g x) are multiples of C and
     m1, m2 are INTEGERS (in general they are multiples of 1 / C, and 9000 rows of those would leave 2^24).  Worst case C = 1024:
     |sum g x| <= 183 392, |m2| <= 179, |m1| <= 61, |dx| <= 128 + 61 + 537 + 250 = 976, 9000 rows of it 8.8e6 < 2^24 = 1.67e7.
     colsum / group_sum / reduce_add / rows_copy / head_bwd: |x| <= 8 (or 2, 3), at most 9000 terms; bf16 results <= 256.
B. fp64 numerics tests on random data.  Every reference is plain float64 PyTorch (F.layer_norm + autograd, x / x.norm(),
   F.interpolate, x * sigmoid(1.702 x)) of the values the kernel read (bf16 inputs upcast).  Every bound is
       output rounding (2^-8 |ref| for a bf16 store, 2^-24 |ref| for f32)  +  an f32 evaluation term
   derived next to its assertion from the kernel's structure: the longest chain of additions an output goes through, applied to
   the sum of the magnitudes of the added terms (u = 2^-24).  D_ROW = 14 is the longest chain of a row reduction in this file:
   8 sequential adds per lane + 6 wave levels in the bf16x8 kernels (the generic ones have 2 + NCH + 6 <= 12).  The bounds are worst
   cases, errors are not: a ratio far below 1 is expected, and section A is what catches a structural slip.

Which test enters which kernel (every instantiation the entry points of tan_norm.hip can launch):
  ln_fwd_kernel<f32|bf16, 1|2|4>           test_ln_fwd_fp64 (bf16 NCH = 2 only through the 8-byte-offset case)
  ln_fwd_bf16x8_kernel<2>                  test_ln_fwd_fp64[bf16-512-aligned]
  ln_bwd_kernel<f32|bf16, 1|2|4>           test_ln_bwd_integer_generic, test_ln_bwd_integer_misaligned (bf16 NCH = 2), test_ln_bwd_fp64
  ln_bwd_finalize                          the same tests: nblk 1 .. 129 and the 1024-block cap, empty slices, the unrolled fold
  ln_bwd_bf16x8_kernel<true, 4>            test_ln_bwd_integer_fast_path, test_ln_bwd_fp64[bf16-512-aligned]
  l2n_fwd_kernel / l2n_bwd_kernel<T, NCH>  test_l2norm_fp64
  colsum_kernel<T>, colsum_generic_kernel<T>   test_colsum_integer
  rows_kernel<T, false|true>               test_rows_copy_integer
  rows_gather_kernel<T>                    test_rows_gather
  group_sum_kernel<T>, reduce_add_kernel   test_group_sum_integer, test_reduce_add_integer
  cast_kernel<f32|bf16, f32|bf16>          test_cast_bits
  quickgelu_kernel<T>                      test_quickgelu_fp64
  head_fwd_kernel<T, NCH>                  test_head_fwd_fp64
  head_bwd_kernel<T, NCH>                  test_head_bwd_integer
  interp_kernel, interp_bwd_kernel         test_interp_fp64, test_interp_bwd_identity
  transpose_batch_kernel                   test_transpose_batch_uneven
NOT covered: ln_bwd_bf16x8_kernel<false, 2>.  tan_layernorm_bwd's `atomic_blocks` is a non-zero constant, so no call through the
ABI reaches it.

Measured on an MI355X (worst observed / bound over every case of a kernel; test_report_worst_ratios prints them):
  kernel / output            f32      bf16
  ln_fwd   mean              0.077    0.011
  ln_fwd   rstd              0.123    0.118
  ln_fwd   y                 0.176    0.996
  ln_bwd   dx                0.235    0.996
  ln_bwd   dgamma            0.043    0.041
  ln_bwd   dbeta             0.110    0.175
  ln_bwd   dx_colsum         0.083    0.111
  l2n_fwd  inv_norm          0.234    0.202
  l2n_fwd  y                 0.271    0.981
  l2n_bwd  dx                0.232    0.974
  head_fwd out               0.030    0.026
  quickgelu y                0.479    0.996
  interp   dst               0.346    -
  interp_bwd dsrc            0.356    -
A bf16 output sits at 0.98 - 1.00 because its bound is the store's half ulp and little else, and some element always rounds from
next to a tie; the sums over rows sit at 0.04 - 0.18 because their chains are counted at full length.

Mutants of tan_norm.hip this file was run against once each (none is kept anywhere), with the first assertion that failed:
  wgt[q] -> 1.0f in ln_bwd_bf16x8_kernel            test_ln_bwd_integer_fast_path, every row count but 4096 (rows=1, 7, 1024, 1025, ...)
  s3 left out of ln_bwd_finalize's fold              test_ln_bwd_integer_generic at rows=416 (nblk = 104), every C and type
  second row's addend row0 % add_period (fwd x8)     test_ln_fwd_fp64[bf16-512-aligned] at rows=2 period=3
  variance / (C - 1) in ln_fwd_kernel                test_ln_fwd_fp64 ln_fwd/rstd at rows=1, all six generic configurations
  colsum_kernel's r1 one row short                   test_colsum_integer at C=8 rows=1, both types
  fourth wave left out of head_bwd_kernel's LDS sum  test_head_bwd_integer at rows=15, every C and type
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DT = [F32, BF16]
U = 2.0 ** -24
TAG = {F32: "f32", BF16: "bf16"}
RND = {F32: 2.0 ** -24, BF16: 2.0 ** -8}      # half an ulp of the stored format, relative
D_ROW = 14                                     # longest addition chain of a row reduction (see the module docstring)
EXACT = 2 ** 24
SENT = -77.0                                   # guard value around offset views (exact in bf16)
WORST = {}                                     # "kernel/output" -> worst observed / bound
LN_CONFIGS = [(F32, 256, False), (F32, 512, False), (F32, 1024, False), (BF16, 256, False), (BF16, 512, False),
              (BF16, 1024, False), (BF16, 512, True)]
LN_IDS = [f"{TAG[d]}-{c}-{'offset8' if o else 'aligned'}" for d, c, o in LN_CONFIGS]


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def ri(shape, lo, hi, seed):
    """integers in [lo, hi] as int64 on the device"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed), device=DEV)


def rn(shape, dtype, seed, scale=1.0):
    return (torch.randn(tuple(shape), generator=_gen(seed), device=DEV) * scale).to(dtype)


def off_view(t, lead=4, tail=12):
    """a copy of t that starts `lead` elements into a larger guard-filled buffer (bf16: 8 bytes in, the generic kernels' alignment)"""
    buf = torch.full((lead + t.numel() + tail,), SENT, dtype=t.dtype, device=DEV)
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    return buf, v


def guard_intact(buf, n, lead=4):
    return bool((buf[:lead] == SENT).all()) and bool((buf[lead + n:] == SENT).all())


def place(t, offset):
    return off_view(t)[1] if offset else t


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def ratio(key, case, got, ref, bound):
    """observed / bound, worst element; recorded per kernel; where the bound is 0 the result must be exact.  NaN fails."""
    err = (got.double() - ref).abs()
    bound = bound.expand_as(err)
    pos = bound > 0
    assert bool((err[~pos] == 0).all()), (key, case, "inexact where the bound is 0")
    r = (err[pos] / bound[pos]).max().item() if bool(pos.any()) else 0.0
    assert math.isfinite(r), (key, case, r)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1.0, (key, case, f"observed / bound = {r:.4g}")
    return r


# ======================================================================================================================
# A. exact-integer structure tests
# ======================================================================================================================

def ln_int_case(rows, Cc, seed):
    """Integer x, dy, gamma, dres with sum(g) and sum(g x) multiples of C in every row (see the module docstring), and the exact
    results in int64: core = g - m1 - x m2 (dx without the residual), sum_r dy x, sum_r dy."""
    x, dy = ri((rows, Cc), -3, 3, seed), ri((rows, Cc), -3, 3, seed + 1)
    gamma, dres = ri((Cc,), -20, 20, seed + 2), ri((rows, Cc), -250, 250, seed + 3)
    x[:, 0:4], x[:, 4:8], gamma[0:8], dy[:, 0:8] = 1, 0, 1, 0

    def cmod(t):                               # the representative of t mod C in [-C/2, C/2)
        return (t + Cc // 2) % Cc - Cc // 2

    def spread(t):                             # four integers of magnitude <= C/8 that add up to t
        base = torch.div(t, 4, rounding_mode="floor")
        return base[:, None] + (torch.arange(4, device=DEV)[None] < (t - 4 * base)[:, None]).long()

    g = dy * gamma
    t2 = cmod(-(g * x).sum(1))
    dy[:, 0:4] = spread(t2)                    # x = 1, gamma = 1 there: adds t2 to sum(g x) and to sum(g)
    dy[:, 4:8] = spread(cmod(-(g.sum(1) + t2)))   # x = 0, gamma = 1 there: adds to sum(g) alone
    g = dy * gamma
    s1, s2 = g.sum(1), (g * x).sum(1)
    assert bool((s1 % Cc == 0).all()) and bool((s2 % Cc == 0).all())
    m1, m2 = s1 // Cc, s2 // Cc
    core = g - m1[:, None] - x * m2[:, None]
    # exactness: every per-row and per-column accumulator, bounded by the sum of the magnitudes of its terms
    assert int((g * x).abs().sum(1).max()) < EXACT and int(dy.abs().max()) <= 128
    assert int((core.abs() + dres.abs()).sum(0).max()) + 1000 < EXACT and int((dy * x).abs().sum(0).max()) + 1000 < EXACT
    return x, dy, gamma, dres, core


def ln_bwd_int_check(dtype, rows, Cc, seed, offset=False):
    from temporalalignnet_amd import ops
    xi, dyi, gi, dri, core = ln_int_case(rows, Cc, seed)
    x, dy, dres, gamma = xi.to(dtype), dyi.to(dtype), dri.to(dtype), gi.float()
    assert torch.equal(x.long(), xi) and torch.equal(dy.long(), dyi) and torch.equal(dres.long(), dri)   # all exact in bf16
    if offset:
        x, dy, dres = (off_view(t)[1] for t in (x, dy, dres))
        assert x.data_ptr() % 16 == 8 and gamma.data_ptr() % 16 == 0
    mean, rstd = torch.zeros(rows, device=DEV), torch.ones(rows, device=DEV)
    init = [ri((Cc,), -50, 50, seed + 10 + k).float() for k in range(3)]
    want_sum = [(dyi * xi).sum(0), dyi.sum(0)]
    for none in (None, "dgamma", "dbeta", "dx_colsum", "dres"):
        case = f"rows={rows} C={Cc} {dtype} absent={none} offset={offset}"
        dg, db, cs = (None if none == n else t.clone() for n, t in zip(("dgamma", "dbeta", "dx_colsum"), init))
        exact = core + (0 if none == "dres" else dri)
        dxbuf, dx = off_view(torch.full((rows, Cc), float("nan"), device=DEV, dtype=dtype)) if offset else \
            (None, torch.full((rows, Cc), float("nan"), device=DEV, dtype=dtype))
        ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, dg, db, None if none == "dres" else dres, dx_colsum=cs)
        # the stored dx is the exact value rounded to the storage type (integers up to 976: beyond bf16's 8 bits)
        assert torch.equal(dx, exact.float().to(dtype)), case
        if dg is not None:
            assert torch.equal(dg, init[0] + want_sum[0].float()), case
        if db is not None:
            assert torch.equal(db, init[1] + want_sum[1].float()), case
        if cs is not None:                     # the column sums of the UNROUNDED f32 dx
            assert torch.equal(cs, init[2] + exact.sum(0).float()), case
        if offset:
            assert guard_intact(dxbuf, rows * Cc), case
    if dtype == BF16:                          # the case does tell rounded from unrounded column sums
        full = core + dri
        assert not torch.equal(full.float().to(BF16).long().sum(0), full.sum(0))


@pytest.mark.parametrize("rows", [1, 7, 1024, 1025, 2 * 1024 + 3, 4096, 4096 + 5, 5 * 1024 + 517])
def test_ln_bwd_integer_fast_path(rows):
    """ln_bwd_bf16x8_kernel<true, 4> (bf16, C = 512, aligned): 256 blocks, stride 1024 rows, four rows per iteration.  rows < 1024:
    q = 1..3 all clamped; 1024 < rows < 4096: some of q = 1..3 valid and the rest clamped (weight 0); rows > 4096: a second
    iteration.  dgamma / dbeta / dx_colsum start non-zero and are exact; dx is the exact value rounded to bf16, dx_colsum the sum
    of the UNROUNDED f32 values (what the kernel does: the sums are taken before the store); each optional argument absent alone
    leaves the others unchanged."""
    ln_bwd_int_check(BF16, rows, 512, 100 + rows)


# nblk = ceil(rows / 4): 1, 2, 7, 8, 9, 33, 104, 105, 129 (finalize: one to eight non-empty slices, slices past the end of the
# list, the unrolled fold from nblk = 104 on), then the 1024-block cap where ln_bwd_kernel grid-strides
GENERIC_ROWS = [3, 7, 26, 32, 33, 130, 416, 417, 514, 4096, 4096 + 5, 9000]


@pytest.mark.parametrize("dtype,Cc", [(F32, 256), (F32, 512), (F32, 1024), (BF16, 256), (BF16, 1024)])
def test_ln_bwd_integer_generic(dtype, Cc):
    """ln_bwd_kernel<T, NCH> + ln_bwd_finalize, exact (see test_ln_bwd_integer_fast_path for what is asserted)."""
    for rows in GENERIC_ROWS:
        ln_bwd_int_check(dtype, rows, Cc, 200 + rows + Cc)


@pytest.mark.parametrize("rows", [7, 130, 4096 + 5])
def test_ln_bwd_integer_misaligned(rows):
    """bf16, C = 512 with x, dy, dres, dx starting 8 bytes into their buffers (gamma 16-byte aligned): the generic
    ln_bwd_kernel<bf16, 2>, one step below the fast path's alignment; the bytes around the dx view stay untouched."""
    ln_bwd_int_check(BF16, rows, 512, 300 + rows, offset=True)


@pytest.mark.parametrize("dtype", DT)
def test_colsum_integer(dtype):
    """tan_colsum_acc into a non-zero out, |x| <= 8 and <= 300 rows (sums < 2^12): colsum_kernel's vector paths (tpr = C/8 rounded
    down to a divisor of 256, so the last column block is partly past C; tpr capped at 256 for C = 2056; the C % 512 == 0 layout)
    and colsum_generic_kernel (C % 8 != 0, or a base pointer that is only 8-byte aligned)."""
    from temporalalignnet_amd import ops
    for Cc in (8, 24, 40, 264, 512, 1536, 2056, 12, 36, 260):
        for rows in (1, 15, 16, 17, 63, 64, 65, 300):
            xi = ri((rows, Cc), -8, 8, 400 + Cc + rows)
            out0 = ri((Cc,), -50, 50, 401 + Cc).float()
            out = out0.clone()
            ops.colsum_acc(xi.to(dtype), out, rows, Cc)
            assert torch.equal(out, out0 + xi.sum(0).float()), (Cc, rows, dtype)
    if dtype == BF16:
        for rows in (1, 17, 64, 65, 300):
            xi = ri((rows, 512), -8, 8, 450 + rows)
            buf, xv = off_view(xi.to(BF16))
            assert xv.data_ptr() % 16 == 8
            out0 = ri((512,), -50, 50, 451).float()
            out = out0.clone()
            ops.colsum_acc(xv, out, rows, 512)
            assert torch.equal(out, out0 + xi.sum(0).float()), ("offset8", rows)


@pytest.mark.parametrize("dtype", DT)
def test_group_sum_integer(dtype):
    """out[r][c] = sum_g x[g R + r][c], |x| <= 2 and G <= 128: every sum is an integer <= 256, exact in bf16 too.  Every wave /
    unroll remainder of the g loop (G = 1, 3, 7, 16, 37, 128)."""
    from temporalalignnet_amd import ops
    for G, R, Cc in ((3, 5, 512), (1, 3, 12), (7, 5, 36), (16, 2, 512), (37, 9, 260), (128, 64, 512)):
        xi = ri((G * R, Cc), -2, 2, 500 + G)
        out = torch.full((R, Cc), float("nan"), device=DEV, dtype=dtype)
        ops.group_sum(xi.to(dtype), out, G, R, Cc)
        assert torch.equal(out, xi.view(G, R, Cc).sum(0).to(dtype)), (G, R, Cc)


def test_reduce_add_integer():
    """out += sum_p parts[p], |v| <= 8: the 4-wide part loop and its remainder; n = 2 * 2^20 + 8 is 2049 blocks of 1024 elements
    against the 2048-block cap (a grid-stride second pass for the last block's worth)."""
    from temporalalignnet_amd import ops
    for nparts, n in ((1, 1024), (3, 4096 + 8), (4, 640), (9, 70000), (16, 2048), (5, 2 * 2 ** 20 + 8)):
        parts = ri((nparts, n), -8, 8, 600 + nparts).float()
        o0 = ri((n,), -8, 8, 601 + nparts).float()
        o = o0.clone()
        ops.reduce_add(parts, o, nparts, n)
        assert torch.equal(o, o0 + parts.sum(0)), (nparts, n)


@pytest.mark.parametrize("dtype", DT)
def test_rows_copy_integer(dtype):
    """grouped row copy / accumulate, |v| <= 100 (sums <= 200, exact in bf16); rows of the destination outside the groups keep
    the random integers they started with.  G, R, C = 9, 1000, 512 is 4500 blocks against the 4096-block cap."""
    from temporalalignnet_amd import ops
    for G, R, Cc, sgs, soff, dgs, doff in ((3, 5, 512, 5, 0, 9, 0), (3, 4, 512, 4, 0, 9, 5), (3, 5, 512, 9, 0, 5, 0), (2, 3, 12, 7, 2, 5, 1),
                                           (9, 1000, 512, 1003, 2, 1005, 4)):
        for acc in (False, True):
            src = ri((G * sgs, Cc), -100, 100, 700 + R).to(dtype)
            dst0 = ri((G * dgs, Cc), -100, 100, 701 + R).to(dtype)
            dst = dst0.clone()
            ops.rows_copy(src, dst, G, R, Cc, sgs, soff, dgs, doff, accumulate=acc)
            want = dst0.clone().view(G, dgs, Cc)
            s = src.view(G, sgs, Cc)[:, soff:soff + R]
            want[:, doff:doff + R] = (want[:, doff:doff + R].float() + s.float()).to(dtype) if acc else s
            assert torch.equal(dst.view(G, dgs, Cc), want), (G, R, Cc, acc)


def _rows_gather(src, dst, map_, S, Msrc, Mdst, Cc):
    from temporalalignnet_amd import _lib, ops
    _lib.check(_lib.lib().tan_rows_gather(ops._ptr(src), ops._ptr(dst), ops._ptr(map_), S, Msrc, Mdst, Cc, ops._dt(src), ops._stream()),
               "tan_rows_gather")


@pytest.mark.parametrize("dtype", DT)
def test_rows_gather(dtype):
    """dst[s][m] = map[m] >= 0 ? src[s][map[m]] : 0 with every destination row written (dst starts as NaN): a map of all -1, one
    with repeats, one with -1 in the first and the last position, S > 1, and S, Mdst, C = 2, 2100, 512 with Msrc < Mdst (2100
    blocks against the 2048-block cap)."""
    cases = []
    for S, Msrc, Cc in ((1, 5, 12), (3, 5, 512)):
        cases += [(S, Msrc, Cc, [-1] * 9), (S, Msrc, Cc, [0, 2, 2, 4, 0, 1, 2, 2, 3]), (S, Msrc, Cc, [-1, 3, 0, 4, -1, 1, 1, 2, -1])]
    big = ri((2100,), -1, 1499, 800).tolist()
    big[0], big[-1], big[1] = -1, -1, 1499
    cases.append((2, 1500, 512, big))
    for S, Msrc, Cc, m in cases:
        Mdst = len(m)
        map_ = torch.tensor(m, dtype=torch.int32, device=DEV)
        src = ri((S, Msrc, Cc), -100, 100, 801 + Mdst).to(dtype)
        dst = torch.full((S, Mdst, Cc), float("nan"), device=DEV, dtype=dtype)
        _rows_gather(src, dst, map_, S, Msrc, Mdst, Cc)
        idx = map_.long()
        want = torch.where((idx >= 0)[None, :, None], src[:, idx.clamp(min=0)], torch.zeros((), device=DEV, dtype=dtype))
        assert torch.equal(dst, want), (S, Msrc, Mdst, Cc)


def _from_bits(b, dtype):
    """int64 bit patterns -> f32 / bf16 tensor"""
    if dtype == BF16:
        return (b - (b >= 0x8000) * 0x10000).to(torch.int16).view(BF16)
    return (b - (b >= 2 ** 31) * 2 ** 32).to(torch.int32).view(F32)


# put in front of every source of 1003 elements or more: +-inf, signalling and quiet NaNs (f32: one whose payload lies in the
# dropped half alone), denormals (f32: a tie that rounds up into the smallest normal, one that rounds to the smallest denormal,
# the smallest and the largest denormal), the largest finite value (f32: it rounds to inf)
CAST_SPECIAL = {F32: [0x7F800000, 0xFF800000, 0x7F810000, 0xFF812345, 0x7F800001, 0x7FC00000, 0x007F8000, 0x00018000, 0x00000001,
                      0x007FFFFF, 0x807F8000, 0x7F7FFFFF],
                BF16: [0x7F80, 0xFF80, 0x7F81, 0xFF81, 0x7FBF, 0x7FC1, 0x0001, 0x007F, 0x8001, 0x7F7F]}


def _cast_source(n, dtype, seed):
    """bit patterns: bf16 -> anything; f32 -> any exponent but 255, denormals included, whose low half is a tie (0x8000: exactly
    between two bf16 neighbours, with the kept bit even or odd), one below, one above, zero, or random; CAST_SPECIAL in front"""
    hi = ri((n,), 0, 0xFFFF, seed)
    if dtype == F32:
        hi = torch.where(((hi >> 7) & 0xFF) == 255, (hi & 0x807F) | (127 << 7), hi)       # inf / NaN only from CAST_SPECIAL
        lo = torch.stack([torch.full_like(hi, 0x8000), torch.full_like(hi, 0x7FFF), torch.full_like(hi, 0x8001), torch.zeros_like(hi),
                          ri((n,), 0, 0xFFFF, seed + 1)])
        hi = (hi << 16) | lo.gather(0, ri((1, n), 0, 4, seed + 2))[0]
    if n >= 1003:
        sp = torch.tensor(CAST_SPECIAL[dtype], device=DEV)
        hi[:sp.numel()] = sp
    return _from_bits(hi, dtype)


@pytest.mark.parametrize("src_dt", DT)
@pytest.mark.parametrize("dst_dt", DT)
def test_cast_bits(src_dt, dst_dt):
    """tan_cast in all four type pairs, bit-identical to torch's conversion (round to nearest even on f32 -> bf16, ties, denormals of
    both types and both infinities included); n = 1, 3, 4, 5, 1003 walk the scalar tail, n = 4 * 2^20 + 1027 is 4098 blocks of
    1024 against the 4096-block cap.  Pinned difference: every conversion INTO bf16 goes through
    v_cvt_pk_bf16_f32, which keeps the upper half of a NaN and sets its quiet bit (bf16 0x7F81 -> 0x7FC1, f32 0x7F800001 -> 0x7FC0)
    -- bf16 -> bf16 included, where torch copies the bits, and f32 -> bf16, where torch gives 0x7FC0 for every NaN; into f32
    nothing is converted and every bit is kept."""
    from temporalalignnet_amd import ops
    for n in (1, 3, 4, 5, 1003, 4 * 2 ** 20 + 1027):
        src = _cast_source(n, src_dt, 900 + n % 1000)
        if n >= 1003:
            assert int(torch.isnan(src).sum()) >= 4
            if src_dt == F32:
                assert int(((bits(src) & 0xFFFF) == 0x8000).sum()) > n // 10                 # the ties are there
                assert int(((bits(src) >> 23) & 0xFF == 0).sum()) > n // 1000               # and the denormals
        dst = torch.zeros(n, device=DEV, dtype=dst_dt)
        ops.cast(src, dst)
        nan, same = torch.isnan(src), bits(dst) == bits(src.to(dst_dt))
        bad = ~same & ~nan
        assert not bool(bad.any()), (n, src_dt, dst_dt, int(bad.sum()), bits(src)[bad][:8].tolist(), bits(dst)[bad][:8].tolist())
        if dst_dt == F32:
            assert bool(same.all()), (n, src_dt, dst_dt)
        else:                                  # the upper half of the NaN with the quiet bit set
            upper = (bits(src).long() >> (16 if src_dt == F32 else 0)) & 0xFFFF
            got = bits(dst).long() & 0xFFFF
            assert torch.equal(got[nan], upper[nan] | 0x0040), (n, src_dt, dst_dt, upper[nan][:8].tolist(), got[nan][:8].tolist())


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("Cc", [256, 512, 1024])
def test_head_bwd_integer(dtype, Cc):
    """dx (=|+=) dout w, dw += sum_r dout x, db += sum_r dout with |dout|, |x| <= 3, |w| <= 4, prior dx <= 50 (dx <= 62, sums
    <= 9 * 4100): exact.  rows = 4100 is 257 groups of 16 rows against the 256-block cap; rows < 4 leaves waves empty."""
    from temporalalignnet_amd import ops
    for rows in (1, 15, 16, 17, 37, 4100):
        for acc in (False, True):
            do, xi, w = ri((rows,), -3, 3, 1000 + rows), ri((rows, Cc), -3, 3, 1001 + rows), ri((Cc,), -4, 4, 1002)
            dx0 = ri((rows, Cc), -50, 50, 1003 + rows)
            dw0, db0 = ri((Cc,), -50, 50, 1004).float(), ri((1,), -50, 50, 1005).float()
            dx = dx0.to(dtype) if acc else torch.full((rows, Cc), float("nan"), device=DEV, dtype=dtype)
            dw, db = dw0.clone(), db0.clone()
            ops.head_bwd(do.float(), xi.to(dtype), w.float(), dx, dw, db, rows, Cc, accumulate_dx=acc)
            case = (rows, Cc, dtype, acc)
            assert torch.equal(dx, (do[:, None] * w[None] + (dx0 if acc else 0)).to(dtype)), case
            assert torch.equal(dw, dw0 + (do[:, None] * xi).sum(0).float()), case
            assert torch.equal(db, db0 + do.sum().float()), case


def test_interp_bwd_identity():
    """L_out == L_in: the weights are exactly 1 and 0, so dsrc gains exactly ddst (integers; the clamped last row included)."""
    from temporalalignnet_amd import ops
    for L, Cc in ((1, 4), (7, 4), (64, 512), (1024, 4)):
        dd = ri((L, Cc), -100, 100, 1100 + L).float()
        ds0 = ri((L, Cc), -100, 100, 1101 + L).float()
        ds = ds0.clone()
        ops.interp_linear_bwd(dd, ds, L, L, Cc)
        assert torch.equal(ds, ds0 + dd), (L, Cc)


def test_transpose_batch_uneven():
    """tan_transpose_batch with matrices of 1, 1, 8, 2 and 15 tiles under a 25-tile grid (blocks past a matrix's tile count exit
    early), an 8 x 8 matrix among them; the padding between the matrices keeps its NaN bits."""
    from temporalalignnet_amd import _lib, ops
    shapes = [(8, 8), (64, 64), (200, 72), (72, 40), (136, 264)]
    offs, total = [], 0
    for r, c in shapes:
        offs.append(total)
        total += (r * c + 15) // 16 * 16 + 16
    src = rn((total,), BF16, 1200)
    dst = torch.full_like(src, float("nan"))
    table = torch.tensor([[o, r, c] for o, (r, c) in zip(offs, shapes)], dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().tan_transpose_batch(ops._ptr(src), ops._ptr(dst), ops._ptr(table), len(shapes), 264, 264, _lib.TAN_BF16,
                                              ops._stream()), "tan_transpose_batch")
    written = torch.zeros(total, dtype=torch.bool, device=DEV)
    for o, (r, c) in zip(offs, shapes):
        assert torch.equal(dst[o:o + r * c].view(c, r), src[o:o + r * c].view(r, c).t()), (r, c)
        written[o:o + r * c] = True
    assert bool(torch.isnan(dst[~written]).all())


# ======================================================================================================================
# B. fp64 numerics tests
# ======================================================================================================================

def ln_stats(x64, eps):
    """fp64 mean / var / rstd of the rows and the bounds of the f32 statistics:
    mean   a D_ROW-deep sum of C terms times the exact 1/C, and the rounding of the result:  d_mean = D_ROW u mean|x| + u |mean|
    rstd   v = x - mean^ carries d_mean; sum v^2 = C var + C d^2 - 2 d sum v and sum v = 0, so the mean error enters squared;
           products and sum (3 + D_ROW) u, + eps and its f32 rounding 2u, the square root halves the relative error, rsqrtf is
           good to 2 ulp = 4u:  rho = ((D_ROW + 6) u + d_mean^2 / (var + eps)) / 2 + 4u"""
    mean, var = x64.mean(1), x64.var(1, unbiased=False)
    rstd = (var + eps).rsqrt()
    d_mean = D_ROW * U * x64.abs().mean(1) + U * mean.abs()
    rho = ((D_ROW + 6) * U + d_mean ** 2 / (var + eps)) / 2 + 4 * U
    return mean, var, rstd, d_mean, rho


def ln_input(rows, Cc, dtype, seed):
    """random rows; from 7 rows on: row 0 constant, row 1 = 1000 + noise (f32 only: bf16 has no bits left for the noise), row 2 scaled
    by 1e-3"""
    x = rn((rows, Cc), F32, seed, 2.0)
    if rows >= 7:
        x[0] = 0.75
        if dtype == F32:
            x[1] = 1000.0 + x[1]
        x[2] *= 1e-3
    return x.to(dtype)


@pytest.mark.parametrize("dtype,Cc,offset", LN_CONFIGS, ids=LN_IDS)
def test_ln_fwd_fp64(dtype, Cc, offset):
    """y, mean, rstd of tan_layernorm_fwd against fp64 F.layer_norm (+ the periodic addend), with mean / rstd given and absent
    (same y, bit for bit).  add_period 1, 3, 13 put the two rows of one RPW = 2 pair on both sides of the wrap; rows + 5 is longer
    than the input.  Special rows: constant (rstd = eps^-1/2, y = beta + add), a large common offset, a row scaled by 1e-3."""
    from temporalalignnet_amd import ops
    eps = 1e-5
    gamma, beta = 1 + rn((Cc,), F32, 2000, 0.1), rn((Cc,), F32, 2001, 0.1)
    g64, b64 = gamma.double(), beta.double()
    for rows in (1, 2, 7, 8, 9, 130):
        x = place(ln_input(rows, Cc, dtype, 2002 + rows), offset)
        x64 = x.double()
        mean, var, rstd, d_mean, rho = ln_stats(x64, eps)
        for period in (0, 1, 3, 13, rows + 5):
            case = f"rows={rows} period={period}"
            add = place(rn((period, Cc), dtype, 2100 + period), offset) if period else None
            a64 = add.double()[torch.arange(rows, device=DEV) % period] if period else torch.zeros_like(x64)
            ref = F.layer_norm(x64, (Cc,), g64, b64, eps) + a64
            ybuf, y = off_view(torch.full((rows, Cc), float("nan"), device=DEV, dtype=dtype)) if offset else \
                (None, torch.full((rows, Cc), float("nan"), device=DEV, dtype=dtype))
            m, r = torch.full((rows,), float("nan"), device=DEV), torch.full((rows,), float("nan"), device=DEV)
            ops.layernorm_fwd(x, gamma, beta, y, m, r, add, period, eps)
            ratio(f"ln_fwd/mean {TAG[dtype]}", case, m, mean, d_mean)
            ratio(f"ln_fwd/rstd {TAG[dtype]}", case, r, rstd, rstd * rho)
            # y = v rstd gamma + beta + add with v = x - mean^:  |rstd gamma| d_mean from the mean, t = v rstd gamma carries u (v),
            # rho (rstd) and two products' 2u; the two additions 2u (|t| + |beta| + |add|); then the store
            t = ((x64 - mean[:, None]) * rstd[:, None] * g64).abs()
            e = rstd[:, None] * g64.abs() * d_mean[:, None] + t * (rho[:, None] + 3 * U) + 2 * U * (t + b64.abs() + a64.abs())
            ratio(f"ln_fwd/y {TAG[dtype]}", case, y, ref, e + RND[dtype] * (ref.abs() + e))
            if rows >= 7:                      # the constant row: exactly what the reference model gives there
                assert m[0].item() == 0.75, case             # 0.75 k is exact for every k <= C: so is the mean
                ratio(f"ln_fwd/y {TAG[dtype]}", case + " const row", y[0], b64 + a64[0], e[0] + RND[dtype] * (ref[0].abs() + e[0]))
            y2 = torch.full_like(y, float("nan"))
            ops.layernorm_fwd(x, gamma, beta, y2, None, None, add, period, eps)
            assert torch.equal(y2, y), case
            if offset:
                assert guard_intact(ybuf, rows * Cc), case


def ln_bwd_chain(dtype, Cc, rows, offset):
    """the longest chain of f32 additions a dgamma / dbeta / dx_colsum entry goes through (the value it starts from included)"""
    if dtype == BF16 and Cc == 512 and not offset:     # rows of one wave, 3 for the four waves in LDS, one atomic per block
        nb = min(256, -(-rows // 4))
        return -(-rows // (4 * nb)) + 3 + nb
    nblk = min(1024, -(-rows // 4))                    # rows of one wave, 3 (LDS), a list lane's share of one slice of the partial
    per = -(-nblk // 8)                                # list and its 4 accumulators, the 4 list lanes, 8 slices' atomics
    return -(-rows // (4 * nblk)) + 3 + (-(-per // 4) + 2) + 2 + 8


@pytest.mark.parametrize("dtype,Cc,offset", LN_CONFIGS, ids=LN_IDS)
def test_ln_bwd_fp64(dtype, Cc, offset):
    """tan_layernorm_bwd fed the forward kernel's OWN mean / rstd, against fp64 autograd through F.layer_norm: dx (+ dres),
    dgamma, dbeta, dx_colsum (all three start non-zero).  The bounds carry the error of the f32 statistics (ln_stats)."""
    from temporalalignnet_amd import ops
    eps = 1e-5
    gamma, beta = 1 + rn((Cc,), F32, 3000, 0.1), rn((Cc,), F32, 3001, 0.1)
    for rows in (7, 130, 1500, 4101):
        case = f"rows={rows}"
        x, dy, dres = (place(t, offset) for t in (ln_input(rows, Cc, dtype, 3002 + rows), rn((rows, Cc), dtype, 3003 + rows),
                                                  rn((rows, Cc), dtype, 3004 + rows)))
        y, m, r = torch.empty_like(x), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
        ops.layernorm_fwd(x, gamma, beta, y, m, r, None, 0, eps)
        xr, gr, br = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        F.layer_norm(xr, (Cc,), gr, br, eps).backward(dy.double())
        init = [rn((Cc,), F32, 3010 + k) for k in range(3)]
        dg, db, cs = (t.clone() for t in init)
        dx = place(torch.full((rows, Cc), float("nan"), device=DEV, dtype=dtype), offset)
        ops.layernorm_bwd(dy, x, gamma, m, r, dx, dg, db, dres, dx_colsum=cs)
        x64, d64, g64, r64 = x.double(), dy.double(), gamma.double(), dres.double()
        dx_ref = xr.grad + r64
        mean, var, rstd, d_mean, rho = (t[:, None] for t in ln_stats(x64, eps))
        # xhat^ = (x - mean^) rstd^: the subtraction and the product 2u, rstd rho, the mean d_mean rstd
        xh = (x64 - mean) * rstd
        e_xh = xh.abs() * (rho + 2 * U) + d_mean * rstd
        # g = dy gamma (u);  m1 = sum g / C: products u + chain D_ROW;  m2 = sum g xhat / C: e_xh through |g|, products 2u + chain
        g = d64 * g64
        m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
        e_m1 = (D_ROW + 1) * U * g.abs().mean(1, keepdim=True)
        e_m2 = (g.abs() * e_xh).mean(1, keepdim=True) + (D_ROW + 2) * U * (g * xh).abs().mean(1, keepdim=True)
        # inner = g - m1 - xhat m2: the inputs' errors, the product u, two subtractions 2u of the magnitudes
        e_in = U * g.abs() + e_m1 + m2.abs() * e_xh + xh.abs() * e_m2 + U * (xh * m2).abs() + 2 * U * (g.abs() + m1.abs() + (xh * m2).abs())
        # dx = rstd^ inner + dres: rstd rho and the product u, the addition u; e32 is the f32 value's error, the store comes on top
        core = rstd * (g - m1 - xh * m2)
        e32 = rstd * e_in + core.abs() * (rho + U) + U * (core.abs() + r64.abs())
        ratio(f"ln_bwd/dx {TAG[dtype]}", case, dx, dx_ref, e32 + RND[dtype] * (dx_ref.abs() + e32))
        # the column sums: every term's own error, and `chain` additions over the magnitudes (and the starting value)
        ch = ln_bwd_chain(dtype, Cc, rows, offset)
        ratio(f"ln_bwd/dgamma {TAG[dtype]}", case, dg, init[0].double() + gr.grad,
              (d64.abs() * e_xh + U * (d64 * xh).abs()).sum(0) + ch * U * ((d64 * xh).abs().sum(0) + init[0].double().abs()))
        ratio(f"ln_bwd/dbeta {TAG[dtype]}", case, db, init[1].double() + br.grad, ch * U * (d64.abs().sum(0) + init[1].double().abs()))
        ratio(f"ln_bwd/dx_colsum {TAG[dtype]}", case, cs, init[2].double() + dx_ref.sum(0),      # of the UNROUNDED f32 dx: no store term
              e32.sum(0) + ch * U * (dx_ref.abs().sum(0) + init[2].double().abs()))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("Cc", [256, 512, 1024])
def test_l2norm_fp64(dtype, Cc):
    """tan_l2norm_fwd / _bwd on grouped layouts against fp64 x / x.norm() and its autograd: y, inv_norm (= 1 / ||x||), dx; the same y
    with inv_norm absent; destination rows outside the group untouched; an all-zero row gives NaN there and leaves the rest alone."""
    from temporalalignnet_amd import ops
    rnd = RND[dtype]
    # inv = 1 / sqrt(sum x^2): products u + chain D_ROW, halved by the root, sqrtf and the division correctly rounded (2u)
    rho = ((D_ROW + 1) / 2 + 2) * U
    for B, grp, L, off in ((1, 1, 3, 1), (1, 5, 9, 0), (3, 4, 9, 5), (3, 5, 9, 0)):
        rows = B * grp
        case = f"rows={rows} grp={grp} L={L} off={off}"
        x = rn((B * L, Cc), dtype, 4000 + rows)
        y = torch.full((rows, Cc), float("nan"), device=DEV, dtype=dtype)
        inv = torch.full((rows,), float("nan"), device=DEV)
        ops.l2norm_fwd(x, y, inv, rows, Cc, grp, L, off)
        xs = x.view(B, L, Cc)[:, off:off + grp].reshape(rows, Cc).double().requires_grad_(True)
        nrm = xs.norm(dim=-1, keepdim=True)
        ref = xs / nrm
        yr, ir = ref.detach(), (1 / nrm).detach()
        ratio(f"l2n_fwd/inv_norm {TAG[dtype]}", case, inv, ir[:, 0], ir[:, 0] * rho)
        e_y = yr.abs() * (rho + U)                                     # y = x inv: inv's rho and the product
        b_y = e_y + rnd * (yr.abs() + e_y)
        ratio(f"l2n_fwd/y {TAG[dtype]}", case, y, yr, b_y)
        y2 = torch.full_like(y, float("nan"))
        ops.l2norm_fwd(x, y2, None, rows, Cc, grp, L, off)
        assert torch.equal(y2, y), case
        dy = rn((rows, Cc), dtype, 4001 + rows)
        d64 = dy.double()
        ref.backward(d64)
        dx = torch.full((B * L, Cc), SENT, device=DEV, dtype=dtype)
        ops.l2norm_bwd(dy, y, inv, dx, rows, Cc, grp, L, off)
        # dx = (dy - y^ dot) inv^ with the STORED y^ (b_y off the exact one) and dot = sum dy y^: b_y through |dy|, products u + chain;
        # inner: b_y and e_dot through the product, its u, the subtraction u; then inv's rho, the product u, the store
        dot = (d64 * yr).sum(1, keepdim=True)
        e_dot = (d64.abs() * b_y).sum(1, keepdim=True) + (D_ROW + 1) * U * (d64 * yr).abs().sum(1, keepdim=True)
        e_in = dot.abs() * b_y + yr.abs() * e_dot + U * (yr * dot).abs() + U * (d64.abs() + (yr * dot).abs())
        e = ir * e_in + xs.grad.abs() * (rho + U)
        got = dx.view(B, L, Cc)[:, off:off + grp].reshape(rows, Cc)
        ratio(f"l2n_bwd/dx {TAG[dtype]}", case, got, xs.grad, e + rnd * (xs.grad.abs() + e))
        other = torch.ones(L, dtype=torch.bool, device=DEV)
        other[off:off + grp] = False
        assert bool((dx.view(B, L, Cc)[:, other] == SENT).all()), case
    # documented: no epsilon (tan_model.py:116), so an all-zero row is 0 * inf = NaN as x / ||x|| is in torch; other rows unaffected
    x = rn((5, Cc), dtype, 4100)
    y0, i0 = torch.empty_like(x), torch.empty(5, device=DEV)
    ops.l2norm_fwd(x, y0, i0, 5, Cc)
    x[2] = 0
    y, inv = torch.empty_like(x), torch.empty(5, device=DEV)
    ops.l2norm_fwd(x, y, inv, 5, Cc)
    assert bool(torch.isnan(x.double() / x.double().norm(dim=-1, keepdim=True))[2].all())
    assert bool(torch.isnan(y[2]).all()) and inv[2].item() == float("inf")
    keep = torch.tensor([0, 1, 3, 4], device=DEV)
    assert torch.equal(y[keep], y0[keep]) and torch.equal(inv[keep], i0[keep])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("Cc", [256, 512, 1024])
def test_head_fwd_fp64(dtype, Cc):
    """out[r] = <x[r], w> + b (f32 out) against fp64: the products u, a D_ROW chain and the bias addition over sum |x w| + |b|."""
    from temporalalignnet_amd import ops
    w, b = rn((Cc,), F32, 5000, 0.1), rn((1,), F32, 5001)
    for rows in (1, 3, 4, 5, 37):
        x = rn((rows, Cc), dtype, 5002 + rows)
        out = torch.full((rows,), float("nan"), device=DEV)
        ops.head_fwd(x, w, b, out, rows, Cc)
        ref = x.double() @ w.double() + b.double()
        ratio(f"head_fwd/out {TAG[dtype]}", f"rows={rows}", out, ref, (D_ROW + 2) * U * (x.double().abs() @ w.double().abs() + b.double().abs()))


@pytest.mark.parametrize("dtype", DT)
def test_quickgelu_fp64(dtype):
    """stand-alone tan_quickgelu against fp64 x sigmoid(1.702 x); 0, +-1e-3, +-10, +-88, +-1e4 among the inputs give finite results
    (exp overflows to inf on the negative side: x / inf = -0, never NaN).  n = 4 * 2^20 + 1027 passes the 4096-block cap.
    y = x / (1 + E), E = exp(a), a = -1.702 x.  The exponent is a product of x and one or two rounded constants (<= 3u |a| on E,
    exp itself 1 ulp = 2u); dy / y = -dE / (1 + E), so E's error enters times E / (1 + E) = sigmoid(a); then 1 + E, the division (the
    bf16 variant: v_rcp, 1 ulp, and a product) 4u, and the store.  Where E overflows or its reciprocal is flushed the f32 result
    is 0 and the true one is below |x| 2^-126: an absolute term."""
    from temporalalignnet_amd import _lib, ops
    special = torch.tensor([0.0, 1e-3, -1e-3, 10.0, -10.0, 88.0, -88.0, 1e4, -1e4], device=DEV)
    for n in (1, 3, 5, 1003, 4 * 2 ** 20 + 1027):
        x = rn((n,), F32, 6000 + n % 1000, 3.0)
        if n >= 1003:
            x[500:500 + special.numel()] = special
            x[-special.numel():] = special                      # in the scalar tail too
        x = x.to(dtype)
        y = torch.full_like(x, float("nan"))
        _lib.check(_lib.lib().tan_quickgelu(ops._ptr(x), ops._ptr(y), n, ops._dt(x), ops._stream()), "tan_quickgelu")
        assert bool(torch.isfinite(y).all()), n
        x64 = x.double()
        ref = x64 * torch.sigmoid(1.702 * x64)
        rel = torch.sigmoid(-1.702 * x64) * (3 * (1.702 * x64).abs() + 2) * U + 4 * U
        e = ref.abs() * rel + x64.abs() * 2.0 ** -126
        ratio(f"quickgelu/y {TAG[dtype]}", f"n={n}", y, ref, e + RND[dtype] * (ref.abs() + e))


@pytest.mark.parametrize("Cc", [4, 512])
def test_interp_fp64(Cc):
    """tan_interp_linear and its transpose-add against fp64 F.interpolate (linear, align_corners=False) and its autograd.
    The source position pos = (t + 1/2) L_in / L_out - 1/2 is computed in f32: the ratio, the product and the subtraction give
    |d pos| <= 3u (pos + 1), and that is the error of both weights (w1 = pos - i0 is exact).  Where rounding moves pos across an
    integer the pair of rows changes, with weights (1, 0) against (~0, ~1): still d pos times a neighbouring value."""
    from temporalalignnet_amd import ops
    for L_in, L_out in ((1, 1), (1, 7), (7, 1), (2, 3), (64, 100), (64, 40), (64, 64), (64, 1024), (1024, 64)):
        case = f"L_in={L_in} L_out={L_out}"
        src = rn((L_in, Cc), F32, 7000 + L_in + L_out)
        dst = torch.full((L_out, Cc), float("nan"), device=DEV)
        ops.interp_linear(src, dst, L_in, L_out, Cc)
        s64 = src.double().requires_grad_(True)
        up = lambda t: F.interpolate(t.t()[None], size=L_out, mode="linear", align_corners=False)[0].t()       # noqa: E731
        ref = up(s64)
        pos = (((torch.arange(L_out, device=DEV, dtype=F64) + 0.5) * L_in / L_out) - 0.5).clamp(min=0)
        dpos = 3 * U * (pos + 1)
        # forward: both weights off by d pos on values of at most max|src| per channel; 1 - w1, two products, one addition: 4u
        amax = src.double().abs().amax(0)
        ratio("interp/dst", case, dst, ref.detach(), dpos[:, None] * 2 * amax[None] + 4 * U * up(src.double().abs()))
        dd, ds0 = rn((L_out, Cc), F32, 7001 + L_in + L_out), rn((L_in, Cc), F32, 7002 + L_in + L_out)
        ds = ds0.clone()
        ops.interp_linear_bwd(dd, ds, L_in, L_out, Cc)
        ref.backward(dd.double())
        # backward: dsrc[i] collects, by atomics, the outputs t whose pos is within 2 rows of i (the two true rows, and the
        # neighbours a moved pos can reach): each brings d pos |ddst|; the chain is two atomics per such t and the starting value
        near = ((torch.arange(L_in, device=DEV, dtype=F64)[:, None] - pos[None]).abs() < 2).double()
        WT = F.interpolate(torch.eye(L_in, dtype=F64, device=DEV)[None], size=L_out, mode="linear", align_corners=False)[0]
        mag = WT @ dd.double().abs() + ds0.double().abs()
        ratio("interp_bwd/dsrc", case, ds, ds0.double() + s64.grad,
              near @ (dpos[:, None] * dd.double().abs()) + (2 * near.sum(1, keepdim=True) + 2) * U * mag)


def test_report_worst_ratios():
    for k in sorted(WORST):
        print(f"WORST {k}: {WORST[k]:.4f}")
