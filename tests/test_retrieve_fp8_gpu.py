"""The e4m3 corpus index on the GPU: tan_quantize_rows_e4m3, tan_rank_topk_e4m3, `build_index(dtype="e4m3")`, `VideoIndex.quantize`,
`search` over codes.  The row format is the one include/tan_hip.h fixes; `_host_quant` restates it on the host.

  * quantiser: codes and scales compared with `==` against the host expression, no exclusions.
  * sweep, exact arithmetic: integer rows (codes = 16 x, scale 2^-4, then the scales varied over 2^-6 .. 2^3).  Every accumulation
    is a multiple of 256 of at most 2^25 and every score a power of two times it: exact in f32 in any order, so counts, ties, rows,
    tie order and scores are compared with `==` against int64.  Query and index rows come from different ranges, and Q != N, so a
    swapped operand map cannot pass.
  * sweep, random unit rows: against the fp64 product of the DEQUANTISED operands, with the per-score bound
        eps(q, n) = 512 * 2^-23 * sum_i |a_i b_i|
    (512 accumulation steps, each no worse than an f32 truncation; the products of two e4m3 values and the power-of-two scale
    multiplies are exact).  Order statistics move by at most the largest eps of the query's row.
  * format error against the unquantised scores: derived, not measured --
        |score_e4m3 - s| <= (2^-3 + 2^-8) sum_i |v_i q_i| + 512 * 2^-10 * (v_scale max|q| + q_scale max|v|)
    (2^-4 relative rounding per normal element on both sides: (1 + 2^-4)^2 - 1; the subnormal floor: half of 2^-9 scale per
    element).  The observed figures are printed.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from temporalalignnet_amd import _lib, synth

pytestmark = pytest.mark.gpu

QS, NS, KS = (1, 33, 130), (1, 63, 65, 4097), (0, 1, 10, 32)
SHAPES = [(Q, N) for Q in QS for N in NS] + [(33, 200003)]
ACC_EPS = 512 * 2.0 ** -23


def _ops():
    from temporalalignnet_amd import ops
    return ops


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _host_quant(x):
    """The format of include/tan_hip.h on the host: (codes uint8 [n, 512], scale f32 [n], s int [n])."""
    x = x.detach().float().cpu()
    amax = x.abs().amax(dim=1)
    m, e = torch.frexp(amax)
    s = torch.where(m <= 0.875, e - 9, e - 8).clamp(-126, 127)
    s = torch.where(amax == 0, torch.zeros_like(s), s)
    one = torch.ones_like(amax)
    codes = (x * torch.ldexp(one, -s)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, torch.ldexp(one, s), s


_LUT = {}


def _deq(codes, scale):
    """fp64 values of e4m3 rows (device); the 256 code values come from the host's float8_e4m3fn."""
    if "v" not in _LUT:
        _LUT["v"] = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().cuda()
    return _LUT["v"][codes.long()] * scale.double()[:, None]


def _unit_rows(n, seed):
    x = torch.randn(n, 512, generator=_gen(seed), device="cuda")
    return x / x.norm(dim=-1, keepdim=True)


def _pairs(Q, N, seed):
    p = torch.randint(0, N, (Q,), generator=_gen(seed), device="cuda").int()
    p[0] = N - 1
    p[-1] = 0
    return p


def _cases(Q, N):
    for k, with_pair in itertools.product(KS, (True, False)):
        if k <= N and (k > 0 or with_pair):
            yield k, with_pair


# ------------------------------------------------------------------------------------------------------------------- quantiser
def _quantiser_pool():
    """257 f32 rows: the special rows first (so that n_rows = 1 and 5 hold them), then random rows over many binades."""
    g = torch.Generator().manual_seed(5)
    pool = torch.randn(257, 512, generator=g)
    pool *= torch.ldexp(torch.ones(257, 1), torch.randint(-60, 60, (257, 1), generator=g))          # rows over many binades
    pool *= torch.ldexp(torch.ones(257, 512), torch.randint(-14, 1, (257, 512), generator=g))       # elements down into subnormals
    val = torch.arange(128, dtype=torch.uint8).view(torch.float8_e4m3fn).float()[:127]              # the 127 finite codes >= 0
    mid = (val[:-1] + val[1:]) / 2                                                                  # 126 exact midpoints
    row = torch.zeros(512)
    row[:126], row[126:252], row[252], row[253] = mid, -mid, 448.0, -448.0                          # amax 448: scale 2^0
    pool[0] = row                                                                                   # ties to even, both signs
    pool[1] = 0.0                                                                                   # zero row: scale 1
    small = torch.randn(512, generator=g).abs() * 0.4
    pool[2] = small * 2.0 ** 37
    pool[2, 17] = -448.0 * 2.0 ** 37                                                                # amax exactly 448 * 2^j
    pool[3] = pool[2]
    pool[3, 17] = torch.nextafter(torch.tensor(448.0 * 2.0 ** 37), torch.tensor(float("inf")))      # ... and just above (f32)
    pool[4] = torch.ldexp(torch.rand(512, generator=g) + 0.5, torch.randint(-12, -5, (512,), generator=g))
    pool[4, 500] = 300.0                                                                            # small elements: e4m3 subnormals
    pool[5] = small * 2.0 ** -20
    pool[5, 3] = 450.0 * 2.0 ** -20                                                                 # just above, representable in bf16
    pool[6] = small * 2.0 ** -140                                                                   # subnormal amax: the clamp at -126
    pool[7] = row * 2.0 ** -9                                                                       # midpoints under a scale
    pool[8, 0] = 3.0e38                                                                             # the largest binade
    pool[9] = 0.0
    pool[9, 511] = 464.0                                                                            # 464 -> 448
    pool[10] = 0.0
    pool[10, :3] = torch.tensor([448.0, 2.0 ** -10, 17.0])                                          # 2^-10 -> 0, 17 -> 16
    return pool


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("f32", "bf16"))
def test_quantiser_bit_for_bit(dtype):
    ops = _ops()
    pool = _quantiser_pool().to(dtype)
    want_c, want_s, _ = _host_quant(pool)
    assert want_s[1].item() == 1.0 and want_c[9, 511].item() == 0x76 and want_s[9].item() == 2.0          # 464 / 2 = 232 -> 224
    assert want_c[10, :3].tolist() == [0x7E, 0x00, 0x58]
    for n in (1, 5, 257):
        codes, scale = ops.quantize_rows_e4m3(pool[:n].cuda().contiguous())
        again = ops.quantize_rows_e4m3(pool[:n].cuda().contiguous())
        assert codes.dtype == torch.uint8 and codes.shape == (n, 512) and scale.shape == (n,)
        assert torch.equal(scale.cpu(), want_s[:n]), (n, (scale.cpu() != want_s[:n]).nonzero().flatten().tolist())
        bad = (codes.cpu() != want_c[:n]).nonzero()
        assert bad.numel() == 0, (n, bad[:8].tolist())
        assert torch.equal(again[0], codes) and torch.equal(again[1], scale)


def test_quantiser_writes_its_outputs_and_nothing_else():
    ops = _ops()
    G = 64
    for n in (1, 5, 257):
        x = _unit_rows(n, 40 + n)
        codes = torch.full((n * 512 + G,), 0xA5, dtype=torch.uint8, device="cuda")
        scale = torch.full((n + G,), float("nan"), device="cuda")
        ops.quantize_rows_e4m3(x, codes[:n * 512].view(n, 512), scale[:n])
        want_c, want_s, _ = _host_quant(x)
        assert torch.equal(codes[:n * 512].view(n, 512).cpu(), want_c) and torch.equal(scale[:n].cpu(), want_s)
        assert (codes[n * 512:] == 0xA5).all() and torch.isnan(scale[n:]).all()


# ------------------------------------------------------------------------------------------------------- sweep, exact arithmetic
def _int_codes(x):
    """x: int64 in [-16, 16] (device) -> the e4m3 codes of 16 x, looked up in a table the host conversion made."""
    lut = (torch.arange(-16, 17).float() * 16).to(torch.float8_e4m3fn)
    assert torch.equal(lut.float(), torch.arange(-16, 17).float() * 16)                  # all representable
    return lut.view(torch.uint8).cuda()[x + 16].contiguous()


@pytest.mark.parametrize("Q,N", SHAPES)
def test_rank_topk_e4m3_exact_arithmetic(Q, N):
    ops = _ops()
    xq = torch.randint(-16, 17, (Q, 512), generator=_gen(100 + Q), device="cuda")
    xv = torch.randint(-16, 9, (N, 512), generator=_gen(200 + N % 1000), device="cuda")          # another range than the queries'
    xv[:, 0] = 16                                                                              # and both ends of the code range
    xv[N // 2] = xv[0]                                                                         # on top of the natural ties
    eq = torch.randint(-6, 4, (Q,), generator=_gen(7), device="cuda")                          # scales 2^-6 .. 2^3
    ev = torch.randint(-6, 4, (N,), generator=_gen(8), device="cuda")
    ev[N // 2] = ev[0]
    tq, vn = _int_codes(xq), _int_codes(xv)
    q_scale, v_scale = torch.ldexp(torch.ones(Q, device="cuda"), eq), torch.ldexp(torch.ones(N, device="cuda"), ev)
    acc = ((xq.double() * 16) @ (xv.double() * 16).T).round().long()                           # what the MFMA chain must hold
    assert int(acc.abs().max()) <= 2 ** 25
    S = acc * (2 ** (ev + 6))[None, :] * (2 ** (eq + 6))[:, None]                              # int64: 2^12 x the score
    order = torch.sort(S, dim=1, descending=True, stable=True).indices
    pair = _pairs(Q, N, 7)
    d = S.gather(1, pair.long()[:, None])
    for k, with_pair in _cases(Q, N):
        higher, ties, top_s, top_r = ops.rank_topk_e4m3(tq, q_scale, vn, v_scale, pair if with_pair else None, k, check_pair=True)
        if with_pair:
            assert torch.equal(higher.long(), (S > d).sum(1)) and torch.equal(ties.long(), (S == d).sum(1)), (k, with_pair)
            assert int(ties.min()) >= 1
        else:
            assert higher is None and ties is None
        if k:
            assert torch.equal(top_r.long(), order[:, :k]), (k, with_pair)
            assert torch.equal(top_s.double() * 4096, S.gather(1, order[:, :k]).double()), (k, with_pair)
        else:
            assert top_s is None and top_r is None


# ---------------------------------------------------------------------------------------------------- sweep, random unit rows
def _bounded_checks(S, E, pair, k, higher, ties, top_s, top_r):
    """S: fp64 scores [Q, N]; E: the bound on each computed score's error.  Returns the largest |returned score - fp64 score of
    the returned row| and the largest ratio of that error to its bound."""
    err = ratio = 0.0
    if pair is not None:
        d, ed = S.gather(1, pair.long()[:, None]), E.gather(1, pair.long()[:, None])
        assert ((S - E > d + ed).sum(1) <= higher.long()).all()
        assert (higher.long() + ties.long() <= (S + E >= d - ed).sum(1)).all()
        assert int(ties.min()) >= 1
    if k:
        emax = E.max(dim=1, keepdim=True).values
        best = torch.topk(S, k, dim=1).values
        assert ((top_s.double() - best).abs() <= emax).all()
        got = S.gather(1, top_r.long())
        assert (got >= best[:, -1:] - 2 * emax).all()
        assert all(len(set(r)) == k for r in top_r.tolist())
        e = (top_s.double() - got).abs()
        err, ratio = float(e.max()), float((e / E.gather(1, top_r.long())).max())
    return err, ratio


_UNIT = {}


def _unit_case(Q, N):
    """Shared by the accumulation test and the format-error test, computed once and left unchanged: unit rows, their codes and
    scales from the kernel, the fp64 scores of the dequantised rows and of the original rows, and sum |a_i b_i| of each."""
    if (Q, N) not in _UNIT:
        ops = _ops()
        fq, fv = _unit_rows(Q, 300 + Q), _unit_rows(N, 400 + N % 1000)
        (tq, q_scale), (vn, v_scale) = ops.quantize_rows_e4m3(fq), ops.quantize_rows_e4m3(fv)
        a, b = _deq(tq, q_scale), _deq(vn, v_scale)
        _UNIT[(Q, N)] = dict(fq=fq, fv=fv, tq=tq, q_scale=q_scale, vn=vn, v_scale=v_scale, S=a @ b.T, A=a.abs() @ b.abs().T,
                             S0=fq.double() @ fv.double().T, A0=fq.double().abs() @ fv.double().abs().T)
    return _UNIT[(Q, N)]


@pytest.mark.parametrize("Q,N", SHAPES)
def test_rank_topk_e4m3_random_unit_rows(Q, N):
    ops = _ops()
    c = _unit_case(Q, N)
    want_c, want_s, _ = _host_quant(c["fq"])
    assert torch.equal(c["tq"].cpu(), want_c) and torch.equal(c["q_scale"].cpu(), want_s)
    E = ACC_EPS * c["A"]
    pair = _pairs(Q, N, 9)
    worst = ratio = 0.0
    for k, with_pair in _cases(Q, N):
        p = pair if with_pair else None
        out = ops.rank_topk_e4m3(c["tq"], c["q_scale"], c["vn"], c["v_scale"], p, k)
        e, r = _bounded_checks(c["S"], E, p, k, *out)
        worst, ratio = max(worst, e), max(ratio, r)
    print(f"rank_topk_e4m3 max |score - fp64 of the dequantised rows| Q={Q} N={N}: {worst:.3e} = {ratio:.3f} of 512 * 2^-23 * sum|ab|")
    assert ratio <= 1.0


@pytest.mark.parametrize("Q,N", SHAPES)
def test_format_error_against_the_unquantised_scores(Q, N):
    ops = _ops()
    c = _unit_case(Q, N)
    k = min(32, N)
    pair = _pairs(Q, N, 9)
    _, _, top_s, top_r = ops.rank_topk_e4m3(c["tq"], c["q_scale"], c["vn"], c["v_scale"], pair, k)
    rows = top_r.long()
    floor = 512 * 2.0 ** -10 * (c["v_scale"].double()[None, :] * c["fq"].double().abs().amax(1)[:, None]
                                + c["q_scale"].double()[:, None] * c["fv"].double().abs().amax(1)[None, :])
    bound = ((2.0 ** -3 + 2.0 ** -8) * c["A0"] + floor).gather(1, rows)
    err = (top_s.double() - c["S0"].gather(1, rows)).abs()
    print(f"e4m3 format error Q={Q} N={N} over the top {k}: rms {float(err.pow(2).mean().sqrt()):.3e} max {float(err.max()):.3e} "
          f"(max {float((err / bound).max()):.4f} of the bound; scores up to {float(c['S0'].gather(1, rows).abs().max()):.3f})")
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ ties, splits, determinism
def test_constructed_ties_across_tiles_and_splits():
    ops = _ops()
    Q, N = 7, 200003
    (tq, q_scale), (vn, v_scale) = ops.quantize_rows_e4m3(_unit_rows(Q, 1)), ops.quantize_rows_e4m3(_unit_rows(N, 2))
    a, b, c = 5, 64 * 700 + 33, N - 4                  # different rows of a tile, different tiles, different splits
    for r in (a, b, c):                                # query 0's best match by far (cosine about 1)
        vn[r], v_scale[r] = tq[0], q_scale[0]
    for paired in (a, b, c):
        pair = torch.full((Q,), paired, dtype=torch.int32, device="cuda")
        for splits in (1, 3, 0):
            higher, ties, top_s, top_r = ops.rank_topk_e4m3(tq, q_scale, vn, v_scale, pair, 10, splits=splits)
            assert ties.tolist() == [3] * Q, (paired, splits, ties.tolist())
            assert higher[0].item() == 0
            assert top_r[0, :3].tolist() == [a, b, c]
            assert top_s[0, 0].item() == top_s[0, 1].item() == top_s[0, 2].item()
            for q in range(1, Q):                      # wherever the three land in another query's list they are adjacent, ascending
                rows = top_r[q].tolist()
                hit = [i for i, r in enumerate(rows) if r in (a, b, c)]
                if len(hit) == 3:
                    assert hit[2] - hit[0] == 2 and [rows[i] for i in hit] == [a, b, c]


def test_rank_topk_e4m3_is_deterministic_and_split_invariant():
    ops = _ops()
    for Q, N, k in ((130, 4097, 32), (33, 200003, 10), (7, 63, 10)):
        (tq, q_scale), (vn, v_scale) = ops.quantize_rows_e4m3(_unit_rows(Q, 21)), ops.quantize_rows_e4m3(_unit_rows(N, 22))
        vn[N // 3], v_scale[N // 3] = vn[N // 7], v_scale[N // 7]
        pair = _pairs(Q, N, 5)
        ref = ops.rank_topk_e4m3(tq, q_scale, vn, v_scale, pair, k)
        for splits in (1, 3, 0, 0):                    # the second automatic run: run to run
            got = ops.rank_topk_e4m3(tq, q_scale, vn, v_scale, pair, k, splits=splits)
            for x, y in zip(ref, got):
                assert torch.equal(x, y), (Q, N, k, splits)


def test_rank_topk_e4m3_writes_every_output_and_nothing_else():
    ops = _ops()
    G = 64                                             # guard elements after every buffer
    for Q, N, k in ((7, 63, 10), (130, 4097, 32), (1, 1, 1), (33, 200003, 0)):
        (tq, q_scale), (vn, v_scale) = ops.quantize_rows_e4m3(_unit_rows(Q, 31)), ops.quantize_rows_e4m3(_unit_rows(N, 32))
        pair = _pairs(Q, N, 3)
        higher = torch.full((Q + G,), -777, dtype=torch.int32, device="cuda")
        ties = torch.full((Q + G,), -777, dtype=torch.int32, device="cuda")
        top_s = torch.full((Q * k + G,), float("nan"), device="cuda")
        top_r = torch.full((Q * k + G,), -777, dtype=torch.int32, device="cuda")
        nws = ops.rank_topk_ws_bytes(Q, N, k)
        ws = torch.full((nws + G,), 0xFF, dtype=torch.uint8, device="cuda")      # NaN / -1 patterns in the scratch
        out = (higher[:Q], ties[:Q], top_s[:Q * k].view(Q, k) if k else None, top_r[:Q * k].view(Q, k) if k else None)
        ops.rank_topk_e4m3(tq, q_scale, vn, v_scale, pair, k, out=out, ws=ws[:nws])
        assert (higher[:Q] >= 0).all() and (ties[:Q] >= 1).all()
        assert (higher[Q:] == -777).all() and (ties[Q:] == -777).all() and (ws[nws:] == 0xFF).all()
        assert (top_r[Q * k:] == -777).all() and torch.isnan(top_s[Q * k:]).all()
        if k:
            assert torch.isfinite(top_s[:Q * k]).all() and ((top_r[:Q * k] >= 0) & (top_r[:Q * k] < N)).all()
            a, b = _deq(tq, q_scale), _deq(vn, v_scale)
            _bounded_checks(a @ b.T, ACC_EPS * (a.abs() @ b.abs().T), pair, k, *out)


def test_e4m3_entry_points_reject_invalid_arguments():
    ops = _ops()
    L = _lib.lib()
    x = _unit_rows(40, 2)
    (tq, qs), (vn, vs) = ops.quantize_rows_e4m3(_unit_rows(4, 1)), ops.quantize_rows_e4m3(x)
    pair = torch.zeros(4, dtype=torch.int32, device="cuda")
    hi, ti = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    ts, tr = torch.zeros(4, 40, device="cuda"), torch.zeros(4, 40, dtype=torch.int32, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    f = lambda t: None if t is None else C.c_void_p(t.data_ptr())                     # noqa: E731

    def call(Q=4, N=40, Cc=512, pr=pair, k=10, splits=0, h=hi, t=ti, s=ts, r=tr, w=ws, a=tq, b=vn, sa=qs, sb=vs):
        return L.tan_rank_topk_e4m3(f(a), f(sa), f(b), f(sb), Q, N, Cc, f(pr), k, splits, f(h), f(t), f(s), f(r), f(w), None)

    assert call() == 0
    torch.cuda.synchronize()
    for kw in (dict(Cc=256), dict(Cc=1024), dict(k=33), dict(k=41, N=40), dict(k=-1), dict(Q=0), dict(N=0), dict(N=1 << 31),
               dict(k=0, pr=None), dict(splits=-1), dict(h=None), dict(s=None), dict(r=None), dict(w=None), dict(a=None), dict(b=None),
               dict(sa=None), dict(sb=None)):
        assert call(**kw) == -1, kw
    codes, scale = torch.zeros(40, 512, dtype=torch.uint8, device="cuda"), torch.zeros(40, device="cuda")

    def quant(src=x, dtype=0, n=40, Cc=512, c=codes, s=scale):
        return L.tan_quantize_rows_e4m3(f(src), dtype, n, Cc, f(c), f(s), None)

    assert quant() == 0
    torch.cuda.synchronize()
    for kw in (dict(Cc=256), dict(Cc=1024), dict(n=0), dict(n=-1), dict(n=1 << 31), dict(dtype=2), dict(src=None), dict(c=None), dict(s=None)):
        assert quant(**kw) == -1, kw
    with pytest.raises(_lib.TanHipError):
        ops.rank_topk_e4m3(tq, qs, vn, vs, None, 0)
    with pytest.raises(ValueError):
        ops.rank_topk_e4m3(tq, qs, vn, vs, torch.full((4,), 40, dtype=torch.int32, device="cuda"), 1, check_pair=True)
    with pytest.raises(_lib.TanHipError):
        ops.rank_topk_e4m3(tq.cpu(), qs.cpu(), vn.cpu(), vs.cpu(), None, 1)
    with pytest.raises(_lib.TanHipError):
        ops.quantize_rows_e4m3(x.cpu())


# ---------------------------------------------------------------------------------------------------------------- index and search
def _model(E=2, D=1, seed=113):
    from temporalalignnet_amd.tan_model import TemporalAligner
    m = TemporalAligner(num_encoder_layers=E, num_decoder_layers=D, use_alignability_head=0, language_model=None, random_pos_start=0,
                        compute_dtype="fp32")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_params(seed, E, D, False).items()})
    return m.cuda().eval()


def _embed(strs):
    return torch.stack([torch.from_numpy(synth.yc2_text_embedding(s)) for s in strs])


def _videos(vlens, seed=9):
    rng = np.random.default_rng(seed)
    return [{"vid": f"v{i:03d}", "video": np.abs(rng.standard_normal((int(v), 1024)) * 0.4 + rng.standard_normal((1, 1024)) * 0.5)
             .astype(np.float32)} for i, v in enumerate(vlens)]


def test_e4m3_index_and_search(tmp_path):
    from temporalalignnet_amd import search as srch
    m = _model()
    vlens = [70, 33, 150, 64, 20, 90]                  # windows straddle the video boundaries; 8 windows per chunk below
    vids = _videos(vlens)
    f32 = srch.build_index(m, vids, dtype=torch.float32)
    idx = srch.build_index(m, vids, windows_per_pass=2, dtype="e4m3")
    chunks = [len(ch.items) for ch in srch._index_chunks(vids, 64, 2)]
    assert len(chunks) >= 2                            # the codes and scales of several chunks, concatenated
    want_c, want_s, _ = _host_quant(f32.feat)
    assert idx.e4m3 and idx.feat.dtype == torch.uint8 and idx.scale.dtype == torch.float32 and len(idx) == sum(vlens)
    assert torch.equal(idx.feat.cpu(), want_c) and torch.equal(idx.scale.cpu(), want_s)
    assert torch.equal(_deq(idx.feat, idx.scale), _deq(want_c.cuda(), want_s.cuda()))
    assert idx.v_off.tolist() == f32.v_off.tolist() and idx.vids == f32.vids
    for other in (srch.build_index(m, vids, dtype=torch.float8_e4m3fn), f32.quantize()):
        assert torch.equal(other.feat, idx.feat) and torch.equal(other.scale, idx.scale)
    assert idx.quantize() is idx and f32.scale is None and not f32.e4m3

    queries = [f"query {i}" for i in range(9)]
    tq, q_scale = srch.query_features(idx, m, _embed, queries)
    fq = srch.query_features(f32, m, _embed, queries)
    hq_c, hq_s, _ = _host_quant(fq)
    assert torch.equal(tq.cpu(), hq_c) and torch.equal(q_scale.cpu(), hq_s)
    # every unplanted row's e4m3 score stays below its unquantised score plus the format bound; the planted rows score the
    # query's own dequantised square, less the accumulation bound
    S0, A0 = fq.double() @ f32.feat.double().T, fq.double().abs() @ f32.feat.double().abs().T
    others = (S0 + (2.0 ** -3 + 2.0 ** -8) * A0 + 512 * 2.0 ** -10 * (idx.scale.double()[None, :] * fq.double().abs().amax(1)[:, None]
              + q_scale.double()[:, None] * f32.feat.double().abs().amax(1)[None, :])).amax(1)
    dq = _deq(tq, q_scale)
    own = dq.pow(2).sum(1) * (1 - ACC_EPS)
    cross = fq.double() @ fq.double().T
    qa, qb = divmod(int(cross.argmin()), 9)            # the two least similar queries get planted rows
    assert (own[[qa, qb]] > others[[qa, qb]]).all(), (own.tolist(), others.tolist())
    assert min(own[qa], own[qb]) > (dq[qa] * dq[qb]).sum().abs() + ACC_EPS * (dq[qa] * dq[qb]).abs().sum()
    off = idx.v_off
    first_of_chunk_2 = int(off[chunks[0]])
    # query qa: the last second of video 1, the first second of video 2 (adjacent rows of different videos), the first row of the
    # second chunk; query qb: row 0 and the last row of the index
    planted = {qa: sorted({int(off[2]) - 1, int(off[2]), first_of_chunk_2}), qb: [0, int(off[-1]) - 1]}
    for q, rows in planted.items():
        for r in rows:
            idx.feat[r], idx.scale[r] = tq[q], q_scale[q]
    res = srch.search(idx, m, _embed, queries, k=10)
    assert len(res) == 9 and all(len(h) == 10 for h in res)
    for q, rows in planted.items():
        v, sec = idx.locate(np.array(rows))
        got = res[q][:len(rows)]
        assert [(vid, s) for vid, s, _ in got] == [(idx.vids[a], int(b)) for a, b in zip(v, sec)], (q, got)
        assert len({score for _, _, score in got}) == 1 and got[0][2] > res[q][len(rows)][2]
    assert res[qa][0][:2] == ("v001", 32) and res[qa][1][:2] == ("v002", 0) and res[qb][0][:2] == ("v000", 0)
    for q, hits in enumerate(res):                     # descending scores; every hit inside its video
        assert all(hits[i][2] >= hits[i + 1][2] for i in range(9))
        assert all(0 <= sec < vlens[idx.vids.index(vid)] for vid, sec, _ in hits)
    p = str(tmp_path / "index.npz")
    idx.save(p)
    back = srch.VideoIndex.load(p)
    assert back.e4m3 and torch.equal(back.feat, idx.feat) and torch.equal(back.scale, idx.scale) and back.vids == idx.vids
    assert srch.search(back, m, _embed, queries, k=10) == res


# -------------------------------------------------------------------------------------------------------------------------- memory
def test_rank_topk_e4m3_memory_stays_far_below_the_score_matrix():
    ops = _ops()
    Q, N, k = 2048, 2_000_000, 10
    vn = torch.empty(N, 512, dtype=torch.uint8, device="cuda")
    v_scale = torch.empty(N, device="cuda")
    for a in range(0, N, 250_000):                     # random rows, made and quantised in slices to keep the temporaries small
        ops.quantize_rows_e4m3(torch.randn(250_000, 512, generator=_gen(a), device="cuda").mul_(512 ** -0.5), vn[a:a + 250_000],
                               v_scale[a:a + 250_000])
    tq, q_scale = ops.quantize_rows_e4m3(_unit_rows(Q, 77))
    pair = _pairs(Q, N, 1)
    ws_bytes = ops.rank_topk_ws_bytes(Q, N, k)
    out_bytes = Q * 4 * 2 + Q * k * 8
    # caller-owned scratch and outputs of exactly the documented sizes: the call itself must not allocate a byte
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = (torch.empty(Q, dtype=torch.int32, device="cuda"), torch.empty(Q, dtype=torch.int32, device="cuda"),
           torch.empty(Q, k, device="cuda"), torch.empty(Q, k, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ops.rank_topk_e4m3(tq, q_scale, vn, v_scale, pair, k, out=out, ws=ws)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == base
    first = [t.clone() for t in out]
    del ws, out
    # the wrapper's own allocations: scratch + outputs, each rounded up by the caching allocator (512 bytes for a small block; a
    # large block is not split when less than 1 MiB of it would remain)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    higher, ties, top_s, top_r = ops.rank_topk_e4m3(tq, q_scale, vn, v_scale, pair, k)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra <= ws_bytes + out_bytes + 4 * 512 + 2 ** 20, (extra, ws_bytes, out_bytes)
    assert all(torch.equal(x, y) for x, y in zip(first, (higher, ties, top_s, top_r)))
    assert ws_bytes + out_bytes < 64 * 2 ** 20 < Q * N * 4 // 100
    assert int(ties.min()) >= 1 and torch.isfinite(top_s).all()
    # spot check a few queries against fp64 of the dequantised rows (a [8, N] slice, not the matrix)
    a = _deq(tq[:8], q_scale[:8])
    S, A = [], []
    for r in range(0, N, 250_000):
        b = _deq(vn[r:r + 250_000], v_scale[r:r + 250_000])
        S.append(a @ b.T)
        A.append(a.abs() @ b.abs().T)
    _bounded_checks(torch.cat(S, 1), ACC_EPS * torch.cat(A, 1), pair[:8], k, higher[:8], ties[:8], top_s[:8], top_r[:8])
