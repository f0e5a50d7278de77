"""The sentence embedder (csrc/tan_w2v.hip, temporalalignnet_amd/word2vec_model.py) against tests/w2v_cases.py.

Part 1 calls tan_embed_gather, tan_unpad_add, tan_wordpool_fwd and tan_wordpool_bwd through the C ABI.  They select and copy, so every
output is compared bit for bit with the expectation (the bias gradient, an f32 sum, against its float64 value).  Outputs start as NaN
(int32: a sentinel), accumulated outputs as noise, and a guard region behind every output must come back untouched.  Which branch each
case reaches:

  tan_embed_gather   (D, Dpad) = (300, 320): whole float4 chunks + whole pad chunks; (5, 8) and (302, 304): the partial tail (1 and 2
                     live columns); (4, 4): no pad.  ids 0, V - 1 and -1, V, V + 7 (row 0); ids NULL (identity); rows = 1;
                     rows = 16384 at (300, 320): 5120 workgroups' worth of chunks on the capped grid of 4096 (the grid-stride loop)
  tan_unpad_add      (3, 5, 8); (2048, 300, 320): 2400 workgroups' worth on the capped grid of 2048; NaN in the pad columns of src
  tan_wordpool_fwd   M in {1, 3, 65} x W in {1, 9, 32} at H = 2048, and H = 4 with M = 1 (one thread works); mask NULL / sentences with
                     a hole, a masked first word, every word masked; ties between unmasked words and between masked and unmasked
  tan_wordpool_bwd   M in {1, 64, 65, 130}: the 64-row chunks of the bias kernel (1, 1, 2 and 3 chunks, the last of 1 and 2 rows);
                     (M, W) = (130, 32): 8320 workgroups' worth on the capped grid of 8192; pooled == 0 and < 0; db NULL
  every TAN_REQUIRE  returns -1 and writes nothing

Part 2 runs Word2VecModel forward and backward in fp32 and bf16 against float64 autograd of w2v_cases.forward on the operands the
kernels read, every element of both outputs and of the four gradients, norm-relative per tensor.  Shapes (M sentences, W words) and the
branch of _SentenceFn.backward each reaches (R = M W rows; split-K of the two weight-gradient GEMMs = min(8, M // 256), min(32, R // 512)):

  (1, 32)     one sentence -- a single search query; K = 1 in fc2's weight-gradient GEMM
  (9, 32)     synth.w2v_tokens: its all-stop-word sentence and mid-sentence unknown word
  (65, 7)     nothing a multiple of anything; R = 455 < 512: both split-K 1
  (512, 4)    split-K 2 and 4
  (2048, 8)   the split-K caps 8 and 32; tan_unpad_add and tan_embed_gather past their grid caps

each with an attention mask, without one (the trailing id-0 words are then unmasked duplicates: exact ties), with ids outside [0, V),
and with pooler_output unused (the backward receives None).

Parameters.  Every shape runs with w2v_cases.exact_params: synth.w2v_params with the table, fc1.weight and fc1.bias snapped to grids on
which h = relu(x fc1.weight^T + fc1.bias) is exact in f32 in any order of accumulation.  The pooling's choice of a word then never hangs on
a rounding error -- with the random parameters at (2048, 8) in fp32 the kernel picks another word than float64 in 2 of 4 194 304
selections (float64 gaps 4.5e-8 and 4.7e-8, below what an f32 dot product of 300 terms resolves), which moves fc1.weight's gradient
3.9e-4 from the reference though it is 4.4e-7 from float64 with the kernel's own selection -- and exact ties between DIFFERENT words are
common, so the first-index rule decides where gradients go.  (9, 32) also runs with the random parameters as they are."""
import pytest
import torch

import w2v_cases as wc
from temporalalignnet_amd import _lib, ops, synth

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
V = 500
GUARD = 256

# Norm-relative bounds, ||got - ref|| / ||ref|| per tensor: twice the worst measured on MI355X over every case of this file, against
# the float64 reference.  Caps the measurement may not exceed: 1e-5 in fp32, 0.016 in bf16.
#   db increment of tan_wordpool_bwd (f32 atomics over 64-row partial sums, onto noise): worst 1.04e-7 (M=130 W=32 and M=64 W=3, f32)
DB_REL = 2.1e-7
#   the model in fp32 -- forward (pooler_output, last_hidden_state): worst 8.67e-7 (synth (9, 32) mask, pooler_output)
F32_FWD_REL = 1.8e-6
#   the model in fp32 -- the four gradients: worst 4.50e-7 (exact (512, 4) nomask, fc1.weight)
F32_GRAD_REL = 9e-7
#   the model in bf16 -- forward: worst 1.71e-3 (exact (1, 32) oob, last_hidden_state) -- the bf16 rounding of h and of the output
BF16_FWD_REL = 3.5e-3
#   the model in bf16 -- gradients: worst 2.45e-3 (exact (512, 4) nomask, fc1.bias; synth (9, 32): 2.45e-3 too) -- bf16 g, d_pooled, dh
BF16_GRAD_REL = 4.9e-3


def _p(t):
    return None if t is None else t.data_ptr()


def _dt(dtype):
    return _lib.TAN_F32 if dtype == F32 else _lib.TAN_BF16


def bits(t):
    """the bit pattern (NaN == NaN): bitwise comparisons"""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


SENTINEL = -77


def _fill(dtype):
    return SENTINEL if dtype == torch.int32 else float("nan")


class Guarded:
    """an output buffer of `shape` that starts as NaN (int32: a sentinel; `init`: given values) with GUARD elements behind it"""

    def __init__(self, shape, dtype, init=None):
        n = 1
        for s in shape:
            n *= s
        self.n, self.dtype = n, dtype
        self.full = torch.full((n + GUARD,), _fill(dtype), dtype=dtype, device="cuda")
        self.t = self.full[:n].view(shape)
        if init is not None:
            self.t.copy_(init)
        self.before = self.full.clone()

    def ptr(self):
        return self.full.data_ptr()

    def guard_ok(self):
        return torch.equal(bits(self.full[self.n:]), bits(self.before[self.n:]))

    def untouched(self):
        return torch.equal(bits(self.full), bits(self.before))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def rn(seed, *shape):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, generator=g, device="cuda")


# ---------------------------------------------------------------------------------------------------------------- part 1: gather
def run_gather(ids, table, rows, D, Dpad, dtype):
    out = Guarded((rows, Dpad), dtype)
    rc = _lib.lib().tan_embed_gather(_p(ids), _p(table), out.ptr(), rows, D, Dpad, table.shape[0], _dt(dtype), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert out.guard_ok(), "tan_embed_gather wrote behind its output"
    return out.t


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("D,Dpad", [(300, 320), (5, 8), (302, 304), (4, 4)])
def test_gather_is_exact(D, Dpad, dtype):
    Vt = 23
    table = rn(D, Vt, D)
    ids = torch.tensor([0, Vt - 1, -1, Vt, Vt + 7, 3, 22, 1, 0, 2 ** 40, -2 ** 40, 11, 5], device="cuda")
    got = run_gather(ids, table, ids.numel(), D, Dpad, dtype)
    assert same(got, wc.gather_expected(table, ids, ids.numel(), D, Dpad, dtype))
    assert same(got[2], got[0]) and same(got[3], got[0]) and same(got[4], got[0])          # -1, V, V + 7 read row 0
    # ids NULL: the identity (how fc1.weight is padded), every row of the table
    assert same(run_gather(None, table, Vt, D, Dpad, dtype), wc.gather_expected(table, None, Vt, D, Dpad, dtype))
    # one row
    one = ids[1:2].clone()
    assert same(run_gather(one, table, 1, D, Dpad, dtype), wc.gather_expected(table, one, 1, D, Dpad, dtype))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gather_past_the_grid_cap(dtype):
    rows, D, Dpad = 16384, 300, 320
    assert rows * (Dpad // 4) // 256 > 4096
    table = rn(1, V, D)
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(-3, V + 3, (rows,), generator=g).cuda()
    ids[-1] = V - 1                                   # (the last row is a grid-stride row: rows beyond 4096 * 256 / 80 = 13107)
    assert same(run_gather(ids, table, rows, D, Dpad, dtype), wc.gather_expected(table, ids, rows, D, Dpad, dtype))


# ---------------------------------------------------------------------------------------------------------------- part 1: unpad_add
@pytest.mark.parametrize("rows,D,Dpad", [(3, 5, 8), (2048, 300, 320)])
def test_unpad_add_increment_is_exact(rows, D, Dpad):
    assert (rows, D) == (3, 5) or rows * D // 256 > 2048
    src = rn(3, rows, Dpad)
    src[:, D:] = float("nan")                         # the pad columns must not reach dst
    noise = rn(4, rows, D) * 0.5
    dst = Guarded((rows, D), F32, init=noise)
    rc = _lib.lib().tan_unpad_add(_p(src), dst.ptr(), rows, D, Dpad, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0 and dst.guard_ok()
    assert same(dst.t, noise + src[:, :D])            # one f32 addition per element: exact


# ---------------------------------------------------------------------------------------------------------------- part 1: pool forward
def run_pool_fwd(h, mask, dtype):
    M, W, H = h.shape
    pooled, arg = Guarded((M, H), dtype), Guarded((M, H), torch.int32)
    rc = _lib.lib().tan_wordpool_fwd(_p(h), _p(mask), pooled.ptr(), arg.ptr(), M, W, H, _dt(dtype), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert pooled.guard_ok() and arg.guard_ok(), "tan_wordpool_fwd wrote behind an output"
    return pooled.t, arg.t


POOL_SHAPES = [(M, W, 2048) for M in (1, 3, 65) for W in (1, 9, 32)] + [(1, 9, 4)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("M,W,H", POOL_SHAPES)
def test_wordpool_fwd_picks_the_first_maximum(M, W, H, dtype):
    for masked in (False, True):
        mask = wc.masks(M, W, 7 * M + W).cuda() if masked else None
        h = wc.tied_h(M, W, H, dtype, mask, 100 * M + W + masked).cuda()
        want_p, want_a = wc.wordpool_expected(h, mask, dtype)
        got_p, got_a = run_pool_fwd(h, mask, dtype)
        assert same(got_a, want_a), f"argmax, mask={masked}: {int((got_a != want_a).sum())} of {got_a.numel()} differ"
        assert same(got_p, want_p), f"pooled, mask={masked}"
        hd = h.double() if mask is None else h.double().masked_fill(~mask.bool()[:, :, None], wc.FILL)
        if W > 1:                                        # the case is what it says: ties whose first index is not the last
            assert bool(((hd == hd.amax(1, keepdim=True)).sum(1) > 1).any())
            assert not same(got_a, wc.last_max(h, mask)[1].to(torch.int32))
        if masked and M >= 3:                            # sentence 2: every word masked, handed to the kernel as it is
            fill = torch.tensor(wc.FILL).to(dtype)
            assert bool((got_p[2] == fill.cuda()).all()) and bool((got_a[2] == 0).all())


def test_wordpool_fwd_masked_and_unmasked_tie():
    """a masked first word (filled with -6e4) and unmasked words holding -6e4: f32 ties and takes word 0; bf16 stores -59904 > -6e4
    and takes the first unmasked word"""
    mask = torch.tensor([[0, 1, 0, 1]], dtype=torch.uint8, device="cuda")
    for dtype, want in ((F32, 0), (BF16, 1)):
        h = torch.full((1, 4, 8), wc.FILL, device="cuda").to(dtype)
        p, a = run_pool_fwd(h, mask, dtype)
        assert bool((a == want).all()) and same(p, torch.full((1, 8), wc.FILL, device="cuda").to(dtype))


# ---------------------------------------------------------------------------------------------------------------- part 1: pool backward
def pool_bwd_inputs(M, W, H, dtype, seed):
    pooled = (rn(seed, M, H) * 2).round() / 2                              # a third of the channels exactly 0, a third negative
    d_pooled = rn(seed + 1, M, H)
    g = torch.Generator().manual_seed(seed + 2)
    arg = torch.randint(0, W, (M, H), generator=g, dtype=torch.int32).cuda()
    return d_pooled.to(dtype), pooled.to(dtype), arg


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("M,W", [(1, 3), (64, 3), (65, 3), (130, 3), (130, 32)])
def test_wordpool_bwd_scatters_exactly_and_sums_the_bias_gradient(M, W, dtype):
    H = 2048
    assert W == 3 or M * W * (H // 4) // 256 > 8192
    d_pooled, pooled, arg = pool_bwd_inputs(M, W, H, dtype, 10 * M + W)
    assert bool((pooled == 0).any()) and bool((pooled < 0).any()) and bool((pooled > 0).any())
    want_dh, gated = wc.wordpool_bwd_expected(d_pooled, pooled, arg, W)
    noise = rn(5, H) * 1e-2
    L, st = _lib.lib(), ops._stream()
    outs = {}
    for with_db in (True, False):
        dh = Guarded((M, W, H), dtype)
        db = Guarded((H,), F32, init=noise)
        rc = L.tan_wordpool_bwd(_p(d_pooled), _p(pooled), _p(arg), dh.ptr(), db.ptr() if with_db else None, M, W, H, _dt(dtype), st)
        torch.cuda.synchronize()
        assert rc == 0 and dh.guard_ok() and db.guard_ok()
        assert same(dh.t, want_dh), f"dh (db {'given' if with_db else 'NULL'}): {int((dh.t != want_dh).sum())} elements differ"
        outs[with_db] = (dh, db)
    assert outs[False][1].untouched()                                       # db NULL: no bias launch
    e = wc.rel_err(outs[True][1].t.double() - noise.double(), gated.sum(0))
    print(f"\n[w2v fp64] wordpool_bwd db M={M} W={W} {dtype}: {e:.3e}")
    assert e <= DB_REL, e


# ---------------------------------------------------------------------------------------------------------------- part 1: rejections
def test_every_require_returns_bad_arg_and_writes_nothing():
    L, st = _lib.lib(), ops._stream()
    D, Dpad, rows, M, W, H = 5, 8, 4, 2, 3, 8
    table, ids = rn(1, 9, D), torch.tensor([1, 2, 3, 4], device="cuda")
    out = Guarded((rows, Dpad), F32)
    ok = dict(ids=_p(ids), table=_p(table), out=out.ptr(), rows=rows, D=D, Dpad=Dpad, V=9, dtype=_lib.TAN_F32)
    bad = [dict(table=None), dict(out=None), dict(rows=0), dict(rows=-1), dict(D=0), dict(Dpad=4), dict(Dpad=6), dict(V=0), dict(V=-1),
           dict(dtype=2), dict(dtype=-1)]
    for kw in bad:
        a = {**ok, **kw}
        rc = L.tan_embed_gather(a["ids"], a["table"], a["out"], a["rows"], a["D"], a["Dpad"], a["V"], a["dtype"], st)
        assert rc == -1, ("tan_embed_gather", kw, rc)
    src = rn(2, rows, Dpad)
    dst = Guarded((rows, D), F32, init=rn(3, rows, D))
    ok = dict(src=_p(src), dst=dst.ptr(), rows=rows, D=D, Dpad=Dpad)
    for kw in [dict(src=None), dict(dst=None), dict(rows=0), dict(rows=-3), dict(D=0), dict(Dpad=4)]:
        a = {**ok, **kw}
        assert L.tan_unpad_add(a["src"], a["dst"], a["rows"], a["D"], a["Dpad"], st) == -1, ("tan_unpad_add", kw)
    h = rn(4, M, W, H)
    pooled, arg = Guarded((M, H), F32), Guarded((M, H), torch.int32)
    ok = dict(h=_p(h), pooled=pooled.ptr(), argmax=arg.ptr(), M=M, W=W, H=H, dtype=_lib.TAN_F32)
    for kw in [dict(h=None), dict(pooled=None), dict(argmax=None), dict(M=0), dict(M=-1), dict(W=0), dict(H=0), dict(H=-4), dict(H=6),
               dict(dtype=2)]:
        a = {**ok, **kw}
        assert L.tan_wordpool_fwd(a["h"], None, a["pooled"], a["argmax"], a["M"], a["W"], a["H"], a["dtype"], st) == -1, ("tan_wordpool_fwd", kw)
    dp, pl, ar = pool_bwd_inputs(M, W, H, F32, 5)
    dh, db = Guarded((M, W, H), F32), Guarded((H,), F32, init=rn(6, H))
    ok = dict(d_pooled=_p(dp), pooled=_p(pl), argmax=_p(ar), dh=dh.ptr(), M=M, W=W, H=H, dtype=_lib.TAN_F32)
    for kw in [dict(d_pooled=None), dict(pooled=None), dict(argmax=None), dict(dh=None), dict(M=0), dict(W=0), dict(W=-2), dict(H=0),
               dict(H=6), dict(dtype=2), dict(dtype=-1)]:
        a = {**ok, **kw}
        rc = L.tan_wordpool_bwd(a["d_pooled"], a["pooled"], a["argmax"], a["dh"], db.ptr(), a["M"], a["W"], a["H"], a["dtype"], st)
        assert rc == -1, ("tan_wordpool_bwd", kw, rc)
    torch.cuda.synchronize()
    for name, buf in (("gather out", out), ("unpad dst", dst), ("pooled", pooled), ("argmax", arg), ("dh", dh), ("db", db)):
        assert buf.untouched(), f"{name} was written by a refused call"


# ---------------------------------------------------------------------------------------------------------------- part 2: the model
_PARAMS, _MODELS = {}, {}


def _params(kind):
    """ "synth": synth.w2v_params as they are; "exact": the same with the fc1 path on grids (w2v_cases.exact_params: h is exact in f32,
    so rounding never decides which word the pooling picks)"""
    if kind not in _PARAMS:
        p = {k: torch.from_numpy(v) for k, v in synth.w2v_params(31, V).items()}
        if kind == "exact":
            p = wc.exact_params(p)
            wc.assert_h_exact(p)
        _PARAMS[kind] = p
    return _PARAMS[kind]


def _model(dtype, kind):
    from temporalalignnet_amd.word2vec_model import Word2VecModel
    if (dtype, kind) not in _MODELS:
        m = Word2VecModel(num_embeddings=V, compute_dtype=dtype)
        m.load_state_dict(_params(kind))
        _MODELS[dtype, kind] = m.cuda()
    m = _MODELS[dtype, kind]
    for p in m.parameters():
        p.grad = None
    return m


class _IgnoreFirst(torch.autograd.Function):
    """b, while staying a consumer of a: the backward hands a no gradient at all (None, not zeros)"""

    @staticmethod
    def forward(ctx, a, b):
        ctx.set_materialize_grads(False)
        return b.clone()

    @staticmethod
    def backward(ctx, g):
        return None, g


def _case_inputs(M, W, variant):
    if (M, W) == (9, 32):
        ids, mask = (torch.from_numpy(a) for a in synth.w2v_tokens(32, 9, V))
    else:
        ids, mask = wc.tokens(1000 * M + W, M, W, V)
    if variant == "nomask":
        mask = None
    if variant == "oob":                                 # masked in or out as the word they replace was
        ids = ids.clone()
        flat = ids.view(-1)
        n = flat.numel()
        for i, bad in zip((0, n // 3, n // 2, n - 1, min(5, n - 1)), (-1, V, V + 7, 2 ** 40, -2 ** 40)):
            flat[i] = bad
    return ids.cuda(), None if mask is None else mask.cuda()


# every shape with the exact-h parameters; the existing shape also with the random ones
SHAPES = [("exact", 1, 32), ("exact", 9, 32), ("exact", 65, 7), ("exact", 512, 4), ("exact", 2048, 8), ("synth", 9, 32)]


@pytest.mark.parametrize("variant", ["mask", "nomask", "oob", "unused"])
@pytest.mark.parametrize("kind,M,W", SHAPES)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_model_matches_fp64_autograd(dtype, kind, M, W, variant):
    bf16 = dtype == "bf16"
    fwd_rel, grad_rel = (BF16_FWD_REL, BF16_GRAD_REL) if bf16 else (F32_FWD_REL, F32_GRAD_REL)
    ids, mask = _case_inputs(M, W, variant)
    m = _model(dtype, kind)
    cot = rn(M + W, M, 512)
    out = m(ids, mask)
    pooler = out["pooler_output"]
    assert pooler.shape == (M, 512) and pooler.dtype == F32 and pooler.requires_grad
    named = dict(m.named_parameters())
    if variant == "unused":
        other = torch.zeros(M, 512, device="cuda", requires_grad=True)
        (_IgnoreFirst.apply(pooler, other) * cot).sum().backward()
        assert torch.equal(other.grad, cot)
        assert all(p.grad is None for p in named.values())       # the sentence embedder's backward saw None and returned at once
        with torch.no_grad():
            ref = wc.forward(wc.operands(_params(kind), bf16, "cuda"), ids, mask, bf16)
        grads = {}
    else:
        (pooler * cot).sum().backward()
        ref, grads = wc.forward_backward(_params(kind), ids, mask, cot, bf16, "cuda")
        assert named["word_embd.weight"].grad is None
    torch.cuda.synchronize()
    errs = {}
    for k in ("pooler_output", "last_hidden_state"):
        got = out[k].detach()
        assert got.shape == ref[k].shape and bool(torch.isfinite(got).all()), k
        errs[k] = (wc.rel_err(got, ref[k]), fwd_rel)
    for k, want in grads.items():
        got = named[k].grad
        assert got is not None and got.shape == want.shape and got.dtype == F32 and bool(torch.isfinite(got).all()), k
        errs[k] = (wc.rel_err(got, want), grad_rel)
    print(f"\n[w2v fp64] model {dtype} {kind} M={M} W={W} {variant}: " + ", ".join(f"{k} {e:.3e}" for k, (e, _) in errs.items()))
    bad = {k: e for k, (e, b) in errs.items() if not e <= b}
    assert not bad, f"{dtype} {kind} M={M} W={W} {variant}: over the bound: {bad}"
