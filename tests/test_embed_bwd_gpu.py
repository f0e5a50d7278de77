"""The fused input embeddings' backward (csrc/tan_embed.hip: tan_embed_bwd, tan_pos_ln_bwd) against float64 autograd, tensor by tensor.

Part 1 calls the two kernels through the C ABI.  proj is bf16; mean / rstd are computed in float64 from that bf16 proj and stored as
f32, as the forward would; upstream gradients are bf16.  The reference is float64 autograd of LayerNorm(proj) and, for the position
part, of LayerNorm(table rows) on the same values.  Every output starts as NaN; g_ln_g / g_ln_b / g_gamma / g_beta / g_table start as
noise and the INCREMENT is checked.  A sentinel d_proj row after the last row, a sentinel partial plane after the last ceil(B / 8),
and the table rows outside the used slices must come back bit-unchanged.  Each problem has a constant row and a nearly constant row
(rstd ~ 1/sqrt(eps)) and a padded row whose upstream gradient is zero.

Part 2 runs the engine's _embed_fused / _embed_bwd_fused on a seeded bf16 TemporalAligner and compares every front-end gradient with
float64 autograd of oracle.tan_ref.front_end on the same bf16 features and parameters.

Which branch each case reaches (EB_VG = 8 videos per partial plane, a wave owns one position t, 8 waves = 8 positions per workgroup):

  tan_embed_bwd
  B = 1, 7             one partial group: the v >= nvid rows of the only group are masked (nparts = 1)
  B = 8, 64, 128       exact groups (nparts = 1, 8, 16)
  B = 9, 65, 129       one video in the last group (nparts = 2, 9, 17)
  T = 3, 13, 65        t >= T waves in the last of the tblocks (T = 8, 64: none)
  two problems         video (T) and text (N) in one launch: the blk0 split, different tblocks / nparts plane strides
  d_out patterns       both, only [0], only [1]; d_pos[k] NULL with d_out[k] present; d_pos[k] given with d_out[k] NULL (ignored)
  tan_pos_ln_bwd
  nparts = 1, 8        one round of the 8-wide plane reduction, no clamped tail / exactly full
  nparts = 2, 9, 17    the clamped tail with weight 0 (17: a third round of 8)
  nuse = 2, 3          n = 13, 5, 65: workgroups of four rows straddle two uses; overlapping slices of one table (atomics on the
                       same rows); a use with g_table = NULL (the sine table) next to uses with a table
  host-side limits     each refused with TanHipError before any launch (buffers are in bounds for the launch anyway)
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import tan_ref
from temporalalignnet_amd import _lib, ops

pytestmark = pytest.mark.gpu

W, EPS, VG = 512, 1e-5, 8          # VG: tan_embed_bwd_group()

# Norm-relative bounds, ||got - ref|| / ||ref|| per tensor, a little over twice the worst measured on MI355X over every case here:
#   d_proj (bf16 output of the LayerNorm backward, f32 inside): worst 1.75e-3 (B=128 T=13) -- bf16 rounding
BF16_REL = 4e-3
#   f32 sums (d_pos planes, g_ln_g / g_ln_b, g_table, g_gamma / g_beta): worst 2.4e-7 (B=129 T=65, two problems) -- f32 summation
F32_REL = 5e-7
#   the engine's front-end gradients against fp64 autograd of the oracle on bf16 features: worst 2.4e-3 (d_lang), 1.8e-3 for the
#   weight gradients -- bf16 proj / d_proj / d_lang rounding and the bf16 weight-gradient GEMM operands.  The gradients that see
#   only bf16 d_out and f32 sums (E2E_F32 below) are held to F32_REL: worst 1.4e-7 (B=128 ln_position_init.weight)
E2E_REL = 5e-3
#   x0 of the next fused forward after an optimizer step against the oracle on the updated parameters: worst 2.0e-3
X0_REL = 5e-3


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def bits(t):
    """the bit pattern (NaN == NaN): bitwise comparisons"""
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def rel_err(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    den = ref.norm().item()
    return (got - ref).norm().item() / den if den > 0 else (got.norm().item() + 0.0)


def nparts(B):
    return -(-B // VG)


def ln_stats(x):
    """f64 LayerNorm statistics of `x` as the forward stores them: (mean, rstd) f32"""
    x = x.double()
    m = x.mean(-1)
    v = ((x - m[:, None]) ** 2).mean(-1)
    return m.float(), torch.rsqrt(v + EPS).float()


# ---------------------------------------------------------------------------------------------------------------- references
def _leaf(t):
    """a float64 leaf of its own (never the caller's tensor, whose .grad would accumulate over calls)"""
    return t.detach().double().clone().requires_grad_(True)


def embed_bwd_reference(B, T, proj, gamma, d0, d1, fault=None):
    """float64 autograd of y = LayerNorm(proj; gamma) with upstream d0 + d1 ([B * T, W] each, None = absent), and the per-group
    position-row sums.  Keys: d_proj, g_ln_g, g_ln_b, d_pos0, d_pos1 (planes [ceil(B / 8), T, W]).
    fault (test_embed_bwd_cpu.py): "drop_last_group" (the last partial plane lost), "omit_dout1" (dy without d_out[1])."""
    dev = proj.device
    x, g = _leaf(proj), _leaf(gamma)
    b = torch.zeros(W, dtype=torch.float64, device=dev, requires_grad=True)
    y = F.layer_norm(x, (W,), g, b, EPS)
    dy = torch.zeros_like(x)
    for k, d in enumerate((d0, d1)):
        if d is not None and not (k == 1 and fault == "omit_dout1"):
            dy = dy + d.double()
    y.backward(dy)
    out = {"d_proj": x.grad, "g_ln_g": g.grad, "g_ln_b": b.grad}
    P = nparts(B)
    for k, d in enumerate((d0, d1)):
        if d is None:
            continue
        planes = torch.zeros(P * VG, T, W, dtype=torch.float64, device=dev)
        planes[:B] = d.double().view(B, T, W)
        planes = planes.view(P, VG, T, W).sum(1)
        if fault == "drop_last_group":
            planes[-1] = 0
        out[f"d_pos{k}"] = planes
    return out


def pos_ln_bwd_reference(tables, uses, gamma, fault=None):
    """float64 autograd of ln_position_init over the used table slices.  tables: {name: [P, W]}; uses: [(name, start, n, planes
    [>= nparts, n, W], nparts)].  Keys: g_table.<name> (every table), g_gamma, g_beta.
    fault: "drop_plane" (the first use reduces one plane fewer), "skip_table" (the last use adds nothing to its table)."""
    dev = gamma.device
    leaf = {k: _leaf(t) for k, t in tables.items()}
    g = _leaf(gamma)
    b = torch.zeros(W, dtype=torch.float64, device=dev, requires_grad=True)
    loss = 0
    for i, (name, start, n, planes, P) in enumerate(uses):
        parts = planes[:P - 1 if (fault == "drop_plane" and i == 0) else P].double()
        tab = leaf[name].detach() if (fault == "skip_table" and i == len(uses) - 1) else leaf[name]
        loss = loss + (F.layer_norm(tab[start:start + n], (W,), g, b, EPS) * parts.sum(0)).sum()
    loss.backward()
    out = {f"g_table.{k}": (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in leaf.items()}
    out |= {"g_gamma": g.grad, "g_beta": b.grad}
    return out


# ---------------------------------------------------------------------------------------------------------------- part 1
class EmbProb:
    """One problem of tan_embed_bwd: B videos of T rows.  d_out[0] in its own [B * T] layout (grp T, off 0); d_out[1] in a joint
    layout [B, grp1, W] at row offset off1 (a caller's buffer may be shared between problems)."""

    def __init__(self, B, T, seed, *, d_out=(True, True), d_pos=(True, True), grp1=None, off1=0, joint=None):
        g = torch.Generator(device="cuda").manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g, device="cuda")      # noqa: E731
        R = B * T
        self.B, self.T, self.R, self.P = B, T, R, nparts(B)
        proj = rn(R, W) * 1.5 + 0.3
        proj[0] = 0.75                                          # a constant row: xhat = 0, rstd = 1/sqrt(eps)
        if R > 1:
            proj[1] = 1.0                                       # nearly constant: one bf16 ulp up on every 7th feature
            proj[1, ::7] = 1.0078125
        self.proj = proj.bfloat16()
        self.mean, self.rstd = ln_stats(self.proj)
        self.gamma = 1 + 0.2 * rn(W)
        self.grp1 = grp1 if grp1 is not None else T
        self.off1 = off1
        self.d0 = rn(R, W).bfloat16() if d_out[0] else None
        if d_out[1]:
            self.d1buf = joint if joint is not None else rn(B * self.grp1, W).bfloat16()
        else:
            self.d1buf = None
        if self.d0 is not None:                                 # a padded position: zero upstream gradient on both paths
            self.d0.view(B, T, W)[B - 1, T - 1] = 0
        if self.d1buf is not None:
            self.rows(1)[B - 1, T - 1] = 0
        self.d_proj = _nan(R + 1, W, dtype=torch.bfloat16)      # (+ a sentinel row)
        self.g_g, self.g_b = rn(W) * 1e-2, rn(W) * 1e-2
        self.g_g0, self.g_b0 = self.g_g.clone(), self.g_b.clone()
        self.d_pos = [_nan(self.P + 1, T, W) if want else None for want in d_pos]       # (+ a sentinel plane)

    def rows(self, k):
        """the [R, W] rows of d_out[k] the problem reads (a view)"""
        if k == 0:
            return self.d0
        if self.d1buf is None:
            return None
        return self.d1buf.view(self.B, self.grp1, W)[:, self.off1:self.off1 + self.T]

    def fill(self, d):
        d.rows, d.T, d.C = self.R, self.T, W
        d.d_out[0], d.d_out_grp_rows[0], d.d_out_off[0] = _p(self.d0), self.T, 0
        d.d_out[1], d.d_out_grp_rows[1], d.d_out_off[1] = _p(self.d1buf), self.grp1, self.off1
        d.d_pos[0], d.d_pos[1] = _p(self.d_pos[0]), _p(self.d_pos[1])
        d.proj, d.mean, d.rstd, d.ln_g = _p(self.proj), _p(self.mean), _p(self.rstd), _p(self.gamma)
        d.d_proj, d.g_ln_g, d.g_ln_b = _p(self.d_proj), _p(self.g_g), _p(self.g_b)

    def check(self, tag, errs):
        d1 = self.rows(1)
        ref = embed_bwd_reference(self.B, self.T, self.proj, self.gamma, self.d0, None if d1 is None else d1.reshape(self.R, W))
        got = {"d_proj": self.d_proj[:self.R], "g_ln_g": self.g_g.double() - self.g_g0.double(),
               "g_ln_b": self.g_b.double() - self.g_b0.double()}
        assert torch.equal(bits(self.d_proj[self.R]), bits(_nan(W, dtype=torch.bfloat16))), f"{tag}: d_proj sentinel row written"
        for k in range(2):
            buf = self.d_pos[k]
            if buf is None:
                ref.pop(f"d_pos{k}", None)                      # (not wanted: nothing to check)
                continue
            if f"d_pos{k}" in ref:
                got[f"d_pos{k}"] = buf[:self.P]
                assert torch.equal(bits(buf[self.P]), bits(_nan(self.T, W))), f"{tag}: d_pos{k} sentinel plane written"
            else:       # d_pos given without its d_out: never touched
                assert torch.equal(bits(buf), bits(_nan(*buf.shape))), f"{tag}: d_pos{k} written without d_out[{k}]"
        for k, r in ref.items():
            t = got[k]
            assert t.shape == r.shape, (tag, k, t.shape, r.shape)
            assert torch.isfinite(t).all(), f"{tag}: {k} has NaN/inf (an unwritten row or plane?)"
            bound = BF16_REL if k == "d_proj" else F32_REL
            e = rel_err(t, r)
            errs[f"{tag} {k}"] = e
            assert e <= bound, f"{tag}: {k} {e:.3e} over {bound}"


def run_embed_bwd(probs):
    D = (_lib.EmbedBwdDesc * 2)()
    for i, pr in enumerate(probs):
        pr.fill(D[i])
    _lib.check(_lib.lib().tan_embed_bwd(D, len(probs), ops._stream()), "tan_embed_bwd")
    torch.cuda.synchronize()


def _report(errs):
    worst = max(errs, key=errs.get)
    dp = max((e for k, e in errs.items() if k.endswith("d_proj")), default=0.0)
    f32 = max((e for k, e in errs.items() if not k.endswith("d_proj")), default=0.0)
    print(f"\n[embed bwd] worst d_proj {dp:.2e}, worst f32 sum {f32:.2e} ({worst})")


@pytest.mark.parametrize("B,T", [(1, 13), (7, 13), (8, 13), (9, 13), (64, 13), (65, 13), (128, 13), (129, 13),
                                 (9, 3), (9, 8), (9, 64), (9, 65), (65, 65)])
def test_embed_bwd_one_problem_matches_fp64(B, T):
    """the video problem alone, joint layout (grp = T + 5, off = 0) for d_out[1]"""
    pr = EmbProb(B, T, seed=100 * B + T, grp1=T + 5, off1=0)
    run_embed_bwd([pr])
    errs = {}
    pr.check(f"B={B} T={T}", errs)
    _report(errs)


@pytest.mark.parametrize("B,T,N", [(128, 64, 16), (65, 13, 5), (1, 3, 7), (129, 65, 9)])
def test_embed_bwd_video_and_text_in_one_launch(B, T, N):
    """video (T) and text (N) in one launch sharing the joint buffer [B, T + N]: video at off 0, text at off T (the engine's layout)"""
    g = torch.Generator(device="cuda").manual_seed(B + T + N)
    joint = torch.randn(B * (T + N), W, generator=g, device="cuda").bfloat16()
    v = EmbProb(B, T, seed=1, grp1=T + N, off1=0, joint=joint)
    t = EmbProb(B, N, seed=2, grp1=T + N, off1=T, joint=joint)
    run_embed_bwd([v, t])
    errs = {}
    v.check(f"video B={B} T={T}", errs)
    t.check(f"text B={B} N={N}", errs)
    _report(errs)


PATTERNS = {  # d_out present, d_pos present
    "both": ((True, True), (True, True)),
    "only0": ((True, False), (True, True)),          # (d_pos[1] given, d_out[1] NULL: ignored)
    "only1": ((False, True), (True, True)),
    "pos0_null": ((True, True), (False, True)),
    "pos1_null": ((True, True), (True, False)),
    "no_pos": ((True, True), (False, False)),
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_embed_bwd_d_out_patterns(pattern):
    B, T, N = 65, 13, 5
    d_out, d_pos = PATTERNS[pattern]
    g = torch.Generator(device="cuda").manual_seed(7)
    joint = torch.randn(B * (T + N), W, generator=g, device="cuda").bfloat16()
    v = EmbProb(B, T, seed=3, d_out=d_out, d_pos=d_pos, grp1=T + N, off1=0, joint=joint)
    t = EmbProb(B, N, seed=4, d_out=d_out[::-1], d_pos=d_pos, grp1=T + N, off1=T, joint=joint)
    run_embed_bwd([v, t])
    errs = {}
    v.check(f"video {pattern}", errs)
    t.check(f"text {pattern}", errs)
    _report(errs)


POS_CASES = {  # [(table, start, n)], nparts; table "s" is a fixed sine-like table (g_table NULL)
    "one_use_nparts1": ([("a", 0, 13)], 1),
    "one_use_nparts17": ([("a", 2, 13)], 17),
    "overlap_nparts9": ([("a", 3, 13), ("a", 7, 13)], 9),
    "three_uses_nparts8": ([("a", 0, 65), ("a", 20, 65), ("b", 3, 7)], 8),
    "headline_nparts16": ([("a", 2, 64), ("a", 17, 64), ("b", 4, 16)], 16),
    "sine_with_text_nparts2": ([("s", 2, 13), ("s", 5, 13), ("b", 1, 5)], 2),
    "sine_between_tables_nparts9": ([("a", 1, 5), ("s", 0, 13), ("b", 6, 13)], 9),
    "sine_only_nparts17": ([("s", 0, 3)], 17),
}


def pos_case(uses, P, seed=11):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")      # noqa: E731
    tables = {k: rn(100, W) * 0.01 + 0.002 * rn(100, 1) for k in sorted({u[0] for u in uses})}
    tables.setdefault("a", rn(100, W) * 0.01)
    stats = {k: ln_stats(t) for k, t in tables.items()}
    g_tab = {k: rn(100, W) * 1e-2 for k in tables if k != "s"}
    planes = [rn(P, n, W) for _, _, n in uses]
    return tables, stats, g_tab, planes


@pytest.mark.parametrize("case", list(POS_CASES))
def test_pos_ln_bwd_matches_fp64(case):
    uses, P = POS_CASES[case]
    tables, stats, g_tab, planes = pos_case(uses, P)
    g = torch.Generator(device="cuda").manual_seed(5)
    gamma = 1 + 0.2 * torch.randn(W, generator=g, device="cuda")
    g_gamma, g_beta = torch.randn(W, generator=g, device="cuda") * 1e-2, torch.randn(W, generator=g, device="cuda") * 1e-2
    before = {k: v.clone() for k, v in g_tab.items()} | {"g_gamma": g_gamma.clone(), "g_beta": g_beta.clone()}
    U = (_lib.PosLnBwdUse * len(uses))()
    for i, (name, start, n) in enumerate(uses):
        m, r = stats[name]
        gt = g_tab.get(name)
        U[i] = _lib.PosLnBwdUse(planes[i].data_ptr(), tables[name][start].data_ptr(), m[start].data_ptr(), r[start].data_ptr(),
                                None if gt is None else gt[start].data_ptr(), n, P)
    _lib.check(_lib.lib().tan_pos_ln_bwd(U, len(uses), gamma.data_ptr(), g_gamma.data_ptr(), g_beta.data_ptr(), W, ops._stream()),
               "tan_pos_ln_bwd")
    torch.cuda.synchronize()
    ref = pos_ln_bwd_reference(tables, [(name, start, n, planes[i], P) for i, (name, start, n) in enumerate(uses)], gamma)
    got = {"g_gamma": g_gamma.double() - before["g_gamma"].double(), "g_beta": g_beta.double() - before["g_beta"].double()}
    for k, t in g_tab.items():
        got[f"g_table.{k}"] = t.double() - before[k].double()
        used = torch.zeros(t.shape[0], dtype=torch.bool, device="cuda")
        for name, start, n in uses:
            if name == k:
                used[start:start + n] = True
        assert torch.equal(bits(t[~used]), bits(before[k][~used])), f"{case}: table {k} rows outside the used slices changed"
    errs = {}
    for k, t in got.items():
        if not any(u[0] == k[-1] for u in uses) and k.startswith("g_table"):
            continue                    # a table no use reads (checked bit-unchanged above)
        assert torch.isfinite(t).all(), (case, k)
        errs[f"{case} {k}"] = e = rel_err(t, ref[k])
        assert e <= F32_REL, f"{case}: {k} {e:.3e} over {F32_REL}"
    _report(errs)


def _bwd_desc(B=2, T=4):
    """a valid one-problem descriptor over in-bounds buffers (d_out[1] has room for any layout the limits below try)"""
    pr = EmbProb(B, T, seed=9, grp1=4 * T, off1=0)
    D = (_lib.EmbedBwdDesc * 3)()
    pr.fill(D[0])
    pr.fill(D[1])
    return pr, D


def test_embed_bwd_host_limits_raise():
    pr, D = _bwd_desc()
    L, st = _lib.lib(), ops._stream()

    def refused(nprob=1, **kw):
        for k, v in kw.items():
            if k in ("d_out", "grp", "off"):
                idx, val = v
                getattr(D[0], {"d_out": "d_out", "grp": "d_out_grp_rows", "off": "d_out_off"}[k])[idx] = val
            else:
                setattr(D[0], k, v)
        with pytest.raises(_lib.TanHipError):
            _lib.check(L.tan_embed_bwd(D, nprob, st), "tan_embed_bwd")
        pr.fill(D[0])
    refused(nprob=0)
    refused(nprob=3)
    refused(C=256)
    refused(rows=pr.R - 1)                                  # rows % T != 0
    D[0].d_out[0] = D[0].d_out[1] = None
    refused()
    refused(grp=(1, pr.T - 1))                              # d_out_grp_rows < T + d_out_off
    refused(grp=(1, pr.T + 2), off=(1, 3))
    refused(off=(1, -1))
    refused(grp=(0, pr.T - 1))
    # the accepted edge: grp == T + off
    D[0].d_out_grp_rows[1], D[0].d_out_off[1] = pr.T + 3, 3
    _lib.check(L.tan_embed_bwd(D, 1, st), "tan_embed_bwd")
    torch.cuda.synchronize()


def test_pos_ln_bwd_host_limits_raise():
    tables, stats, g_tab, planes = pos_case([("a", 0, 8)], 2)
    g = torch.ones(W, device="cuda")
    gg, gb = torch.zeros(W, device="cuda"), torch.zeros(W, device="cuda")
    m, r = stats["a"]
    U = (_lib.PosLnBwdUse * 4)(*[_lib.PosLnBwdUse(planes[0].data_ptr(), tables["a"].data_ptr(), m.data_ptr(), r.data_ptr(),
                                                  g_tab["a"].data_ptr(), 8, 2) for _ in range(4)])
    L, st = _lib.lib(), ops._stream()

    def refused(nuse=1, C_=W, **kw):
        saved = {k: getattr(U[0], k) for k in kw}
        for k, v in kw.items():
            setattr(U[0], k, v)
        with pytest.raises(_lib.TanHipError):
            _lib.check(L.tan_pos_ln_bwd(U, nuse, g.data_ptr(), gg.data_ptr(), gb.data_ptr(), C_, st), "tan_pos_ln_bwd")
        for k, v in saved.items():
            setattr(U[0], k, v)
    refused(nuse=0)
    refused(nuse=4)
    refused(nparts=0)
    refused(n=0)
    refused(C_=256)
    refused(d_pos=None)
    _lib.check(L.tan_pos_ln_bwd(U, 3, g.data_ptr(), gg.data_ptr(), gb.data_ptr(), W, st), "tan_pos_ln_bwd")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- part 2
FRONT = ["video_pre_proj.weight", "text_pre_proj.weight", "ln_video_init.weight", "ln_video_init.bias", "ln_text_init.weight",
         "ln_text_init.bias", "ln_position_init.weight", "ln_position_init.bias", "temporal_pos_embed", "text_temporal_pos_embed"]
E2E_F32 = {"ln_video_init.bias", "ln_text_init.bias", "ln_position_init.weight", "ln_position_init.bias", "temporal_pos_embed",
           "text_temporal_pos_embed"}


def _model(pos_enc="learned", text_pos=0, Dv=1024, Dt=512, seed=3):
    from temporalalignnet_amd import synth
    from temporalalignnet_amd.tan_model import TemporalAligner
    m = TemporalAligner(num_encoder_layers=1, num_decoder_layers=1, compute_dtype="bf16", random_pos_start=0,
                        language_model="bert" if Dt == 768 else None, use_text_pos_enc=text_pos, pos_enc=pos_enc, d_video=Dv).cuda()
    sd = m.state_dict()
    for k, v in synth.make_params(seed, 1, 1, False, d_video=Dv, d_text=Dt).items():
        if k == "temporal_pos_embed" and pos_enc != "learned":
            continue                                         # (the sine table is a buffer of the model, not a parameter)
        if k in sd and sd[k].shape == torch.Size(v.shape):
            sd[k].copy_(torch.from_numpy(v))
    m.invalidate_shadow()
    m._ensure_flat()
    m._bind_grads()
    return m


def _ref_params(m):
    """what the fused path reads, in float64: the bf16 shadow of the pre-projections, the f32 masters of the rest"""
    p = {}
    for n in FRONT:
        if n == "temporal_pos_embed" and m.pos_enc != "learned":
            p[n] = m.temporal_pos_embed.double()
        elif n.endswith("pre_proj.weight"):
            p[n] = m._w(n).double()
        else:
            p[n] = m._f(n).double()
    return p


E2E_CASES = {  # B, T, N, Dv, Dt, pos_enc, text_pos, (p_v, p_t, p_j), features, d_x0, d_lang_dual
    "B6_overlap": (6, 32, 9, 1024, 512, "learned", 0, (3, 0, 11), torch.float32, True, True),
    "B9_same_offset_bert_K2048": (9, 20, 7, 2048, 768, "learned", 1, (5, 2, 5), torch.bfloat16, True, True),
    "B128_headline_K128": (128, 64, 16, 128, 512, "learned", 1, (0, 4, 17), torch.float32, True, True),
    "B9_sine": (9, 13, 5, 1024, 512, "sine", 0, (2, 0, 4), torch.bfloat16, True, True),
    "B9_sine_text_pos": (9, 13, 5, 1024, 768, "sine", 1, (6, 3, 6), torch.float32, True, True),
    "B6_no_d_x0_no_d_lang": (6, 16, 4, 1024, 512, "learned", 1, (1, 2, 6), torch.float32, False, False),
    "B128_no_d_lang": (128, 64, 16, 2048, 512, "learned", 0, (7, 0, 30), torch.bfloat16, True, False),
}


@pytest.mark.parametrize("case", list(E2E_CASES))
def test_fused_embedding_backward_matches_fp64_oracle(case):
    B, T, N, Dv, Dt, pos_enc, text_pos, (p_v, p_t, p_j), fdt, has_x0, has_lang = E2E_CASES[case]
    m = _model(pos_enc, text_pos, Dv, Dt)
    f = m._flat
    g = torch.Generator(device="cuda").manual_seed(B * 7 + T)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")      # noqa: E731
    video = (rn(B, T, Dv).abs() * 0.5).to(fdt)
    lang = rn(B, N, Dt).to(fdt)
    L = T + N
    d_x0 = rn(B * T, W).bfloat16() if has_x0 else None
    d_xj = rn(B * L, W).bfloat16()
    d_lang_dual = rn(B * N, W).bfloat16() if has_lang else None
    f.grad.copy_(rn(f.grad.numel()) * 1e-2)
    g0 = f.grad.clone()
    fe = m._embed_fused(video, lang, None, None, p_v, p_t, p_j, save=True)
    assert (fe["sv_video_j"] is None) == (p_v == p_j)
    run = {"em": fe["em"], "B": B, "T": T, "N": N, **{k: fe[k] for k in ("sv_video", "sv_video_j", "sv_text", "sv_text_t")}}
    d_lang = m._embed_bwd_fused(run, d_x0, d_xj, d_lang_dual, True)
    torch.cuda.synchronize()                                 # (the text weight-gradient GEMM and d_lang ran on the side stream)
    # ---- reference
    p = {k: v.clone().requires_grad_(True) for k, v in _ref_params(m).items()}
    v64 = video.bfloat16().double()
    l64 = lang.bfloat16().double().requires_grad_(True)
    x0, xjv, lang_raw, lang_t = tan_ref.front_end(v64, l64, p, p_v, p_t, p_j, text_pos)
    dxj = d_xj.double().view(B, L, W)
    loss = (xjv * dxj[:, :T]).sum() + (lang_t * dxj[:, T:]).sum()
    if has_x0:
        loss = loss + (x0 * d_x0.double().view(B, T, W)).sum()
    if has_lang:
        loss = loss + (lang_raw * d_lang_dual.double().view(B, N, W)).sum()
    loss.backward()
    errs = {}
    for n in FRONT:
        if n == "temporal_pos_embed" and pos_enc != "learned":
            continue
        got = f.view(f.grad, n).double() - f.view(g0, n).double()
        want = p[n].grad if p[n].grad is not None else torch.zeros_like(p[n])
        assert torch.isfinite(got).all(), (case, n)
        if want.abs().max().item() == 0:                     # (text table without use_text_pos_enc): untouched, bit for bit
            assert torch.equal(bits(f.view(f.grad, n)), bits(f.view(g0, n))), (case, n)
            continue
        if n.endswith("pos_embed"):                          # rows outside the used slices: untouched
            used = want.abs().amax(-1) > 0
            assert torch.equal(bits(f.view(f.grad, n)[~used]), bits(f.view(g0, n)[~used])), (case, n)
        errs[n] = rel_err(got, want)
    assert d_lang is not None and d_lang.shape == (B, N, Dt)
    errs["d_lang"] = rel_err(d_lang, l64.grad)
    # every other parameter's gradient is untouched by the front end's backward
    for n in f.names:
        if n not in FRONT and f.off[n][1] > 0:
            assert torch.equal(bits(f.view(f.grad, n)), bits(f.view(g0, n))), (case, n)
    print(f"\n[embed bwd e2e] {case}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if e > (F32_REL if k in E2E_F32 else E2E_REL)}
    assert not bad, f"{case}: over {F32_REL} (f32 path) / {E2E_REL}: {bad}"


def test_position_layernorm_cache_follows_an_optimizer_step():
    """the fused forward reads ln_position_init(table) from a cache rebuilt per optimizer step (_pos_ln_full): after one Trainer step
    (AdamW moves the table and ln_position_init) the next fused x0 matches the oracle on the UPDATED parameters, and a stale position
    term would be more than 3x the bound away"""
    from temporalalignnet_amd import synth
    from temporalalignnet_amd.train import Trainer, default_args, to_device_batch
    m = _model("learned", 0, 1024, 512)
    b_np = synth.make_batch(11, B=6, T=32, n_min=3, n_max=9)
    tr = Trainer(m, default_args(model="init", num_encoder_layers=1, num_decoder_layers=1, lr=2e-3, wd=1e-2))
    video = torch.from_numpy(b_np["video"]).cuda()
    lang = torch.from_numpy(b_np["text_embed"]).cuda()
    B, T, _ = video.shape
    m._ensure_flat()
    m._embed_fused(video, lang, None, None, 0, 0, 0, save=False)          # the cache is built for the pre-step parameters
    old = {k: v.clone() for k, v in _ref_params(m).items()}
    tr.step(to_device_batch(b_np))
    m._ensure_flat()
    fe = m._embed_fused(video, lang, None, None, 0, 0, 0, save=False)
    torch.cuda.synchronize()
    new = _ref_params(m)
    v64 = video.bfloat16().double()
    want = tan_ref.video_embedding(v64, new, T, 0)
    e = rel_err(fe["x0"].view(B, T, W), want)
    pos_new = tan_ref.layer_norm(new["temporal_pos_embed"][:T], new, "ln_position_init")
    pos_old = tan_ref.layer_norm(old["temporal_pos_embed"][:T], old, "ln_position_init")
    stale = rel_err(want - pos_new + pos_old, want)
    print(f"\n[embed bwd] x0 after a step: {e:.2e} (a stale position term: {stale:.2e})")
    assert stale > 3 * X0_REL
    assert e <= X0_REL, e
