"""The fused input embeddings' forward (csrc/tan_embed.hip: tan_embed_fwd) through the C ABI against a float64 chain on what the kernel
reads, with NO intermediate rounding: bf16-rounded a and the bf16 W upcast, f32 LayerNorm parameters and position rows upcast;
projection, LayerNorm, + pos, block 0's ln_1.  Every bf16 and f32 output is compared norm-relative per tensor (a_bf16, the RNE cast, and
pad_dst exactly); mean / rstd / mean1 / rstd1 against the float64 statistics of that chain.  Every output starts as NaN and pad_dst as
the byte 7, so an unwritten row shows; the rows of a joint buffer no problem owns (out_grp_rows > T + out_off, or the other modality's
rows when a problem runs alone) and a guard region behind every buffer must come back untouched.

The layout is the engine's (_embed_fused): video rows -> out[0] = x0 [B, T] and out[1] = rows 0 .. T - 1 of the joint xj [B, L];
text rows -> out[0] = lang_raw [B, N] (no position term, no ln_1) and out[1] = rows T .. T + N - 1 of xj; one joint xn1 / mean1 /
rstd1 and one joint key-padding mask [B, L].  L = T + N + gap.

Which branch each case reaches (one workgroup owns 32 rows; LDS holds [32][max K] bf16, at least the [32][512] result panel):

  rows = B T in {1, 31, 32, 33, 97}   a partial only workgroup, one row short, exact, one row over, three full + one row; T = 1
  (Kv, Kt) = (128, 128)               the smallest K: two rounds of the 4-deep weight prefetch; LDS sized by the result panel
             (1024, 768)              the benchmark's video width and the BERT width; unequal K
             (2048, 128), (128, 2048) the limit (128 KiB of LDS) in either problem: the other problem indexes its panel with its own pitch
  a f32 / bf16                        the cast in the kernel (a_bf16 written) / rows copied as they are
  training / inference form           a_bf16, proj, mean, rstd given / NULL (engine._embed_fused save=False): the other outputs bit-equal
  pad_dst NULL; pad_src NULL          no mask / zeros written
  nprob = 1                           each modality alone
  out[0] NULL; pos NULL; xn1 NULL     each optional piece off with the rest on
  (128, 64, 13, 1024, 512)            the benchmark's shape
  rejections                          -1 and nothing written"""
import pytest
import torch

from test_panel_gpu import pack

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
CW, EPS, GUARD = 512, 1e-5, 1024

# Norm-relative bounds, ||got - ref|| / ||ref|| per tensor over the rows a problem writes: twice the worst measured on MI355X over every
# case of this file, against the float64 chain.  Cap for each: 0.0115.  (B, T, N, Kv, Kt) of the case in brackets.
BOUNDS = {
    "proj": 3.5e-3,      # worst 1.75e-3 (video, (1, 1, 1, 128, 128)): the bf16 rounding of proj
    "mean": 6.8e-3,      # worst 3.37e-3 (video, (2, 16, 3, 128, 128)): the mean of the 512 bf16-rounded proj values
    "rstd": 3.6e-4,      # worst 1.77e-4 (text, (1, 31, 5, 128, 128))
    "out": 4.8e-3,       # worst 2.35e-3 (text out[0], (1, 31, 5, 128, 128)): bf16 proj through the LayerNorm, bf16 out
    "xn1": 5.7e-3,       # worst 2.82e-3 (video xn1[0], pos NULL, (2, 33, 40, 128, 1024)): the same through a second LayerNorm
    "mean1": 1.4e-3,     # worst 6.62e-4 (video mean1[0], (97, 1, 1, 128, 128))
    "rstd1": 3.3e-4,     # worst 1.62e-4 (video rstd1[1], (3, 11, 2, 128, 128))
}


def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def rel_err(got, ref):
    got, ref = got.to(F64).reshape(-1), ref.to(F64).reshape(-1)
    den = ref.norm().item()
    return (got - ref).norm().item() / den if den > 0 else got.norm().item()


class Buf:
    """an output of `rows` x `width` that starts as NaN (uint8: the byte 7) with a guard region behind it"""

    def __init__(self, rows, width, dtype):
        fill = 7 if dtype == torch.uint8 else float("nan")
        self.rows, self.width = rows, width
        self.full = torch.full((rows * width + GUARD,), fill, dtype=dtype, device="cuda")
        self.t = self.full[:rows * width].view(rows, width) if width > 1 else self.full[:rows]
        self.before = self.full.clone()
        self.written = torch.zeros(rows, dtype=torch.bool, device="cuda")      # rows some problem is expected to write

    def ptr(self):
        return self.full.data_ptr()

    def check_untouched_rest(self, what):
        n = self.rows * self.width
        assert torch.equal(bits(self.full[n:]), bits(self.before[n:])), f"{what}: the guard region was written"
        rest = ~self.written
        if bool(rest.any()):
            assert torch.equal(bits(self.t[rest]), bits(self.before[:n].view(self.t.shape)[rest])), f"{what}: rows no problem owns were written"

    def untouched(self):
        return torch.equal(bits(self.full), bits(self.before))


def stats(x):
    m = x.mean(-1, keepdim=True)
    r = torch.rsqrt(((x - m) ** 2).mean(-1, keepdim=True) + EPS)
    return m, r


def ln(x, g, b):
    m, r = stats(x)
    return (x - m) * r * g.double() + b.double(), m[:, 0], r[:, 0]


class Case:
    """Inputs, buffers and descriptors of one launch.  which: "vt" | "v" | "t"; save: the training form; pad: "src" (pad_src and
    pad_dst) | "zeros" (pad_dst only) | None; out0 / pos / xn1: False switches that piece off in every problem; gap: unowned rows at the
    end of every video's slice of the joint buffers."""

    def __init__(self, B, T, N, Kv, Kt, a_dtype=F32, *, which="vt", save=True, pad="src", out0=True, pos=True, xn1=True, gap=0, seed=0):
        g = torch.Generator(device="cuda").manual_seed(seed * 7919 + B * 1000 + T * 10 + N)
        rn = lambda *s: torch.randn(*s, generator=g, device="cuda")      # noqa: E731
        self.B, self.T, self.N, self.L = B, T, N, T + N + gap
        self.which, self.save, self.pad, self.has_out0, self.has_pos, self.has_xn1, self.a_dtype = which, save, pad, out0, pos, xn1, a_dtype
        L, R, Mp = self.L, B * T, B * N
        self.a = {"v": (rn(R, Kv).abs() * 0.3).to(a_dtype), "t": rn(Mp, Kt).to(a_dtype)}
        self.W = {"v": (rn(CW, Kv) * Kv ** -0.5).bfloat16(), "t": (rn(CW, Kt) * Kt ** -0.5).bfloat16()}
        self.pw = dict(zip("vt", pack([self.W["v"], self.W["t"]])))
        # LayerNorm biases around 0.25, not 0: the mean over the features of a LayerNorm output is the mean of its bias (+ ~0.01), and
        # the stored mean1 carries the absolute rounding noise of 512 bf16 values, ~2^-9 / sqrt(512) ~ 1e-4.  Against a mean that cancels
        # to ~0.01 a norm-relative figure measures the cancellation (1e-2), not the kernel.
        self.par = {k: (1 + 0.2 * rn(CW)) if k.endswith("g") else 0.25 + 0.2 * rn(CW)
                    for k in ("v_g", "v_b", "t_g", "t_b", "l1v_g", "l1v_b", "l1j_g", "l1j_b")}
        self.posrows = {"v0": rn(T, CW), "v1": rn(T, CW), "t1": rn(N, CW)}
        self.pad_src = {"v": (torch.rand(R, generator=g, device="cuda") < 0.3).to(torch.uint8),
                        "t": (torch.rand(Mp, generator=g, device="cuda") < 0.3).to(torch.uint8)}
        b = self.buf = {}
        b["a16_v"], b["a16_t"] = Buf(R, Kv, BF16), Buf(Mp, Kt, BF16)
        b["proj_v"], b["proj_t"] = Buf(R, CW, BF16), Buf(Mp, CW, BF16)
        for k, n in (("mean_v", R), ("rstd_v", R), ("mean_t", Mp), ("rstd_t", Mp), ("m1v", R), ("r1v", R), ("m1j", B * L), ("r1j", B * L)):
            b[k] = Buf(n, 1, F32)
        b["x0"], b["xj"], b["lang_raw"] = Buf(R, CW, BF16), Buf(B * L, CW, BF16), Buf(Mp, CW, BF16)
        b["xn1_v"], b["xn1_j"] = Buf(R, CW, BF16), Buf(B * L, CW, BF16)
        b["keypad"] = Buf(B * L, 1, torch.uint8)
        self.K = {"v": Kv, "t": Kt}
        self.Tn = {"v": T, "t": N}
        self.off1 = {"v": 0, "t": T}

    def jrows(self, m):
        """the rows of the joint buffers modality m owns"""
        Tn = self.Tn[m]
        return (torch.arange(self.B, device="cuda")[:, None] * self.L + self.off1[m] + torch.arange(Tn, device="cuda")[None, :]).reshape(-1)

    def fill(self, d, m):
        from temporalalignnet_amd import _lib
        b, p = self.buf, lambda t: t.data_ptr()        # noqa: E731
        rows, Tn = self.a[m].shape[0], self.Tn[m]
        d.a, d.a_dtype, d.rows, d.K, d.T, d.C = p(self.a[m]), (_lib.TAN_F32 if self.a_dtype == F32 else _lib.TAN_BF16), rows, self.K[m], Tn, CW
        d.pw, d.ln_g, d.ln_b = p(self.pw[m]), p(self.par[m + "_g"]), p(self.par[m + "_b"])
        if self.save:
            d.a_bf16 = b["a16_" + m].ptr() if self.a_dtype == F32 else None
            d.proj, d.mean, d.rstd = b["proj_" + m].ptr(), b["mean_" + m].ptr(), b["rstd_" + m].ptr()
        if self.has_out0:
            d.out[0], d.out_grp_rows[0], d.out_off[0] = b["x0" if m == "v" else "lang_raw"].ptr(), Tn, 0
            if m == "v":
                d.pos[0] = p(self.posrows["v0"]) if self.has_pos else None
                if self.has_xn1:
                    d.ln1_g[0], d.ln1_b[0] = p(self.par["l1v_g"]), p(self.par["l1v_b"])
                    d.xn1[0], d.mean1[0], d.rstd1[0] = b["xn1_v"].ptr(), b["m1v"].ptr(), b["r1v"].ptr()
        d.out[1], d.out_grp_rows[1], d.out_off[1] = b["xj"].ptr(), self.L, self.off1[m]
        d.pos[1] = p(self.posrows[m + "1"]) if self.has_pos else None
        if self.has_xn1:
            d.ln1_g[1], d.ln1_b[1] = p(self.par["l1j_g"]), p(self.par["l1j_b"])
            d.xn1[1], d.mean1[1], d.rstd1[1] = b["xn1_j"].ptr(), b["m1j"].ptr(), b["r1j"].ptr()
        if self.pad is not None:
            d.pad_src = p(self.pad_src[m]) if self.pad == "src" else None
            d.pad_dst, d.pad_grp_rows, d.pad_off = b["keypad"].ptr(), self.L, self.off1[m]

    def descs(self):
        from temporalalignnet_amd import _lib
        D = (_lib.EmbedDesc * 3)()
        for i, m in enumerate(self.which):
            self.fill(D[i], m)
        return D

    def run(self):
        from temporalalignnet_amd import _lib, ops
        _lib.check(_lib.lib().tan_embed_fwd(self.descs(), len(self.which), ops._stream()), "tan_embed_fwd")
        torch.cuda.synchronize()
        return self

    def reference(self, m):
        """the float64 chain of modality m: {tensor: value over the rows the problem writes}"""
        a16 = self.a[m].bfloat16().double()
        proj = a16 @ self.W[m].double().t()
        y, mean, rstd = ln(proj, self.par[m + "_g"], self.par[m + "_b"])
        Tn, B = self.Tn[m], self.B
        ref = {"a_bf16": a16, "proj": proj, "mean": mean, "rstd": rstd}
        for d, pk, l1 in ((0, "v0" if m == "v" else None, "l1v"), (1, m + "1", "l1j")):
            pos = self.posrows[pk].double() if (pk is not None and self.has_pos) else None
            o = y if pos is None else (y.view(B, Tn, CW) + pos).view(-1, CW)
            ref[f"out{d}"] = o
            ref[f"xn1{d}"], ref[f"mean1{d}"], ref[f"rstd1{d}"] = ln(o, self.par[l1 + "_g"], self.par[l1 + "_b"])
        return ref

    def check(self, tag, errs):
        b = self.buf
        got = {}
        for m in self.which:
            ref = self.reference(m)
            jr = self.jrows(m)
            if self.save:
                if self.a_dtype == F32:
                    b["a16_" + m].written[:] = True
                    assert torch.equal(bits(b["a16_" + m].t), bits(self.a[m].bfloat16())), f"{tag}: {m} a_bf16 is not the RNE cast"
                for k in ("proj", "mean", "rstd"):
                    b[f"{k}_{m}"].written[:] = True
                    got[f"{m}.{k}"] = (b[f"{k}_{m}"].t, ref[k], k)
            if self.has_out0:
                o0 = b["x0" if m == "v" else "lang_raw"]
                o0.written[:] = True
                got[f"{m}.out0"] = (o0.t, ref["out0"], "out")
                if m == "v" and self.has_xn1:
                    for k, name in (("xn1", "xn1_v"), ("mean1", "m1v"), ("rstd1", "r1v")):
                        b[name].written[:] = True
                        got[f"{m}.{k}0"] = (b[name].t, ref[k + "0"], k)
            b["xj"].written[jr] = True
            got[f"{m}.out1"] = (b["xj"].t[jr], ref["out1"], "out")
            if self.has_xn1:
                for k, name in (("xn1", "xn1_j"), ("mean1", "m1j"), ("rstd1", "r1j")):
                    b[name].written[jr] = True
                    got[f"{m}.{k}1"] = (b[name].t[jr], ref[k + "1"], k)
            if self.pad is not None:
                b["keypad"].written[jr] = True
                want = self.pad_src[m] if self.pad == "src" else torch.zeros_like(self.pad_src[m])
                assert torch.equal(b["keypad"].t[jr], want), f"{tag}: {m} pad_dst"
        for name, buf in b.items():
            buf.check_untouched_rest(f"{tag}: {name}")
        bad = {}
        for k, (t, r, kind) in got.items():
            assert t.shape == r.shape, (tag, k, t.shape, r.shape)
            assert bool(torch.isfinite(t.float()).all()), f"{tag}: {k} has NaN / inf (an unwritten row?)"
            e = rel_err(t, r)
            errs[f"{tag} {k}"] = (e, kind)
            if not e <= BOUNDS[kind]:
                bad[k] = e
        return bad


def _report(errs):
    worst = {}
    for k, (e, kind) in errs.items():
        if e >= worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (e, k)
    print("\n[embed fwd fp64] " + "; ".join(f"{kind} {e:.3e} ({k})" for kind, (e, k) in sorted(worst.items())))


KEEP = ("x0", "xj", "lang_raw", "xn1_v", "xn1_j", "m1v", "r1v", "m1j", "r1j", "keypad")

SHAPES = [  # B, T, N, Kv, Kt, a dtype
    (1, 1, 1, 128, 128, F32), (1, 31, 5, 128, 128, F32), (2, 16, 3, 128, 128, F32), (3, 11, 2, 128, 128, F32), (97, 1, 1, 128, 128, F32),
    (3, 11, 5, 128, 128, BF16), (3, 16, 5, 1024, 768, F32), (3, 16, 5, 1024, 768, BF16), (4, 16, 5, 2048, 128, F32), (4, 5, 16, 128, 2048, F32),
    (4, 16, 16, 2048, 2048, BF16), (128, 64, 13, 1024, 512, F32),
]


@pytest.mark.parametrize("B,T,N,Kv,Kt,a_dtype", SHAPES)
def test_training_and_inference_forms_match_fp64(B, T, N, Kv, Kt, a_dtype):
    errs = {}
    train = Case(B, T, N, Kv, Kt, a_dtype, save=True).run()
    bad = train.check("train", errs)
    infer = Case(B, T, N, Kv, Kt, a_dtype, save=False).run()
    bad |= infer.check("infer", errs)
    _report(errs)
    for k in ("a16_v", "a16_t", "proj_v", "proj_t", "mean_v", "rstd_v", "mean_t", "rstd_t"):
        assert infer.buf[k].untouched(), f"inference form wrote {k}"
    for k in KEEP:
        assert torch.equal(bits(train.buf[k].full), bits(infer.buf[k].full)), f"{k} differs between the training and the inference form"
    assert not bad, f"over the bound: {bad}"


VARIANTS = {
    "pad_dst_null": dict(pad=None),
    "pad_src_null": dict(pad="zeros"),
    "video_alone": dict(which="v"),
    "text_alone": dict(which="t"),
    "video_alone_inference": dict(which="v", save=False, pad=None),
    "out0_null": dict(out0=False),
    "pos_null": dict(pos=False),
    "xn1_null": dict(xn1=False),
    "gap_rows": dict(gap=3),
    "gap_rows_text_alone": dict(gap=2, which="t", pad="zeros"),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("B,T,N,Kv,Kt", [(3, 11, 5, 256, 128), (2, 33, 40, 128, 1024)])
def test_optional_pieces(B, T, N, Kv, Kt, variant):
    errs = {}
    c = Case(B, T, N, Kv, Kt, F32, seed=1, **VARIANTS[variant]).run()
    bad = c.check(variant, errs)
    _report(errs)
    # what a launch writes does not depend on what else it is asked for (the position term and the zero mask aside)
    full = Case(B, T, N, Kv, Kt, F32, seed=1, gap=VARIANTS[variant].get("gap", 0)).run()
    for k in KEEP:
        w = c.buf[k].written
        if bool(w.any()) and variant != "pos_null" and not (k == "keypad" and c.pad == "zeros"):
            assert torch.equal(bits(c.buf[k].t[w]), bits(full.buf[k].t[w])), (variant, k)
    assert not bad, f"over the bound: {bad}"


def test_wrong_position_row_would_show():
    """the bound on out tells pos[0] from pos[1]: the reference with the other offset's rows is far outside it"""
    c = Case(3, 11, 5, 128, 128, F32, seed=2)
    ref = c.reference("v")
    wrong = ref["out1"] - c.posrows["v1"].double().repeat(3, 1) + c.posrows["v0"].double().repeat(3, 1)
    assert rel_err(wrong, ref["out1"]) > 10 * 0.0115


def test_rejections_write_nothing():
    from temporalalignnet_amd import _lib, ops
    L, st = _lib.lib(), ops._stream()
    c = Case(2, 4, 3, 128, 128, F32, seed=3, gap=1)

    def refused(nprob=2, prob=0, **kw):
        D = c.descs()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(D[prob], k)[v[0]] = v[1]
            else:
                setattr(D[prob], k, v)
        rc = L.tan_embed_fwd(D, nprob, st)
        assert rc == -1, (nprob, prob, kw, rc)
    for prob in (0, 1):
        for K in (64, 192, 2176, 0, -128):
            refused(prob=prob, K=K)
        refused(prob=prob, C=256)
        refused(prob=prob, rows=0)
        refused(prob=prob, rows=-4)
        refused(prob=prob, T=0)
        refused(prob=prob, T=-1)
        refused(prob=prob, out_grp_rows=(1, c.Tn["vt"[prob]] + c.off1["vt"[prob]] - 1))
        refused(prob=prob, out_grp_rows=(0, c.Tn["vt"[prob]] - 1))
        refused(prob=prob, out=(1, None))                       # xn1[1] without out[1]
        refused(prob=prob, ln1_g=(1, None))
        refused(prob=prob, ln1_b=(1, None))
        refused(prob=prob, mean1=(1, None))
        refused(prob=prob, rstd1=(1, None))
        refused(prob=prob, a=None)
        refused(prob=prob, pw=None)
        refused(prob=prob, ln_g=None)
        refused(prob=prob, ln_b=None)
    refused(nprob=0)
    refused(nprob=3)
    refused(nprob=-1)
    assert L.tan_embed_fwd(None, 1, st) == -1
    torch.cuda.synchronize()
    for name, buf in c.buf.items():
        assert buf.untouched(), f"{name} was written by a refused call"
    # the accepted edge: out_grp_rows == T + out_off (the text rows end the joint slice when gap = 0)
    errs = {}
    ok = Case(2, 4, 3, 128, 128, F32, seed=3).run()
    assert not ok.check("edge", errs)
