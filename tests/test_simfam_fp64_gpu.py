"""`tan_simfam_fwd / tan_simfam_bwd` (one feature family of the logits-free NCE, from the stacks' stage outputs to their stage
gradients) through `loss.SimFam`, against float64 autograd of `oracle.loss_ref.nce_family_ref` on the same bf16 stage values.
tests/test_simfam_gpu.py pins the family launches to the separate launches they replaced; both share the sweep, the one-pass d-logits
kernel and the corrections kernel, so an error in shared code cancels there.  Here nothing is shared with the library.

Inputs (`make_case`) are built so that a wrong answer shows: same-video cosines reach above 0.9 (exponentials near e^0, where a badly
rounded kept exponential or a positive read from the wrong column moves a term), cross-video cosines spread over [-0.3, 0.5] (the
row / column sums are not sums of equal terms), row norms are log-uniform over [0.05, 30] (the 1/|x| of the normalisation's backward
is not a constant), one real sentence and several frames have no positive, one video keeps one sentence, one (compaction) keeps none,
and `row_leak` flags frames that hold positives.  Every buffer the library writes starts as the all-ones bit pattern (NaN in f32 and
bf16); the text-gradient accumulator starts as noise unless the case says it is zeroed.  tests/test_simfam_cpu.py shows on the
reference which kernel faults these inputs expose and `randn` features would not.

Bounds.  Checks 1-3 and 5 are derived (see each).  The gradient bounds of check 4 cannot be: bf16 unit rows, kept exponentials,
d logits and the stored gradient are four roundings of 2^-9, the text gradient adds a fifth.  They are set to at most twice the worst
value measured over all cases on MI355X against the fp64 reference, and the tensor bound stays below 5 * 2^-9:

    tensor norm-relative   worst 8.9e-3 (d_text, N = 1), 8.5e-3 (d_video)      bound 5 * 2^-9 = 9.8e-3
    per row                worst 0.153 (T = 621)                               bound 0.3

The tensor error is 4.4e-3 to 8.9e-3 where `randn` features give 2e-3: a frame's d v_hat is nearly parallel to v_hat when its
positives have cosines near 1, the normalisation's backward removes that part, and the bf16 rounding of the d logits is measured
against what is left.  It is largest at N = 1, where a frame has one sentence to be parallel to.

Leaked frames on few videos.  The finishing launch gives a `row_leak` frame its terms by SUBTRACTING its same-video exponentials from
the sweep's row and column sums.  That is exact enough while the other videos' part is above about 1e-4 of the sum.  With one video
nothing is left (the terms are log(0 +- rounding): -inf or NaN), and with two or three videos whose cosines to the frame are all below
-0.4 the rest is 1e-9 of the sum: measured on these inputs, B = 3, T = 43, N = 8 leaked rows miss the reference by 1.70 and
B = 1 / B = 2 give non-finite terms.  include/tan_hip.h states the condition; the `row_leak` cases here have eight or more videos.
"""
import math

import pytest
import torch

from oracle import loss_ref
from test_loss_kernels_gpu import check_terms

pytestmark = pytest.mark.gpu

C = 512
F64 = torch.float64
GRAD_REL = 5 * 2.0 ** -9        # per stage tensor: |got - ref| / |ref|            (measured worst 8.9e-3)
ROW_REL = 0.3                   # per row: |got_r - ref_r| / (|ref_r| + 0.05 rms)  (measured worst 0.153)
TERM_ATOL = 1e-3                # tests/test_loss_kernels_gpu.py: f32 MFMA sums of 512 bf16 products scaled by 1/0.07
DIAG_ATOL = 2 * 512 * 2.0 ** -24        # an f32 sum of 512 bf16 products of unit rows, in any order
INV_REL = (512 / 2 + 4) * 2.0 ** -24    # 1/sqrt of an f32 sum of 512 squares in any order (<= 511 u on the sum, half of it on the root)
                                        # + the roundings of sqrt and the division
_VID3 = ((1.0, 0.0, 0.0), (-0.8, 0.6, 0.0), (0.95, 0.3122, 0.0))      # videos 0..2: cosines -0.8 and 0.95 between their directions


def compaction(tpad_flat, mc_round):
    """`loss.compaction_prep` with a free rounding of Mc: (idx [Mc] sweep column -> padded sentence, colmap [Mp] int32, flags [Mc])."""
    ci = tpad_flat.to(torch.uint8)
    Mp = ci.shape[0]
    n_valid = int((ci == 0).sum())
    Mc = min(Mp, (n_valid + mc_round - 1) // mc_round * mc_round)
    idx = torch.sort(ci, stable=True).indices[:Mc]
    colmap = (torch.cumsum(ci == 0, 0, dtype=torch.int32) - 1).masked_fill(ci != 0, -1)
    return idx, colmap, ci[idx].contiguous()


def make_case(S, B, T, N, fam, compact=False, leak=False, seed=0, mc_round=64, pad="random", randn=False):
    """One family's inputs on the CPU.  fam: 'dual' (St = 1, v_grp (T, 0), t_grp (N, 0)), 'joint' (St = S, frame and sentence rows of
    the same stage buffers: (T+N, 0) / (T+N, T)) or 'slack' (joint with three rows per video no one owns: (T+N+3, 1) / (T+N+3, T+1)).
    The asserts are the properties the module docstring promises; a case that misses one is an error of the case table."""
    g = torch.Generator().manual_seed(1000 + seed)
    R, Mp = B * T, B * N
    rnd = lambda *s: torch.rand(*s, generator=g)
    gau = lambda *s: torch.randn(*s, generator=g)
    # ---- padding
    tpad = torch.zeros(B, N, dtype=torch.bool)
    if N > 1 and pad == "random":
        for b in range(B):
            tpad[b, int(torch.randint(1, N + 1, (1,), generator=g)):] = True
        tpad[0, :N // 2 + 1] = False                              # (video 0 keeps the sentence that gets no positive below)
    elif N > 1:
        tpad[:, N - 1] = True                                     # pad == "last": as few padded sentences as a compaction needs
    if N > 1 and B > 1:
        tpad[B - 1, 1:] = True                                    # a video with every sentence but one padded
    if compact and B >= 3:
        tpad[B - 2, :] = True                                     # a video with every sentence padded
    # ---- targets
    kt = (torch.arange(T) * N) // T                               # the sentence a frame is nearest to
    own = kt[None, :, None] == torch.arange(N)[None, None, :]
    tgt = (rnd(B, T, N) < 0.2) if N == 1 else ((rnd(B, T, N) < 0.12) | (own & (rnd(B, T, N) < 0.7)))
    tgt = tgt.float() * (~tpad)[:, None, :].float()
    if N > 1:
        tgt[0::2, :, N // 2] = 0                                  # a sentence column without any positive
    elif B > 1:
        tgt[0] = 0
    tgt[:, T // 3, :] = 0                                         # frames without any positive
    row_leak = None
    if leak:
        row_leak = torch.zeros(R, dtype=torch.uint8)
        row_leak[max(T - 2, 0):T] = 1
        row_leak[R - 3:] = 1
        row_leak[R // 2] = 1
        hit = (0, T - 1, 0) if N > 1 else (B - 1, T - 1, 0)       # a flagged frame that holds a positive
        assert not tpad[hit[0], hit[2]] and T - 1 != T // 3
        tgt[hit] = 1.0
    # ---- features
    if fam == "dual":
        v_grp, t_grp, St = (T, 0), (N, 0), 1
    elif fam == "joint":
        v_grp, t_grp, St = (T + N, 0), (T + N, T), S
    else:
        v_grp, t_grp, St = (T + N + 3, 1), (T + N + 3, T + 1), S
    zdirs = gau(3, C) / math.sqrt(C)
    m = torch.nn.functional.normalize(gau(B, 3), dim=-1)
    m[:min(B, 3)] = torch.tensor(_VID3)[:min(B, 3)]
    u = m @ zdirs                                                 # [B, C] video directions, |u| ~ 1
    w = gau(B, N, C) / math.sqrt(C)                               # sentence directions

    def rows(s, kind, n_rows_of):
        if randn:
            return gau(B, n_rows_of, C) * (1.0 + 0.3 * s)
        a, c = math.sqrt(0.6 - 0.02 * s), math.sqrt(0.33)
        sig = math.sqrt(0.07 * (1.0 + 0.15 * s))                  # stages differ in their noise, its seed and the mix
        ws_ = w[:, kt] if kind == "v" else w
        x = a * u[:, None, :] + c * ws_ + sig * gau(B, n_rows_of, C) / math.sqrt(C)
        norm = torch.exp(math.log(0.05) + rnd(B, n_rows_of, 1) * (math.log(30.0) - math.log(0.05)))
        return x * norm

    x_video, x_text = [], []
    for s in range(S):
        buf = gau(B, v_grp[0], C)                                 # (slack rows and, in the joint family, padded sentences: finite noise)
        buf[:, v_grp[1]:v_grp[1] + T] = rows(s, "v", T)
        if fam != "dual":
            buf[:, t_grp[1]:t_grp[1] + N] = rows(s, "t", N)
        x_video.append(buf.view(-1, C).to(torch.bfloat16))
    if fam == "dual":
        x_text = [rows(0, "t", N).reshape(-1, C).to(torch.bfloat16)]
    else:
        x_text = x_video
    # ---- compaction, upstream gradients (the size of `nce_term_grads`' mean weights, dense: rows and columns with an empty positive
    # set have a gradient too, through their log-sum-exp over everything; zero on padded and filler columns)
    nv = compaction(tpad.view(-1), mc_round) if compact else None
    keep = ~tpad.view(-1)
    g_v = 0.25 / (S * R) * (0.5 + rnd(S, R))
    g_t_pad = 0.25 / (S * max(int(keep.sum()), 1)) * (0.5 + rnd(S, Mp)) * keep[None].float()
    g_t = g_t_pad[:, nv[0]].contiguous() if nv is not None else g_t_pad
    case = dict(joint=fam != "dual", S=S, St=St, B=B, T=T, N=N, fam=fam, v_grp=v_grp, t_grp=t_grp, x_video=x_video, x_text=x_text, tgt=tgt, tpad=tpad,
                row_leak=row_leak, nv=nv, Mc=nv[0].shape[0] if nv is not None else Mp, g_v=g_v, g_t=g_t, g_t_pad=g_t_pad)
    # ---- the promised properties
    has_row = ((tgt != 0) & keep.view(B, 1, N)).any(-1)
    assert (~has_row).any(), "no frame with an empty positive set"
    has_col = (tgt != 0).any(1).view(-1)
    assert (keep & ~has_col).any(), "no real sentence with an empty positive set"
    if leak:
        assert (has_row.view(-1) & (row_leak != 0)).any(), "no leaked frame holds a positive"
    if compact:
        assert case["Mc"] <= Mp and (B < 3 or tpad[B - 2].all())
    if not randn:
        xv = loss_ref.family_rows(x_video[0].double(), v_grp, T, B)
        xt = loss_ref.family_rows(x_text[0].double(), t_grp, N, B)
        cos = (torch.nn.functional.normalize(xv, dim=-1) @ torch.nn.functional.normalize(xt, dim=-1).t()).view(B, T, B, N)
        same = torch.eye(B, dtype=torch.bool)[:, None, :, None].expand(B, T, B, N)
        real = keep.view(1, 1, B, N).expand(B, T, B, N)
        assert cos[same & real].max().item() > 0.9, cos[same & real].max().item()
        if B >= 3:                                                # (two videos have one cross-video cosine level, one video none)
            cross = cos[~same & real]
            assert cross.min().item() < -0.3 and cross.max().item() > 0.5, (cross.min().item(), cross.max().item())
        nrm = xv.norm(dim=-1)
        assert nrm.min().item() > 0.03 and nrm.max().item() < 40.0 and (R < 64 or nrm.max().item() / nrm.min().item() > 20.0)
    return case


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference side (runs on whatever device the case is on; tests/test_simfam_cpu.py calls it on the CPU)

def reference(case, unit=None, grads=True):
    """fp64 family of `case` (+ autograd of sum(v_terms g_v) + sum(t_terms g_t) towards the bf16 stage buffers when `grads`)."""
    S, St, B, T, N = (case[k] for k in ("S", "St", "B", "T", "N"))
    leaves = [x.double().requires_grad_(grads) for x in case["x_video"]]
    tleaves = leaves if case["x_text"] is case["x_video"] else [x.double().requires_grad_(grads) for x in case["x_text"]]
    ref = loss_ref.nce_family_ref(leaves, case["v_grp"], tleaves, case["t_grp"], case["tgt"], case["tpad"], case["row_leak"], B, T, N,
                                  unit=unit)
    if grads:
        keep = ~case["tpad"].view(-1)
        loss = (ref["v_terms"] * case["g_v"].double()).sum() + (ref["t_terms"] * case["g_t_pad"].double()[:, keep]).sum()
        loss.backward()
        ref["d_video"] = [loss_ref.family_rows(x.grad, case["v_grp"], T, B) for x in leaves]
        ref["d_text"] = [loss_ref.family_rows(x.grad, case["t_grp"], N, B) for x in tleaves]
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in ref.items()}


def grad_errors(got, want):
    """(tensor norm-relative error, worst per-row error) of one stage's gradient rows [n, C] (check 4)."""
    got, want = got.double(), want.double()
    err = (got - want).norm(dim=-1)
    wn = want.norm(dim=-1)
    rms = wn.pow(2).mean().sqrt()
    tensor = (err.norm() / wn.norm().clamp_min(1e-300)).item()
    return tensor, (err / (wn + 0.05 * rms).clamp_min(1e-300)).max().item()


def ulps_bf16(a, b):
    """Distance of two bf16 tensors of the same sign pattern in units of the last place."""
    return (a.contiguous().view(torch.int16).int() - b.contiguous().view(torch.int16).int()).abs()


# ---------------------------------------------------------------------------------------------------------------------------------
# the library side

def _to(case, dev):
    mv = lambda x: x.to(dev) if torch.is_tensor(x) else x
    out = {k: mv(v) for k, v in case.items()}
    out["x_video"] = [x.to(dev) for x in case["x_video"]]
    out["x_text"] = out["x_video"] if case["x_text"] is case["x_video"] else [x.to(dev) for x in case["x_text"]]
    out["nv"] = tuple(x.to(dev) for x in case["nv"]) if case["nv"] is not None else None
    return out


def _nan_like(t):
    t.view(torch.uint8).fill_(0xFF)              # all ones: NaN as f32 and as bf16
    return t


def run_family(case, monkeypatch, mode="one", with_g=True, acc_zeroed=False, norm_in_sweep=True, split_k=0):
    """`case` (on the GPU) through loss.SimFam.  mode 'one': tan_simfam_fwd once; 'two': SWEEP_ONLY then FINISH_ONLY.  with_g: the
    forward gets g_v / g_t and builds the corrections (CORR_DONE), else the backward launches simnce_corr_kernel."""
    from temporalalignnet_amd import _lib, loss as L
    monkeypatch.setattr(L, "_SIMFAM_NORM", bool(norm_in_sweep))
    S, St, B, T, N, Mc = (case[k] for k in ("S", "St", "B", "T", "N", "Mc"))
    R = B * T
    assert L.simfam_ok(S, N, Mc, torch.bfloat16, T)
    d_video = [_nan_like(torch.empty_like(x)) for x in case["x_video"]]
    d_text = d_video if case["joint"] else [_nan_like(torch.empty_like(x)) for x in case["x_text"]]
    ci = case["tpad"].view(-1).to(torch.uint8).contiguous()
    inputs = case["x_video"] + ([] if case["joint"] else case["x_text"]) + [case["tgt"], case["g_v"], case["g_t"]]
    before = [x.clone() for x in inputs]
    fam = L.SimFam(case["x_video"], case["v_grp"], case["x_text"], case["t_grp"], d_video, d_text, case["tgt"], ci, B, T, N,
                   case["nv"], case["g_v"], case["g_t"], split_k, row_leak=case["row_leak"])
    assert fam.d.flags == (1 if norm_in_sweep else 0) and (fam.d.row_leak is not None) == (case["row_leak"] is not None)
    f32, vn, tn, ekeep, dl, ws = fam._keep[:6]
    for t in (f32, vn, tn, ekeep, dl, ws):
        _nan_like(t)
    # the f32 block of SimFam: rowsum, possum_v, inv_v, v_terms [S*R], colsum, possum_t, t_terms [S*Mc], inv_t [St*Mc], acc
    sizes = [S * R] * 4 + [S * Mc] * 3 + [St * Mc, St * Mc * C]
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + (n + 3) // 4 * 4)
    assert offs[-1] == f32.numel() and fam.v_terms.data_ptr() == f32.data_ptr() + 4 * offs[3]
    inv_v, inv_t, acc = f32[offs[2]:offs[2] + sizes[2]], f32[offs[7]:offs[7] + sizes[7]], f32[offs[8]:offs[8] + sizes[8]]
    if acc_zeroed:
        acc.zero_()
        fam.base_flags |= 16                     # TAN_SIMFAM_ACC_ZEROED
    else:
        acc.normal_()                            # whatever the last step left: the library has to clear it
    if mode == "one":
        fam._fwd(0, with_g)
    else:
        fam._fwd(4, False)                       # TAN_SIMFAM_SWEEP_ONLY
        fam._fwd(8, with_g)                      # TAN_SIMFAM_FINISH_ONLY
    assert bool(fam.base_flags & 2) == bool(with_g)      # TAN_SIMFAM_CORR_DONE
    torch.cuda.synchronize()
    lib = _lib.lib()
    diag = []
    for s in range(S):
        off = lib.tan_simfam_diag_offset(S, St, B, T, N, Mc, s)
        diag.append(ws[off:off + 4 * B * T * N].view(torch.float32).view(B, T, N).clone())
    assert torch.equal(diag[-1], fam.diag_last)
    fam.backward()
    torch.cuda.synchronize()
    for x, x0 in zip(inputs, before):            # check 5: the library's inputs are inputs
        assert torch.equal(x.view(torch.uint8), x0.view(torch.uint8))
    return dict(vn=vn, tn=tn, inv_v=inv_v.view(S, R), inv_t=inv_t.view(St, Mc), v_terms=fam.v_terms, t_terms=fam.t_terms,
                diag=torch.stack(diag), d_video=d_video, d_text=d_text, fam=fam)


def check_family(case, out, figures=None):
    """Checks 1-5 of one run against the fp64 reference."""
    S, St, B, T, N, Mc = (case[k] for k in ("S", "St", "B", "T", "N", "Mc"))
    R, Mp = B * T, B * N
    dev = out["vn"].device
    nv, tpad, keep = case["nv"], case["tpad"], ~case["tpad"].view(-1)
    idx = nv[0] if nv is not None else torch.arange(Mp, device=dev)
    flags = nv[2] if nv is not None else tpad.view(-1).to(torch.uint8)
    ref = reference(case)
    # 1. unit rows: the kernel's f32 norm may move a value across a bf16 rounding boundary of the fp64 one, it may not move it further.
    #    Every sweep column c holds the unit row of padded sentence idx[c], filler columns (flagged) included.
    assert ulps_bf16(out["vn"], ref["vn"].to(torch.bfloat16)).max().item() <= 1
    assert ulps_bf16(out["tn"], ref["tn"][:, idx].to(torch.bfloat16)).max().item() <= 1
    assert ((out["inv_v"].double() - ref["inv_v"]).abs() <= INV_REL * ref["inv_v"]).all()
    assert ((out["inv_t"].double() - ref["inv_t"][:, idx]).abs() <= INV_REL * ref["inv_t"][:, idx]).all()
    # 2. terms: the reference on the kernel's OWN unit rows (the bf16 rounding of the features is check 1's business), so what is left
    #    is the f32 arithmetic of the sweep and the finishing launch
    tn_full = torch.zeros(St, Mp, C, dtype=torch.bfloat16, device=dev)
    real_c = flags == 0
    tn_full[:, idx[real_c]] = out["tn"][:, real_c]
    if nv is None:
        tn_full = out["tn"]
    own = reference(case, unit=(out["vn"], tn_full), grads=False)
    assert torch.isfinite(out["v_terms"]).all() and torch.isfinite(out["t_terms"]).all()          # (filler columns too)
    check_terms(out["v_terms"], out["t_terms"], own["v_terms"], own["t_terms"], case["tgt"], tpad, case["row_leak"],
                col_of=idx if nv is not None else None, atol=TERM_ATOL)
    # 3. same-video cosine blocks of EVERY stage (the stage-2 losses read the last one, the corrections all of them): entries of real
    #    sentences; of padded ones too when the sweep is not compacted (with compaction they have no sweep column and are undefined)
    blocks = own["cos"].view(S, B, T, B, N)[:, torch.arange(B), :, torch.arange(B)].permute(1, 0, 2, 3)     # [S,B,T,N]
    derr = (out["diag"].double() - blocks).abs()
    if nv is not None:
        derr = derr.permute(0, 2, 1, 3).reshape(S, T, Mp)[:, :, keep]
    assert derr.max().item() <= DIAG_ATOL, derr.max().item()
    # 4. stage gradients against fp64 autograd through the WHOLE reference, normalisation included
    worst_t, worst_r = 0.0, 0.0
    for name, grp, G in (("d_video", case["v_grp"], T), ("d_text", case["t_grp"], N)):
        for s, buf in enumerate(out[name]):
            got = loss_ref.family_rows(buf, grp, G, B)
            assert torch.isfinite(got).all(), (name, s)
            et, er = grad_errors(got, ref[name][s])
            if figures is not None:
                figures.append((name, s, et, er))
            worst_t, worst_r = max(worst_t, et), max(worst_r, er)
            assert et <= GRAD_REL, (name, s, et)
            assert er <= ROW_REL, (name, s, er)
    # 5. exact: dropped (padded) sentences take part in nothing; rows outside the family's addressing keep their bit pattern
    for s, buf in enumerate(out["d_text"]):
        got = loss_ref.family_rows(buf, case["t_grp"], N, B)
        assert (got[tpad.view(-1)] == 0).all(), s
        assert (ref["d_text"][s][tpad.view(-1)] == 0).all()
    grp_rows = case["v_grp"][0]
    owned = torch.zeros(grp_rows, dtype=torch.bool, device=dev)
    owned[case["v_grp"][1]:case["v_grp"][1] + T] = True
    if case["joint"]:
        owned[case["t_grp"][1]:case["t_grp"][1] + N] = True
    for buf in out["d_video"]:
        rest = buf.view(B, grp_rows, C)[:, ~owned]
        assert (rest.contiguous().view(torch.int16) == -1).all()
    return worst_t, worst_r


D = dict(S=3, B=8, T=64, N=16, fam="dual", compact=True)
J = dict(S=3, B=8, T=64, N=16, fam="joint", compact=True)


def K(S, B, T, N, fam, **kw):
    return dict(S=S, B=B, T=T, N=N, fam=fam, **kw)


CASES = [
    # ---- the six shapes of tests/test_simfam_gpu.py
    ("dual-compact", D),                                              # dual family, compacted columns (filler blocks: nfill = 1)
    ("joint-compact", J),                                             # joint: R = 512, tan_gemm_atb with two K slices
    ("joint-40cols", K(1, 8, 24, 5, "joint")),                        # Mc = B*N = 40, R = 192: R % 128 != 0 -> fall-back to tan_gemm
    ("dual-144cols", K(2, 16, 64, 9, "dual")),                        # no compaction, Mc = 144
    ("joint-T256", K(2, 8, 256, 24, "joint", compact=True)),          # T = 256: eight 32-frame units per wave in the finishing launch
    ("joint-bench", K(6, 128, 64, 16, "joint", compact=True)),        # the benchmarked size, row_leak NULL
    ("joint-bench-leak", K(6, 128, 64, 16, "joint", compact=True, leak=True)),      # ... and set
    ("dual-bench-leak", K(6, 128, 64, 16, "dual", compact=True, leak=True)),        # dual at that size: 8 K slices of tan_gemm
    # ---- stages
    ("dual-S1", K(1, 8, 16, 5, "dual")),                              # S = 1; S*R = 128: one K slice
    ("dual-S8", K(8, 8, 16, 5, "dual", leak=True)),                   # S = 8, the most the descriptor holds
    ("joint-S8-R128", K(8, 8, 16, 5, "joint", compact=True, mc_round=8)),   # R = 128 < two slices of 128: tan_gemm_atb refused -> tan_gemm
    ("slack-S6-R128", K(6, 8, 16, 5, "slack")),                       # v_grp_rows > T + N: slack rows stay untouched
    # ---- sentences per video
    ("dual-N1", K(2, 8, 20, 1, "dual")),                              # N = 1, Mc = 8
    ("joint-N1", K(2, 16, 20, 1, "joint", leak=True)),
    ("dual-N32", K(2, 4, 40, 32, "dual", compact=True)),              # N = 32: the correction arrays' limit
    ("joint-N32", K(2, 4, 40, 32, "joint", leak=True)),
    # ---- sweep columns
    ("dual-Mc8", K(2, 1, 50, 8, "dual")),                             # Mc = 8, B = 1: one 32-column block, mostly repeats of the last column
    ("joint-Mc8", K(2, 1, 50, 8, "joint")),
    ("joint-filler-ragged", K(3, 24, 20, 16, "joint", compact=True, mc_round=8, leak=True)),   # Mc % 128 != 0, filler block of simfam_finish_kernel
    ("dual-filler-2blocks", K(2, 40, 12, 16, "dual", compact=True)),    # Mc > 256 and % 128 != 0: two filler blocks (nfill = 2)
    ("dual-maxcols", K(1, 256, 3, 32, "dual")),                       # Mc = tan_simnce_max_cols() without compaction
    ("joint-maxcols-compact", K(1, 265, 3, 32, "joint", compact=True, pad="last")),   # 8480 padded columns compacted to the limit
    # ---- rows
    ("dual-T3", K(2, 16, 3, 8, "dual")),                              # T = 3: below one wave's rows; R = 48 < one panel
    ("joint-T3", K(2, 16, 3, 8, "joint", leak=True)),
    ("dual-R129", K(2, 3, 43, 8, "dual")),                            # B*T = 129: one row in the second 128-row panel
    ("joint-R129", K(3, 3, 43, 8, "joint", compact=True, mc_round=8)),    # ... joint: R % 128 != 0 -> tan_gemm
    ("slack-R129", K(2, 3, 43, 8, "slack")),
    ("dual-T621", K(1, 2, 621, 32, "dual")),                          # the largest [T, N] block the finishing launch holds (160 KB of LDS)
    ("joint-T621", K(2, 2, 621, 32, "joint")),
    # ---- flags, on one dual and one joint shape
    ("dual-norm-launch", dict(D, norm_in_sweep=False)),               # TAN_SIMFAM_NORM_IN_SWEEP off: tan_l2norm_fwd_multi in front
    ("joint-norm-launch", dict(J, norm_in_sweep=False, leak=True)),
    ("dual-two-calls", dict(D, mode="two", leak=True)),               # SWEEP_ONLY then FINISH_ONLY
    ("joint-two-calls", dict(J, mode="two")),
    ("dual-no-g", dict(D, with_g=False, leak=True)),                  # forward without g_v / g_t: the backward launches simnce_corr_kernel
    ("joint-no-g", dict(J, with_g=False)),
    ("joint-two-calls-no-g", dict(J, mode="two", with_g=False, leak=True)),         # the stage-2 step's order of calls
    ("dual-acc-zeroed", dict(D, with_g=False, acc_zeroed=True)),      # ACC_ZEROED: simnce_corr_kernel gets no accumulator to clear
    ("joint-acc-zeroed", dict(J, with_g=False, acc_zeroed=True, leak=True)),
    ("joint-acc-zeroed-g", dict(J, acc_zeroed=True)),                 # ... with the corrections built by the forward
    ("dual-leak", dict(D, leak=True)),                                # row_leak set on the default flags
    ("joint-leak", dict(J, leak=True)),
    ("slack-leak", K(3, 8, 64, 16, "slack", compact=True, leak=True)),
    # ---- the text-gradient GEMM
    ("dual-split3", dict(D, split_k=3)),                              # tan_gemm, three K slices
    ("dual-atb1", dict(D, split_k=-1)),                               # tan_gemm_atb over S*R = 1536 rows, one slice
    ("dual-atb3", dict(D, split_k=-3, leak=True)),                    # ... three slices
    ("joint-split3", dict(J, split_k=3, leak=True)),                  # batched tan_gemm, three slices per stage
    ("joint-atb1", dict(J, split_k=-1)),
    ("joint-atb3", dict(J, split_k=-3)),
    ("joint-ragged-atb3", K(2, 3, 43, 8, "joint", split_k=-3)),       # R = 129: tan_gemm_atb asked for, refused -> tan_gemm
]


@pytest.mark.parametrize("name,spec", CASES, ids=[c[0] for c in CASES])
def test_family_matches_fp64_autograd(name, spec, monkeypatch):
    spec = dict(spec)
    run_kw = {k: spec.pop(k) for k in ("mode", "with_g", "acc_zeroed", "norm_in_sweep", "split_k") if k in spec}
    from temporalalignnet_amd import _lib
    case = _to(make_case(seed=len(name) + 7 * spec["S"] + spec["T"], **spec), "cuda")
    if "maxcols" in name:
        assert case["Mc"] == _lib.lib().tan_simnce_max_cols()
    if "filler" in name:
        assert case["Mc"] % 128 != 0 and case["Mc"] < case["B"] * case["N"] and bool(case["nv"][2].any())
    out = run_family(case, monkeypatch, **run_kw)
    fig = []
    try:
        check_family(case, out, fig)
    finally:
        if fig:
            print(f"\n[simfam-fp64] {name}: tensor {max(f[2] for f in fig):.3e} row {max(f[3] for f in fig):.3e} "
                  f"(d_video {max(f[2] for f in fig if f[0] == 'd_video'):.3e} d_text {max(f[2] for f in fig if f[0] == 'd_text'):.3e})")


def _same_forward(a, b):
    # vn / tn / norms / the same-video blocks / column sums and t_terms come from fixed-order sums: bit-equal between call patterns.
    # Each row sum meets in FOUR f32 atomic adds (two column groups x two column waves of simnce_res_kernel) whose order is free, and
    # v_terms is its logarithm: 4 f32 ulps of the sum, as an absolute error of the log, plus the rounding of the term itself.
    for k in ("vn", "tn"):
        assert torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)), k
    for k in ("inv_v", "inv_t", "t_terms", "diag"):
        assert torch.equal(a[k], b[k]), k
    assert ((a["v_terms"] - b["v_terms"]).abs() <= 4 * 2.0 ** -23 * (1 + a["v_terms"].abs())).all()


@pytest.mark.parametrize("spec", [dict(D, leak=True), J], ids=["dual", "joint"])
def test_call_patterns_agree(spec, monkeypatch):
    """Check 6: one call against SWEEP_ONLY + FINISH_ONLY, forward with g_v / g_t against without (each is checked against fp64 in the
    table above): the same forward results, gradients within the bound each has against the reference."""
    case = _to(make_case(seed=61, **spec), "cuda")
    base = run_family(case, monkeypatch)
    ref = reference(case)
    for kw in (dict(mode="two"), dict(with_g=False), dict(mode="two", with_g=False, acc_zeroed=True)):
        other = run_family(case, monkeypatch, **kw)
        _same_forward(base, other)
        for name, grp, G in (("d_video", case["v_grp"], case["T"]), ("d_text", case["t_grp"], case["N"])):
            for s in range(len(base[name])):
                a, b = (loss_ref.family_rows(o[name][s], grp, G, case["B"]) for o in (base, other))
                et, er = grad_errors(a, b)
                assert et <= GRAD_REL and er <= ROW_REL, (kw, name, s, et, er)
                assert grad_errors(b, ref[name][s])[0] <= GRAD_REL


@pytest.mark.parametrize("spec", [D, dict(J, leak=True)], ids=["dual", "joint"])
def test_split_k_variants_agree(spec, monkeypatch):
    """Check 7: the K slicing of the text-gradient GEMM moves d_text by f32 summation order only and d_video not at all."""
    case = _to(make_case(seed=67, **spec), "cuda")
    ref = reference(case)
    runs = [run_family(case, monkeypatch, split_k=k) for k in (0, 3, -1, -3)]
    for o in runs:
        for s in range(len(o["d_text"])):
            got = loss_ref.family_rows(o["d_text"][s], case["t_grp"], case["N"], case["B"])
            et, er = grad_errors(got, ref["d_text"][s])
            assert et <= GRAD_REL and er <= ROW_REL, (s, et, er)
        for s in range(case["S"]):
            a, b = (loss_ref.family_rows(x["d_video"][s], case["v_grp"], case["T"], case["B"]) for x in (runs[0], o))
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), s


def _fresh(spec, monkeypatch):
    """A SimFam over NaN-pattern outputs that has not run; every rejection below changes one descriptor field of it."""
    from temporalalignnet_amd import loss as L
    monkeypatch.setattr(L, "_SIMFAM_NORM", True)
    case = _to(make_case(seed=71, **spec), "cuda")
    S, St, B, T, N = (case[k] for k in ("S", "St", "B", "T", "N"))
    d_video = [_nan_like(torch.empty_like(x)) for x in case["x_video"]]
    d_text = d_video if case["joint"] else [_nan_like(torch.empty_like(x)) for x in case["x_text"]]
    fam = L.SimFam(case["x_video"], case["v_grp"], case["x_text"], case["t_grp"], d_video, d_text, case["tgt"],
                   case["tpad"].view(-1).to(torch.uint8).contiguous(), B, T, N, case["nv"], case["g_v"], case["g_t"])
    outs = list(fam._keep[:6]) + d_video + ([] if case["joint"] else d_text)
    for t in outs:
        _nan_like(t)
    return fam, outs


def _untouched(outs):
    torch.cuda.synchronize()
    return all(bool((t.view(torch.uint8) == 0xFF).all()) for t in outs)


SMALL = K(2, 4, 16, 8, "dual", compact=True, mc_round=8)
SMALL_FULL = K(2, 4, 16, 8, "dual")


@pytest.mark.parametrize("what", ["S9", "N33", "Mc%8", "Mc>max", "idx-no-colmap", "Mc!=B*N", "ws-align", "g_v-no-g_t", "both-only",
                                  "bwd-no-dl", "T622"])
def test_rejections_come_before_any_launch(what, monkeypatch):
    """Check 8: every limit of include/tan_hip.h is a host check in front of the first launch: TAN_ERR_BAD_ARG, and no byte of the
    NaN-pattern outputs changes.  (Nothing here reaches a kernel: each call is expected to return before launching.)"""
    from temporalalignnet_amd import _lib
    spec = K(1, 1, 622, 32, "dual") if what == "T622" else (SMALL_FULL if what == "Mc!=B*N" else SMALL)
    fam, outs = _fresh(spec, monkeypatch)
    d = fam.d
    call = lambda: fam._fwd(0, True)
    if what == "S9":
        d.S = 9
    elif what == "N33":
        d.N = 33
    elif what == "Mc%8":
        d.Mc = d.Mc + 4
    elif what == "Mc>max":
        d.Mc = _lib.lib().tan_simnce_max_cols() + 8
    elif what == "idx-no-colmap":
        d.colmap = None
    elif what == "Mc!=B*N":
        assert d.idx is None
        d.Mc = d.Mc - 8
    elif what == "ws-align":
        d.ws = d.ws + 16
    elif what == "g_v-no-g_t":
        def call():
            d.flags = fam.base_flags
            d.g_v, d.g_t = fam.g_v.data_ptr(), None
            _lib.check(_lib.lib().tan_simfam_fwd(_byref(d), _stream()), "tan_simfam_fwd")
    elif what == "both-only":
        call = lambda: fam._fwd(4 | 8, False)
    elif what == "bwd-no-dl":
        d.dl = None
        call = fam.backward
    elif what == "T622":
        # 261 * T + 1584 bytes of LDS at N = 32: T = 621 fits the CU's 160 KB (the table above runs it), T = 622 does not.  The buffers
        # ARE those of T = 622, so the refusal is not what keeps the launches in bounds
        assert 261 * 621 + 1584 <= 160 * 1024 < 261 * 622 + 1584
    with pytest.raises(_lib.TanHipError, match="bad argument"):
        call()
    assert _untouched(outs)


def _byref(d):
    import ctypes
    return ctypes.byref(d)


def _stream():
    from temporalalignnet_amd import ops
    return ops._stream()
