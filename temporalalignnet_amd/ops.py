"""Thin torch-tensor -> C-ABI wrappers (device pointers, sizes, current HIP stream).

PyTorch is plumbing here: it owns the device memory and the stream; every arithmetic op is a
hand-written HIP kernel in libtan_hip.so.  All wrappers require CUDA(HIP) tensors and raise otherwise.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._lib import ACT_NONE, ACT_QUICKGELU, ACT_QUICKGELU_GRAD, ACT_RELU, TAN_BF16, TAN_F32  # noqa: F401


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return TAN_F32
    if t.dtype == torch.bfloat16:
        return TAN_BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.TanHipError("HIP path needs device tensors (no CPU fallback)")
    return C.c_void_p(t.data_ptr())


def _stream():
    # the raw handle of torch's CURRENT stream on the current device; the public torch.cuda.current_stream() builds a Stream
    # object through three Python layers (~3 us) and this is called once per launch (~120 times per training step)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def gemm_atb(As, Bs, Cs, *, lda, M, N, K, accumulate=False, split=1):
    """C_p [M_p, N_p] (=|+=) A_p^T B_p for up to eight problems (lists of tensors; A_p [K, lda_p], B_p [K, N_p] bf16 row-major, C_p f32
    or bf16): tan_gemm_atb, the 256 x 256-tile kernel.  lda / M / N: ints (the same for every problem) or lists."""
    if len(As) > 8:                                    # the kernel takes eight problems per launch
        sl = lambda v, a, b: v if isinstance(v, int) else v[a:b]                        # noqa: E731
        for a in range(0, len(As), 8):
            gemm_atb(As[a:a + 8], Bs[a:a + 8], Cs[a:a + 8], lda=sl(lda, a, a + 8), M=sl(M, a, a + 8), N=sl(N, a, a + 8), K=K,
                     accumulate=accumulate, split=split)
        return
    n = len(As)
    ints = lambda v: (C.c_int * n)(*([v] * n if isinstance(v, int) else v))          # noqa: E731
    ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])                    # noqa: E731
    _lib.check(_lib.lib().tan_gemm_atb(n, ptrs(As), ptrs(Bs), ptrs(Cs), ints(lda), ints(M), ints(N), K, _dt(Cs[0]), int(accumulate),
                                       split, _stream()), "tan_gemm_atb")


def gemm(A, B, C_out, *, M, N, K, a_kc=True, b_kc=True, lda=None, ldb=None, ldc=None, bias=None, residual=None,
         ldr=None, act=ACT_NONE, aux=None, ldaux=None, accumulate=False, split_k=1, alpha=1.0, batch=1,
         sA=0, sB=0, sC=0, colsum=None):
    """C[M,N] (=|+=) alpha * opA(A) @ opB(B) (+bias)(act)(+residual); see include/tan_hip.h:tan_gemm."""
    d = _lib.GemmDesc()
    d.dtype, d.out_dtype = _dt(A), _dt(C_out)
    assert _dt(B) == d.dtype
    d.M, d.N, d.K = M, N, K
    d.a_kc, d.b_kc = int(a_kc), int(b_kc)
    d.A, d.lda = _ptr(A), lda if lda is not None else (K if a_kc else M)
    d.B, d.ldb = _ptr(B), ldb if ldb is not None else (K if b_kc else N)
    d.C, d.ldc = _ptr(C_out), ldc if ldc is not None else N
    d.bias = _ptr(bias)
    d.residual, d.ldr = _ptr(residual), ldr if ldr is not None else N
    d.act = act
    d.aux, d.ldaux = _ptr(aux), ldaux if ldaux is not None else N
    d.accumulate, d.split_k, d.alpha = int(accumulate), split_k, alpha
    d.batch, d.sA, d.sB, d.sC = batch, sA, sB, sC
    d.colsum = _ptr(colsum)
    _lib.check(_lib.lib().tan_gemm(C.byref(d), _stream()), "tan_gemm")
    return C_out


def _f32(t):
    assert t is None or t.dtype == torch.float32
    return _ptr(t)


_ln_ws = {}


def _ws_f32(n, device):
    # one workspace per (device, stream): two LayerNorm backwards issued on different streams must not share their partial tables
    key = (device, "ln", torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0)
    buf = _ln_ws.get(key)
    if buf is None or buf.numel() < n:
        buf = torch.empty(n, device=device, dtype=torch.float32)
        _ln_ws[key] = buf
    return buf


def layernorm_fwd(x, gamma, beta, y, mean=None, rstd=None, add=None, add_period=0, eps=1e-5):
    rows, Cc = x.numel() // x.shape[-1], x.shape[-1]
    _lib.check(_lib.lib().tan_layernorm_fwd(_ptr(x), _f32(gamma), _f32(beta), _ptr(y), _f32(mean), _f32(rstd), _ptr(add),
                                             C.c_int(add_period), C.c_long(rows), C.c_int(Cc), C.c_float(eps), _dt(x),
                                             _stream()), "tan_layernorm_fwd")
    return y


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma=None, dbeta=None, dres=None, dx_colsum=None):
    rows, Cc = x.numel() // x.shape[-1], x.shape[-1]
    L = _lib.lib()
    ws = _ws_f32(L.tan_layernorm_bwd_ws_floats(C.c_int(Cc)), x.device)
    _lib.check(L.tan_layernorm_bwd(_ptr(dy), _ptr(x), _f32(gamma), _f32(mean), _f32(rstd), _ptr(dres), _ptr(dx),
                                   _f32(dgamma), _f32(dbeta), _f32(dx_colsum), _ptr(ws), C.c_long(rows), C.c_int(Cc), _dt(x),
                                   _stream()),
               "tan_layernorm_bwd")
    return dx


def l2norm_fwd(x, y, inv_norm, rows, Cc, grp=None, src_grp_rows=None, src_off=0):
    grp = grp or rows
    _lib.check(_lib.lib().tan_l2norm_fwd(_ptr(x), _ptr(y), _f32(inv_norm), C.c_long(rows), C.c_int(Cc), C.c_int(grp),
                                          C.c_int(src_grp_rows if src_grp_rows is not None else grp), C.c_int(src_off),
                                          _dt(x), _stream()), "tan_l2norm_fwd")
    return y


def l2norm_bwd(dy, y, inv_norm, dx, rows, Cc, grp=None, dst_grp_rows=None, dst_off=0):
    grp = grp or rows
    _lib.check(_lib.lib().tan_l2norm_bwd(_ptr(dy), _ptr(y), _f32(inv_norm), _ptr(dx), C.c_long(rows), C.c_int(Cc),
                                          C.c_int(grp), C.c_int(dst_grp_rows if dst_grp_rows is not None else grp),
                                          C.c_int(dst_off), _dt(y), _stream()), "tan_l2norm_bwd")
    return dx


def _ptr8(tensors):
    if not 1 <= len(tensors) <= 8:
        raise ValueError(f"1..8 stage buffers, got {len(tensors)}")
    t = _lib.Ptr8()
    for i, x in enumerate(tensors):
        t.p[i] = x.data_ptr()
    return t


def l2norm_fwd_multi(xs, y, inv_norm, rows, Cc, grp=None, src_grp_rows=None, src_off=0):
    """all stages of one feature family in one launch: xs = list of per-stage buffers, y [S, rows, C], inv_norm [S * rows] or None"""
    grp = rows if grp is None else grp
    if len(xs) > 8:          # the C entry point takes up to 8 stage pointers: deeper stacks go in groups of 8
        for s0 in range(0, len(xs), 8):
            l2norm_fwd_multi(xs[s0:s0 + 8], y[s0:s0 + 8], None if inv_norm is None else inv_norm[s0 * rows:(s0 + 8) * rows],
                             rows, Cc, grp, src_grp_rows, src_off)
        return y
    t = _ptr8(xs)
    _lib.check(_lib.lib().tan_l2norm_fwd_multi(C.byref(t), _ptr(y), _f32(inv_norm), C.c_int(len(xs)), C.c_long(rows), C.c_int(Cc),
                                                C.c_int(grp), C.c_int(src_grp_rows if src_grp_rows is not None else grp),
                                                C.c_int(src_off), _dt(y), _stream()), "tan_l2norm_fwd_multi")
    return y


def l2norm_bwd_multi(dy, y, inv_norm, dxs, rows, Cc, grp=None, dst_grp_rows=None, dst_off=0):
    grp = rows if grp is None else grp
    if len(dxs) > 8:
        for s0 in range(0, len(dxs), 8):
            l2norm_bwd_multi(dy[s0:s0 + 8], y[s0:s0 + 8], inv_norm[s0 * rows:(s0 + 8) * rows], dxs[s0:s0 + 8], rows, Cc, grp,
                             dst_grp_rows, dst_off)
        return
    t = _ptr8(dxs)
    _lib.check(_lib.lib().tan_l2norm_bwd_multi(_ptr(dy), _ptr(y), _f32(inv_norm), C.byref(t), C.c_int(len(dxs)), C.c_long(rows),
                                                C.c_int(Cc), C.c_int(grp), C.c_int(dst_grp_rows if dst_grp_rows is not None else grp),
                                                C.c_int(dst_off), _dt(y), _stream()), "tan_l2norm_bwd_multi")



def colsum_acc(x, out, rows, Cc):
    _lib.check(_lib.lib().tan_colsum_acc(_ptr(x), _f32(out), C.c_long(rows), C.c_int(Cc), _dt(x), _stream()), "tan_colsum_acc")
    return out


def reduce_add(parts, out, nparts, n):
    """out[n] (f32) += sum_p parts[p][n] -- folds split-K partial tiles."""
    assert parts.dtype == torch.float32 and out.dtype == torch.float32 and parts.is_contiguous() and out.is_contiguous()
    _lib.check(_lib.lib().tan_reduce_add(_f32(parts), _f32(out), C.c_int(nparts), C.c_long(n), _stream()), "tan_reduce_add")
    return out


def rows_copy(src, dst, G, R, Cc, src_grp_rows, src_off, dst_grp_rows, dst_off, accumulate=False):
    assert _dt(src) == _dt(dst)
    _lib.check(_lib.lib().tan_rows_copy(_ptr(src), _ptr(dst), C.c_int(G), C.c_int(R), C.c_int(Cc), C.c_long(src_grp_rows),
                                         C.c_long(src_off), C.c_long(dst_grp_rows), C.c_long(dst_off), C.c_int(int(accumulate)),
                                         _dt(src), _stream()), "tan_rows_copy")
    return dst


def group_sum(x, out, G, R, Cc):
    _lib.check(_lib.lib().tan_group_sum(_ptr(x), _ptr(out), C.c_int(G), C.c_int(R), C.c_int(Cc), _dt(x), _stream()),
               "tan_group_sum")
    return out


def cast(src, dst):
    assert src.numel() == dst.numel()
    _lib.check(_lib.lib().tan_cast(_ptr(src), _dt(src), _ptr(dst), _dt(dst), C.c_long(src.numel()), _stream()), "tan_cast")
    return dst


def head_fwd(x, w, b, out, rows, Cc):
    _lib.check(_lib.lib().tan_head_fwd(_ptr(x), _f32(w), _f32(b), _f32(out), C.c_long(rows), C.c_int(Cc), _dt(x), _stream()),
               "tan_head_fwd")
    return out


def head_bwd(dout, x, w, dx, dw, db, rows, Cc, accumulate_dx=False):
    _lib.check(_lib.lib().tan_head_bwd(_f32(dout), _ptr(x), _f32(w), _ptr(dx), _f32(dw), _f32(db), C.c_long(rows), C.c_int(Cc),
                                        C.c_int(int(accumulate_dx)), _dt(x), _stream()), "tan_head_bwd")
    return dx


def interp_linear(src, dst, L_in, L_out, Cc):
    _lib.check(_lib.lib().tan_interp_linear(_f32(src), _f32(dst), C.c_int(L_in), C.c_int(L_out), C.c_int(Cc), _stream()),
               "tan_interp_linear")
    return dst


def interp_linear_bwd(ddst, dsrc, L_in, L_out, Cc):
    _lib.check(_lib.lib().tan_interp_linear_bwd(_f32(ddst), _f32(dsrc), C.c_int(L_in), C.c_int(L_out), C.c_int(Cc), _stream()),
               "tan_interp_linear_bwd")
    return dsrc


def attn_fwd(qkv, keypad_u8, o, lse, B, L, H):
    _lib.check(_lib.lib().tan_attn_fwd(_ptr(qkv), _ptr(keypad_u8), _ptr(o), _f32(lse), C.c_int(B), C.c_int(L), C.c_int(H),
                                        _dt(qkv), _stream()), "tan_attn_fwd")
    return o


def attn_bwd(qkv, keypad_u8, o, lse, d_o, dqkv, B, L, H, g_b_qkv=None):
    """g_b_qkv [3C] f32: += the column sums of dqkv (in_proj bias gradient), by the same call."""
    if g_b_qkv is not None:
        _lib.check(_lib.lib().tan_attn_bwd_bias(_ptr(qkv), _ptr(keypad_u8), _ptr(o), _f32(lse), _ptr(d_o), _ptr(dqkv),
                                                 _f32(g_b_qkv), C.c_int(B), C.c_int(L), C.c_int(H), _dt(qkv), _stream()),
                   "tan_attn_bwd_bias")
        return dqkv
    _lib.check(_lib.lib().tan_attn_bwd(_ptr(qkv), _ptr(keypad_u8), _ptr(o), _f32(lse), _ptr(d_o), _ptr(dqkv), C.c_int(B),
                                        C.c_int(L), C.c_int(H), _dt(qkv), _stream()), "tan_attn_bwd")
    return dqkv


def _elem_bytes(t):
    if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"unsupported dtype {t.dtype}")
    return t.element_size()


def window_pack(video, text, table, T, Kp, out_video, vmask, out_text, tmask):
    """One pass's `eval_windows` input from the chunk's packed features (tan_window_pack): video [sum vlen, Dv], text [sum K, Dt]
    (f32 / f16 / bf16), table [W, 8] int32 -> out_video [W, T, Dv], vmask [W, T] bool, out_text [W, Kp, Dt], tmask [W, Kp] bool."""
    W = table.shape[0]
    assert table.dtype == torch.int32 and table.is_contiguous() and video.is_contiguous() and text.is_contiguous()
    assert out_video.dtype == video.dtype and out_text.dtype == text.dtype and vmask.dtype == tmask.dtype == torch.bool
    assert out_video.shape == (W, T, video.shape[-1]) and out_text.shape == (W, Kp, text.shape[-1])
    assert vmask.shape == (W, T) and tmask.shape == (W, Kp)
    _lib.check(_lib.lib().tan_window_pack(_ptr(video), _elem_bytes(video), video.shape[-1], _ptr(text), _elem_bytes(text),
                                          text.shape[-1], _ptr(table), W, T, Kp, _ptr(out_video), _ptr(vmask), _ptr(out_text),
                                          _ptr(tmask), _stream()), "tan_window_pack")


def window_pack_fresh(video, text, table, T, Kp):
    """`window_pack` into four fresh outputs on video's device, which it returns: (out_video, vmask, out_text, tmask)"""
    W, dev = table.shape[0], video.device
    out = (torch.empty(W, T, video.shape[-1], dtype=video.dtype, device=dev), torch.empty(W, T, dtype=torch.bool, device=dev),
           torch.empty(W, Kp, text.shape[-1], dtype=text.dtype, device=dev), torch.empty(W, Kp, dtype=torch.bool, device=dev))
    window_pack(video, text, table, T, Kp, *out)
    return out


def window_stitch_acc(sim_j, sim_d, a_joint, table, acc_j, acc_d, cnt, tcnt, a_sum):
    """acc_j / acc_d / cnt [sum K*vlen], tcnt / a_sum [sum K] += one pass (tan_window_stitch_acc); sim_j / sim_d [W, T, Kp] f32 (one
    stage of eval_windows' output, read in place), a_joint [W, Kp] f32 or None (no alignability head: a_sum is None too)."""
    W, T, Kp = sim_j.shape
    assert sim_j.is_contiguous() and sim_d.is_contiguous() and sim_d.shape == sim_j.shape and table.shape == (W, 8)
    assert a_joint is None or (a_joint.is_contiguous() and a_joint.shape == (W, Kp))
    _lib.check(_lib.lib().tan_window_stitch_acc(_f32(sim_j), _f32(sim_d), _f32(a_joint), _ptr(table), W, T, Kp, _f32(acc_j),
                                                _f32(acc_d), _f32(cnt), acc_j.numel(), _f32(tcnt), _f32(a_sum), tcnt.numel(),
                                                _stream()), "tan_window_stitch_acc")


def window_stitch_final(acc_j, acc_d, cnt, tcnt, a_sum, rows, res):
    """acc_j <- the stitched rows in place; res [4, sum K] f32 <- arg-max, softmax max, score, covered (tan_window_stitch_final).
    rows [sum K, 2] int32: each sentence's accumulator offset and vlen."""
    n = tcnt.numel()
    assert rows.dtype == torch.int32 and rows.shape == (n, 2) and res.shape == (4, n)
    _lib.check(_lib.lib().tan_window_stitch_final(_f32(acc_j), _f32(acc_d), _f32(cnt), _f32(tcnt), _f32(a_sum), _ptr(rows), n,
                                                  acc_j.numel(), _f32(res), _stream()), "tan_window_stitch_final")


def monotonic_decode(sim, rows, order, vtab, keep, bp, run, ts, path):
    """ts [sum K] int32 <- per video the non-decreasing seconds with the largest summed similarity over its kept rows, -1 for the
    rows not kept; path [n_videos] f32 <- the path's score (tan_monotonic_decode).  sim [sum K*vlen] f32: the stitched rows; rows
    [sum K, 2] int32 as for window_stitch_final; order [sum K] int32: packed row ids, each video's contiguous and in decode order;
    vtab [n_videos, 3] int32 = (first index into order, count, offset of the video's row in run); keep [sum K] bool / uint8 or None
    = every row.  Scratch: bp [sim.numel()] int32, run [>= sum vlen] f32."""
    n = rows.shape[0]
    assert rows.dtype == torch.int32 and rows.shape == (n, 2) and rows.is_contiguous() and sim.is_contiguous()
    assert order.dtype == torch.int32 and order.shape == (n,) and order.is_contiguous()
    assert vtab.dtype == torch.int32 and vtab.dim() == 2 and vtab.shape[1] == 3 and vtab.is_contiguous()
    assert keep is None or (keep.dtype in (torch.bool, torch.uint8) and keep.shape == (n,) and keep.is_contiguous())
    assert bp.dtype == torch.int32 and bp.numel() == sim.numel() and bp.is_contiguous() and run.is_contiguous()
    assert ts.dtype == torch.int32 and ts.shape == (n,) and ts.is_contiguous() and path.shape == (vtab.shape[0],)
    _lib.check(_lib.lib().tan_monotonic_decode(_f32(sim), _ptr(rows), _ptr(order), _ptr(vtab), vtab.shape[0], _ptr(keep), n,
                                               sim.numel(), run.numel(), _ptr(bp), _f32(run), _ptr(ts), _f32(path), _stream()),
               "tan_monotonic_decode")


def segment_decode(sim, rows, order, vtab, keep, bias, bp, run, seg, path):
    """seg [sum K, 2] int32 <- per video the ordered, disjoint inclusive intervals (s, e) with the largest summed gain
    sim[r][t] - bias[r] over its kept rows, (-1, -1) for the rows not kept; path [n_videos] f32 <- the path's score, -inf for a video
    with more kept rows than seconds (tan_segment_decode).  sim, rows, order, vtab, keep: as for monotonic_decode; bias [sum K] f32.
    Scratch: bp [2 * sim.numel()] int32, run [>= sum vlen] f32."""
    n = rows.shape[0]
    assert rows.dtype == torch.int32 and rows.shape == (n, 2) and rows.is_contiguous() and sim.is_contiguous()
    assert order.dtype == torch.int32 and order.shape == (n,) and order.is_contiguous()
    assert vtab.dtype == torch.int32 and vtab.dim() == 2 and vtab.shape[1] == 3 and vtab.is_contiguous()
    assert keep is None or (keep.dtype in (torch.bool, torch.uint8) and keep.shape == (n,) and keep.is_contiguous())
    assert bias.dtype == torch.float32 and bias.shape == (n,) and bias.is_contiguous()
    assert bp.dtype == torch.int32 and bp.numel() == 2 * sim.numel() and bp.is_contiguous() and run.is_contiguous()
    assert seg.dtype == torch.int32 and seg.shape == (n, 2) and seg.is_contiguous() and path.shape == (vtab.shape[0],)
    _lib.check(_lib.lib().tan_segment_decode(_f32(sim), _ptr(rows), _ptr(order), _ptr(vtab), vtab.shape[0], _ptr(keep), _f32(bias),
                                             n, sim.numel(), run.numel(), _ptr(bp), _f32(run), _ptr(seg), _f32(path), _stream()),
               "tan_segment_decode")


def _bytes(name):
    """ops.<name>(*sizes) = tan_<name>(*sizes): a scratch buffer's or a filter image's bytes; TanHipError for sizes the library refuses"""
    def ask(*sizes):
        n = getattr(_lib.lib(), f"tan_{name}")(*sizes)
        if n < 0:
            raise _lib.TanHipError(f"tan_{name}({', '.join(str(a) for a in sizes)}): bad argument")
        return n
    ask.__name__ = name
    return ask


rank_topk_ws_bytes = _bytes("rank_topk_ws_bytes")                    # (Q, N, k)
rank_topk_video_ws_bytes = _bytes("rank_topk_video_ws_bytes")        # (Q, N, n_videos, k)
row_filter_bytes = _bytes("row_filter_bytes")                        # (N)
label_runs_ws_bytes = _bytes("label_runs_ws_bytes")                  # (N)
label_decode_ws_bytes = _bytes("label_decode_ws_bytes")              # (N, k)
local_align_ws_bytes = _bytes("local_align_ws_bytes")                # (P, sum_V)
local_align_path_ws_bytes = _bytes("local_align_path_ws_bytes")      # (P, sum_V, n_trace)
sequence_topk_ws_bytes = _bytes("sequence_topk_ws_bytes")            # (n_seq, N, k)
clip_topk_ws_bytes = _bytes("clip_topk_ws_bytes")                    # (n_clip, N, k)
compound_topk_ws_bytes = _bytes("compound_topk_ws_bytes")            # (n_query, N, k)


def _rows_args(what, tq, vn, q_scale, v_scale):
    """The one check of a wrapper's row arguments: tq [Q, 512] / vn [N, 512] contiguous and of one dtype; uint8 rows are e4m3 codes
    and come with their f32 scales q_scale [Q] / v_scale [N], any other rows without.  Returns whether the rows are e4m3."""
    assert tq.dim() == 2 and vn.dim() == 2 and tq.is_contiguous() and vn.is_contiguous() and tq.dtype == vn.dtype
    e4m3 = tq.dtype == torch.uint8
    if (q_scale is not None) != e4m3 or (v_scale is not None) != e4m3:
        raise TypeError(f"{what}: q_scale / v_scale go with uint8 e4m3 codes, and only with them")
    if e4m3:
        assert q_scale.shape == (tq.shape[0],) and v_scale.shape == (vn.shape[0],) and q_scale.is_contiguous() and v_scale.is_contiguous()
    return e4m3


def _call(name, tq, q_scale, vn, v_scale, *tail):
    """tan_<name>(tq, vn, dtype, *tail, stream) or, with scales, its twin tan_<name>_e4m3(tq, q_scale, vn, v_scale, *tail, stream)"""
    L = _lib.lib()
    if q_scale is not None:
        _lib.check(getattr(L, f"tan_{name}_e4m3")(_ptr(tq), _f32(q_scale), _ptr(vn), _f32(v_scale), *tail, _stream()), f"tan_{name}_e4m3")
    else:
        _lib.check(getattr(L, f"tan_{name}")(_ptr(tq), _ptr(vn), _dt(tq), *tail, _stream()), f"tan_{name}")


def _scratch(ws, need, dev, refuse=None, contiguous=True):
    """`ws`, or fresh scratch of `need` bytes (a tan_*_ws_bytes answer); need < 0: invalid sizes, which the entry point itself refuses
    (`ws` stays as it came, None included).  refuse: the ValueError text of the wrappers that answer bad scratch by an exception of
    their own (contiguous=False: `label_runs` never asked for contiguous scratch); without it the sweeps' assertion."""
    if need >= 0:
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        if refuse is None:
            assert ws.dtype == torch.uint8 and ws.numel() >= need
        elif ws.dtype != torch.uint8 or ws.numel() < need or (contiguous and not ws.is_contiguous()):
            raise ValueError(refuse)
    return ws


def _lists(n, k, dev, video=False):
    """fresh top-k outputs: (score f32, row int32[, video int32]), [n, k] each"""
    return (torch.empty(n, k, dtype=torch.float32, device=dev),) + tuple(torch.empty(n, k, dtype=torch.int32, device=dev)
                                                                         for _ in range(2 if video else 1))


def _rank_topk(what, tq, q_scale, vn, v_scale, pair, k, splits, check_pair, out, ws):
    _rows_args(what, tq, vn, q_scale, v_scale)
    Q, N, dev = tq.shape[0], vn.shape[0], tq.device
    if pair is not None:
        assert pair.dtype == torch.int32 and pair.shape == (Q,) and pair.is_contiguous()
        if check_pair and Q and (int(pair.min()) < 0 or int(pair.max()) >= N):
            raise ValueError(f"{what}: pair outside [0, N)")
    if out is None:
        higher, ties = (torch.empty(Q, dtype=torch.int32, device=dev) for _ in range(2)) if pair is not None else (None, None)
        top_s, top_r = _lists(Q, k, dev) if k > 0 else (None, None)
    else:
        higher, ties, top_s, top_r = out
    ws = _scratch(ws, _lib.lib().tan_rank_topk_ws_bytes(Q, N, k), dev)
    _call("rank_topk", tq, q_scale, vn, v_scale, Q, N, tq.shape[1], _ptr(pair), k, splits, _ptr(higher), _ptr(ties), _ptr(top_s),
          _ptr(top_r), _ptr(ws))
    return higher, ties, top_s, top_r


def rank_topk(tq, vn, pair=None, k=0, *, splits=0, check_pair=False, out=None, ws=None):
    """Matrix-free rank / top-k of scores = tq @ vn.T (tan_rank_topk): tq [Q, 512], vn [N, 512], both bf16 or both f32, contiguous.
    pair [Q] int32 (device) or None.  Returns (higher [Q] int32, ties [Q] int32, top_score [Q, k] f32, top_row [Q, k] int32); the
    pieces that were not asked for (no pair / k == 0) are None.  splits: 0 = automatic; the result does not depend on it.
    check_pair: verify pair in [0, N) on the host (one synchronisation); otherwise that is the caller's contract.
    out / ws: caller-owned outputs (the same 4-tuple) and scratch (uint8, >= rank_topk_ws_bytes) instead of fresh ones."""
    return _rank_topk("rank_topk", tq, None, vn, None, pair, k, splits, check_pair, out, ws)


def quantize_rows_e4m3(x, codes=None, scale=None):
    """x [n, 512] (f32 / bf16, contiguous) -> (codes uint8 [n, 512]: OCP e4m3fn bit patterns, scale f32 [n]: a power of two per row),
    the row format of include/tan_hip.h (tan_quantize_rows_e4m3).  codes / scale: caller-owned outputs instead of fresh ones."""
    assert x.dim() == 2 and x.is_contiguous()
    n, dev = x.shape[0], x.device
    codes = torch.empty(n, x.shape[1], dtype=torch.uint8, device=dev) if codes is None else codes
    scale = torch.empty(n, dtype=torch.float32, device=dev) if scale is None else scale
    assert codes.dtype == torch.uint8 and codes.shape == x.shape and codes.is_contiguous() and scale.shape == (n,) and scale.is_contiguous()
    _lib.check(_lib.lib().tan_quantize_rows_e4m3(_ptr(x), _dt(x), n, x.shape[1], _ptr(codes), _f32(scale), _stream()),
               "tan_quantize_rows_e4m3")
    return codes, scale


def rank_topk_e4m3(tq, q_scale, vn, v_scale, pair=None, k=0, *, splits=0, check_pair=False, out=None, ws=None):
    """`rank_topk` over e4m3 rows (tan_rank_topk_e4m3): tq [Q, 512] / vn [N, 512] uint8 codes with their f32 row scales q_scale [Q] /
    v_scale [N], as `quantize_rows_e4m3` makes them; score = (acc * v_scale[n]) * q_scale[q].  Everything else as `rank_topk`."""
    assert tq.dtype == torch.uint8
    return _rank_topk("rank_topk_e4m3", tq, q_scale, vn, v_scale, pair, k, splits, check_pair, out, ws)


def quantize_rows_mxfp4(x, codes=None, scales=None):
    """x [n, 512] (f32 / bf16, contiguous) -> (codes uint8 [n, 256]: two e2m1 codes per byte, scales uint8 [n, 16]: one e8m0 byte per
    block of 32 elements), the coarse row format of include/tan_hip.h (tan_quantize_rows_mxfp4).  codes / scales: caller-owned
    outputs instead of fresh ones."""
    assert x.dim() == 2 and x.is_contiguous()
    n, dev = x.shape[0], x.device
    codes = torch.empty(n, x.shape[1] // 2, dtype=torch.uint8, device=dev) if codes is None else codes
    scales = torch.empty(n, x.shape[1] // 32, dtype=torch.uint8, device=dev) if scales is None else scales
    assert codes.dtype == torch.uint8 and codes.shape == (n, x.shape[1] // 2) and codes.is_contiguous()
    assert scales.dtype == torch.uint8 and scales.shape == (n, x.shape[1] // 32) and scales.is_contiguous()
    _lib.check(_lib.lib().tan_quantize_rows_mxfp4(_ptr(x), _dt(x), n, x.shape[1], _ptr(codes), _ptr(scales), _stream()),
               "tan_quantize_rows_mxfp4")
    return codes, scales


def rank_topk_mxfp4(tq, q_scale, codes, scales, k, *, splits=0, below=None, out=None, ws=None):
    """The k best rows per query of a coarse image (tan_rank_topk_mxfp4): tq [Q, 512] uint8 e4m3 codes with q_scale [Q] f32, as
    `quantize_rows_e4m3` makes them; codes [N, 256] / scales [N, 16] uint8, as `quantize_rows_mxfp4` makes them.  Returns
    (top_score [Q, k] f32, top_row [Q, k] int32) by descending coarse score, equal scores by ascending row.
    below = (score [Q] f32, row [Q] int32): only rows strictly after that entry in this order are admitted (row -1: every row at an
    equal score, 0x7fffffff: none); with fewer than k of them the tail holds empty slots (-inf, 0x7fffffff).
    out / ws: caller-owned outputs (the same pair) and scratch (uint8, >= tan_rank_topk_mxfp4_ws_bytes) instead of fresh ones."""
    assert tq.dim() == 2 and tq.dtype == torch.uint8 and tq.is_contiguous()
    Q, N, dev = tq.shape[0], codes.shape[0], tq.device
    assert q_scale.dtype == torch.float32 and q_scale.shape == (Q,) and q_scale.is_contiguous()
    assert codes.dtype == torch.uint8 and codes.shape == (N, tq.shape[1] // 2) and codes.is_contiguous()
    assert scales.dtype == torch.uint8 and scales.shape == (N, tq.shape[1] // 32) and scales.is_contiguous()
    b_score, b_row = (None, None) if below is None else below
    if below is not None:
        assert b_score.dtype == torch.float32 and b_row.dtype == torch.int32 and b_score.shape == b_row.shape == (Q,)
        assert b_score.is_contiguous() and b_row.is_contiguous()
    top_s, top_r = _lists(Q, k, dev) if out is None else out
    ws = _scratch(ws, _lib.lib().tan_rank_topk_mxfp4_ws_bytes(Q, N, k), dev)
    _lib.check(_lib.lib().tan_rank_topk_mxfp4(_ptr(tq), _f32(q_scale), _ptr(codes), _ptr(scales), Q, N, tq.shape[1], k, splits,
                                              _f32(b_score), _ptr(b_row), _f32(top_s), _ptr(top_r), _ptr(ws), _stream()),
               "tan_rank_topk_mxfp4")
    return top_s, top_r


def _video_args(what, tq, vn, v_off, q_scale, v_scale):
    assert v_off.dtype == torch.int32 and v_off.dim() == 1 and v_off.numel() >= 2 and v_off.is_contiguous()
    return _rows_args(what, tq, vn, q_scale, v_scale)


def rank_topk_video(tq, vn, v_off, k, *, q_scale=None, v_scale=None, splits=0, check_v_off=False, out=None, ws=None):
    """The k best DISTINCT videos per query (tan_rank_topk_video / _e4m3): tq [Q, 512], vn [N, 512], both bf16, both f32, or both
    uint8 e4m3 codes with q_scale [Q] / v_scale [N]; v_off [n_videos + 1] int32 (device): each video's first row, then N.
    Returns (top_score [Q, k] f32: the video's best score, top_row [Q, k] int32: the first index row that attains it,
    top_video [Q, k] int32), by descending score, equal scores by ascending row.  splits: 0 = automatic; the result does not depend
    on it.  check_v_off: verify on the host (one synchronisation) that v_off starts at 0, ends at N and strictly increases;
    otherwise that is the caller's contract.  out / ws: caller-owned outputs (the same 3-tuple) and scratch (uint8,
    >= rank_topk_video_ws_bytes) instead of fresh ones."""
    _video_args("rank_topk_video", tq, vn, v_off, q_scale, v_scale)
    Q, N, nv, dev = tq.shape[0], vn.shape[0], v_off.numel() - 1, tq.device
    if check_v_off:
        v = v_off.cpu()
        if int(v[0]) != 0 or int(v[-1]) != N or not bool((v[1:] > v[:-1]).all()):
            raise ValueError("rank_topk_video: v_off must start at 0, end at N and strictly increase")
    top_s, top_r, top_v = _lists(Q, k, dev, video=True) if out is None else out
    ws = _scratch(ws, _lib.lib().tan_rank_topk_video_ws_bytes(Q, N, nv, k), dev)
    _call("rank_topk_video", tq, q_scale, vn, v_scale, Q, N, tq.shape[1], _ptr(v_off), nv, k, splits, _f32(top_s), _ptr(top_r),
          _ptr(top_v), _ptr(ws))
    return top_s, top_r, top_v


def row_filter_build(spans, N, out=None):
    """The filter image of row spans over an index of N rows (tan_row_filter_build; layout in include/tan_hip.h): spans [n, 2] int32
    (device, contiguous), [lo, hi) each, ascending, disjoint, non-empty, inside [0, N) -- the caller's contract.  Returns the image,
    uint8 [row_filter_bytes(N)]; out: caller-owned memory instead of a fresh one.  Nothing is read back."""
    assert spans.dtype == torch.int32 and spans.dim() == 2 and spans.shape[1] == 2 and spans.is_contiguous()
    out = _scratch(out, _lib.lib().tan_row_filter_bytes(N), spans.device)
    assert out is None or out.is_contiguous()
    _lib.check(_lib.lib().tan_row_filter_build(_ptr(spans), spans.shape[0], N, _ptr(out), _stream()), "tan_row_filter_build")
    return out


def rank_topk_filtered(tq, vn, filt, k, *, q_scale=None, v_scale=None, splits=0, out=None, ws=None):
    """The k best ADMITTED rows per query (tan_rank_topk_filtered / _e4m3): tq [Q, 512], vn [N, 512], both bf16, both f32, or both
    uint8 e4m3 codes with q_scale [Q] / v_scale [N]; filt: `row_filter_build`'s image for N rows.  Returns (top_score [Q, k] f32,
    top_row [Q, k] int32: rows of vn), by descending score, equal scores by ascending row: bit for bit `rank_topk` over the
    gathered admitted rows; with fewer than k of them the tail is (-inf, 0x7fffffff).  splits: 0 = automatic; the result does not
    depend on it.  out / ws: caller-owned outputs (the same 2-tuple) and scratch (uint8, >= rank_topk_ws_bytes) instead of fresh
    ones."""
    _rows_args("rank_topk_filtered", tq, vn, q_scale, v_scale)
    Q, N, dev = tq.shape[0], vn.shape[0], tq.device
    L = _lib.lib()
    assert filt.dtype == torch.uint8 and filt.is_contiguous() and filt.numel() >= max(L.tan_row_filter_bytes(N), 0)
    top_s, top_r = _lists(Q, k, dev) if out is None else out
    ws = _scratch(ws, L.tan_rank_topk_ws_bytes(Q, N, k), dev)
    _call("rank_topk_filtered", tq, q_scale, vn, v_scale, Q, N, tq.shape[1], _ptr(filt), k, splits, _f32(top_s), _ptr(top_r), _ptr(ws))
    return top_s, top_r


def rank_topk_video_filtered(tq, vn, v_off, filt, k, *, q_scale=None, v_scale=None, splits=0, out=None, ws=None):
    """`rank_topk_video` over the admitted rows of filt (`row_filter_build`'s image for N rows; tan_rank_topk_video_filtered /
    _e4m3): a video's entry is its best admitted row, a video without one never appears, and with fewer than k admitted videos the
    tail is (-inf, 0x7fffffff, -1).  Everything else as `rank_topk_video`."""
    _video_args("rank_topk_video_filtered", tq, vn, v_off, q_scale, v_scale)
    Q, N, nv, dev = tq.shape[0], vn.shape[0], v_off.numel() - 1, tq.device
    L = _lib.lib()
    assert filt.dtype == torch.uint8 and filt.is_contiguous() and filt.numel() >= max(L.tan_row_filter_bytes(N), 0)
    top_s, top_r, top_v = _lists(Q, k, dev, video=True) if out is None else out
    ws = _scratch(ws, L.tan_rank_topk_video_ws_bytes(Q, N, nv, k), dev)
    _call("rank_topk_video_filtered", tq, q_scale, vn, v_scale, Q, N, tq.shape[1], _ptr(v_off), nv, _ptr(filt), k, splits, _f32(top_s),
          _ptr(top_r), _ptr(top_v), _ptr(ws))
    return top_s, top_r, top_v


def _label_topk(what, e4m3, tl, l_scale, vn, v_scale, k, out):
    """The body of `label_topk` (e4m3 = False, no scales) and `label_topk_e4m3`.  Unlike the sweeps' wrappers, this family answers
    every bad argument with an exception of its own instead of an assertion."""
    if tl.dim() != 2 or vn.dim() != 2 or not tl.is_contiguous() or not vn.is_contiguous() or (not e4m3 and tl.dtype != vn.dtype):
        raise ValueError(f"{what}: tl [L, 512] and vn [N, 512] are contiguous" + ("" if e4m3 else " and of one dtype"))
    if e4m3 and (tl.dtype != torch.uint8 or vn.dtype != torch.uint8):
        raise TypeError(f"{what}: uint8 e4m3 codes")
    if not e4m3 and tl.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{what}: bf16 or f32 rows (e4m3 codes go to label_topk_e4m3)")
    L_, N, k = tl.shape[0], vn.shape[0], int(k)
    if tl.shape[1] != 512 or vn.shape[1] != 512 or N < 1 or not 1 <= k <= min(32, L_):
        raise ValueError(f"{what}: width 512, N >= 1 and 1 <= k <= min(32, L)")
    for s, n in ((l_scale, L_), (v_scale, N)) if e4m3 else ():
        if s is None or s.dtype != torch.float32 or s.shape != (n,) or not s.is_contiguous():
            raise ValueError(f"{what}: l_scale [L] and v_scale [N] are contiguous f32")
    if out is None:
        out = _lists(N, k, vn.device)
    top_s, top_l = out
    if top_s.dtype != torch.float32 or top_l.dtype != torch.int32 or top_s.shape != (N, k) or top_l.shape != (N, k) \
            or not top_s.is_contiguous() or not top_l.is_contiguous():
        raise ValueError(f"{what}: out is (top_score f32 [N, k], top_label int32 [N, k]), contiguous")
    _call("label_topk", tl, l_scale, vn, v_scale, L_, N, 512, k, _f32(top_s), _ptr(top_l))
    return top_s, top_l


def label_topk(tl, vn, k=1, *, out=None):
    """The k best LABELS of every index row (tan_label_topk): tl [L, 512] label features, vn [N, 512] index rows, both bf16 or both
    f32, contiguous.  Returns (top_score [N, k] f32, top_label [N, k] int32), by descending score, equal scores by ascending label;
    1 <= k <= min(32, L).  One launch without scratch; nothing of size N * L is stored.  out: caller-owned outputs (the same
    2-tuple) instead of fresh ones."""
    return _label_topk("label_topk", False, tl, None, vn, None, k, out)


def label_topk_e4m3(tl, l_scale, vn, v_scale, k=1, *, out=None):
    """`label_topk` over e4m3 rows (tan_label_topk_e4m3): tl [L, 512] / vn [N, 512] uint8 codes with their f32 row scales l_scale [L]
    / v_scale [N], as `quantize_rows_e4m3` makes them; score = (acc * v_scale[n]) * l_scale[l].  Everything else as `label_topk`."""
    return _label_topk("label_topk_e4m3", True, tl, l_scale, vn, v_scale, k, out)


RUN_FIELDS = ("video", "start", "end", "label", "peak_row")             # label_runs' int32 columns, in this order; then peak_score f32


def _label_lists(what, top_score, top_label, v_off):
    """The one check of `label_topk`'s lists and the videos' offsets as `label_runs` and `label_decode` take them: (N, k, n_videos)"""
    if top_score.dim() != 2 or top_score.shape != top_label.shape or top_score.dtype != torch.float32 \
            or top_label.dtype != torch.int32 or not top_score.is_contiguous() or not top_label.is_contiguous():
        raise ValueError(f"{what}: top_score f32 and top_label int32 are contiguous [N, k]")
    if v_off.dtype != torch.int32 or v_off.dim() != 1 or v_off.numel() < 2 or not v_off.is_contiguous():
        raise ValueError(f"{what}: v_off is int32 [n_videos + 1], contiguous")
    return (*top_score.shape, v_off.numel() - 1)


def label_runs(top_score, top_label, L, v_off, threshold, min_len=1, *, cap=None, label_rows=False, out=None, ws=None):
    """Label segments from `label_topk`'s lists (tan_label_runs; the exact definition is in include/tan_hip.h): top_score f32 /
    top_label int32 [N, k] (only column 0 is read), L labels, v_off [n_videos + 1] int32 (device).  A row's label is its best one
    if its score is >= threshold, else background; a run is a maximal range of rows of one video with one label; runs shorter
    than min_len are dropped.  Returns (n_runs int32 [1], runs int32 [5, cap]: RUN_FIELDS -- video, first and last row
    (inclusive), label, peak row --, peak_score f32 [cap], label_rows int32 [L] or None), all on the device and nothing read
    back: n_runs[0] is the number of kept runs even above cap (default: N, which always suffices), and only the first
    min(n_runs, cap) columns are written.  label_rows=True: also count the rows of every label (whatever min_len is).
    out: caller-owned (n_runs, runs, peak_score, label_rows) instead of fresh ones; ws: scratch (uint8, >= label_runs_ws_bytes)."""
    (N, stride, nv), dev = _label_lists("label_runs", top_score, top_label, v_off), top_score.device
    threshold, min_len, cap = float(threshold), int(min_len), N if cap is None else int(cap)
    if N < 1 or stride < 1 or int(L) < 1 or not 1 <= nv <= N or threshold != threshold or min_len < 1 or cap < 0:
        raise ValueError("label_runs: N, k, L >= 1, 1 <= n_videos <= N, threshold not NaN, min_len >= 1, cap >= 0")
    if out is None:
        out = (torch.empty(1, dtype=torch.int32, device=dev), torch.empty(5, cap, dtype=torch.int32, device=dev),
               torch.empty(cap, dtype=torch.float32, device=dev), torch.empty(int(L), dtype=torch.int32, device=dev) if label_rows else None)
    n_runs, runs, peak, counts = out
    if n_runs.dtype != torch.int32 or n_runs.numel() < 1 or runs.dtype != torch.int32 or runs.shape != (5, cap) or not runs.is_contiguous() \
            or peak.dtype != torch.float32 or peak.shape != (cap,) or not peak.is_contiguous():
        raise ValueError("label_runs: out is (n_runs int32 [1], runs int32 [5, cap], peak_score f32 [cap], label_rows int32 [L] or None)")
    if counts is not None and (counts.dtype != torch.int32 or counts.shape != (int(L),) or not counts.is_contiguous()):
        raise ValueError("label_runs: label_rows is int32 [L], contiguous")
    lib = _lib.lib()
    ws = _scratch(ws, lib.tan_label_runs_ws_bytes(N), dev, "label_runs: ws is uint8 of at least label_runs_ws_bytes(N) bytes", False)
    if cap > 0:
        _ptr(runs)
        col = [C.c_void_p(runs.data_ptr() + 4 * cap * j) for j in range(5)] + [_f32(peak)]
    else:
        col = [_ptr(n_runs)] * 6                   # an empty tensor has no address, and with cap == 0 no run is written
    _lib.check(lib.tan_label_runs(_f32(top_score), _ptr(top_label), stride, N, int(L), _ptr(v_off), nv, threshold, min_len, cap,
                                  _ptr(n_runs), *col, _ptr(counts), _ptr(ws), _stream()), "tan_label_runs")
    return n_runs, runs, peak, counts


def label_decode(top_score, top_label, v_off, threshold, switch, *, out=None, ws=None):
    """Temporally consistent labels from `label_topk`'s lists: a Viterbi decode per video (tan_label_decode; the exact definition
    is in include/tan_hip.h).  top_score f32 / top_label int32 [N, k], 1 <= k <= 32; v_off [n_videos + 1] int32 (device).  A path
    gains score - threshold per second on a list entry, 0 on background, and pays `switch` (in [0, +inf]) wherever its label
    changes; threshold is finite.  Returns (dec_label int32 [N]: the chosen label or -1 for background, dec_score f32 [N]: its
    list score or -inf), on the device, nothing read back.  out: caller-owned (dec_label, dec_score) instead of fresh ones;
    ws: scratch (uint8, >= label_decode_ws_bytes(N, k))."""
    (N, k, nv), dev = _label_lists("label_decode", top_score, top_label, v_off), top_score.device
    threshold, switch = float(threshold), float(switch)
    if N < 1 or not 1 <= k <= 32 or not 1 <= nv <= N or not math.isfinite(threshold) or not switch >= 0:
        raise ValueError("label_decode: N >= 1, 1 <= k <= 32, 1 <= n_videos <= N, threshold finite, switch in [0, +inf]")
    if out is None:
        out = (torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.float32, device=dev))
    dec_l, dec_s = out
    if dec_l.dtype != torch.int32 or dec_s.dtype != torch.float32 or dec_l.shape != (N,) or dec_s.shape != (N,) \
            or not dec_l.is_contiguous() or not dec_s.is_contiguous():
        raise ValueError("label_decode: out is (dec_label int32 [N], dec_score f32 [N]), contiguous")
    lib = _lib.lib()
    ws = _scratch(ws, lib.tan_label_decode_ws_bytes(N, k), dev, "label_decode: ws is uint8 of at least label_decode_ws_bytes(N, k) bytes")
    _lib.check(lib.tan_label_decode(_f32(top_score), _ptr(top_label), k, N, _ptr(v_off), nv, threshold, switch, _ptr(dec_l), _f32(dec_s),
                                    _ptr(ws), _stream()), "tan_label_decode")
    return dec_l, dec_s


CLUSTER_SLAB_ROWS = 256           # tan_cluster_slab_rows(): the positions of `order` one wave of tan_cluster_accumulate walks


def _is(t, dtype, shape):
    return t is not None and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()


def cluster_accumulate(vn, assign, order, sums, v_scale=None):
    """sums[assign[n]] += the fixed-point image of row n, for every row (tan_cluster_accumulate / _e4m3; the exact definition is in
    include/tan_hip.h): vn [N, 512] f32 / bf16 rows, or uint8 e4m3 codes with v_scale f32 [N]; assign int32 [N]: the rows'
    clusters (a row outside [0, K) is skipped); order int32 [N]: a permutation of the rows, which decides only how many atomics
    are issued (sorted by cluster: the fewest); sums int64 [K, 512], caller-owned: the call ADDS, so zero it once and let one call
    per shard add into it.  The result is the same bits for every order and every split of the rows over calls.  Returns sums."""
    if vn.dim() != 2 or vn.shape[1] != 512 or vn.shape[0] < 1 or not vn.is_contiguous():
        raise ValueError("cluster_accumulate: vn is [N, 512], contiguous, N >= 1")
    if vn.dtype not in (torch.float32, torch.bfloat16, torch.uint8):
        raise TypeError("cluster_accumulate: f32 or bf16 rows, or uint8 e4m3 codes")
    N, e4m3 = vn.shape[0], vn.dtype == torch.uint8
    if (v_scale is not None) != e4m3 or (e4m3 and not _is(v_scale, torch.float32, (N,))):
        raise ValueError("cluster_accumulate: v_scale f32 [N], contiguous, goes with uint8 e4m3 codes, and only with them")
    if not _is(assign, torch.int32, (N,)) or not _is(order, torch.int32, (N,)):
        raise ValueError("cluster_accumulate: assign and order are int32 [N], contiguous")
    if sums is None or sums.dtype != torch.int64 or sums.dim() != 2 or sums.shape[0] < 1 or sums.shape[1] != 512 or not sums.is_contiguous():
        raise ValueError("cluster_accumulate: sums is int64 [K, 512], contiguous, K >= 1")
    K, lib = sums.shape[0], _lib.lib()
    if e4m3:
        _lib.check(lib.tan_cluster_accumulate_e4m3(_ptr(vn), _f32(v_scale), N, 512, _ptr(assign), _ptr(order), K, _ptr(sums), _stream()),
                   "tan_cluster_accumulate_e4m3")
    else:
        _lib.check(lib.tan_cluster_accumulate(_ptr(vn), _dt(vn), N, 512, _ptr(assign), _ptr(order), K, _ptr(sums), _stream()),
                   "tan_cluster_accumulate")
    return sums


def cluster_centroids(sums, counts, prev, *, out=None):
    """The new unit centroids of `cluster_accumulate`'s sums (tan_cluster_centroids; the exact definition is in include/tan_hip.h):
    sums int64 [K, 512], counts int32 [K]: the rows of every cluster, prev f32 [K, 512].  Returns (cent f32 [K, 512], cohesion f32
    [K]: the mean resultant length of the cluster's rows); an empty cluster, or one whose rows cancel, keeps prev's centroid bit
    for bit with cohesion 0.  out: caller-owned (cent, cohesion) instead of fresh ones; cent may be prev."""
    if sums.dtype != torch.int64 or sums.dim() != 2 or sums.shape[0] < 1 or sums.shape[1] != 512 or not sums.is_contiguous():
        raise ValueError("cluster_centroids: sums is int64 [K, 512], contiguous, K >= 1")
    K, dev = sums.shape[0], sums.device
    if not _is(counts, torch.int32, (K,)) or not _is(prev, torch.float32, (K, 512)):
        raise ValueError("cluster_centroids: counts is int32 [K] and prev f32 [K, 512], contiguous")
    if out is None:
        out = (torch.empty(K, 512, dtype=torch.float32, device=dev), torch.empty(K, dtype=torch.float32, device=dev))
    cent, cohesion = out
    if not _is(cent, torch.float32, (K, 512)) or not _is(cohesion, torch.float32, (K,)):
        raise ValueError("cluster_centroids: out is (cent f32 [K, 512], cohesion f32 [K]), contiguous")
    _lib.check(_lib.lib().tan_cluster_centroids(_ptr(sums), _ptr(counts), _f32(prev), K, 512, _f32(cent), _f32(cohesion), _stream()),
               "tan_cluster_centroids")
    return cent, cohesion


def _align_args(what, x, x_off, table, theta, skew, sum_V, path_off=(), check_table=False):
    """The checks that `local_align` and `local_align_path` share, in their order: (P, theta, skew, sum_V).  path_off: a 1-tuple from
    `local_align_path`; check_table: `local_align`'s option.  Without sum_V the table's last entry is read back."""
    if x.dim() != 1 or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() < 1:
        raise ValueError(f"{what}: x is f32 [n_x], contiguous, n_x >= 1")
    if x_off.dim() != 1 or x_off.dtype != torch.int64 or not x_off.is_contiguous() or x_off.numel() < 1:
        raise ValueError(f"{what}: x_off is int64 [P], contiguous, P >= 1")
    P = x_off.numel()
    if table.dtype != torch.int32 or table.shape != (P, 3) or not table.is_contiguous():
        raise ValueError(f"{what}: table is int32 [P, 3] = (m, V, first boundary slot), contiguous")
    for po in path_off:
        if po.dtype != torch.int64 or po.shape != (P, 2) or not po.is_contiguous():
            raise ValueError(f"{what}: path_off is int64 [P, 2] = (first map row, first trace entry), contiguous")
    theta, skew = float(theta), float(skew)
    if not math.isfinite(theta) or not (skew >= 0 and math.isfinite(skew)):
        raise ValueError(f"{what}: theta finite, skew in [0, +inf)")
    if check_table or sum_V is None:
        t = (table if check_table else table[-1:]).cpu().long()
        if check_table and (int(t[0, 2]) != 0 or bool((t[:, 1] < 1).any()) or not torch.equal(t[1:, 2], torch.cumsum(t[:, 1], 0)[:-1])):
            raise ValueError(f"{what}: the table's third column is the running sum of its V (from 0, every V >= 1)")
        sum_V = int(t[-1, 1] + t[-1, 2]) if sum_V is None else sum_V
    sum_V = int(sum_V)
    if not P <= sum_V < 2 ** 31:
        raise ValueError(f"{what}: P <= sum_V < 2^31 (sum_V: the sum of the table's V)")
    return P, theta, skew, sum_V


def _align_out(what, out, P, dev, more=""):
    """(score f32 [P], span int32 [P, 5]): the pair `out`, checked, or fresh ones; more: what else the caller's `out` holds"""
    score, span = (torch.empty(P, dtype=torch.float32, device=dev), torch.empty(P, 5, dtype=torch.int32, device=dev)) if out is None else out
    if score.dtype != torch.float32 or span.dtype != torch.int32 or score.shape != (P,) or span.shape != (P, 5) \
            or not score.is_contiguous() or not span.is_contiguous():
        raise ValueError(f"{what}: out is (score f32 [P], span int32 [P, 5]{more}), contiguous")
    return score, span


def local_align(x, x_off, table, theta, skew, *, sum_V=None, check_table=False, out=None, ws=None):
    """The best local alignment of every block of `x` (tan_local_align; the exact definition is in include/tan_hip.h): x f32 [n_x]
    holds row-major [m, V] blocks of query second x video second scores as `sequence_scores` writes them; x_off int64 [P] each
    block's first element, table int32 [P, 3] = (m, V, first boundary slot = the running sum of V), both on the device; 1 <= m <=
    4096, 1 <= V < 2^20.  A cell gains x - theta (theta finite), a step along one axis alone pays `skew` (in [0, +inf)).
    Returns (score f32 [P], span int32 [P, 5] = (a_first, a_last, b_first, b_last, cells): query seconds a_first .. a_last appear
    as video seconds b_first .. b_last), on the device, nothing read back; a block without a positive cell, or a table entry that
    breaks the limits, gives (0, (-1, -1, -1, -1, 0)).  sum_V: the number of boundary slots, the sum of the table's V; the caller
    built the table and knows it -- without it the wrapper reads the table's last entry back (slot + V: one synchronisation).
    check_table: verify on the host (one synchronisation) that the slots are the running sum of V, so no two entries share one --
    otherwise that is the caller's contract: overlapping slots stay in bounds but give wrong results for strips beyond the first.
    out: caller-owned (score, span) instead of fresh ones; ws: scratch (uint8, >= local_align_ws_bytes(P, sum_V))."""
    P, theta, skew, sum_V = _align_args("local_align", x, x_off, table, theta, skew, sum_V, check_table=check_table)
    score, span = _align_out("local_align", out, P, x.device)
    lib = _lib.lib()
    ws = _scratch(ws, lib.tan_local_align_ws_bytes(P, sum_V), x.device,
                  "local_align: ws is uint8 of at least local_align_ws_bytes(P, sum_V) bytes")
    _lib.check(lib.tan_local_align(_f32(x), x.numel(), _ptr(x_off), _ptr(table), P, sum_V, theta, skew, _f32(score), _ptr(span), _ptr(ws),
                                   _stream()), "tan_local_align")
    return score, span


def local_align_path(x, x_off, table, theta, skew, path_off, *, sum_V=None, n_map, n_trace, out=None, ws=None):
    """`local_align` with the best path's second-to-second time map (tan_local_align_path; the exact definition is in
    include/tan_hip.h).  x, x_off, table, theta, skew, sum_V as for `local_align`; path_off int64 [P, 2] on the device = (each
    block's first map row: the running sum of m, its first trace entry: the running sum of ceil(m / 64) * (V + 63)), n_map and
    n_trace their totals (`search.path_tables`).  Returns (score f32 [P], span int32 [P, 5], qmap int32 [n_map, 2]) on the device:
    score and span are `local_align`'s bit for bit; a block's m map rows hold (first, last video second) of query seconds a_first ..
    a_last and (-1, -1) elsewhere.  A table entry that breaks the limits, or whose map rows or trace entries leave [0, n_map) /
    [0, n_trace), gives the empty result and its map rows are NOT written.
    out: caller-owned (score, span, qmap); ws: scratch (uint8, >= local_align_path_ws_bytes(P, sum_V, n_trace))."""
    P, theta, skew, sum_V = _align_args("local_align_path", x, x_off, table, theta, skew, sum_V, (path_off,))
    n_map, n_trace = int(n_map), int(n_trace)
    if not 1 <= n_map < 2 ** 31 or n_trace < 1:
        raise ValueError("local_align_path: 1 <= n_map < 2^31, n_trace >= 1")
    pair, qmap = (None, None) if out is None else ((out[0], out[1]), *out[2:])
    score, span = _align_out("local_align_path", pair, P, x.device, ", qmap")
    if out is None:
        qmap = torch.empty(n_map, 2, dtype=torch.int32, device=x.device)
    if qmap.dtype != torch.int32 or qmap.shape != (n_map, 2) or not qmap.is_contiguous():
        raise ValueError("local_align_path: qmap is int32 [n_map, 2], contiguous")
    lib = _lib.lib()
    need = lib.tan_local_align_path_ws_bytes(P, sum_V, n_trace)
    if need < 0:
        raise ValueError("local_align_path: n_trace out of range")
    ws = _scratch(ws, need, x.device, "local_align_path: ws is uint8 of at least local_align_path_ws_bytes(P, sum_V, n_trace) bytes")
    _lib.check(lib.tan_local_align_path(_f32(x), x.numel(), _ptr(x_off), _ptr(table), P, sum_V, theta, skew, _ptr(path_off), n_map, n_trace,
                                        _f32(score), _ptr(span), _ptr(qmap), _ptr(ws), _stream()), "tan_local_align_path")
    return score, span, qmap


def moment_extent(tq, vn, v_off, top_score, top_row, top_video, width, *, q_scale=None, v_scale=None, out=None):
    """(start, end) int32 [Q, k]: for every hit of `rank_topk_video`'s lists, the contiguous run of index rows around top_row,
    inside the hit's video, whose score is >= top_score - width -- global rows, inclusive (tan_moment_extent / _e4m3; the exact
    definition is in include/tan_hip.h).  tq / vn / v_off / q_scale / v_scale as for `rank_topk_video`; width >= 0.
    out: caller-owned (start, end) instead of fresh ones."""
    _video_args("moment_extent", tq, vn, v_off, q_scale, v_scale)
    Q, N, nv, dev = tq.shape[0], vn.shape[0], v_off.numel() - 1, tq.device
    k = top_row.shape[1]
    for t, dt in ((top_score, torch.float32), (top_row, torch.int32), (top_video, torch.int32)):
        assert t.dtype == dt and t.shape == (Q, k) and t.is_contiguous()
    if out is None:
        out = (torch.empty(Q, k, dtype=torch.int32, device=dev), torch.empty(Q, k, dtype=torch.int32, device=dev))
    start, end = out
    assert all(t.dtype == torch.int32 and t.shape == (Q, k) and t.is_contiguous() for t in out)
    _call("moment_extent", tq, q_scale, vn, v_scale, Q, N, tq.shape[1], _ptr(v_off), nv, k, _f32(top_score), _ptr(top_row),
          _ptr(top_video), float(width), _ptr(start), _ptr(end))
    return start, end


def _sequence_args(what, tq, vn, s_off, v_off, q_scale, v_scale, check_offsets):
    e4m3 = _video_args(what, tq, vn, v_off, q_scale, v_scale)
    assert s_off.dtype == torch.int32 and s_off.dim() == 1 and s_off.numel() >= 2 and s_off.is_contiguous()
    if check_offsets:
        s, v = s_off.cpu(), v_off.cpu()
        if int(s[0]) != 0 or int(s[-1]) != tq.shape[0] or not bool(((s[1:] - s[:-1] >= 1) & (s[1:] - s[:-1] <= 32)).all()):
            raise ValueError(f"{what}: s_off must start at 0, end at Qt and grow by 1 to 32 per sequence")
        if int(v[0]) != 0 or int(v[-1]) != vn.shape[0] or not bool((v[1:] > v[:-1]).all()):
            raise ValueError(f"{what}: v_off must start at 0, end at N and strictly increase")
    return e4m3


def sequence_topk(tq, vn, s_off, v_off, k, *, q_scale=None, v_scale=None, splits=0, check_offsets=False, out=None, ws=None):
    """The k videos that show each SEQUENCE of steps best in order (tan_sequence_topk / _e4m3; the path is defined in
    include/tan_hip.h): tq [Qt, 512] holds the sequences' steps one after the other, s_off [n_seq + 1] int32 (device) each sequence's
    first row, then Qt (1 to 32 steps each); vn / v_off / q_scale / v_scale as for `rank_topk_video`.
    Returns (top_score [n_seq, k] f32: the path score, top_video [n_seq, k] int32), by descending path, equal paths by ascending
    video.  splits: 0 = automatic; the result does not depend on it.  check_offsets: verify s_off and v_off on the host (one
    synchronisation); otherwise they are the caller's contract.  out / ws: caller-owned outputs (the same 2-tuple) and scratch
    (uint8, >= sequence_topk_ws_bytes) instead of fresh ones."""
    _sequence_args("sequence_topk", tq, vn, s_off, v_off, q_scale, v_scale, check_offsets)
    Qt, N, ns, nv, dev = tq.shape[0], vn.shape[0], s_off.numel() - 1, v_off.numel() - 1, tq.device
    top_s, top_v = _lists(ns, k, dev) if out is None else out
    ws = _scratch(ws, _lib.lib().tan_sequence_topk_ws_bytes(ns, N, k), dev)
    _call("sequence_topk", tq, q_scale, vn, v_scale, Qt, N, tq.shape[1], _ptr(s_off), ns, _ptr(v_off), nv, k, splits, _f32(top_s),
          _ptr(top_v), _ptr(ws))
    return top_s, top_v


def sequence_scores(tq, vn, s_off, v_off, hits, x_off, x, *, q_scale=None, v_scale=None, check_offsets=False):
    """x [n_x] f32 (caller-owned, returned): for every hit h of hits [P, 2] int32 = (sequence, video), the [m, V] block of step x
    second scores at x[x_off[h]:], x_off [P] int64 -- the scores `sequence_topk` ranked by, bit for bit (tan_sequence_scores /
    _e4m3).  Everything else as `sequence_topk`."""
    _sequence_args("sequence_scores", tq, vn, s_off, v_off, q_scale, v_scale, check_offsets)
    Qt, N, ns, nv = tq.shape[0], vn.shape[0], s_off.numel() - 1, v_off.numel() - 1
    P = hits.shape[0]
    assert hits.dtype == torch.int32 and hits.shape == (P, 2) and hits.is_contiguous()
    assert x_off.dtype == torch.int64 and x_off.shape == (P,) and x_off.is_contiguous()
    assert x.dtype == torch.float32 and x.dim() == 1 and x.is_contiguous()
    _call("sequence_scores", tq, q_scale, vn, v_scale, Qt, N, tq.shape[1], _ptr(s_off), ns, _ptr(v_off), nv, _ptr(hits), _ptr(x_off), P,
          _f32(x), x.numel())
    return x


def clip_topk(tq, vn, c_off, v_off, k, *, q_scale=None, v_scale=None, splits=0, check_offsets=False, out=None, ws=None):
    """The k videos in which each CLIP appears best second for second (tan_clip_topk / _e4m3; the match is defined in
    include/tan_hip.h): tq [Qt, 512] holds the clips' rows one after the other, c_off [n_clip + 1] int32 (device) each clip's first
    row, then Qt (1 to 32 rows each); vn / v_off / q_scale / v_scale as for `rank_topk_video`.
    Returns (top_score [n_clip, k] f32: the SUM of the clip's scores along the best diagonal, top_row [n_clip, k] int32: the index
    row where that diagonal starts, top_video [n_clip, k] int32), by descending score, equal scores by ascending row; when fewer
    than k videos are as long as the clip, the tail is (-inf, 0x7fffffff, -1).  splits: 0 = automatic; the result does not depend
    on it.  check_offsets: verify c_off and v_off on the host (one synchronisation); otherwise they are the caller's contract.
    out / ws: caller-owned outputs (the same 3-tuple) and scratch (uint8, >= clip_topk_ws_bytes) instead of fresh ones."""
    _sequence_args("clip_topk", tq, vn, c_off, v_off, q_scale, v_scale, check_offsets)
    Qt, N, nc, nv, dev = tq.shape[0], vn.shape[0], c_off.numel() - 1, v_off.numel() - 1, tq.device
    top_s, top_r, top_v = _lists(nc, k, dev, video=True) if out is None else out
    ws = _scratch(ws, _lib.lib().tan_clip_topk_ws_bytes(nc, N, k), dev)
    _call("clip_topk", tq, q_scale, vn, v_scale, Qt, N, tq.shape[1], _ptr(c_off), nc, _ptr(v_off), nv, k, splits, _f32(top_s),
          _ptr(top_r), _ptr(top_v), _ptr(ws))
    return top_s, top_r, top_v


def _compound_args(what, tq, vn, t_off, role, v_off, q_scale, v_scale, check_offsets):
    _sequence_args(what, tq, vn, t_off, v_off, q_scale, v_scale, check_offsets)
    if role is None:
        return
    assert role.dtype == torch.int32 and role.shape == (tq.shape[0],) and role.is_contiguous()
    if check_offsets:
        r, t = role.cpu(), t_off.cpu().long()
        if not bool(((r >= -1) & (r <= 31)).all()):
            raise ValueError(f"{what}: role must lie in [-1, 31] (a clause, or -1 = banned)")
        clause = torch.cat((torch.zeros(1, dtype=torch.long), torch.cumsum((r >= 0).long(), 0)))
        if not bool((clause[t[1:]] > clause[t[:-1]]).all()):
            raise ValueError(f"{what}: every query needs at least one clause term (role >= 0)")


def compound_topk(tq, vn, t_off, role, v_off, k, *, veto=float("inf"), q_scale=None, v_scale=None, splits=0, check_offsets=False,
                  out=None, ws=None):
    """The k videos that satisfy each COMPOUND query best (tan_compound_topk / _e4m3; peak, clause, score and veto are defined in
    include/tan_hip.h): tq [Qt, 512] holds the queries' terms one after the other, t_off [n_query + 1] int32 (device) each query's
    first row, then Qt (1 to 32 terms each); role [Qt] int32 (device): the term's clause in [0, 31], or -1 = banned; vn / v_off /
    q_scale / v_scale as for `rank_topk_video`.  A term's peak is its best score over the video's rows, a clause is worth its best
    term (OR), a video its weakest clause (AND), and a video where a banned term's peak is >= veto is no candidate (NOT).
    Returns (top_score [n_query, k] f32, top_video [n_query, k] int32), by descending score, equal scores by ascending video; with
    fewer than k candidates the tail is (-inf, 0x7fffffff).  splits: 0 = automatic; the result does not depend on it.
    check_offsets: verify t_off, role and v_off on the host (one synchronisation): 1 to 32 terms per query, roles in [-1, 31], at
    least one clause term per query; otherwise they are the caller's contract.  out / ws: caller-owned outputs (the same 2-tuple)
    and scratch (uint8, >= compound_topk_ws_bytes) instead of fresh ones.  ValueError: a NaN veto."""
    _compound_args("compound_topk", tq, vn, t_off, role, v_off, q_scale, v_scale, check_offsets)
    veto = float(veto)
    if veto != veto:
        raise ValueError("compound_topk: veto is NaN")
    Qt, N, nq, nv, dev = tq.shape[0], vn.shape[0], t_off.numel() - 1, v_off.numel() - 1, tq.device
    top_s, top_v = _lists(nq, k, dev) if out is None else out
    ws = _scratch(ws, _lib.lib().tan_compound_topk_ws_bytes(nq, N, k), dev)
    _call("compound_topk", tq, q_scale, vn, v_scale, Qt, N, tq.shape[1], _ptr(t_off), _ptr(role), nq, _ptr(v_off), nv, veto, k, splits,
          _f32(top_s), _ptr(top_v), _ptr(ws))
    return top_s, top_v


def compound_peaks(tq, vn, t_off, v_off, hits, *, q_scale=None, v_scale=None, check_offsets=False, out=None):
    """(peak_score f32 [P, 32], peak_row int32 [P, 32]): for every hit h of hits [P, 2] int32 = (query, video), each term's peak
    over the video and the first index row (global) that attains it, term t in column t -- the peaks `compound_topk` ranked by, bit
    for bit (tan_compound_peaks / _e4m3).  Columns beyond the query's terms hold (-inf, 0x7fffffff).  out: caller-owned outputs
    (the same 2-tuple).  Everything else as `compound_topk`."""
    _compound_args("compound_peaks", tq, vn, t_off, None, v_off, q_scale, v_scale, check_offsets)
    Qt, N, nq, nv, dev = tq.shape[0], vn.shape[0], t_off.numel() - 1, v_off.numel() - 1, tq.device
    P = hits.shape[0]
    assert hits.dtype == torch.int32 and hits.shape == (P, 2) and hits.is_contiguous()
    peak_s, peak_r = _lists(P, 32, dev) if out is None else out
    assert peak_s.dtype == torch.float32 and peak_r.dtype == torch.int32 and peak_s.shape == peak_r.shape == (P, 32)
    assert peak_s.is_contiguous() and peak_r.is_contiguous()
    _call("compound_peaks", tq, q_scale, vn, v_scale, Qt, N, tq.shape[1], _ptr(t_off), nq, _ptr(v_off), nv, _ptr(hits), P, _f32(peak_s),
          _ptr(peak_r))
    return peak_s, peak_r


COVER_MAX_ROWS = 4096                                                 # tan_cover_max_rows(): the longest set of `cover_topk`
COVER_RANKS = {"query": 0, "video": 1, "both": 2}                     # TAN_COVER_QUERY / _VIDEO / _BOTH


def cover_topk(tq, vn, q_off, v_off, k, *, rank="both", q_scale=None, v_scale=None, check_offsets=False, out=None):
    """The k videos that share the most seconds with each SET of query rows, in any order (tan_cover_topk / _e4m3; the Chamfer
    similarity in 64-bit fixed point is defined in include/tan_hip.h): tq [Qt, 512] holds the sets' rows one after the other, q_off
    [n_set + 1] int32 (device) each set's first row, then Qt (1 to 4096 rows each, at most 65535 sets); vn / v_off / q_scale /
    v_scale as for `rank_topk_video`.  rank: "query" = fwd, the mean over the set's rows of each row's best second in the video
    ("how much of my video is in v"); "video" = bwd, the mean over the video's seconds of each second's best row of the set ("how
    much of v is in my video"); "both" = their mean.
    Returns (top_score [n_set, k] f32, top_row [n_set, k] int32: the video's first index row, top_video [n_set, k] int32, fwd
    [n_set, n_videos] f32, bwd [n_set, n_videos] f32): the lists by descending score, equal scores by ascending row; fwd / bwd are
    the all-pairs result.  check_offsets: verify q_off and v_off on the host (one synchronisation); otherwise they are the caller's
    contract.  out: caller-owned outputs (the same 5-tuple) instead of fresh ones.  ValueError: an unknown rank, or sizes the entry
    point would refuse -- raised before anything touches the device."""
    _video_args("cover_topk", tq, vn, v_off, q_scale, v_scale)
    assert q_off.dtype == torch.int32 and q_off.dim() == 1 and q_off.numel() >= 2 and q_off.is_contiguous()
    if rank not in COVER_RANKS:
        raise ValueError(f"cover_topk: rank must be one of {sorted(COVER_RANKS)}, not {rank!r}")
    Qt, N, ns, nv, dev = tq.shape[0], vn.shape[0], q_off.numel() - 1, v_off.numel() - 1, tq.device
    if ns > 65535 or not ns <= Qt <= COVER_MAX_ROWS * ns:
        raise ValueError(f"cover_topk: at most 65535 sets of 1 to {COVER_MAX_ROWS} rows each, not {ns} sets over {Qt} rows")
    if not 1 <= int(k) <= min(32, nv):
        raise ValueError(f"cover_topk: k must lie in [1, min(32, n_videos = {nv})]")
    if check_offsets:
        s, v = q_off.cpu(), v_off.cpu()
        if int(s[0]) != 0 or int(s[-1]) != Qt or not bool(((s[1:] - s[:-1] >= 1) & (s[1:] - s[:-1] <= COVER_MAX_ROWS)).all()):
            raise ValueError(f"cover_topk: q_off must start at 0, end at Qt and grow by 1 to {COVER_MAX_ROWS} per set")
        if int(v[0]) != 0 or int(v[-1]) != N or not bool((v[1:] > v[:-1]).all()):
            raise ValueError("cover_topk: v_off must start at 0, end at N and strictly increase")
    if out is None:
        top_s, top_r, top_v = _lists(ns, k, dev, video=True)
        fwd, bwd = (torch.empty(ns, nv, dtype=torch.float32, device=dev) for _ in range(2))
    else:
        top_s, top_r, top_v, fwd, bwd = out
        assert all(t.is_contiguous() for t in out) and fwd.shape == bwd.shape == (ns, nv) and top_s.shape == (ns, k)
    _call("cover_topk", tq, q_scale, vn, v_scale, Qt, N, tq.shape[1], _ptr(q_off), ns, _ptr(v_off), nv,
          COVER_RANKS[rank], int(k), _f32(fwd), _f32(bwd), _f32(top_s), _ptr(top_r), _ptr(top_v))
    return top_s, top_r, top_v, fwd, bwd


STORYBOARD_MAX_ROWS = 4096                                            # tan_storyboard_max_rows(): the longest video of `storyboard_select`
STORYBOARD_MAX_K = 4096


def storyboard_select(x, x_off, table, k, *, min_gain=0.0, sum_V=None, out=None):
    """The k seconds that together show each video best (tan_storyboard_select; greedy facility location in 64-bit fixed point, defined
    bit for bit in include/tan_hip.h): x f32 [n_x] holds row-major [V, V] blocks of a video's second x second scores as
    `sequence_scores` writes them for the video's own rows; x_off int64 [P] each block's first element, table int32 [P, 2] = (V,
    first owner slot = the running sum of V), both on the device; 1 <= V <= 4096, 1 <= k <= 4096, min_gain finite and >= 0: the
    selection stops when the next second would raise the mean coverage by less than min_gain (or not at all).
    Returns (second int32 [P, k], coverage f32 [P, k], owner int32 [sum_V]) on the device, nothing read back: the chosen seconds in
    the order they were chosen, the mean over the video's seconds of the best score to any second chosen so far, and per second of
    the video the entry (0-based) that shows it best.  Entries after a stop or beyond V are (-1, 0).  A table entry that breaks the
    limits, or whose block or owner slots leave x / owner, gives the empty result and its owner slots are NOT written.
    sum_V: the number of owner slots, the sum of the table's V; the caller built the table and knows it -- without it the wrapper
    reads the table's last entry back (V + slot: one synchronisation).  out: caller-owned (second, coverage, owner) instead of fresh
    ones.  ValueError: shapes, dtypes or sizes the entry point would refuse -- raised before anything touches the device."""
    what = "storyboard_select"
    if x.dim() != 1 or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() < 1:
        raise ValueError(f"{what}: x is f32 [n_x], contiguous, n_x >= 1")
    if x_off.dim() != 1 or x_off.dtype != torch.int64 or not x_off.is_contiguous() or x_off.numel() < 1:
        raise ValueError(f"{what}: x_off is int64 [P], contiguous, P >= 1")
    P = x_off.numel()
    if table.dtype != torch.int32 or table.shape != (P, 2) or not table.is_contiguous():
        raise ValueError(f"{what}: table is int32 [P, 2] = (V, first owner slot), contiguous")
    k, min_gain = int(k), float(min_gain)
    if not 1 <= k <= STORYBOARD_MAX_K:
        raise ValueError(f"{what}: k must lie in [1, {STORYBOARD_MAX_K}]")
    if not (min_gain >= 0 and math.isfinite(min_gain)):
        raise ValueError(f"{what}: min_gain finite and >= 0")
    if sum_V is not None and not P <= int(sum_V) < 2 ** 31:
        raise ValueError(f"{what}: P <= sum_V < 2^31 (sum_V: the sum of the table's V)")
    if out is not None:
        second, coverage, owner = out
        if second.dtype != torch.int32 or coverage.dtype != torch.float32 or owner.dtype != torch.int32 or second.shape != (P, k) \
                or coverage.shape != (P, k) or owner.dim() != 1 or (sum_V is not None and owner.numel() != int(sum_V)) \
                or not all(t.is_contiguous() for t in out):
            raise ValueError(f"{what}: out is (second int32 [P, k], coverage f32 [P, k], owner int32 [sum_V]), contiguous")
    if sum_V is None:
        t = table[-1:].cpu().long()
        sum_V = int(t[0, 0] + t[0, 1])
        if not P <= sum_V < 2 ** 31 or (out is not None and out[2].numel() != sum_V):
            raise ValueError(f"{what}: P <= sum_V < 2^31, and owner holds sum_V slots (sum_V: the sum of the table's V)")
    sum_V = int(sum_V)
    if out is None:
        dev = x.device
        second, coverage, owner = (torch.empty(P, k, dtype=torch.int32, device=dev), torch.empty(P, k, dtype=torch.float32, device=dev),
                                   torch.empty(sum_V, dtype=torch.int32, device=dev))
    _lib.check(_lib.lib().tan_storyboard_select(_f32(x), x.numel(), _ptr(x_off), _ptr(table), P, sum_V, k, min_gain, _ptr(second),
                                                _f32(coverage), _ptr(owner), _stream()), "tan_storyboard_select")
    return second, coverage, owner


CHAPTER_MAX_ROWS = 4096                                               # tan_chapter_max_rows(): the longest video of `chapter_costs` / `chapter_decode`
CHAPTER_MAX_K = 256


def _chapter_tables(what, x_off, table):
    if x_off.dim() != 1 or x_off.dtype != torch.int64 or not x_off.is_contiguous() or x_off.numel() < 1:
        raise ValueError(f"{what}: x_off is int64 [P], contiguous, P >= 1")
    P = x_off.numel()
    if table.dtype != torch.int32 or table.shape != (P, 2) or not table.is_contiguous():
        raise ValueError(f"{what}: table is int32 [P, 2] = (V, first chapter slot), contiguous")
    return P


def chapter_costs(x, x_off, table, *, out=None):
    """The cost of making seconds [s, e) of a video one chapter, for every s < e (tan_chapter_costs; the within-segment scatter in
    64-bit fixed point, defined bit for bit in include/tan_hip.h): x f32 [n_x] holds row-major [V, V] blocks of a video's second x
    second scores as `sequence_scores` writes them for the video's own rows; x_off int64 [P] and table int32 [P, 2] = (V, first
    chapter slot) are `storyboard_select`'s tables, on the device; 1 <= V <= 4096.
    Returns cost int64 [n_x] on the device: cost[x_off[p] + (e-1) * V + s] = J(s, e) for 0 <= s < e <= V; the other half of a block
    is unspecified, and nothing outside the blocks is written.  A table entry that breaks the limits or whose block leaves x is
    skipped.  out: a caller-owned cost instead of a fresh one.  ValueError: shapes, dtypes or sizes the entry point would refuse --
    raised before anything touches the device."""
    what = "chapter_costs"
    if x.dim() != 1 or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() < 1:
        raise ValueError(f"{what}: x is f32 [n_x], contiguous, n_x >= 1")
    P = _chapter_tables(what, x_off, table)
    if out is not None and (out.dtype != torch.int64 or out.shape != x.shape or not out.is_contiguous()):
        raise ValueError(f"{what}: out is int64 [n_x], contiguous")
    cost = torch.empty(x.numel(), dtype=torch.int64, device=x.device) if out is None else out
    _lib.check(_lib.lib().tan_chapter_costs(_f32(x), x.numel(), _ptr(x_off), _ptr(table), P, _ptr(cost), _stream()), "tan_chapter_costs")
    return cost


def chapter_decode_ws_bytes(P, sum_V, k):
    """the scratch `chapter_decode` needs: sum_V * k * 2 bytes (the arguments of every level as 16 bits)"""
    return int(sum_V) * int(k) * 2


def chapter_decode(cost, x_off, table, k, *, penalty, min_len=1, sum_V=None, out=None, ws=None):
    """Each video cut into at most k contiguous chapters of at least min_len seconds (tan_chapter_decode; an exact dynamic programme
    over `chapter_costs`' costs, defined bit for bit in include/tan_hip.h): the boundaries that minimise the summed scatter plus
    `penalty` (finite, >= 0; absolute, in score x seconds) per boundary.  cost int64 [n_x], x_off, table as `chapter_costs` took
    them; 1 <= k <= 256, 1 <= min_len <= 4096.
    Returns (count int32 [P], start int32 [P, k], scatter f32 [P, k], chapter int32 [sum_V]) on the device, nothing read back: the
    number of chapters, each chapter's first second (-1 from `count` on), the summed scatter of the best cut into j chapters at
    [j - 1] (+inf where j chapters are not possible) and per second of the video its chapter.  A table entry that breaks the limits,
    or whose block or slots leave cost / chapter, gives the empty result (0, -1, +inf) and its chapter slots are NOT written.
    sum_V: the number of chapter slots, the sum of the table's V; without it the wrapper reads the table's last entry back (one
    synchronisation).  out: caller-owned outputs (the same 4-tuple).  ws: caller-owned scratch, uint8 of at least
    `chapter_decode_ws_bytes(P, sum_V, k)`.  ValueError: shapes, dtypes or sizes the entry point would refuse -- raised before
    anything touches the device."""
    what = "chapter_decode"
    if cost.dim() != 1 or cost.dtype != torch.int64 or not cost.is_contiguous() or cost.numel() < 1:
        raise ValueError(f"{what}: cost is int64 [n_x], contiguous, n_x >= 1")
    P = _chapter_tables(what, x_off, table)
    k, min_len, penalty = int(k), int(min_len), float(penalty)
    if not 1 <= k <= CHAPTER_MAX_K:
        raise ValueError(f"{what}: k must lie in [1, {CHAPTER_MAX_K}]")
    if not 1 <= min_len <= CHAPTER_MAX_ROWS:
        raise ValueError(f"{what}: min_len must lie in [1, {CHAPTER_MAX_ROWS}]")
    if not (penalty >= 0 and math.isfinite(penalty)):
        raise ValueError(f"{what}: penalty finite and >= 0")
    if sum_V is not None and not P <= int(sum_V) < 2 ** 31:
        raise ValueError(f"{what}: P <= sum_V < 2^31 (sum_V: the sum of the table's V)")

    def out_ok(n):
        count, start, scatter, chapter = out
        return (count.dtype == start.dtype == chapter.dtype == torch.int32 and scatter.dtype == torch.float32 and count.shape == (P,)
                and start.shape == (P, k) and scatter.shape == (P, k) and chapter.dim() == 1 and (n is None or chapter.numel() == n)
                and all(t.is_contiguous() for t in out))
    text = f"{what}: out is (count int32 [P], start int32 [P, k], scatter f32 [P, k], chapter int32 [sum_V]), contiguous"
    if out is not None and (len(out) != 4 or not out_ok(None if sum_V is None else int(sum_V))):
        raise ValueError(text)
    if ws is not None and (ws.dtype != torch.uint8 or ws.dim() != 1 or not ws.is_contiguous()
                           or (sum_V is not None and ws.numel() < chapter_decode_ws_bytes(P, sum_V, k))):
        raise ValueError(f"{what}: ws is uint8, contiguous, of at least chapter_decode_ws_bytes(P, sum_V, k) bytes")
    if sum_V is None:
        t = table[-1:].cpu().long()
        sum_V = int(t[0, 0] + t[0, 1])
        if not P <= sum_V < 2 ** 31 or (out is not None and not out_ok(sum_V)) \
                or (ws is not None and ws.numel() < chapter_decode_ws_bytes(P, sum_V, k)):
            raise ValueError(f"{what}: P <= sum_V < 2^31, and chapter and ws are sized for it (sum_V: the sum of the table's V)")
    sum_V = int(sum_V)
    dev = cost.device
    if out is None:
        out = (torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, k, dtype=torch.int32, device=dev),
               torch.empty(P, k, dtype=torch.float32, device=dev), torch.empty(sum_V, dtype=torch.int32, device=dev))
    count, start, scatter, chapter = out
    if ws is None:
        ws = torch.empty(max(chapter_decode_ws_bytes(P, sum_V, k), 1), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().tan_chapter_decode(_ptr(cost), cost.numel(), _ptr(x_off), _ptr(table), P, sum_V, k, min_len, penalty, _ptr(count),
                                             _ptr(start), _f32(scatter), _ptr(chapter), _ptr(ws), _stream()), "tan_chapter_decode")
    return count, start, scatter, chapter


def segment_pool_acc(stage, table, sum_, cnt, normalize=True):
    """sum_ [n_clips, 512] / cnt [n_clips] f32 += the (L2-normalised) frames table [W, 3] int32 = (clip, first_frame, n_frames)
    selects from stage [W, T, 512] (f32 / bf16; the window stride may exceed T * 512: a stage view of a [W, S, T, 512] stack)."""
    W, T, Cc = stage.shape
    assert Cc == 512 and stage.stride(2) == 1 and stage.stride(1) == Cc and table.dtype == torch.int32 and table.shape == (W, 3)
    assert table.is_contiguous() and sum_.is_contiguous() and sum_.shape[1] == Cc and cnt.shape == (sum_.shape[0],)
    _lib.check(_lib.lib().tan_segment_pool_acc(_ptr(stage), _dt(stage), stage.stride(0), T, _ptr(table), W, int(normalize), _f32(sum_),
                                               _f32(cnt), sum_.shape[0], _stream()), "tan_segment_pool_acc")


def segment_pool_final(sum_, cnt, out, normalize=True):
    """out [n_clips, 512] f32 = sum_ / cnt, L2-normalised when `normalize` (tan_segment_pool_final)."""
    assert out.shape == sum_.shape and out.is_contiguous()
    _lib.check(_lib.lib().tan_segment_pool_final(_f32(sum_), _f32(cnt), sum_.shape[0], int(normalize), _f32(out), _stream()),
               "tan_segment_pool_final")
    return out


def window_feat_acc(feat, table, acc, cnt):
    """acc [n_rows, 512] / cnt [n_rows] f32 += one pass (tan_window_feat_acc); feat [W, T, 512] (f32 / bf16, window stride free):
    the last video stage of the pass's windows, table [W, 8] int32 its window table."""
    W, T, Cc = feat.shape
    assert Cc == 512 and feat.stride(2) == 1 and feat.stride(1) == Cc and table.dtype == torch.int32 and table.shape == (W, 8)
    assert table.is_contiguous() and acc.is_contiguous() and acc.shape == (cnt.numel(), Cc)
    _lib.check(_lib.lib().tan_window_feat_acc(_ptr(feat), _dt(feat), feat.stride(0), _ptr(table), W, T, _f32(acc), _f32(cnt),
                                              cnt.numel(), _stream()), "tan_window_feat_acc")


def window_feat_final(acc, cnt, out):
    """out [n_rows, 512] (bf16 / f32) = acc / max(cnt, 1) (tan_window_feat_final)."""
    assert out.shape == acc.shape and out.is_contiguous()
    _lib.check(_lib.lib().tan_window_feat_final(_f32(acc), _f32(cnt), cnt.numel(), _ptr(out), _dt(out), _stream()),
               "tan_window_feat_final")
    return out


def rerank_tail(stage_last, stage_head, table, T, head_w, head_b, out, sim=None):
    """out [W, 4] f32 <- per window of a joint pass (max cosine, window start + first arg-max as int32 bits, softmax maximum of
    cos / 0.07, alignability logit) (tan_rerank_tail; the arithmetic is in include/tan_hip.h).  stage_last / stage_head [W * L, 512]
    (f32 / bf16): the last joint stage and stage index 2 (or None, with head_w / head_b None: out[:, 3] = 0); table [W, 8] int32 the
    pass's window table; sim [W, T] f32 or None <- every frame's cosine, -inf beyond the window's t."""
    W = table.shape[0]
    L = stage_last.shape[0] // W
    assert stage_last.shape == (W * L, 512) and stage_last.is_contiguous() and table.dtype == torch.int32 and table.shape == (W, 8)
    assert table.is_contiguous() and out.dtype == torch.float32 and out.shape == (W, 4) and out.is_contiguous()
    assert stage_head is None or (stage_head.shape == stage_last.shape and stage_head.dtype == stage_last.dtype and stage_head.is_contiguous())
    assert sim is None or (sim.dtype == torch.float32 and sim.shape == (W, T) and sim.is_contiguous())
    _lib.check(_lib.lib().tan_rerank_tail(_ptr(stage_last), _ptr(stage_head), _dt(stage_last), L, T, _ptr(table), W, _f32(head_w),
                                          _f32(head_b), _f32(out), _f32(sim), _stream()), "tan_rerank_tail")
    return out


def rerank_select(score, k, stride=1, out=None):
    """out [Q, k] int32 <- per query the k of its P <= 32 candidates with the largest score, descending, equal scores by ascending
    candidate (tan_rerank_select).  score [Q, P] f32, or [Q, P, stride] with the score in element 0 (rerank_tail's out: stride 4)."""
    Q, P = score.shape[:2]
    assert score.dtype == torch.float32 and score.is_contiguous() and score.numel() == Q * P * stride
    if out is None:
        out = torch.empty(Q, k, dtype=torch.int32, device=score.device)
    assert out.dtype == torch.int32 and out.shape == (Q, k) and out.is_contiguous()
    _lib.check(_lib.lib().tan_rerank_select(_f32(score), Q, P, stride, k, _ptr(out), _stream()), "tan_rerank_select")
    return out


def topk_fold(run, incoming, shard, reset=False):
    """Fold one shard's top-k lists into the running lists, in place (tan_topk_fold; the order and the empty slots are defined in
    include/tan_hip.h).  run = (score [Q, k] f32, shard [Q, k] int32, row [Q, k] int32, aux [n_aux, Q, k] int32 or None), caller-owned
    and returned; incoming = (score [Q, k_in] f32, row [Q, k_in] int32, then n_aux int32 [Q, k_in] payload columns), k_in <= k <= 32,
    n_aux <= 3; `shard`: the number the incoming entries get.  reset: the run lists' old content is ignored (they may be
    uninitialised).  The run lists end as the k best of both by (score descending, shard ascending, row ascending)."""
    r_score, r_shard, r_row, r_aux = run
    in_score, in_row, *in_aux = incoming
    Q, k = r_score.shape
    k_in, n_aux = in_score.shape[1], len(in_aux)
    assert r_score.dtype == torch.float32 and r_score.dim() == 2 and r_score.is_contiguous()
    assert all(t.dtype == torch.int32 and t.shape == (Q, k) and t.is_contiguous() for t in (r_shard, r_row))
    assert in_score.dtype == torch.float32 and in_score.shape == (Q, k_in) and in_score.is_contiguous()
    assert all(t.dtype == torch.int32 and t.shape == (Q, k_in) and t.is_contiguous() for t in (in_row, *in_aux))
    assert (r_aux is None and n_aux == 0) or (r_aux is not None and r_aux.dtype == torch.int32 and r_aux.shape == (n_aux, Q, k)
                                               and r_aux.is_contiguous())
    aux = [_ptr(t) for t in in_aux] + [None] * (3 - n_aux) if n_aux <= 3 else [None] * 3   # n_aux > 3: the entry point refuses it
    _lib.check(_lib.lib().tan_topk_fold(_f32(r_score), _ptr(r_shard), _ptr(r_row), _ptr(r_aux), Q, k, n_aux, int(bool(reset)),
                                        _f32(in_score), _ptr(in_row), *aux, k_in, int(shard), _stream()), "tan_topk_fold")
    return run


def clip_chunk():
    """elements per chunk of the gradient-clipping tables (tan_clip_chunk)"""
    return int(_lib.lib().tan_clip_chunk())


def _clip_ranges(g, chunk_table, seg_table, chunks, segs, partials, norms=None):
    """the chunk / segment ranges of one clipping launch against the sizes of its tables and buffers: the kernels index all of them"""
    (c0, c1), (s0, s1) = chunks, segs
    ok = (g.dtype == torch.float32 and g.dim() == 1 and g.is_contiguous() and g.numel() < 2 ** 31
          and chunk_table.dtype == torch.int32 and chunk_table.dim() == 2 and chunk_table.shape[1] == 4 and chunk_table.is_contiguous()
          and seg_table.dtype == torch.int32 and seg_table.dim() == 2 and seg_table.shape[1] == 2 and seg_table.is_contiguous()
          and 0 <= c0 <= c1 <= chunk_table.shape[0] and 0 <= s0 <= s1 <= seg_table.shape[0]
          and partials.is_contiguous() and partials.numel() >= c1 and (norms is None or (norms.is_contiguous() and norms.numel() >= s1)))
    if not ok:
        raise _lib.TanHipError(f"gradient clipping: chunks {chunks} / segments {segs} do not fit the tables or buffers")
    return c0, c1, s0, s1


def clip_sumsq(g, chunk_table, seg_table, chunks, segs, partials):
    """partials[c] = sum of squares of chunk c of the flat f32 gradient g, for the chunks [c0, c1) (tan_clip_sumsq; tables: include/tan_hip.h)"""
    c0, c1, s0, s1 = _clip_ranges(g, chunk_table, seg_table, chunks, segs, partials)
    _lib.check(_lib.lib().tan_clip_sumsq(_f32(g), _ptr(chunk_table), _ptr(seg_table), c0, c1, s0, s1, g.numel(), _f32(partials), _stream()),
               "tan_clip_sumsq")


def clip_apply(g, chunk_table, seg_table, chunks, segs, partials, clip, grad_scale, norms):
    """per segment of [s0, s1): norms[s] = ||g_s|| * grad_scale from the partials; g_s *= clip / (norm + 1e-6) where that is below 1
    (tan_clip_apply: utils/train_utils.py:3-13)"""
    c0, c1, s0, s1 = _clip_ranges(g, chunk_table, seg_table, chunks, segs, partials, norms)
    _lib.check(_lib.lib().tan_clip_apply(_f32(g), _ptr(chunk_table), _ptr(seg_table), c0, c1, s0, s1, g.numel(), _f32(partials),
                                         float(clip), float(grad_scale), _f32(norms), _stream()), "tan_clip_apply")
