"""CPU side of test_encoder_stack_gpu.py: its bf16 bounds must still catch a wrong or missing piece of a stack's backward, and the
C ABI refuses layer_done together with a dw_stream tail (include/tan_hip.h, tan_encoder_desc) without touching a device."""
import ctypes as C
from types import SimpleNamespace

import torch

from temporalalignnet_amd import _lib
from test_encoder_stack_gpu import BF16_FWD_REL, BF16_GRAD_REL, GRADS, LNS, MATS, POST, PREFIX, W, reference, rel_err


def _stack_run(B, L, layers, seed=3):
    """fp64 weights / inputs on the CPU, shaped like test_encoder_stack_gpu.Run for reference()"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    p = {}
    for i in range(layers):
        base = f"{PREFIX}.resblocks.{i}."
        for wn, bn, N, K in MATS.values():
            p[base + wn], p[base + bn] = rn(N, K) * K ** -0.5, 0.1 * rn(N)
        for n in LNS.values():
            p[base + n] = (1 + 0.1 * rn(W)) if n.endswith("weight") else 0.1 * rn(W)
    p[POST + ".weight"], p[POST + ".bias"] = 1 + 0.1 * rn(W), 0.1 * rn(W)
    mask = torch.zeros(B, L, dtype=torch.uint8)
    mask[B - 1, L - L // 4:] = 1
    return SimpleNamespace(st=SimpleNamespace(ref=p), B=B, L=L, S=layers, x0=rn(B * L, W), mask=mask,
                           d_stage=[rn(B * L, W) for _ in range(layers)])


def _worst_over_bound(got, ref, bound):
    return max(rel_err(got[k], ref[k]) / bound for k in ref)


def test_the_bf16_bounds_catch_a_missing_panel_or_stage_gradient():
    """B=16, L=64, two blocks (R = 1024: 16 row panels).  Each fault must move some checked tensor by more than 3x its bound."""
    run = _stack_run(16, 64, 2)
    o, g = reference(run, device="cpu")

    def drop(gr):
        gr = gr.clone()
        gr.view(-1, W)[64:128] = 0
        return gr

    def zero_panel(i, x):            # the gradient entering block 1 (w.r.t. its output) loses rows 64..127: one row panel
        if i == 1:
            x.register_hook(drop)
        return x

    o1, g1 = reference(run, tap=zero_panel, device="cpu")
    assert _worst_over_bound(o1, o, BF16_FWD_REL) == 0            # (the hook changes no forward value)
    assert _worst_over_bound(g1, g, BF16_GRAD_REL) > 3

    run.d_stage[0] = None                                           # stage 0 (block 1's xn1) gradient dropped
    _, g2 = reference(run, device="cpu")
    assert _worst_over_bound(g2, g, BF16_GRAD_REL) > 3


def test_layer_done_with_a_dw_stream_tail_is_refused_before_any_launch():
    """no device is touched: the check comes before the first launch, every pointer is a placeholder"""
    S, fake = 2, C.c_void_p(0x1000)
    params, bufs = (_lib.LayerParams * S)(), (_lib.LayerBufs * S)()
    for i in range(S):
        for n, _ in _lib.LayerParams._fields_:
            setattr(params[i], n, fake)
        for n, _ in _lib.LayerBufs._fields_:
            setattr(bufs[i], n, fake)
    d = _lib.EncoderDesc()
    d.dtype, d.B, d.L, d.C, d.H, d.layers = _lib.TAN_BF16, 2, 64, W, 8, S
    d.x0, d.params, d.bufs = fake, params, bufs
    for n in ("post_g", "post_b", "g_post_g", "g_post_b", "post_out", "post_mean", "post_rstd", "scr_dx", "scr_dx2", "scr_do",
              "scr_dxn", "scr_dh", "scr_dqkv", "ln_ws", "d_x0"):
        setattr(d, n, fake)
    stages = (C.c_void_p * S)(fake.value, fake.value)
    events = (C.c_void_p * S)(fake.value, fake.value)
    d.d_stage, d.layer_done = stages, events
    d.dw_stream, d.dw_tail = C.c_void_p(0x2000), 1          # a stream other than the stack's (NULL here)
    assert _lib.lib().tan_encoder_bwd(C.byref(d), None) == -1
