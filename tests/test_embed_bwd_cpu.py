"""CPU side of test_embed_bwd_gpu.py: its bounds must catch a missing piece of the fused embedding backward.  The same float64
references run on the CPU at B = 129 (17 partial planes, one video in the last), T = 13; each injected fault must move some checked
tensor by more than 3x its bound."""
import torch

from test_embed_bwd_gpu import BF16_REL, F32_REL, W, embed_bwd_reference, nparts, pos_ln_bwd_reference, rel_err

B, T, N = 129, 13, 5


def _inputs(seed=3):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    proj = (rn(B * T, W) * 1.5 + 0.3).bfloat16()
    return proj, 1 + 0.2 * rn(W), rn(B * T, W).bfloat16(), rn(B * T, W).bfloat16(), {"a": rn(100, W) * 0.01, "b": rn(100, W) * 0.01}


def _worst_over_bound(got, ref):
    return max(rel_err(got[k], ref[k]) / (BF16_REL if k == "d_proj" else F32_REL) for k in ref)


def _pos_uses(planes, text_planes):
    P = nparts(B)
    return [("a", 2, T, planes["d_pos0"], P), ("a", 5, T, planes["d_pos1"], P), ("b", 1, N, text_planes, P)]


def test_the_bounds_catch_a_lost_group_plane_or_use():
    proj, gamma, d0, d1, tables = _inputs()
    ref = embed_bwd_reference(B, T, proj, gamma, d0, d1)
    ratios = {}
    for fault in ("drop_last_group", "omit_dout1"):
        ratios[fault] = _worst_over_bound(embed_bwd_reference(B, T, proj, gamma, d0, d1, fault=fault), ref)
    text_planes = torch.randn(nparts(B), N, W, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    uses = _pos_uses(ref, text_planes)
    pref = pos_ln_bwd_reference(tables, uses, gamma)
    for fault in ("drop_plane", "skip_table"):
        ratios[fault] = _worst_over_bound(pos_ln_bwd_reference(tables, uses, gamma, fault=fault), pref)
    print("\n[embed bwd] fault / bound:", {k: f"{v:.3g}" for k, v in ratios.items()})
    assert all(r > 3 for r in ratios.values()), ratios
    # the faults are what they claim: the last plane holds ONE video, the dropped plane is the clamped tail's
    assert ref["d_pos0"].shape == (17, T, W)
    assert torch.equal(ref["d_pos0"][-1], d0.double().view(B, T, W)[-1])
