"""The fp64 family reference of tests/test_simfam_fp64_gpu.py on the CPU: its input builder keeps its promises, the reference agrees
with the golden-tested `loss_ref.get_loss`, and six faults a family kernel could have -- applied to the reference's own output --
each move a checked quantity by more than three times its bound.

With `randn` features in place of the structured ones (`make_case(randn=True)`, the inputs of tests/test_simfam_gpu.py) all six
faults are still caught against the fp64 reference, but the two that depend on the inputs' structure by much less: the dropped
projection term of the normalisation's backward reaches 6 times its bound instead of 209 (a gradient nearly orthogonal to its row
has little to project out), the missing row panel 713 instead of 6673.  Factors, structured / randn: leak ignored 7.7e6 / 7.7e6,
panel missing 6673 / 713, wrong sentence 419 / 237, projection dropped 209 / 6.2, one stage 68 / 87, neighbour block 7.7e6 / 7.7e6."""
import pytest
import torch

from oracle import loss_ref
from test_loss_kernels_gpu import FILL_TOL
from test_simfam_fp64_gpu import GRAD_REL, ROW_REL, TERM_ATOL, K, grad_errors, make_case, reference

DUAL = K(3, 4, 24, 8, "dual")
JOINT = K(2, 8, 30, 8, "joint", compact=True, leak=True, mc_round=8)        # R = 240: two 128-row panels


@pytest.mark.parametrize("spec", [DUAL, JOINT], ids=["dual", "joint"])
def test_builder_and_reference_are_consistent(spec):
    case = make_case(seed=5, **spec)                                          # (its asserts are the builder's promises)
    ref = reference(case)
    S, B, T, N = case["S"], case["B"], case["T"], case["N"]
    assert ref["cos"].shape == (S, B * T, B * N) and ref["t_terms"].shape == (S, int((~case["tpad"]).sum()))
    assert torch.allclose(ref["vn"].norm(dim=-1), torch.ones(S, B * T, dtype=torch.float64), atol=1e-12)
    # the normalisation's backward written out, from the gradient towards the unit rows: the autograd of the whole reference is it
    d_vn, _ = _unit_grads(case, ref)
    want = (d_vn - ref["vn"] * (ref["vn"] * d_vn).sum(-1, keepdim=True)) * ref["inv_v"][..., None]
    for s in range(S):
        assert grad_errors(want[s], ref["d_video"][s])[0] < 1e-12


def test_reference_agrees_with_get_loss():
    """`nce_family_ref` against the NCE terms inside `loss_ref.get_loss` (pinned to the goldens by tests/test_oracle_golden.py) on a
    batch both take: the same stage features as dual and as joint logits, targets from the batch's time stamps."""
    from oracle import train_ref
    from temporalalignnet_amd import synth
    B, T, S = 4, 16, 2
    b = train_ref.to_torch_batch(synth.make_batch(9, B=B, T=T, n_min=2, n_max=5))
    N = b["text_embed"].shape[1]
    case = make_case(seed=11, **K(S, B, T, N, "joint"))
    tpad = b["text_padding_mask"].bool()
    tgt_raw, _, _ = loss_ref.mask_from_time(b["start"], b["end"], T, N)
    tgt = tgt_raw.permute(0, 2, 1).float()
    ref = loss_ref.nce_family_ref([x.double() for x in case["x_video"]], case["v_grp"], [x.double() for x in case["x_text"]],
                                  case["t_grp"], tgt, tpad, None, B, T, N)
    logits = ref["cos"].view(S, B, T, B, N).permute(1, 0, 2, 3, 4)
    out, aux = loss_ref.get_loss(b, b["video"], b["text_embed"], b["padding_mask"], tpad, {"logits_dual": logits, "logits_joint": logits},
                                 loss_ref.default_args(model="init"))
    rows_pos, cols_pos = aux["tgt_cols"].sum(-1) > 0, aux["tgt_cols"].sum(-2) > 0
    mine = (ref["v_terms"][:, rows_pos].mean() + ref["t_terms"][:, cols_pos].mean()) / 2
    assert abs(mine.item() - out["loss-dual"].item()) < 1e-12 and abs(mine.item() - out["loss-joint"].item()) < 1e-12


def _unit_grads(case, ref, stages=None):
    """d loss / d (unit frame rows, unit sentence rows) of the reference; `stages`: the loss of those stages only."""
    vn, tn = ref["vn"].clone().requires_grad_(True), ref["tn"].clone().requires_grad_(True)
    r = loss_ref.nce_family_ref([x.double() for x in case["x_video"]], case["v_grp"], [x.double() for x in case["x_text"]],
                                case["t_grp"], case["tgt"], case["tpad"], case["row_leak"], case["B"], case["T"], case["N"], unit=(vn, tn))
    keep = ~case["tpad"].view(-1)
    w = torch.ones(case["S"], 1, dtype=torch.float64)
    if stages is not None:
        w = torch.zeros(case["S"], 1, dtype=torch.float64)
        w[stages] = 1.0
    ((r["v_terms"] * case["g_v"].double() * w).sum() + (r["t_terms"] * case["g_t_pad"].double()[:, keep] * w).sum()).backward()
    return vn.grad, tn.grad


def _term_factor(a, b):
    """Worst |a - b| in units of the bound check 2 has for that entry (FILL_TOL where either is an empty-positive fill)."""
    bound = torch.where((a > 5e4) | (b > 5e4), torch.tensor(FILL_TOL, dtype=torch.float64), torch.tensor(TERM_ATOL, dtype=torch.float64))
    return ((a - b).abs() / bound).max().item()


def _grad_factor(got, want):
    et, er = grad_errors(got, want)
    return max(et / GRAD_REL, er / ROW_REL)


def fault_factors(randn):
    dual, joint = make_case(seed=5, randn=randn, **DUAL), make_case(seed=5, randn=randn, **JOINT)
    rd, rj = reference(dual), reference(joint)
    f = {}
    B, T, N, S = joint["B"], joint["T"], joint["N"], joint["S"]
    keep = ~joint["tpad"].view(-1)
    # 1. leak flags ignored
    no_leak = reference(dict(joint, row_leak=None), grads=False)
    f["leak ignored"] = max(_term_factor(no_leak["v_terms"], rj["v_terms"]), _term_factor(no_leak["t_terms"], rj["t_terms"]))
    # 2. the second 128-row panel missing from the column sums
    x = (rj["cos"] / loss_ref.TEMPERATURE).view(S, B, T, B, N).clone()
    lk = joint["row_leak"].view(B, T).bool()
    for b in range(B):
        x[:, b, lk[b], b, :] = loss_ref.FILL
    x = x.view(S, B * T, B * N)[:, :, keep]
    rows = torch.ones(B * T, dtype=torch.bool)
    rows[128:256] = False
    f["panel missing"] = _term_factor(rj["t_terms"] - torch.logsumexp(x, 1) + torch.logsumexp(x[:, rows], 1), rj["t_terms"])
    # 3. one compacted column mapped to its neighbour's sentence
    t = rj["t_terms"]
    f["wrong sentence"] = _term_factor(t[:, 1:2], t[:, 2:3])
    # 4. the projection term of the normalisation's backward dropped
    d_vn, _ = _unit_grads(joint, rj)
    f["projection dropped"] = max(_grad_factor(d_vn[s] * rj["inv_v"][s][:, None], rj["d_video"][s]) for s in range(S))
    # 5. the dual family's text gradient from one stage instead of the sum over stages
    _, d_tn0 = _unit_grads(dual, rd, stages=[0])
    one = (d_tn0[0] - rd["tn"][0] * (rd["tn"][0] * d_tn0[0]).sum(-1, keepdim=True)) * rd["inv_t"][0][:, None]
    f["one stage"] = _grad_factor(one, rd["d_text"][0])
    # 6. positives read from the neighbouring video's block
    rolled = reference(dict(joint, tgt=joint["tgt"].roll(1, 0)), grads=False)
    f["neighbour block"] = _term_factor(rolled["v_terms"], rj["v_terms"])
    return f


def test_faults_move_a_checked_quantity():
    f = fault_factors(randn=False)
    print("structured:", {k: round(v, 1) for k, v in f.items()})
    assert all(v > 3.0 for v in f.values()), f
    r = fault_factors(randn=True)
    print("randn:", {k: round(v, 1) for k, v in r.items()})
    assert r["projection dropped"] < f["projection dropped"] / 10, (r, f)      # (what the structured features buy)
