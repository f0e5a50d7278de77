"""CPU side of test_optim_fp64_gpu.py: its references, bounds and image oracle checked without a GPU.  The f32 restatement of the
kernel's operation order (ref32) and torch.optim.AdamW itself must both sit inside the fp64 bounds on the test's own inputs, the
bounds must catch a wrong formula, the trajectory figure of ref32 must be within twice torch.optim.AdamW's, and the expected-state
builder of the image tests must be consistent with itself (windows add up to a whole call)."""
import pytest
import torch

from test_optim_fp64_gpu import (DEFAULT_ENTRIES, F32, HP, PLAIN_ENTRIES, STATE_KEYS, Table, bits, bits_equal, check64, check_ema64,
                                 check_statements, ema_ref32, expected_images_call, make_inputs, pack_index, ratio, ref32, ref64,
                                 torch_adamw_trajectory, trajectory_errors, trajectory_inputs, transpose_index, GUARD, S16, S32)

HPS = [HP(lr=lr, wd=wd, betas=betas, eps=eps, step=step, grad_scale=gs)
       for (lr, wd) in ((1e-3, 1e-2), (1e-4, 0.0), (0.0, 0.1)) for step in (1, 2, 1000, 200000)
       for (betas, eps, gs) in (((0.9, 0.999), 1e-8, 1.0), ((0.9, 0.98), 1e-6, 1.0 / 3.0), ((0.9, 0.999), 1e-8, 0.125))]


def torch_adamw_step(inp, hp):
    """one torch.optim.AdamW(foreach=False) step in f32 from the given state"""
    w = torch.nn.Parameter(inp["p"].clone())
    opt = torch.optim.AdamW([w], lr=hp.lr, betas=(hp.beta1, hp.beta2), eps=hp.eps, weight_decay=hp.wd, foreach=False)
    opt.state[w] = {"step": torch.tensor(float(hp.step - 1)), "exp_avg": inp["m"].clone(), "exp_avg_sq": inp["v"].clone()}
    w.grad = inp["g"] * torch.tensor(hp.grad_scale, dtype=F32)
    opt.step()
    s = opt.state[w]
    assert int(s["step"]) == hp.step
    return dict(p=w.detach(), m=s["exp_avg"], v=s["exp_avg_sq"])


@pytest.mark.parametrize("i", range(len(HPS)))
def test_ref32_and_torch_adamw_sit_inside_the_fp64_bounds(i):
    hp = HPS[i]
    inp = make_inputs(4096 + 257, seed=40 + i)
    args = (inp["p"], inp["g"], inp["m"], inp["v"])
    ones = torch.ones(inp["p"].numel(), dtype=torch.uint8)
    r = ref32(*args, ones, hp)
    check64("cpu/ref32", r, *args, ones, hp)
    check_statements(inp, r, ones, hp)
    check64("cpu/torch", torch_adamw_step(inp, hp), *args, ones, hp)
    mode = (torch.arange(inp["p"].numel()) % 4).to(torch.uint8)
    r = ref32(*args, mode, hp)
    check64("cpu/ref32", r, *args, mode, hp)
    check_statements(inp, r, mode, hp)
    for k in "pmv":
        assert bits_equal(r[k][mode >= 2], inp[k][mode >= 2])
    for m in (0.0, 0.999, 1.0):
        check_ema64("cpu/ref32", ema_ref32(inp["e"], r["p"], m), inp["e"], r["p"], m)


def test_the_bounds_catch_a_wrong_formula():
    hp = HP(step=3, grad_scale=0.5)
    inp = make_inputs(4096, seed=7)
    args = (inp["p"], inp["g"], inp["m"], inp["v"])
    ones = torch.ones(4096, dtype=torch.uint8)
    want = ref64(*args, ones, hp)
    # eps inside the division by bc2_sqrt (= eps / bc2_sqrt outside it), a doubled decay, the next step's bias corrections, a beta2
    # off by 1e-7: each leaves some tensor outside its bound
    for wrong in (HP(step=3, grad_scale=0.5, eps=1e-8 / (1 - 0.999 ** 3) ** 0.5), HP(step=3, grad_scale=0.5, wd=2e-2), HP(step=4, grad_scale=0.5),
                  HP(step=3, grad_scale=0.5, betas=(0.9, 0.9990001))):
        got = ref32(*args, ones, wrong)
        worst = max(ratio(got[k], want[k], want["b" + k], want["skip_" + k] if k != "m" else None) for k in "pmv")
        assert worst > 1.0, worst


def test_trajectory_of_the_f32_restatement_is_within_twice_torch_adamw():
    from test_optim_fp64_gpu import TRAJ_HP
    p0, gs = trajectory_inputs()

    def stepper(p, g, m, v, step):
        r = ref32(p, g, m, v, None, HP(step=step, **TRAJ_HP))
        return r["p"], r["m"], r["v"]
    ours, ref = trajectory_errors(p0, gs, stepper), torch_adamw_trajectory(p0, gs)
    print("trajectory (p, m, v): ref32", ours, "torch.optim.AdamW", ref)
    for a, b in zip(ours, ref):
        assert 0 < a <= 2.0 * b and b < 1e-5


def test_pack_index_states_the_documented_layout():
    for (N, K, tn_w, tk_w, tn_t, tk_t) in DEFAULT_ENTRIES:
        for (n, k, tn, tk) in ((N, K, tn_w, tk_w), (K, N, tn_t, tk_t)):
            if tn:
                idx = pack_index(n, k, tn, tk)
                assert torch.equal(torch.sort(idx)[0], torch.arange(n * k))
    # general format, [2048][512] in tiles [256][32]: positions written out by hand from the header's description
    K = 512
    idx = pack_index(2048, K, 256, 32).view(8, 16, 8, 1, 2, 64, 8)      # [n-block][k-block][wave][row block][k step][lane][8]
    assert idx[0, 0, 0, 0, 0, 0].tolist() == list(range(8))
    assert idx[0, 0, 0, 0, 0, 4, 0].item() == 16 * K                    # lane 4: f(4) = 16
    assert idx[0, 0, 0, 0, 0, 8, 0].item() == 4 * K                     # lane 8: f(8) = 4
    assert idx[0, 0, 0, 0, 0, 32, 0].item() == 8                        # upper half-wave: the next 8 k
    assert idx[0, 0, 0, 0, 1, 0, 0].item() == 16                        # k step 1
    assert idx[0, 0, 3, 0, 0, 1, 0].item() == (3 * 32 + 1) * K          # wave 3 owns rows 96..127
    assert idx[2, 5, 7, 0, 1, 45, 3].item() == (2 * 256 + 7 * 32 + (1 + 4 + 16)) * K + 5 * 32 + 16 + 8 + 3
    idx = pack_index(512, 2048, 512, 16).view(1, 128, 8, 2, 1, 64, 8)
    assert idx[0, 9, 2, 1, 0, 33, 2].item() == (2 * 64 + 32 + 1) * 2048 + 9 * 16 + 8 + 2
    # "qkv16": tile (head pair, k step) of 24 fragments; fragment 13 = wave 4, fb 1: head 1 of the pair, which = 0 (q), fblk 1
    idx = pack_index(1536, K, 384, 32).view(4, 16, 24, 64, 8)
    assert idx[1, 2, 13, 18, 5].item() == (0 * 512 + (2 * 1 + 1) * 64 + 1 * 16 + 2) * K + 2 * 32 + 8 * 1 + 5
    assert idx[3, 15, 23, 63, 7].item() == (2 * 512 + 7 * 64 + 3 * 16 + 15) * K + 15 * 32 + 24 + 7
    assert idx[0, 0, 4, 0, 0].item() == 512 * K                         # fragment 4: k of head 0
    t = transpose_index(64, 192)
    assert t[5 * 64 + 3].item() == 3 * 192 + 5


def _fresh(tab, inp):
    n = tab.n
    st = {}
    for k in STATE_KEYS:
        if k in inp or k == "mode":
            x = tab.mode if k == "mode" else inp[k]
            buf = torch.empty(n + GUARD, dtype=x.dtype)
            (bits(buf) if x.dtype == F32 else buf)[n:] = S32 if x.dtype == F32 else 0xA5
            buf[:n] = x
        else:
            buf = torch.full((n + GUARD,), S16, dtype=torch.int16).view(torch.bfloat16)
        st[k] = buf
    return st


def test_the_test_tables_partition_and_the_expected_windows_add_up():
    tab = Table(DEFAULT_ENTRIES[1:2] + PLAIN_ENTRIES + DEFAULT_ENTRIES[5:], modes=[1, 0, 2, 3, 1])
    count = torch.zeros(tab.n, dtype=torch.int32)
    count[tab.owned] += 1
    count[tab.rest] += 1
    count[tab.nobody] += 1
    assert (count == 1).all() and tab.nobody.numel() > 8 and all(o % 8 == 0 for o in tab.offs)
    assert tab.unit_of.max().item() == tab.n_units - 1 and (torch.bincount(tab.unit_of[tab.owned]) == 4096).all()
    inp = make_inputs(tab.n, seed=9)
    hp = HP(step=4, grad_scale=0.5)
    whole, touched = expected_images_call(tab, _fresh(tab, inp), hp, 0.999, rest=tab.rest)
    assert int(touched.sum()) == tab.n - tab.nobody.numel()
    st = _fresh(tab, inp)
    a, b = 37, tab.prefix[2] + 1
    for units, rest in (((0, a), None), ((a, b), None), ((b, 0), None), ((tab.n_units, tab.n_units), tab.rest)):
        st, _ = expected_images_call(tab, st, hp, 0.999, units=units, rest=rest)
    for k in STATE_KEYS:
        assert torch.equal(bits(st[k]), bits(whole[k])), k
    n = tab.n
    for (N, K, *_), o, md in zip(tab.entries, tab.offs, [1, 0, 2, 3, 1]):
        sl = slice(o, o + N * K)
        W = whole["p"][:n][sl].bfloat16().view(N, K)
        assert bits_equal(whole["p16"][:n][sl], W.reshape(-1)) and bits_equal(whole["pt"][:n][sl], W.t().reshape(-1))
        assert bits_equal(whole["p"][:n][sl], inp["p"][sl]) == (md >= 2)
    assert (bits(whole["pt"])[:n][~tab.owned] == S16).all() and (bits(whole["e16"])[:n][tab.nobody] == S16).all()
