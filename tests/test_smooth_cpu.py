"""Host-side pieces of the label decode: the C ABI of tan_label_decode with its argument checks, the Python argument checks of
`ops.label_decode` and `Annotation.decode / segments / label_seconds`, the three references of smooth_ref.py against each other
(float32 recurrence == int64 Viterbi on exact inputs; the recurrence's path attains the brute-force optimum on every tiny case), a
hand case, and `annotate --smooth` on the command line.  No device needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import smooth_ref as ref
from temporalalignnet_amd import _lib

i, l, p, f = C.c_int, C.c_long, C.c_void_p, C.c_float
INF = float("inf")

ENTRY_POINTS = {
    "tan_label_decode_ws_bytes": (l, [l, i]),
    "tan_label_decode": (i, [p, p, i, l, p, l, f, f, p, p, p, p]),
}


# ------------------------------------------------------------------------------------------------------------------- the C ABI
def test_library_exports_the_entry_points_with_the_headers_prototypes():
    names, protos, L = _lib.declared_symbols(), _lib.declared_prototypes(), _lib.lib()
    for name, proto in ENTRY_POINTS.items():
        assert name in names and getattr(L, name) is not None
        assert protos[name] == proto, name
        assert getattr(L, name).argtypes == proto[1] and getattr(L, name).restype == proto[0]
    assert L.tan_version() >= 102


def test_ws_bytes_is_positive_for_valid_sizes_and_minus_one_otherwise():
    L = _lib.lib()
    for k in (1, 2, 5, 31, 32):
        last = 0
        for N in (1, 63, 64, 65, 4210693, 2 ** 31 - 1):
            n = L.tan_label_decode_ws_bytes(N, k)
            assert n >= last > -1 and n >= N * (k + 1) and n - N * (k + 1) < 64, (N, k)   # a back-pointer byte per state, plus alignment
            last = n
    for N, k in ((0, 5), (-1, 5), (2 ** 31, 5), (100, 0), (100, -1), (100, 33)):
        assert L.tan_label_decode_ws_bytes(N, k) == -1


def test_bad_arguments_are_rejected_without_touching_a_device():
    L = _lib.lib()
    a = C.c_void_p(1 << 20)                            # never dereferenced: every call below fails its argument checks

    def decode(ts=a, tl=a, k=5, N=1000, v_off=a, nv=5, thr=0.5, pen=0.5, dl=a, ds=a, ws=a):
        return L.tan_label_decode(ts, tl, k, N, v_off, nv, thr, pen, dl, ds, ws, None)

    for kw in (dict(ts=None), dict(tl=None), dict(v_off=None), dict(dl=None), dict(ds=None), dict(ws=None), dict(k=0), dict(k=-1),
               dict(k=33), dict(N=0), dict(N=-4), dict(N=1 << 31), dict(nv=0), dict(nv=-1), dict(nv=1001), dict(thr=float("nan")),
               dict(thr=INF), dict(thr=-INF), dict(pen=float("nan")), dict(pen=-0.5), dict(pen=-INF)):
        assert decode(**kw) == -1, kw


def test_python_argument_checks_come_before_any_device_call():
    from temporalalignnet_amd import ops, search
    score, label, v_off = torch.zeros(9, 2), torch.zeros(9, 2, dtype=torch.int32), torch.tensor([0, 4, 9], dtype=torch.int32)
    good = dict(top_score=score, top_label=label, v_off=v_off, threshold=0.5, switch=0.25)
    for bad in (dict(top_label=label.long()), dict(top_score=score.double()), dict(top_label=label[:, :1]), dict(top_score=score.T),
                dict(top_score=torch.zeros(9, 33), top_label=torch.zeros(9, 33, dtype=torch.int32)),
                dict(top_score=torch.zeros(0, 2), top_label=torch.zeros(0, 2, dtype=torch.int32)),
                dict(v_off=v_off.long()), dict(v_off=v_off[:1]), dict(v_off=torch.arange(11, dtype=torch.int32)),
                dict(threshold=float("nan")), dict(threshold=INF), dict(threshold=-INF), dict(switch=float("nan")), dict(switch=-1.0),
                dict(ws=torch.zeros(8, dtype=torch.uint8)), dict(ws=torch.zeros(64, dtype=torch.int32)),
                dict(out=(torch.zeros(9), torch.zeros(9))), dict(out=(torch.zeros(8, dtype=torch.int32), torch.zeros(9))),
                dict(out=(torch.zeros(9, dtype=torch.int32), torch.zeros(9, dtype=torch.float64)))):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.label_decode(**kw)
    for switch in (0.0, 0.25, INF):
        with pytest.raises(_lib.TanHipError, match="device tensors"):
            ops.label_decode(**dict(good, switch=switch))              # valid, but on the host
    assert ops.label_decode_ws_bytes(9, 2) >= 27
    for N, k in ((0, 2), (9, 0), (9, 33)):
        with pytest.raises(_lib.TanHipError):
            ops.label_decode_ws_bytes(N, k)

    ann = search.Annotation(label, score, ["w", "x", "y", "z"], [0, 4, 9], ["a", "b"])
    for call in (lambda: ann.decode(float("nan"), 0.5), lambda: ann.decode(-INF, 0.5), lambda: ann.decode(INF, 0.5),
                 lambda: ann.decode(0.5, -1.0), lambda: ann.decode(0.5, float("nan")), lambda: ann.segments(0.5, 1, switch=-1.0),
                 lambda: ann.segments(-INF, 1, switch=0.5), lambda: ann.segments(0.5, 0, switch=0.5),
                 lambda: ann.segments(0.5, switch=float("nan")), lambda: ann.label_seconds(0.5, switch=float("nan")),
                 lambda: ann.label_seconds(-INF, switch=0.5), lambda: ann.label_seconds(float("nan"), switch=0.5)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: ann.decode(0.5, 0.5), lambda: ann.segments(0.5, switch=INF), lambda: ann.label_seconds(0.5, switch=0.0)):
        with pytest.raises(_lib.TanHipError, match="device tensors"):
            call()


# ------------------------------------------------------------------------------------------------------------- the references
def exact_lists(rng, N, k, L, levels=8, nonfinite=0.0):
    """[N, k] lists as tan_label_topk writes them (k distinct labels, descending scores) with scores that are multiples of
    1 / levels in [-1, 1]; a share `nonfinite` of the entries is NaN or +-inf (anywhere in a list: the decode does not care)"""
    label = np.stack([rng.permutation(L)[:k] for _ in range(N)]).astype(np.int32)
    score = -np.sort(-rng.integers(-levels, levels + 1, (N, k)), axis=1).astype(np.float32) / levels
    if nonfinite:
        bad = rng.random((N, k)) < nonfinite
        score[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), int(bad.sum()))
    return score, label


def sticky_lists(rng, N, k, L, levels=8):
    """`exact_lists` whose labels persist: a row keeps each of its labels from the row above with probability 3/4, so paths that stay
    exist and ties between them are common"""
    score, label = exact_lists(rng, N, k, L, levels)
    for t in range(1, N):
        keep = rng.random(k) < 0.75
        row = [int(x) for x, kp in zip(label[t - 1], keep) if kp]
        row += [int(x) for x in rng.permutation(L) if x not in row][:k - len(row)]
        label[t] = rng.permutation(row)
    return score, label


def test_the_float32_reference_equals_the_int64_one_on_exact_inputs():
    rng = np.random.default_rng(7)
    for k, L in ((1, 3), (2, 3), (5, 8), (32, 40)):
        N = 400 if k < 32 else 150
        score, label = sticky_lists(rng, N, k, L)
        score[rng.random((N, k)) < 0.03] = np.nan
        score[rng.random((N, k)) < 0.02] = -np.inf
        v_off = [0, 1, 3, 66, 130, N]
        labelled = 0
        for thr, pen in ((0.0, 0.0), (0.25, 0.5), (-0.5, 0.125), (0.125, 3.0), (0.25, INF)):
            a, b = ref.decode_f32(score, label, v_off, thr, pen), ref.decode_i64(score, label, v_off, thr, pen, 1 / 8)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)), (k, thr, pen)
            assert ((a[0] == -1) == np.isneginf(a[1])).all()
            labelled += int((a[0] != -1).sum())
        assert labelled > N                                            # the sweep is not all background


def test_the_recurrence_attains_the_brute_force_optimum_on_every_tiny_case():
    """T <= 6, k <= 2: scores, threshold and penalty are multiples of 1/8 in [-1, 1] (the penalty in [0, 1], and 0 and +inf more
    often than chance), labels from three so that lists share labels, some scores not finite.  Sums of eighths are exact in f32."""
    rng = np.random.default_rng(11)
    eighths = np.arange(-8, 9) / 8
    cases = 0
    for T in range(1, 7):
        for k in (1, 2):
            for _ in range(40):
                score, label = (sticky_lists if rng.random() < 0.7 else exact_lists)(rng, T, k, 3)
                score[rng.random((T, k)) < 0.05] = rng.choice(np.array([np.nan, -np.inf, np.inf], dtype=np.float32))
                thr = float(rng.choice(eighths))
                pen = float(rng.choice([0.0, INF, *eighths[eighths >= 0]]))
                states = ref.states_f32(score, label, thr, pen)
                got, best = ref.objective(states, score, label, thr, pen), ref.brute_force(score, label, thr, pen)
                assert got == best, (T, k, thr, pen, score, label, states)
                assert states == ref.states_i64([[None if not np.isfinite(x) else int(x * 8) for x in r] for r in score], label,
                                                int(thr * 8), None if pen == INF else int(pen * 8))
                cases += 1
    assert cases == 480


# ---- a hand case: twelve seconds of one video, k = 2, threshold 1/2.  Label 0 scores 7/8 except for a two-second dip to 1/4
# (seconds 3, 4), a one-second flicker (second 7: label 1 scores 3/4, label 0 5/8) and a tail of 1/8 (seconds 10, 11).
HAND_SCORE = np.array([[.875, 0], [.875, 0], [.875, 0], [.25, 0], [.25, 0], [.875, 0], [.875, 0], [.75, .625], [.875, 0], [.875, 0],
                       [.125, 0], [.125, 0]], dtype=np.float32)
HAND_LABEL = np.array([[0, 1]] * 7 + [[1, 0]] + [[0, 1]] * 4, dtype=np.int32)
HAND_RAW = [0, 0, 0, -1, -1, 0, 0, 1, 0, 0, -1, -1]                   # the per-second choice: what penalty 0 gives
HAND_SMOOTH = [0] * 10 + [-1, -1]                                      # penalty 1/2: the dip and the flicker are bridged, the tail is not


def test_hand_case_bridges_a_dip_and_a_flicker_at_one_half_and_not_at_zero():
    for decode in (lambda thr, pen: ref.decode_f32(HAND_SCORE, HAND_LABEL, [0, 12], thr, pen),
                   lambda thr, pen: ref.decode_i64(HAND_SCORE, HAND_LABEL, [0, 12], thr, pen, 1 / 8)):
        lab, sc = decode(0.5, 0.0)
        assert lab.tolist() == HAND_RAW
        assert sc.tolist() == [.875, .875, .875, -INF, -INF, .875, .875, .75, .875, .875, -INF, -INF]
        # staying through the dip costs 2 * (1/4 - 1/2) = -1/2, leaving and coming back two penalties = -1; staying on label 0
        # at second 7 gains 1/8 where label 1 gains 1/4 but costs two penalties; the tail costs 2 * -3/8 against one penalty
        lab, sc = decode(0.5, 0.5)
        assert lab.tolist() == HAND_SMOOTH
        assert sc.tolist() == [.875, .875, .875, .25, .25, .875, .875, .625, .875, .875, -INF, -INF]   # a bridged second's own score
        lab, _ = decode(0.5, INF)                                       # one label for the whole video: label 0 gains 21/8 in all
        assert lab.tolist() == [0] * 12
        lab, _ = decode(0.5, 0.25)                                      # 1/4: the flicker is still bridged (1/8 against 1/4 - 1/2)
        assert lab.tolist()[5:10] == [0] * 5 and lab.tolist()[10:] == [-1, -1]     # (the dip costs 1/2 either way: a tie, not asserted)
    # penalty 3/8 still bridges the dip (-1/2 against -3/4) -- unless the video ends inside it: leaving costs one penalty then.
    # Videos do not see each other: the second one starts on label 0 as if nothing came before.
    assert ref.decode_f32(HAND_SCORE, HAND_LABEL, [0, 12], 0.5, 0.375)[0].tolist() == HAND_SMOOTH
    assert ref.decode_f32(HAND_SCORE, HAND_LABEL, [0, 5, 12], 0.5, 0.375)[0].tolist() == [0, 0, 0, -1, -1, 0, 0, 0, 0, 0, -1, -1]


# ------------------------------------------------------------------------------------------------------------- command line
def test_cli_accepts_smooth_and_refuses_the_conflicts():
    from temporalalignnet_amd import search
    argv = ["annotate", "--checkpoint", "c", "--vocab", "/nonexistent/s3d_dict.npy", "--index", "i.npz", "--labels", "steps.txt", "--out",
            "o.csv"]
    assert search.parse_args(argv).smooth is None
    a = search.parse_args(argv + ["-k", "5", "--threshold", "0.25", "--smooth", "0.5", "--min-len", "3"])
    assert (a.k, a.threshold, a.smooth, a.min_len, a.per_second) == (5, 0.25, 0.5, 3, False)
    assert search.parse_args(argv + ["--threshold", "-0.5", "--smooth", "0"]).smooth == 0.0
    assert search.parse_args(argv + ["--threshold", "0", "--smooth", "inf"]).smooth == INF
    for bad in (["--smooth", "0.5"], ["--smooth", "0.5", "--threshold=-inf"], ["--smooth", "0.5", "--threshold", "inf"],
                ["--smooth", "0.5", "--threshold", "nan"], ["--smooth=-0.5", "--threshold", "0.25"], ["--smooth", "nan", "--threshold", "0.25"],
                ["--smooth", "0.5", "--per-second"], ["--smooth", "0.5", "--threshold", "0.25", "--per-second"], ["--smooth"]):
        with pytest.raises(SystemExit):
            search.parse_args(argv + bad)
    # --per-second keeps its rules without --smooth
    assert search.parse_args(argv + ["--per-second"]).per_second
    with pytest.raises(SystemExit):
        search.parse_args(argv + ["--per-second", "--threshold", "0.1"])
