"""The label decode on the GPU: tan_label_decode / `ops.label_decode` against smooth_ref.py with `==` -- the int64 Viterbi on
exact-arithmetic inputs, the float32 recurrence on random floats (the definition has no contraction, so no tolerance applies) --
its properties, and `Annotation.decode / segments(switch=) / label_seconds(switch=)` and `annotate --smooth` end to end.

A wave decodes one video and walks its back-pointers back in blocks of 64 rows: the videos hold 1, 2, 63, 64, 65, 129 and 200 rows
(the block edge exactly, one past, twice plus one), seven videos -- more than a workgroup's four waves -- and a single video alone.
k runs over 1, 2, 5, 31 and 32 (33 live lanes), about 40 labels.  Outputs and scratch start as garbage, the scratch at an odd
address, and guard regions around all three are checked."""
import functools

import numpy as np
import pytest
import torch

import smooth_ref as ref
from test_smooth_cpu import HAND_LABEL, HAND_SCORE, exact_lists, sticky_lists

pytestmark = pytest.mark.gpu

INF = float("inf")
KS = (1, 2, 5, 31, 32)
L = 40
LAYOUTS = {"seven": [1, 2, 63, 64, 65, 129, 200], "one": [200], "a single row": [1]}
PARAMS = ((0.0, 0.0), (0.25, 0.5), (-0.125, 0.125), (0.125, 2.0), (0.25, INF))          # (threshold, penalty): eighths
GUARD = 64


def _ops():
    from temporalalignnet_amd import ops
    return ops


def _srch():
    from temporalalignnet_amd import search
    return search


def _v_off(layout):
    return np.concatenate([[0], np.cumsum(LAYOUTS[layout])]).astype(np.int64)


def _dev(v_off):
    return torch.from_numpy(np.asarray(v_off).astype(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def _lists(kind, k, layout):
    """(score f32 [N, k], label int32 [N, k]) on the host, seeded by the case.  exact: eighths with NaN and -inf entries; float:
    distinct random floats (no two gains of a row are equal) with NaN and +-inf entries"""
    N = int(_v_off(layout)[-1])
    rng = np.random.default_rng(1000 * k + len(layout) + (7 if kind == "exact" else 0))
    score, label = sticky_lists(rng, N, k, max(L, k + 1))
    if kind == "float":
        score = -np.sort(-rng.uniform(-1, 1, (N, k)).astype(np.float32), axis=1)
        assert all(len(set(r)) == k for r in score.tolist())
        bad = rng.random((N, k)) < 0.04
        score[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), int(bad.sum()))
    else:
        score[rng.random((N, k)) < 0.03] = np.nan
        score[rng.random((N, k)) < 0.02] = -np.inf
    return score, label


@functools.lru_cache(maxsize=None)
def _want(kind, k, layout, thr, pen):
    """the reference's (dec_label, dec_score), computed once per case and shared"""
    score, label = _lists(kind, k, layout)
    if kind == "exact":
        return ref.decode_i64(score, label, _v_off(layout), thr, pen, 1 / 8)
    return ref.decode_f32(score, label, _v_off(layout), thr, pen)


def _decode(score, label, v_off, thr, pen):
    """ops.label_decode into garbage-filled, guarded outputs and scratch (at an odd address) -> (dec_label, dec_score) on the host;
    asserts that the guards are untouched"""
    ops = _ops()
    score, label = torch.as_tensor(score).cuda(), torch.as_tensor(label).cuda()
    N, k = score.shape
    need = ops.label_decode_ws_bytes(N, k)
    ws = torch.full((GUARD + 3 + need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    dl = torch.full((N + 2 * GUARD,), -77, dtype=torch.int32, device="cuda")
    ds = torch.full((N + 2 * GUARD,), -77.0, device="cuda")
    out = (dl[GUARD:GUARD + N], ds[GUARD:GUARD + N])
    got_l, got_s = ops.label_decode(score, label, _dev(v_off), thr, pen, out=out, ws=ws[GUARD + 3:GUARD + 3 + need])
    assert got_l.data_ptr() == out[0].data_ptr() and got_s.data_ptr() == out[1].data_ptr()
    assert (ws[:GUARD + 3] == 0xA5).all() and (ws[GUARD + 3 + need:] == 0xA5).all()
    for t, fill in ((dl, -77), (ds, -77.0)):
        assert (t[:GUARD] == fill).all() and (t[GUARD + N:] == fill).all()
    return got_l.cpu().numpy(), got_s.cpu().numpy()


def _same(got, want):
    return np.array_equal(got[0].astype(np.int64), want[0]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))


# ------------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("k", KS)
def test_decode_equals_the_int64_reference_on_exact_inputs(k):
    for layout in LAYOUTS:
        score, label = _lists("exact", k, layout)
        for thr, pen in PARAMS:
            got = _decode(score, label, _v_off(layout), thr, pen)
            want = _want("exact", k, layout, thr, pen)
            assert _same(got, want), (layout, thr, pen, int((got[0] != want[0]).sum()))


@pytest.mark.parametrize("k", KS)
def test_decode_equals_the_float32_reference_on_random_floats(k):
    for layout in ("seven", "one"):
        score, label = _lists("float", k, layout)
        for thr, pen in ((0.1, 0.3), (-0.2, 0.05), (0.37, INF)):
            got = _decode(score, label, _v_off(layout), thr, pen)
            want = _want("float", k, layout, thr, pen)
            assert _same(got, want), (layout, thr, pen, int((got[0] != want[0]).sum()))
            chosen = got[0] != -1
            assert np.isfinite(got[1][chosen]).all() and np.isneginf(got[1][~chosen]).all()      # NaN and +-inf are never chosen


def test_hand_case_on_the_device():
    for pen, want in ((0.0, [0, 0, 0, -1, -1, 0, 0, 1, 0, 0, -1, -1]), (0.5, [0] * 10 + [-1, -1]), (INF, [0] * 12)):
        lab, sc = _decode(HAND_SCORE, HAND_LABEL, [0, 12], 0.5, pen)
        assert lab.tolist() == want
        assert sc.tolist() == [float(HAND_SCORE[t, list(HAND_LABEL[t]).index(x)]) if x >= 0 else -INF for t, x in enumerate(want)]


@pytest.mark.parametrize("k", (1, 5, 32))
def test_penalty_zero_is_the_per_second_choice_of_label_runs(k):
    """No two scores of a row are equal and none equals the threshold: the decode at penalty 0 picks every row's best label if it
    scores above the threshold -- tan_label_runs' lab -- so the runs of the decoded columns are the runs of the lists."""
    ops = _ops()
    score, label = _lists("float", k, "seven")
    score = np.where(np.isfinite(score), score, np.float32(-2)).astype(np.float32)      # label_runs has no rule for +inf: finite lists
    score = -np.sort(-score, axis=1)
    v_off = _v_off("seven")
    thr = 0.3
    dec_l, dec_s = _decode(score, label, v_off, thr, 0.0)
    assert dec_l.tolist() == np.where(score[:, 0] >= np.float32(thr), label[:, 0], -1).tolist()
    a = ops.label_runs(torch.from_numpy(score).cuda(), torch.from_numpy(label).cuda(), L, _dev(v_off), thr, 1, label_rows=True)
    b = ops.label_runs(torch.from_numpy(dec_s).cuda()[:, None], torch.from_numpy(dec_l).cuda()[:, None], L, _dev(v_off),
                       float(np.finfo(np.float32).min), 1, label_rows=True)
    n = int(a[0][0])
    assert n == int(b[0][0]) > 10 and torch.equal(a[1][:, :n], b[1][:, :n]) and torch.equal(a[2][:n], b[2][:n]) and torch.equal(a[3], b[3])


@pytest.mark.parametrize("k", (2, 32))
def test_infinite_penalty_gives_one_label_per_video(k):
    for kind in ("exact", "float"):
        score, label = _lists(kind, k, "seven")
        label = label.copy()
        label[:, 0] = 3                                                # one label every row lists: a whole video can stay on it
        label[:, 1:] = np.where(label[:, 1:] == 3, L + 1, label[:, 1:])
        v_off = _v_off("seven")
        dec_l, _ = _decode(score, label, v_off, -0.5, INF)
        per_video = [set(dec_l[a:b].tolist()) for a, b in zip(v_off[:-1], v_off[1:])]
        assert all(len(s) == 1 for s in per_video) and any(s != {-1} for s in per_video)


def test_identical_videos_decode_identically_wherever_they_stand_and_two_runs_give_the_same_bits():
    k = 5
    score, label = _lists("float", k, "one")                           # 200 rows
    lens = [200, 7, 200, 64, 1, 200, 200, 33, 200]                    # the same video as wave 0, 2 of one workgroup, 1, 2 of the next, 0 of a third
    rng = np.random.default_rng(3)
    parts_s, parts_l = [], []
    for n in lens:
        if n == 200:
            parts_s.append(score), parts_l.append(label)
        else:
            s, lab = exact_lists(rng, n, k, L)
            parts_s.append(s), parts_l.append(lab)
    S, Lb = np.concatenate(parts_s), np.concatenate(parts_l)
    v_off = np.concatenate([[0], np.cumsum(lens)])
    first = _decode(S, Lb, v_off, 0.1, 0.3)
    again = _decode(S, Lb, v_off, 0.1, 0.3)
    assert _same(first, (again[0].astype(np.int64), again[1]))
    alone = _decode(score, label, [0, 200], 0.1, 0.3)
    for v, n in enumerate(lens):
        if n == 200:
            a = int(v_off[v])
            assert np.array_equal(first[0][a:a + 200], alone[0]) and np.array_equal(first[1][a:a + 200].view(np.int32), alone[1].view(np.int32))
    assert (alone[0] != -1).any()


# ------------------------------------------------------------------------------------------------------------- 2. end to end
PLANTED = [f"step {i}" for i in range(6)]


class _OneHotText:
    """A text side whose feature of "step i" is the unit vector e_i: the score of label i at a row is the row's coordinate i,
    exactly, in f32, bf16 and e4m3 alike (the planted values are eighths)."""

    def get_textual_feature(self, x):
        return x


def _one_hot(strs):
    x = torch.zeros(len(strs), 512)
    for j, s in enumerate(strs):
        x[j, int(s.split()[1])] = 1.0
    return x


def _planted_index(fmt):
    """video "dip": label 2 scores 7/8 for 18 seconds with a two-second dip to 1/4 at seconds 8 and 9; video "hand": the hand case of
    test_smooth_cpu.py (labels 0 and 1); video "quiet": nothing above 1/8"""
    srch = _srch()
    dip = np.zeros((18, 512), dtype=np.float32)
    dip[:, 2] = .875
    dip[8:10, 2] = .25
    hand = np.zeros((12, 512), dtype=np.float32)
    for t in range(12):
        for j in range(2):
            hand[t, HAND_LABEL[t, j]] = HAND_SCORE[t, j]
    quiet = np.zeros((5, 512), dtype=np.float32)
    quiet[:, 4] = .125
    parts = [srch.VideoIndex(torch.from_numpy(x).cuda().bfloat16(), [0, len(x)], [vid]) for x, vid in ((dip, "dip"), (hand, "hand"), (quiet, "quiet"))]
    return [p.quantize() for p in parts] if fmt == "e4m3" else parts


@pytest.mark.parametrize("fmt", ("bf16", "e4m3"))
def test_a_planted_dip_is_one_segment_with_switch_and_two_without(fmt):
    srch = _srch()
    idx = srch.VideoIndex.concat(_planted_index(fmt))
    ann = srch.annotate(idx, _OneHotText(), _one_hot, PLANTED, k=5)
    raw = ann.segments(0.5)
    assert [s[:4] for s in raw] == [("dip", 0, 7, "step 2"), ("dip", 10, 17, "step 2"), ("hand", 0, 2, "step 0"), ("hand", 5, 6, "step 0"),
                                    ("hand", 7, 7, "step 1"), ("hand", 8, 9, "step 0")]
    smooth = ann.segments(0.5, switch=0.5)
    assert [s[:4] for s in smooth] == [("dip", 0, 17, "step 2"), ("hand", 0, 9, "step 0")]
    assert [s[4] for s in smooth] == [0, 0] and all(abs(s[5] - .875) < 1e-3 for s in smooth)     # the peak: the first second at 7/8
    assert ann.segments(0.5, 11, switch=0.5) == smooth[:1] and ann.segments(0.5, switch=0.0) == raw
    # the decode itself is the reference's on the lists the kernel returned, and a bridged second keeps its own score
    lab, sc = ann.decode(0.5, 0.5)
    want = ref.decode_f32(ann.score.cpu().numpy(), ann.label.cpu().numpy(), idx.v_off, 0.5, 0.5)
    assert _same((lab.cpu().numpy(), sc.cpu().numpy()), want)
    assert lab.tolist() == [2] * 18 + [0] * 10 + [-1] * 7 and abs(float(sc[8]) - .25) < 1e-3 and abs(float(sc[18 + 7]) - .625) < 1e-3
    seconds = ann.label_seconds(0.5, switch=0.5)
    assert seconds == {"step 0": 10, "step 1": 0, "step 2": 18, "step 3": 0, "step 4": 0, "step 5": 0}
    assert ann.label_seconds(0.5) == {"step 0": 7, "step 1": 1, "step 2": 16, "step 3": 0, "step 4": 0, "step 5": 0}


@pytest.mark.parametrize("fmt", ("bf16", "e4m3"))
def test_three_shards_give_the_concatenated_index_segments(fmt):
    srch = _srch()
    parts = _planted_index(fmt)
    whole = srch.annotate(srch.VideoIndex.concat(parts), _OneHotText(), _one_hot, PLANTED, k=5)
    want_l, want_s = whole.decode(0.5, 0.5)
    segs = whole.segments(0.5, 2, switch=0.5)
    assert len(segs) == 2
    pinned = [srch.VideoIndex(p.feat.cpu().pin_memory(), p.v_off, p.vids, None if p.scale is None else p.scale.cpu().pin_memory())
              for p in parts]
    for sharded in (srch.ShardedIndex(parts), srch.ShardedIndex(pinned, resident="host")):
        got = srch.annotate(sharded, _OneHotText(), _one_hot, PLANTED, k=5)
        lab, sc = got.decode(0.5, 0.5)
        assert torch.equal(lab, want_l) and torch.equal(sc.view(torch.int32), want_s.view(torch.int32))
        assert got.segments(0.5, 2, switch=0.5) == segs
        assert got.label_seconds(0.5, switch=0.5) == whole.label_seconds(0.5, switch=0.5)
    torch.cuda.synchronize()


def test_cli_annotate_smooth(tmp_path, capsys):
    """`index`, then `annotate --smooth` writes the csv that `annotate()` + `segments(switch=)` give through the API -- in process
    (`search.main`), as test_annotate_gpu.py runs the command line."""
    import io

    from temporalalignnet_amd import search as srch, synth
    from temporalalignnet_amd.infer_align import build_aligner, make_embed_text
    from temporalalignnet_amd.train import build_model, default_args
    from temporalalignnet_amd.word2vec_model import Word2VecModel, Word2VecTokenizer
    paths = synth.write_htm_fixture(str(tmp_path / "htm"), synth.htm_fixture())
    vocab = synth.w2v_vocab(40)
    np.save(str(tmp_path / "s3d_dict.npy"), vocab)
    m = build_model(default_args(model="init", num_encoder_layers=1, num_decoder_layers=1), compute_dtype="bf16", language_model=None,
                    random_pos_start=0)
    sd = m.state_dict()
    for key, v in synth.make_params(31, 1, 1, False).items():
        sd[key].copy_(torch.from_numpy(v))
    m.bert = Word2VecModel(num_embeddings=len(vocab) + 1, compute_dtype="bf16")
    for key, v in synth.w2v_params(32, len(vocab) + 1).items():
        m.bert.state_dict()[key].copy_(torch.from_numpy(v))
    ckpt = str(tmp_path / "ckpt.pth.tar")
    torch.save({"state_dict": m.state_dict(), "epoch": 3}, ckpt)
    common = ["--checkpoint", ckpt, "--vocab", str(tmp_path / "s3d_dict.npy")]
    index = str(tmp_path / "i.npz")
    assert srch.main(["index", *common, "--feature-dir", paths["features"], "--asr-json", paths["asr"], "--vlen-csv", paths["vlen"],
                      "--out", index]) == 0
    labels = ["stir the eggs", "w3 w7 w11", "w1 w2", "w5", "w9 w4"]
    (tmp_path / "labels.txt").write_text("\n".join(labels) + "\n")
    model = build_aligner(ckpt, vocab, "init", "bf16")
    embed = make_embed_text(model, Word2VecTokenizer(max_words=32, vocab=vocab))
    ann = srch.annotate(srch.VideoIndex.load(index), model, embed, labels, 5)
    threshold = float(ann.score[:, 0].median())
    spread = float(ann.score[:, 0].max() - ann.score[:, 0].min())

    def run(*more):
        out = str(tmp_path / f"out{len(more)}.csv")
        assert srch.main(["annotate", *common, "--index", index, "--labels", str(tmp_path / "labels.txt"), "-k", "5", "--out", out,
                          f"--threshold={threshold!r}", *more]) == 0
        with open(out) as f:
            return f.read()

    for pen, min_len in ((spread / 4, 2), (0.0, 1)):
        want = io.StringIO()
        srch.write_segments_csv(want, ann.segments(threshold, min_len, switch=pen))
        got = run(f"--smooth={pen!r}", "--min-len", str(min_len))
        assert got == want.getvalue()
    assert len(got.splitlines()) > 1                                    # penalty 0: the seconds above the median are segments
    capsys.readouterr()
