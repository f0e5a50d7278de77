"""Corpus annotation on the GPU: tan_label_topk / _e4m3 (the k best labels of every index row), tan_label_runs (labels -> segments),
`ops.label_topk` / `ops.label_runs`, `search.annotate` with `Annotation.segments` / `label_seconds`, on a `VideoIndex` and on
device- and host-resident `ShardedIndex`es.

Inputs are those of test_moments_gpu.py with the labels in the query's place (`_exact_case(fmt, L, N)`: S is [L, N]):
  * exact arithmetic: labels, scores and order are compared with `==` against label_ref.label_topk;
  * random unit rows: every returned score is within EPS = 2e-5 (test_retrieve_gpu.py) of the fp64 score of the stored operands,
    no label outside a list scores more than 2 EPS above the list's last entry, and scores do not increase along a list.
A workgroup holds 128 index rows and a label tile 64 labels: N runs over 1, 127, 128, 129 and 3 * 128 + 17, L over 1, 63, 64, 65
and 5 * 64 + 3.  tan_label_runs is compared with `==` against label_ref.label_runs (row by row) and, at 4 210 693 rows -- 16 449
blocks of 256 rows, so the one-block scan of the block counts takes 65 rounds of 256 -- against its vectorised twin."""
import functools

import numpy as np
import pytest
import torch

import label_ref as ref
from test_moments_gpu import FORMATS, _dev, _exact_case, _unit_case
from test_retrieve_gpu import EPS

pytestmark = pytest.mark.gpu

NS = (1, 127, 128, 129, 128 * 3 + 17)
LS = (1, 63, 64, 65, 64 * 5 + 3)


def _ops():
    from temporalalignnet_amd import ops
    return ops


def _srch():
    from temporalalignnet_amd import search
    return search


def _topk(tl, vn, kw, k, out=None):
    ops = _ops()
    if kw:
        return ops.label_topk_e4m3(tl, kw["q_scale"], vn, kw["v_scale"], k, out=out)
    return ops.label_topk(tl, vn, k, out=out)


def _ks(L):
    return sorted({k for k in (1, 5, 32, L) if k <= min(32, L)})


@functools.lru_cache(maxsize=None)
def _exact(fmt, L, N):
    return _exact_case(fmt, L, N)


# ------------------------------------------------------------------------------------------------------------- 1. label_topk
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("L", LS)
def test_label_topk_exact_arithmetic(L, fmt):
    for N in NS:
        tl, vn, kw, S, mult = _exact(fmt, L, N)
        for k in _ks(L):
            want_s, want_l = ref.label_topk(S, k)
            top_s, top_l = _topk(tl, vn, kw, k)
            assert top_s.shape == (N, k) and top_l.dtype == torch.int32
            assert torch.equal(top_l.long(), want_l), (N, k)
            assert torch.equal(top_s.double() * mult, want_s), (N, k)


@pytest.mark.parametrize("fmt", FORMATS)
def test_equal_labels_come_in_ascending_label_order(fmt):
    L, N = 64 * 5 + 3, 129
    tl, vn, kw, _, mult = _exact_case(fmt, L, N, seed=1)
    tl, kw = tl.clone(), {key: v.clone() for key, v in kw.items()}
    for dst in (L // 2, L - 1):                                        # label 0 three times, scale included
        tl[dst] = tl[0]
        if kw:
            kw["q_scale"][dst] = kw["q_scale"][0]
    # k = 32 of 323 random labels: label 0 makes the list of about a tenth of the rows; the loop counts them
    top_s, top_l = _topk(tl, vn, kw, 32)
    seen = 0
    for row_l, row_s in zip(top_l.tolist(), top_s.tolist()):
        at = [row_l.index(x) for x in (0, L // 2, L - 1) if x in row_l]
        if 0 in row_l:
            seen += 1
            # the twins have label 0's score: they follow it in ascending label order, only equal scores between them, and one
            # is missing only where the list ends inside the tie
            assert at == sorted(at) and all(row_s[j] == row_s[at[0]] for j in range(at[0], at[-1] + 1))
            assert len(at) == 3 or row_s[31] == row_s[at[0]]
        else:
            assert at == []                                             # a twin never enters without label 0 ahead of it
    assert seen >= 3


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("order", ("ascending", "descending"))
def test_buffer_pressure_ascending_and_descending_labels(order, fmt):
    """score(l, n) = c_n * (l + 1) with c_n > 0 (ascending): every label beats every label before it, so each one enters its row's
    64-slot buffer and the buffer compacts every 64 labels.  Descending, c_n * (L - l): nothing after the first k enters.
    Integers throughout: label l spreads its number over 32 columns (entries <= 11), the row holds c_n in 1..8 there."""
    L, N = 64 * 5 + 3, 129
    step = torch.arange(1, L + 1, device="cuda") if order == "ascending" else torch.arange(L, 0, -1, device="cuda")
    c = torch.randint(1, 9, (N,), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda")
    xl, xv = torch.zeros(L, 512, dtype=torch.long, device="cuda"), torch.zeros(N, 512, dtype=torch.long, device="cuda")
    xl[:, :32] = (step // 32)[:, None] + (torch.arange(32, device="cuda")[None] < (step % 32)[:, None])
    xv[:, :32] = c[:, None]
    dots = (xl.double() @ xv.double().T)
    assert torch.equal(dots, (step[:, None] * c[None]).double()) and int(xl.max()) <= 11
    if fmt == "e4m3":
        from test_retrieve_fp8_gpu import _int_codes
        ev = torch.randint(-6, 4, (N,), generator=torch.Generator(device="cuda").manual_seed(6), device="cuda")
        tl, vn = _int_codes(xl), _int_codes(xv)                        # the codes of 16 x: acc = 256 * dots, below 2^24
        pow2 = torch.tensor([2.0 ** e for e in range(-6, 4)], device="cuda")     # made on the host: exact powers of two
        kw = dict(q_scale=torch.full((L,), 0.125, device="cuda"), v_scale=pow2[ev + 6].contiguous())
        S, mult = 256 * dots * kw["v_scale"].double()[None] * 0.125, 1.0
    else:
        dt = {"f32": torch.float32, "bf16": torch.bfloat16}[fmt]
        tl, vn, kw = (xl.float() / 16).to(dt), (xv.float() / 16).to(dt), {}
        S, mult = dots, 256.0
    best = L - 1 if order == "ascending" else 0
    for k in (1, 5, 32):
        want_s, want_l = ref.label_topk(S, k)
        top_s, top_l = _topk(tl, vn, kw, k)
        print(f"pressure {order} {fmt} k={k}: max |score - exact| = {float((top_s.double() * mult - want_s).abs().max()):.3e}")
        assert torch.equal(top_l.long(), want_l) and torch.equal(top_s.double() * mult, want_s), k
        assert (top_l[:, 0] == best).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_label_topk_random_unit_rows(fmt):
    worst = 0.0
    for L, N in ((64 * 5 + 3, 128 * 3 + 17), (65, 129), (1, 1)):
        tl, vn, kw, S, _ = _unit_case(fmt, L, N)
        St = S.T.contiguous()                                          # [N, L] fp64 scores of the stored operands
        for k in _ks(L):
            top_s, top_l = _topk(tl, vn, kw, k)
            got = St.gather(1, top_l.long())
            err = float((top_s.double() - got).abs().max())
            worst = max(worst, err)
            print(f"label_topk {fmt} L={L} N={N} k={k}: max |score - fp64| = {err:.3e}")
            assert err <= EPS
            assert all(len(set(r)) == k for r in top_l.tolist())       # k different labels
            outside = St.scatter(1, top_l.long(), -float("inf")).amax(1)
            assert (outside <= got[:, -1] + 2 * EPS).all()
            assert (top_s[:, 1:] <= top_s[:, :-1]).all()
    print(f"label_topk {fmt}: worst {worst:.3e} against EPS {EPS:.0e}")


@pytest.mark.parametrize("fmt", FORMATS)
def test_label_topk_is_bit_identical_from_run_to_run_in_dirty_memory(fmt):
    L, N, k = 64 * 5 + 3, 128 * 3 + 17, 5
    tl, vn, kw, _, _ = _unit_case(fmt, L, N, seed=2)
    outs = []
    for fill in (float("nan"), 7.0):
        out = (torch.full((N, k), fill, device="cuda"), torch.full((N, k), -9, dtype=torch.int32, device="cuda"))
        top_s, top_l = _topk(tl, vn, kw, k, out=out)
        assert top_s.data_ptr() == out[0].data_ptr() and top_l.data_ptr() == out[1].data_ptr()
        outs.append((top_s.clone(), top_l.clone()))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1], outs[1][1])
    # nothing is written behind row N - 1: three guard rows after the lists keep their fill
    whole_s, whole_l = torch.full((N + 3, k), 7.0, device="cuda"), torch.full((N + 3, k), -9, dtype=torch.int32, device="cuda")
    _topk(tl, vn, kw, k, out=(whole_s[:N], whole_l[:N]))
    assert (whole_s[N:] == 7.0).all() and (whole_l[N:] == -9).all()
    assert torch.equal(whole_l[:N], outs[0][1])


# -------------------------------------------------------------------------------------------------------------- 2. label_runs
def _runs(score, label, L, v_off, threshold, min_len=1, cap=None, label_rows=True):
    """ops.label_runs into guarded caller-owned outputs -> (n_runs, runs int64 [5, n] on the host, peak f32 [n], label_rows or None);
    asserts that nothing is written past min(n_runs, cap)."""
    ops = _ops()
    N = score.shape[0]
    cap = N if cap is None else cap
    n_runs = torch.full((1,), -77, dtype=torch.int32, device="cuda")
    counts = torch.full((L,), -77, dtype=torch.int32, device="cuda") if label_rows else None
    col = torch.full((5, cap), -77, dtype=torch.int32, device="cuda")
    pk = torch.full((cap,), -77.0, device="cuda")
    ops.label_runs(score, label, L, _dev(v_off), threshold, min_len, cap=cap, out=(n_runs, col, pk, counts))
    n = int(n_runs[0])
    w = min(n, cap)
    assert (col[:, w:] == -77).all() and (pk[w:] == -77.0).all()      # the guard region: nothing past the written runs
    return n, col[:, :w].cpu().numpy().astype(np.int64), pk[:w].cpu().numpy(), None if counts is None else counts.cpu().numpy()


def _check_runs(score, label, L, v_off, threshold, min_len=1, cap=None):
    s0, l0 = score[:, 0].cpu().numpy(), label[:, 0].cpu().numpy()
    want = ref.label_runs(s0, l0, v_off, threshold, min_len)
    n, runs, peak, counts = _runs(score, label, L, v_off, threshold, min_len, cap)
    assert n == len(want), (n, len(want))
    w = len(want) if cap is None else min(cap, len(want))
    assert [tuple(int(x) for x in runs[:, j]) for j in range(w)] == [r[:5] for r in want[:w]]
    assert peak.tolist() == [r[5] for r in want[:w]]
    assert counts.tolist() == ref.label_rows(s0, l0, threshold, L).tolist()
    assert counts.sum() == (ref.row_labels(s0, l0, threshold) != -1).sum()
    return want


def _random_lists(N, L, stride, seed, levels=8):
    """[N, stride] lists whose column 0 has runs: labels repeat 1..6 times, scores are eighths (ties for the peak)"""
    rng = np.random.default_rng(seed)
    lab = np.repeat(rng.integers(0, L, N), rng.integers(1, 7, N))[:N]
    sc = rng.integers(0, levels + 1, N).astype(np.float32) / levels
    label = torch.from_numpy(rng.integers(0, L, (N, stride)).astype(np.int32))
    score = torch.from_numpy(rng.random((N, stride)).astype(np.float32) + 2)        # the other columns: never read
    label[:, 0], score[:, 0] = torch.from_numpy(lab.astype(np.int32)), torch.from_numpy(sc)
    return score.cuda(), label.cuda()


@pytest.mark.parametrize("stride", (1, 5))
@pytest.mark.parametrize("min_len", (1, 2, 1000))
def test_label_runs_layouts(min_len, stride):
    N, L = 777, 7
    score, label = _random_lists(N, L, stride, 11)
    score[100:103, 0] = float("nan")
    layouts = {
        "boundaries at 63 / 64 / 65": [0, 63, 64, 65, 300, N],
        "one-row videos": list(range(N + 1)),
        "one video": [0, N],
        "a label continues across a boundary": [0, 40, 41, 500, N],
    }
    label[35:45, 0], score[35:45, 0] = 3, 0.75                         # label 3 through rows 35..44: cut at 40 and 41 in the last layout
    label[34, 0] = label[45, 0] = 4
    for name, v_off in layouts.items():
        want = _check_runs(score, label, L, v_off, 0.5, min_len)
        if name.startswith("a label continues") and min_len <= 2:
            cut = [r[:4] for r in want if 34 < r[1] < 45]
            assert (0, 35, 39, 3) in cut and (2, 41, 44, 3) in cut and ((1, 40, 40, 3) in cut) == (min_len == 1)
        if min_len == 1000:
            assert want == []


def test_label_runs_threshold_peaks_and_background():
    N, L = 130, 4
    t = np.float32(0.3)
    below = np.nextafter(t, np.float32(0))
    label = torch.zeros(N, 1, dtype=torch.int32, device="cuda")
    score = torch.full((N, 1), float(below), device="cuda")
    score[5:9, 0] = float(t)                                           # exactly the threshold: kept; its neighbours, one float below: not
    label[64:70, 0] = 2
    score[64:70, 0] = torch.tensor([.5, .9, .7, .9, .4, .9], device="cuda")      # the peak .9 three times: the smallest row wins
    score[67, 0] = float("nan")                                        # ... and a NaN splits the run: background
    want = _check_runs(score, label, L, [0, N], float(t))
    assert [r[:5] for r in want] == [(0, 5, 8, 0, 5), (0, 64, 66, 2, 65), (0, 68, 69, 2, 69)]
    assert _check_runs(score, label, L, [0, N], 0.95) == []            # all background: n_runs == 0
    n, runs, peak, counts = _runs(score, label, L, [0, N], 0.95, label_rows=False)      # label_rows = NULL is accepted
    assert n == 0 and runs.shape == (5, 0) and counts is None
    assert len(_check_runs(score, label, L, [0, N], float("-inf"))) == 4           # everything but the NaN row, by label


def _guarded_raw_runs(score, label, L, v_off, threshold, min_len, cap, guard=4):
    """tan_label_runs itself into six SEPARATE arrays of cap + guard entries -> (n_runs, the six arrays on the host)"""
    from temporalalignnet_amd import _lib
    ops, lib = _ops(), _lib.lib()
    N, stride = score.shape
    ints = [torch.full((cap + guard,), -77, dtype=torch.int32, device="cuda") for _ in range(5)]
    peak = torch.full((cap + guard,), -77.0, device="cuda")
    n_runs = torch.full((1,), -77, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.label_runs_ws_bytes(N), dtype=torch.uint8, device="cuda")
    v = _dev(v_off)
    rc = lib.tan_label_runs(score.data_ptr(), label.data_ptr(), stride, N, L, v.data_ptr(), v.numel() - 1, threshold, min_len, cap,
                            n_runs.data_ptr(), *(t.data_ptr() for t in ints), peak.data_ptr(), None, ws.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return int(n_runs[0]), [t.cpu().numpy() for t in ints] + [peak.cpu().numpy()]


def test_label_runs_cap_smaller_than_the_count():
    N, L = 1000, 5
    score, label = _random_lists(N, L, 1, 23)
    v_off = [0, 10, 500, N]
    want = ref.label_runs(score[:, 0].cpu().numpy(), label[:, 0].cpu().numpy(), v_off, 0.25)
    total = len(want)
    assert total > 100
    for cap in (0, 1, 17, total - 1, total, total + 5):
        _check_runs(score, label, L, v_off, 0.25, cap=cap)           # n_runs is the total and the first cap runs are written
        n, arrays = _guarded_raw_runs(score, label, L, v_off, 0.25, 1, cap)
        w = min(cap, total)
        assert n == total
        for j, a in enumerate(arrays):                                # every array: its first w entries, then nothing -- past cap too
            assert a[:w].tolist() == [r[j] for r in want[:w]] and (a[w:] == -77).all(), (cap, j)


@pytest.mark.parametrize("N", (1, 64, 65))
def test_label_runs_small_sizes(N):
    L = 3
    score, label = _random_lists(N, L, 2, 40 + N, levels=2)
    for v_off in ([0, N], list(range(N + 1))):
        for min_len in (1, 2):
            _check_runs(score, label, L, v_off, 0.5, min_len)


def test_label_runs_at_a_size_that_needs_the_scans_second_round():
    N, L = 4210693, 50                                                 # 16 449 blocks of 256 rows: more than one 256 x 256 round
    g = torch.Generator(device="cuda").manual_seed(9)
    lab = torch.repeat_interleave(torch.randint(0, L, (N // 2,), generator=g, device="cuda"),
                                  torch.randint(1, 6, (N // 2,), generator=g, device="cuda"))[:N].int()
    assert lab.numel() == N
    score = (torch.randint(0, 17, (N,), generator=g, device="cuda").float() / 16)
    score[1234567] = float("nan")
    v_off = np.unique(np.concatenate([[0, N, 63, 64, 65], np.random.default_rng(2).integers(1, N, 30000)]))
    for min_len, cap in ((1, None), (3, 1000)):
        video, start, end, label, peak_row, peak = ref.runs_fast(score.cpu().numpy(), lab.cpu().numpy(), v_off, 0.25, min_len)
        n, runs, pk, counts = _runs(score[:, None], lab[:, None], L, v_off, 0.25, min_len, cap)
        w = len(start) if cap is None else cap
        assert n == len(start) > 100000
        assert np.array_equal(runs, np.stack((video, start, end, label, peak_row))[:, :w]) and np.array_equal(pk, peak[:w])
        assert counts.tolist() == ref.label_rows(score.cpu().numpy(), lab.cpu().numpy(), 0.25, L).tolist()


def test_label_runs_is_bit_identical_from_run_to_run():
    score, label = _random_lists(70001, 9, 5, 31)
    v_off = [0, 64, 65, 30000, 70001]
    a, b = _runs(score, label, 9, v_off, 0.375, 2), _runs(score, label, 9, v_off, 0.375, 2)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
    assert np.array_equal(a[3], b[3])


# --------------------------------------------------------------------------------------------------------- 3. annotate, end to end
LABELS = [f"step {i}" for i in range(70)]


def _reference_annotation(idx, m, embed, k):
    """fp64 scores of `query_features` against the stored rows -> (score [N, k], label [N, k], S [N, L])"""
    from test_retrieve_fp8_gpu import _deq
    srch = _srch()
    tl = srch.query_features(idx, m, embed, LABELS)
    if idx.e4m3:
        S = _deq(*tl) @ _deq(idx.feat, idx.scale).T
    else:
        S = tl.double() @ idx.feat.double().T
    return (*ref.label_topk(S, k), S.T.contiguous())


@pytest.mark.parametrize("fmt", ("bf16", "e4m3"))
def test_annotate_and_segments_match_the_reference(fmt):
    from test_rerank_gpu import _embed, _index, _model
    srch, m = _srch(), _model("fp32")
    idx = _index("fp32", "e4m3" if fmt == "e4m3" else torch.bfloat16)
    for k in (1, 5):
        ann = srch.annotate(idx, m, _embed, LABELS, k=k)
        assert ann.label.shape == (len(idx), k) and ann.score.device == idx.device and ann.labels == LABELS
        assert ann.vids == idx.vids and ann.v_off.tolist() == idx.v_off.tolist()
        want_s, want_l, S = _reference_annotation(idx, m, _embed, k)
        got = S.gather(1, ann.label.long())
        assert ((ann.score.double() - got).abs() <= EPS).all()
        assert (S.scatter(1, ann.label.long(), -float("inf")).amax(1) <= got[:, -1] + 2 * EPS).all()
        assert ((ann.score.double() - want_s).abs() <= EPS).all()
    # segments and label_seconds: the reference applied to the lists the kernel returned (the runs are exact given the lists)
    ann = srch.annotate(idx, m, _embed, LABELS, k=5)
    s0, l0 = ann.score[:, 0].cpu().numpy(), ann.label[:, 0].cpu().numpy()
    threshold = float(np.median(s0))
    for min_len in (1, 3):
        want = ref.label_runs(s0, l0, idx.v_off, threshold, min_len)
        assert len(want) > 0 or min_len > 1
        assert ann.segments(threshold, min_len) == [
            (idx.vids[v], a - idx.v_off[v], b - idx.v_off[v], LABELS[lab], pr - idx.v_off[v], ps) for v, a, b, lab, pr, ps in want]
    counts = ref.label_rows(s0, l0, threshold, len(LABELS))
    assert ann.label_seconds(threshold) == {text: int(c) for text, c in zip(LABELS, counts)}
    assert sum(ann.label_seconds(float("-inf")).values()) == len(idx)
    assert ann.segments(2.0) == []


@pytest.mark.parametrize("fmt", FORMATS)
def test_sharded_annotation_equals_concat_bit_for_bit(fmt):
    from test_shards_gpu import _embed, _pinned, _shards, _the_model
    srch, m = _srch(), _the_model()
    parts = _shards(fmt)                                                  # 1, 63, 64, 65 and 4097 rows
    whole = srch.VideoIndex.concat(parts)
    want = srch.annotate(whole, m, _embed, LABELS, k=5)
    segs = want.segments(float(want.score[:, 0].median()), 2)
    assert len(segs) > 0
    for sharded in (srch.ShardedIndex(parts), srch.ShardedIndex(_pinned(parts), resident="host")):
        for _ in range(2):                                                # the host slots again, in a second call
            got = srch.annotate(sharded, m, _embed, LABELS, k=5)
            assert got.score.is_cuda and torch.equal(got.label, want.label)
            assert torch.equal(got.score.view(torch.int32), want.score.view(torch.int32))
        assert got.vids == want.vids and got.v_off.tolist() == want.v_off.tolist()
        assert got.segments(float(want.score[:, 0].median()), 2) == segs
        assert got.label_seconds(0.0) == want.label_seconds(0.0)
    torch.cuda.synchronize()


def test_cli_index_then_annotate(tmp_path, capsys):
    """`index`, then `annotate` writes the csv that `annotate()` + `segments()` / the per-second writer give through the API, and
    the same file for `--host-resident` -- in process (`search.main`), as test_shards_gpu.py runs the command line."""
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
    (tmp_path / "labels.txt").write_text("\n".join(labels[:2]) + "\n\n" + "\n".join(labels[2:]) + "\n")       # a blank line is skipped
    model = build_aligner(ckpt, vocab, "init", "bf16")
    embed = make_embed_text(model, Word2VecTokenizer(max_words=32, vocab=vocab))
    ann = srch.annotate(srch.VideoIndex.load(index), model, embed, labels, 2)
    threshold = float(ann.score[:, 0].median())

    def run(*more):
        out = str(tmp_path / f"out{len(more)}_{'h' if '--host-resident' in more else 'd'}.csv")
        assert srch.main(["annotate", *common, "--index", index, "--labels", str(tmp_path / "labels.txt"), "-k", "2", "--out", out,
                          *more]) == 0
        with open(out) as f:
            return f.read()

    want = io.StringIO()
    srch.write_segments_csv(want, ann.segments(threshold, 2))
    got = run(f"--threshold={threshold!r}", "--min-len", "2")
    assert got == want.getvalue() and len(got.splitlines()) > 1
    assert run(f"--threshold={threshold!r}", "--min-len", "2", "--host-resident") == got
    want = io.StringIO()
    srch.write_per_second_csv(want, ann)
    got = run("--per-second")
    assert got == want.getvalue() and len(got.splitlines()) == 1 + 2 * len(ann)
    everything = run()                                                  # no threshold: every second belongs to a segment
    assert sum(int(r.split(",")[2]) - int(r.split(",")[1]) + 1 for r in everything.splitlines()[1:]) == len(ann)
    capsys.readouterr()
