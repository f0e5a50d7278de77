"""Host-side pieces of corpus annotation: the C ABI of tan_label_topk / tan_label_topk_e4m3 / tan_label_runs with their argument
checks, the Python argument checks of `ops.label_*` and `search.annotate`, the runs reference (label_ref.py) by hand, the
`annotate` command line, the csv writers, and `Annotation`'s mapping of runs to (vid, second).  No device needed."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import label_ref as ref
from temporalalignnet_amd import _lib

i, l, p, f = C.c_int, C.c_long, C.c_void_p, C.c_float

ENTRY_POINTS = {
    "tan_label_topk": (i, [p, p, i, l, l, i, i, p, p, p]),
    "tan_label_topk_e4m3": (i, [p, p, p, p, l, l, i, i, p, p, p]),
    "tan_label_runs_ws_bytes": (l, [l]),
    "tan_label_runs": (i, [p, p, i, l, l, p, l, f, i, l, p, p, p, p, p, p, p, p, p, p]),
}


# ------------------------------------------------------------------------------------------------------------------- the C ABI
def test_library_exports_the_entry_points_with_the_headers_prototypes():
    names, protos, L = _lib.declared_symbols(), _lib.declared_prototypes(), _lib.lib()
    for name, proto in ENTRY_POINTS.items():
        assert name in names and getattr(L, name) is not None
        assert protos[name] == proto, name
        assert getattr(L, name).argtypes == proto[1] and getattr(L, name).restype == proto[0]


def test_ws_bytes_is_positive_for_valid_sizes_and_minus_one_otherwise():
    L = _lib.lib()
    last = 0
    for N in (1, 64, 65, 256, 257, 4210693, 2 ** 31 - 1):
        n = L.tan_label_runs_ws_bytes(N)
        assert n > last and n % 16 == 0 and n >= 13 * N, N              # three int32 per row and a flag byte
        last = n
    for N in (0, -1, 2 ** 31):
        assert L.tan_label_runs_ws_bytes(N) == -1


def test_bad_arguments_are_rejected_without_touching_a_device():
    L = _lib.lib()
    a = C.c_void_p(1 << 20)                            # never dereferenced: every call below fails its argument checks
    odd = C.c_void_p((1 << 20) + 8)

    def topk(e4m3, tl=a, vn=a, ls=a, vs=a, dtype=1, Ln=100, N=1000, Cw=512, k=5, ts=a, tlab=a):
        if e4m3:
            return L.tan_label_topk_e4m3(tl, ls, vn, vs, Ln, N, Cw, k, ts, tlab, None)
        return L.tan_label_topk(tl, vn, dtype, Ln, N, Cw, k, ts, tlab, None)

    common = (dict(tl=None), dict(vn=None), dict(ts=None), dict(tlab=None), dict(k=0), dict(k=-1), dict(k=33), dict(k=6, Ln=5),
              dict(Ln=0), dict(Ln=1 << 31), dict(N=0), dict(N=1 << 31), dict(Cw=256), dict(tl=odd), dict(vn=odd))
    for e4m3 in (False, True):
        more = (dict(ls=None), dict(vs=None)) if e4m3 else (dict(dtype=2), dict(dtype=-1))
        for kw in common + more:
            assert topk(e4m3, **kw) == -1, (e4m3, kw)

    def runs(ts=a, tl=a, stride=1, N=1000, Ln=10, v_off=a, nv=5, thr=0.5, min_len=1, cap=1000, n_runs=a, rv=a, rs=a, re=a, rl=a, rp=a,
             rps=a, counts=a, ws=a):
        return L.tan_label_runs(ts, tl, stride, N, Ln, v_off, nv, thr, min_len, cap, n_runs, rv, rs, re, rl, rp, rps, counts, ws, None)

    for kw in (dict(ts=None), dict(tl=None), dict(v_off=None), dict(n_runs=None), dict(rv=None), dict(rs=None), dict(re=None),
               dict(rl=None), dict(rp=None), dict(rps=None), dict(ws=None), dict(stride=0), dict(N=0), dict(N=1 << 31), dict(Ln=0),
               dict(Ln=1 << 31), dict(nv=0), dict(nv=1001), dict(thr=float("nan")), dict(min_len=0), dict(min_len=-3), dict(cap=-1),
               dict(counts=None, cap=-1), dict(ws=C.c_void_p((1 << 20) + 2))):
        assert runs(**kw) == -1, kw


def test_python_argument_checks_come_before_any_device_call():
    from temporalalignnet_amd import ops, search
    tl, vn = torch.zeros(4, 512), torch.zeros(9, 512)
    for kw in (dict(k=0), dict(k=5), dict(k=33)):
        with pytest.raises(ValueError):
            ops.label_topk(tl, vn, **kw)
    with pytest.raises(ValueError):
        ops.label_topk(tl[:, :256].contiguous(), vn[:, :256].contiguous())
    with pytest.raises(ValueError):
        ops.label_topk(tl, vn.bfloat16())
    with pytest.raises(ValueError):
        ops.label_topk(tl, vn[::2])
    with pytest.raises(TypeError):
        ops.label_topk(tl.to(torch.uint8), vn.to(torch.uint8))
    with pytest.raises(ValueError):
        ops.label_topk(tl, vn, 2, out=(torch.zeros(9, 2), torch.zeros(9, 2)))                    # labels are int32
    with pytest.raises(ValueError):
        ops.label_topk(tl, vn, 2, out=(torch.zeros(9, 3), torch.zeros(9, 3, dtype=torch.int32)))
    with pytest.raises(_lib.TanHipError, match="device tensors"):
        ops.label_topk(tl, vn, 2)                                                                # valid, but on the host
    c8, s4, s9 = torch.zeros(4, 512, dtype=torch.uint8), torch.ones(4), torch.ones(9)
    v8 = torch.zeros(9, 512, dtype=torch.uint8)
    with pytest.raises(TypeError):
        ops.label_topk_e4m3(tl, s4, vn, s9)
    for bad in (dict(l_scale=s9), dict(v_scale=s4), dict(l_scale=None), dict(v_scale=s9.double())):
        kw = dict(l_scale=s4, v_scale=s9)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.label_topk_e4m3(c8, kw["l_scale"], v8, kw["v_scale"])
    with pytest.raises(ValueError):
        ops.label_topk_e4m3(c8, s4, v8, s9, 5)
    with pytest.raises(_lib.TanHipError, match="device tensors"):
        ops.label_topk_e4m3(c8, s4, v8, s9, 4)

    score, label, v_off = torch.zeros(9, 2), torch.zeros(9, 2, dtype=torch.int32), torch.tensor([0, 4, 9], dtype=torch.int32)
    good = dict(top_score=score, top_label=label, L=4, v_off=v_off, threshold=0.5)
    for bad in (dict(top_label=label.long()), dict(top_score=score.double()), dict(top_label=label[:, :1]), dict(L=0),
                dict(v_off=v_off.long()), dict(v_off=v_off[:1]), dict(v_off=torch.arange(11, dtype=torch.int32)),
                dict(threshold=float("nan")), dict(min_len=0), dict(cap=-1), dict(ws=torch.zeros(8, dtype=torch.uint8)),
                dict(out=(torch.zeros(1, dtype=torch.int32), torch.zeros(5, 3, dtype=torch.int32), torch.zeros(9), None))):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.label_runs(**kw)
    with pytest.raises(_lib.TanHipError, match="device tensors"):
        ops.label_runs(**good)
    assert ops.label_runs_ws_bytes(9) > 0
    with pytest.raises(_lib.TanHipError):
        ops.label_runs_ws_bytes(0)

    idx = search.VideoIndex(torch.zeros(9, 512), [0, 4, 9], ["a", "b"])
    for labels, k in (([], 1), (["x", "y"], 0), (["x", "y"], 3), (["x"] * 40, 33)):
        with pytest.raises(ValueError):
            search.annotate(idx, None, None, labels, k)                 # refused before the model or the device is touched
    ann = search.Annotation(label, score, ["w", "x", "y", "z"], [0, 4, 9], ["a", "b"])
    for call in (lambda: ann.segments(float("nan")), lambda: ann.segments(0.5, 0), lambda: ann.label_seconds(float("nan"))):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------------------- the reference, by hand
SCORE12 = [.9, .9, .2, .8, .8, .95, .8, .7, float("nan"), .6, .6, .6]
LABEL12 = [3, 3, 3, 1, 1, 1, 1, 2, 2, 2, 0, 0]
V_OFF12 = [0, 5, 6, 12]


def test_runs_reference_by_hand_on_twelve_rows():
    # video 0 = rows 0..4, video 1 = row 5 alone, video 2 = rows 6..11; threshold .5: row 2 (.2) and row 8 (NaN) are background.
    # label 1 runs through rows 3..6 but crosses two video boundaries: three runs.
    runs = ref.label_runs(SCORE12, LABEL12, V_OFF12, 0.5)
    assert [r[:5] for r in runs] == [(0, 0, 1, 3, 0), (0, 3, 4, 1, 3), (1, 5, 5, 1, 5), (2, 6, 6, 1, 6), (2, 7, 7, 2, 7), (2, 9, 9, 2, 9),
                                     (2, 10, 11, 0, 10)]
    assert [r[5] for r in runs] == [np.float32(x) for x in (.9, .8, .95, .8, .7, .6, .6)]
    assert [r[:3] for r in ref.label_runs(SCORE12, LABEL12, V_OFF12, 0.5, min_len=2)] == [(0, 0, 1), (0, 3, 4), (2, 10, 11)]
    assert ref.label_runs(SCORE12, LABEL12, V_OFF12, 0.5, min_len=3) == []
    assert ref.label_runs(SCORE12, LABEL12, V_OFF12, 0.96) == []
    # exactly at the threshold is kept, the next float below is not
    t = np.float32(.7)
    assert (2, 7, 7, 2, 7) in [r[:5] for r in ref.label_runs(SCORE12, LABEL12, V_OFF12, t)]
    assert (2, 7, 7, 2, 7) not in [r[:5] for r in ref.label_runs(SCORE12, LABEL12, V_OFF12, np.nextafter(t, np.float32(1)))]
    # one video, a low threshold: label 3 runs 0..2, and its peak .9 is attained twice -- the smaller row wins
    assert ref.label_runs(SCORE12, LABEL12, [0, 12], 0.1)[0] == (0, 0, 2, 3, 0, float(np.float32(.9)))
    assert ref.label_rows(SCORE12, LABEL12, 0.5, 5).tolist() == [2, 4, 2, 2, 0]
    assert ref.label_rows(SCORE12, LABEL12, 0.5, 5).sum() == 10        # twelve rows, two of them background
    assert ref.row_labels(SCORE12, LABEL12, 0.5).tolist() == [3, 3, -1, 1, 1, 1, 1, 2, -1, 2, 0, 0]


@pytest.mark.parametrize("min_len", (1, 2, 4))
def test_the_vectorised_reference_equals_the_row_by_row_one(min_len):
    rng = np.random.default_rng(3)
    N = 3000
    label = np.repeat(rng.integers(0, 4, N), rng.integers(1, 5, N))[:N]
    score = rng.integers(0, 8, N).astype(np.float32) / 8
    score[rng.integers(0, N, 50)] = np.nan
    v_off = np.array(sorted({0, N, 63, 64, 65} | set(rng.integers(1, N, 40).tolist())))
    slow = ref.label_runs(score, label, v_off, 0.25, min_len)
    fast = ref.runs_fast(score, label, v_off, 0.25, min_len)
    assert len(slow) > 20 and [tuple(int(c[j]) for c in fast[:5]) + (float(fast[5][j]),) for j in range(len(slow))] == slow
    assert len(fast[0]) == len(slow)


# ------------------------------------------------------------------------------------------------- Annotation: runs -> segments
def test_annotation_maps_runs_to_vid_and_second():
    from temporalalignnet_amd import search
    labels = ["whisk", "pour", "fry", "serve"]
    ann = search.Annotation(torch.tensor(LABEL12, dtype=torch.int32)[:, None], torch.tensor(SCORE12)[:, None], labels, V_OFF12,
                            ["a", "b", "a"])
    assert len(ann) == 12 and ann.k == 1 and ann.v_off.dtype == np.int64
    runs = ref.label_runs(SCORE12, LABEL12, V_OFF12, 0.5)
    cols = np.array([r[:5] for r in runs]).T                           # ops.RUN_FIELDS: video, start, end, label, peak_row
    got = ann.runs_to_segments(cols, np.array([r[5] for r in runs], dtype=np.float32))
    want = [(ann.vids[v], a - V_OFF12[v], b - V_OFF12[v], labels[lab], pr - V_OFF12[v], ps) for v, a, b, lab, pr, ps in runs]
    assert got == want
    assert got[0] == ("a", 0, 1, "serve", 0, float(np.float32(.9))) and got[2] == ("b", 0, 0, "pour", 0, float(np.float32(.95)))
    assert got[-1] == ("a", 4, 5, "whisk", 4, float(np.float32(.6)))  # the second video "a": seconds of its own
    assert ann.runs_to_segments(np.zeros((5, 0), dtype=np.int32), np.zeros(0, dtype=np.float32)) == []


# ------------------------------------------------------------------------------------------------------------- command line
def test_cli_parses_annotate_and_refuses_the_conflicts():
    from temporalalignnet_amd import search
    argv = ["annotate", "--checkpoint", "c", "--vocab", "/nonexistent/s3d_dict.npy", "--index", "i.npz", "--labels", "steps.txt", "--out",
            "o.csv"]
    a = search.parse_args(argv)
    assert (a.cmd, a.k, a.threshold, a.min_len, a.per_second, a.labels, a.out) == ("annotate", 1, None, None, False, "steps.txt", "o.csv")
    assert a.shard is None and not a.host_resident and a.dtype == "bf16" and a.model == "init"
    a = search.parse_args(argv + ["-k", "5", "--threshold", "0.25", "--min-len", "3", "--shard", "j.npz", "--shard", "k.npz",
                                  "--host-resident", "--dtype", "fp32"])
    assert (a.k, a.threshold, a.min_len, a.shard, a.host_resident, a.dtype) == (5, 0.25, 3, ["j.npz", "k.npz"], True, "fp32")
    assert search.parse_args(argv + ["--threshold", "-0.5"]).threshold == -0.5
    assert search.parse_args(argv + ["--threshold=-inf"]).threshold == float("-inf")
    assert search.parse_args(argv + ["--per-second", "-k", "32"]).per_second
    for bad in (["-k", "0"], ["-k", "33"], ["--min-len", "0"], ["--threshold", "nan"], ["--per-second", "--threshold", "0.1"],
                ["--per-second", "--min-len", "2"], ["a sentence"]):
        with pytest.raises(SystemExit):
            search.parse_args(argv + bad)
    for missing in ("--labels", "--out", "--index", "--checkpoint"):
        cut = list(argv)
        at = cut.index(missing)
        del cut[at:at + 2]
        with pytest.raises(SystemExit):
            search.parse_args(cut)
    q = search.parse_args(["query", "--checkpoint", "c", "--vocab", "v", "--index", "i.npz", "--shard", "j.npz", "whisk"])
    assert q.shard == ["j.npz"] and q.k == 10 and not q.host_resident   # query keeps its options


def test_csv_writers():
    from temporalalignnet_amd import search
    out = io.StringIO()
    search.write_segments_csv(out, [("v1", 0, 4, "whisk the eggs", 2, 0.5), ("v,2", 7, 7, 'say "hi"', 7, -0.25)])
    assert out.getvalue() == ('vid,start,end,label,peak,score\nv1,0,4,whisk the eggs,2,0.500000\n'
                              '"v,2",7,7,"say ""hi""",7,-0.250000\n')
    out = io.StringIO()
    search.write_segments_csv(out, [])
    assert out.getvalue() == "vid,start,end,label,peak,score\n"
    ann = search.Annotation(torch.tensor([[1, 0], [0, 1], [1, 0]], dtype=torch.int32), torch.tensor([[.5, .25], [1., 0.], [.75, .5]]),
                            ["whisk", "pour"], [0, 2, 3], ["a", "b"])
    out = io.StringIO()
    search.write_per_second_csv(out, ann)
    assert out.getvalue() == ("vid,second,label,score\na,0,pour,0.500000\na,0,whisk,0.250000\na,1,whisk,1.000000\na,1,pour,0.000000\n"
                              "b,0,pour,0.750000\nb,0,whisk,0.500000\n")
