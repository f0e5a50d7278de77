"""Host-side pieces of two-stage search: the window a candidate gets (`search.rerank_window`), the stem store of `VideoIndex` in the
index file, the C ABI of tan_rerank_tail / tan_rerank_select, `search.Reranked` and the `index --keep-stem` / `query --rerank`
command line.  No device needed."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from temporalalignnet_amd import _lib

i, l, p = C.c_int, C.c_long, C.c_void_p


@pytest.mark.parametrize("vlen", (1, 20, 32, 33, 64, 65, 203))
def test_rerank_window_contains_the_second_and_is_centred_unless_clamped(vlen):
    from temporalalignnet_amd.search import rerank_window
    T = 64
    for sec in range(vlen):
        s0, t = rerank_window(sec, vlen, T)
        assert 0 <= s0 and s0 + t <= vlen and t == min(T, vlen)
        assert s0 <= sec < s0 + t
        centred = sec - T // 2
        if 0 <= centred <= vlen - T:
            assert s0 == centred                                   # neither end sticks out: centred on the second
        elif centred < 0:
            assert s0 == 0                                         # clamped at the video's start (or the video is short)
        else:
            assert s0 == max(vlen - T, 0)                          # clamped at its end
    assert rerank_window(0, vlen) == rerank_window(0, vlen, 64)


def _index(dtype, stem_dtype):
    from temporalalignnet_amd.search import VideoIndex
    g = torch.Generator().manual_seed(3)
    feat = torch.randn(17, 512, generator=g).to(dtype)
    stem = None if stem_dtype is None else (torch.randn(17, 512, generator=g) * 3).to(stem_dtype)
    return VideoIndex(feat, [0, 5, 17], ["x", "y"], stem=stem)


@pytest.mark.parametrize("stem_dtype", (torch.bfloat16, torch.float32))
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32))
def test_stem_round_trips_bit_for_bit(tmp_path, dtype, stem_dtype):
    from temporalalignnet_amd.search import VideoIndex
    idx = _index(dtype, stem_dtype)
    path = str(tmp_path / "i.npz")
    idx.save(path)
    back = VideoIndex.load(path, device="cpu")
    assert back.stem.dtype == stem_dtype and back.stem.shape == (17, 512)
    assert torch.equal(back.stem.view(torch.uint8), idx.stem.view(torch.uint8))
    assert back.feat.dtype == dtype and torch.equal(back.feat.view(torch.uint8), idx.feat.view(torch.uint8))
    assert back.vids == idx.vids and back.v_off.tolist() == idx.v_off.tolist() and back.scale is None
    with np.load(path) as z:
        assert z["stem"].dtype == (np.uint16 if stem_dtype == torch.bfloat16 else np.float32)


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32))
def test_a_file_without_a_stem_is_what_it_was(tmp_path, dtype):
    """The bytes `save` writes for an index without a stem equal `np.savez` of the arrays as `save` spelt them before stems existed."""
    from temporalalignnet_amd.search import VideoIndex
    idx = _index(dtype, None)
    path = str(tmp_path / "i.npz")
    idx.save(path)
    f = idx.feat
    bf16 = f.dtype == torch.bfloat16
    want = io.BytesIO()
    np.savez(want, feat=(f.view(torch.int16).numpy().view(np.uint16) if bf16 else f.numpy()), bf16=np.array(bf16),
             e4m3=np.array(False), v_off=idx.v_off, vids=np.array(idx.vids, dtype=np.str_))
    with open(path, "rb") as fh:
        assert fh.read() == want.getvalue()
    back = VideoIndex.load(path, device="cpu")
    assert back.stem is None and torch.equal(back.feat.view(torch.uint8), f.view(torch.uint8))


def test_an_e4m3_index_keeps_its_stem_in_the_file(tmp_path):
    from temporalalignnet_amd.search import VideoIndex
    stem = torch.randn(17, 512).bfloat16()
    idx = VideoIndex(torch.randint(0, 255, (17, 512), dtype=torch.uint8), [0, 5, 17], ["x", "y"], torch.ones(17), stem)
    assert idx.quantize() is idx
    path = str(tmp_path / "i.npz")
    idx.save(path)
    back = VideoIndex.load(path, device="cpu")
    assert back.e4m3 and torch.equal(back.stem.view(torch.uint8), stem.view(torch.uint8)) and torch.equal(back.feat, idx.feat)
    with pytest.raises(AssertionError):
        VideoIndex(torch.zeros(17, 512), [0, 5, 17], ["x", "y"], stem=torch.zeros(16, 512))


def test_library_exports_the_rerank_entry_points():
    names, protos, L = _lib.declared_symbols(), _lib.declared_prototypes(), _lib.lib()
    want = {"tan_rerank_tail": (i, [p, p, i, i, i, p, i, p, p, p, p, p]), "tan_rerank_select": (i, [p, l, i, l, i, p, p])}
    for n, proto in want.items():
        assert n in names and getattr(L, n) is not None and protos[n] == proto, n


def test_bad_arguments_are_rejected_without_touching_a_device():
    L = _lib.lib()
    a = C.c_void_p(1 << 20)                            # never dereferenced: every call below fails its argument checks

    def tail(last=a, head=a, dtype=0, Ln=72, T=64, table=a, W=3, hw=a, hb=a, out=a, sim=None):
        return L.tan_rerank_tail(last, head, dtype, Ln, T, table, W, hw, hb, out, sim, None)

    def select(score=a, Q=4, P=7, stride=4, k=3, out=a):
        return L.tan_rerank_select(score, Q, P, stride, k, out, None)

    odd = C.c_void_p((1 << 20) + 8)
    for kw in (dict(last=None), dict(table=None), dict(out=None), dict(dtype=2), dict(W=0), dict(T=0), dict(T=1025, Ln=1100), dict(Ln=64),
               dict(hw=None), dict(hb=None), dict(last=odd), dict(head=odd), dict(out=odd), dict(hw=odd)):
        assert tail(**kw) == -1, kw
    for kw in (dict(score=None), dict(out=None), dict(Q=0), dict(P=0), dict(P=33), dict(k=0), dict(k=8), dict(stride=0)):
        assert select(**kw) == -1, kw


def test_reranked_fields():
    from temporalalignnet_amd.search import Reranked
    assert Reranked._fields == ("vid", "second", "score", "confidence", "alignability", "dual_second", "dual_score")


def test_cli_takes_keep_stem_rerank_and_pool():
    from temporalalignnet_amd import search
    q = ["query", "--checkpoint", "c", "--vocab", "/nonexistent/s3d_dict.npy", "--index", "i.npz", "-k", "7"]
    a = search.parse_args(q + ["--rerank", "--pool", "16", "crack two eggs"])
    assert a.rerank and a.pool == 16 and a.k == 7 and a.sentences == ["crack two eggs"]
    a = search.parse_args(q + ["--rerank", "whisk"])
    assert a.rerank and a.pool is None
    a = search.parse_args(q + ["whisk"])
    assert not a.rerank and a.pool is None
    for bad in (["--pool", "4", "whisk"], ["--rerank", "--pool", "0", "whisk"], ["--rerank", "--pool", "33", "whisk"],
                ["--rerank", "--moments", "whisk"], ["--rerank", "--sequence", "whisk"]):
        with pytest.raises(SystemExit):
            search.parse_args(q + bad)
    ix = ["index", "--checkpoint", "c", "--vocab", "v", "--feature-dir", "f", "--asr-json", "a", "--vlen-csv", "l", "--out", "o"]
    assert search.parse_args(ix + ["--keep-stem"]).keep_stem and not search.parse_args(ix).keep_stem
    with pytest.raises(FileNotFoundError):
        search.main(q + ["--rerank", "whisk"])                      # parsed; the run stops at the missing vocabulary
