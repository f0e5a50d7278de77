"""Host-side pieces of the e4m3 corpus index: the two entry points of csrc/tan_retrieve.hip as the header declares them, their
argument checks (which run before anything touches a device), the index file in both layouts, and the no-fallback rule."""
import ctypes as C

import numpy as np
import pytest
import torch

from temporalalignnet_amd import _lib


def test_library_exports_the_e4m3_entry_points():
    names, protos, L = _lib.declared_symbols(), _lib.declared_prototypes(), _lib.lib()
    for n in ("tan_quantize_rows_e4m3", "tan_rank_topk_e4m3"):
        assert n in names and getattr(L, n).argtypes == protos[n][1] and getattr(L, n).restype is C.c_int, n
    p, i, l = C.c_void_p, C.c_int, C.c_long                                           # noqa: E741
    assert protos["tan_quantize_rows_e4m3"] == (i, [p, i, l, i, p, p, p])
    assert protos["tan_rank_topk_e4m3"] == (i, [p, p, p, p, l, l, i, p, i, i, p, p, p, p, p, p])


def test_bad_arguments_return_minus_one_without_a_device():
    L = _lib.lib()
    buf = (C.c_char * 4096)()                                                          # host memory: never dereferenced by a refused call
    a = C.c_void_p((C.addressof(buf) + 15) // 16 * 16)
    assert L.tan_quantize_rows_e4m3(None, 0, 4, 512, None, None, None) == -1
    for kw in (dict(n=0), dict(n=-3), dict(n=1 << 31), dict(Cc=256), dict(Cc=1024), dict(dtype=2), dict(dtype=-1)):
        args = dict(dtype=0, n=4, Cc=512)
        args.update(kw)
        assert L.tan_quantize_rows_e4m3(a, args["dtype"], args["n"], args["Cc"], a, a, None) == -1, kw
    assert L.tan_quantize_rows_e4m3(a, 0, 4, 512, C.c_void_p(a.value + 4), a, None) == -1          # codes not 8-byte aligned
    assert L.tan_rank_topk_e4m3(None, None, None, None, 4, 4, 512, None, 1, 0, None, None, None, None, None, None) == -1

    def call(Q=4, N=40, Cc=512, pair=a, k=10, splits=0, tq=a, qs=a, vn=a, vs=a, hi=a, ti=a, ts=a, tr=a, ws=a):
        return L.tan_rank_topk_e4m3(tq, qs, vn, vs, Q, N, Cc, pair, k, splits, hi, ti, ts, tr, ws, None)

    for kw in (dict(Cc=256), dict(k=33), dict(k=41), dict(k=-1), dict(Q=0), dict(N=0), dict(N=1 << 31), dict(k=0, pair=None),
               dict(splits=-1), dict(tq=None), dict(qs=None), dict(vn=None), dict(vs=None), dict(hi=None), dict(ti=None),
               dict(ts=None), dict(tr=None), dict(ws=None), dict(vn=C.c_void_p(a.value + 8))):
        assert call(**kw) == -1, kw


def test_e4m3_index_save_load_roundtrip_on_the_host(tmp_path):
    from temporalalignnet_amd.search import VideoIndex
    g = torch.Generator().manual_seed(2)
    codes = torch.randint(0, 256, (17, 512), dtype=torch.uint8, generator=g)
    scale = torch.ldexp(torch.ones(17), torch.randint(-20, 5, (17,), generator=g))
    p = str(tmp_path / "i_e4m3.npz")
    idx = VideoIndex(codes, [0, 5, 17], ["x", "y"], scale)
    assert idx.e4m3 and idx.quantize() is idx
    idx.save(p)
    with np.load(p, allow_pickle=False) as z:
        assert bool(z["e4m3"]) and not bool(z["bf16"]) and z["feat"].dtype == np.uint8 and z["scale"].dtype == np.float32
    back = VideoIndex.load(p, device="cpu")
    assert back.e4m3 and back.feat.dtype == torch.uint8 and torch.equal(back.feat, codes) and torch.equal(back.scale, scale)
    assert back.v_off.tolist() == [0, 5, 17] and back.vids == ["x", "y"]
    v, sec = back.locate(np.array([4, 5, 16]))
    assert v.tolist() == [0, 1, 1] and sec.tolist() == [4, 0, 11]
    with pytest.raises(AssertionError):
        VideoIndex(codes, [0, 5, 17], ["x", "y"])                                    # codes without scales are not an index


def test_load_still_reads_the_layout_without_an_e4m3_key(tmp_path):
    from temporalalignnet_amd.search import VideoIndex
    for dt in (torch.bfloat16, torch.float32):
        f = torch.randn(17, 512).to(dt)
        p = str(tmp_path / f"old_{dt}.npz".replace("torch.", ""))
        bf16 = dt == torch.bfloat16
        with open(p, "wb") as fh:                                                     # exactly the keys the earlier `save` wrote
            np.savez(fh, feat=(f.view(torch.int16).numpy().view(np.uint16) if bf16 else f.numpy()), bf16=np.array(bf16),
                     v_off=np.array([0, 5, 17]), vids=np.array(["x", "y"], dtype=np.str_))
        back = VideoIndex.load(p, device="cpu")
        assert not back.e4m3 and back.scale is None and back.feat.dtype == dt and torch.equal(back.feat, f)
        assert back.v_off.tolist() == [0, 5, 17] and back.vids == ["x", "y"]
        p2 = str(tmp_path / "new.npz")                                                # and what `save` writes now for such an index
        back.save(p2)
        again = VideoIndex.load(p2, device="cpu")
        assert not again.e4m3 and torch.equal(again.feat, f)


def test_e4m3_ops_raise_on_host_tensors():
    from temporalalignnet_amd import ops
    x = torch.randn(4, 512)
    with pytest.raises(_lib.TanHipError):
        ops.quantize_rows_e4m3(x)
    with pytest.raises(_lib.TanHipError):
        ops.quantize_rows_e4m3(x.bfloat16())
    codes, scale = torch.zeros(4, 512, dtype=torch.uint8), torch.ones(4)
    with pytest.raises(_lib.TanHipError):
        ops.rank_topk_e4m3(codes, scale, codes, scale, None, 1)
    with pytest.raises(_lib.TanHipError):
        ops.rank_topk_e4m3(codes, scale, codes, scale, torch.zeros(4, dtype=torch.int32), 0)


def test_cli_takes_the_index_dtype():
    from temporalalignnet_amd import search
    argv = ["index", "--checkpoint", "c", "--vocab", "/nonexistent/s3d_dict.npy", "--feature-dir", "f", "--asr-json", "a", "--vlen-csv", "l",
            "--out", "o", "--index-dtype"]
    with pytest.raises(SystemExit):
        search.main(argv + ["fp4"])
    for ok in ("e4m3", "bf16", "fp32"):                                               # parsed; the run then stops at the missing vocabulary
        with pytest.raises(FileNotFoundError):
            search.main(argv + [ok])
