"""The C-ABI library loads on a CPU-only box and exports every symbol include/tan_hip.h declares (no compute calls)."""
import ctypes as C
import os
import re

from temporalalignnet_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_library_exports_every_declared_symbol():
    names = _lib.declared_symbols()
    assert len(names) >= 30 and "tan_gemm" in names and "tan_encoder_bwd" in names
    L = _lib.lib()
    for n in names:
        assert getattr(L, n) is not None, n
    assert L.tan_version() >= 100


def test_ctypes_mirrors_have_the_c_layout():
    L = _lib.lib()
    assert L.tan_abi_sizeof(0) == C.sizeof(_lib.GemmDesc)
    assert L.tan_abi_sizeof(1) == C.sizeof(_lib.LayerParams)
    assert L.tan_abi_sizeof(2) == C.sizeof(_lib.LayerBufs)
    assert L.tan_abi_sizeof(3) == C.sizeof(_lib.EncoderDesc)
    assert L.tan_abi_sizeof(4) == C.sizeof(_lib.SimFamDesc)
    assert L.tan_abi_sizeof(5) == C.sizeof(_lib.SimNceDesc)


def test_bad_arguments_are_rejected_without_touching_a_device():
    L = _lib.lib()
    d = _lib.GemmDesc()            # all-null descriptor
    assert L.tan_gemm(C.byref(d), None) == -1
    assert L.tan_layernorm_fwd(None, None, None, None, None, None, None, 0, C.c_long(4), 512, C.c_float(1e-5), 0, None) == -1
    assert L.tan_masked_quantile(None, None, 5, C.c_float(0.3), None, None) == -1
    s = _lib.SimNceDesc()          # all-null descriptor
    assert L.tan_simnce_fwd(C.byref(s), None) == -1 and L.tan_simnce_bwd(C.byref(s), None) == -1


def test_simfam_accepts_agrees_with_the_limits_written_out():
    """tan_simfam_accepts (what `loss.simfam_ok` asks) against the shape limits and the finishing launch's LDS bytes spelled out here."""
    L = _lib.lib()

    def restated(S, N, Mc, T):
        fin_lds = 4 * (2 * T * N + T + 256 + 96) + 4 * 32 + 32 + T + 16
        return S <= 8 and N <= 32 and Mc % 8 == 0 and Mc < 32768 and fin_lds <= 160 * 1024 and Mc <= L.tan_simnce_max_cols()

    assert restated(6, 16, 1344, 64) and L.tan_simfam_accepts(6, 6, 128, 64, 16, 1344) == 1
    assert not restated(6, 32, 1344, 622) and L.tan_simfam_accepts(6, 6, 128, 622, 32, 1344) == 0       # the LDS bound: T <= 621 at N = 32
    assert restated(6, 32, 1344, 621) and L.tan_simfam_accepts(6, 6, 128, 621, 32, 1344) == 1


def test_header_cites_reference_lines_and_has_no_torch_types():
    src = open(os.path.join(ROOT, "include", "tan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)          # declarations only
    assert "torch" not in code.lower() and "at::" not in code and "Tensor" not in code
    assert len(re.findall(r"(tan_model|tfm_model|loss|main)\.py:\d+", src)) >= 15


def test_product_has_no_cpu_fallback():
    """The HIP path must fail loudly on CPU tensors instead of silently computing elsewhere."""
    import pytest
    import torch
    from temporalalignnet_amd.tan_model import TemporalAligner
    m = TemporalAligner(1, 1, language_model=None)
    with pytest.raises(_lib.TanHipError):
        m(torch.zeros(1, 4, 1024), torch.zeros(1, 2, 512), torch.zeros(1, 4).bool(), torch.zeros(1, 2).bool(), None)
    from temporalalignnet_amd import ops
    with pytest.raises(_lib.TanHipError):
        ops.layernorm_fwd(torch.zeros(4, 512), torch.ones(512), torch.zeros(512), torch.zeros(4, 512))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "temporalalignnet_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), fn


def test_every_entry_point_gets_argtypes_from_the_header():
    """`_lib.py` used to set restype only, so every `long` / `float` argument relied on the caller wrapping it."""
    from temporalalignnet_amd import _lib
    protos = _lib.declared_prototypes()
    assert set(protos) == set(_lib.declared_symbols())
    import ctypes as C
    assert protos["tan_nce_ws_floats"] == (C.c_long, [C.c_int] * 4)
    assert protos["tan_adamw_step"][1][5:13] == [C.c_long, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_float]
    assert protos["tan_encoder_fwd"][1] == [C.c_void_p, C.c_void_p]
    L = _lib.lib()
    for name, (res, args) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # a plain Python int for a `long` parameter now converts (no GPU work: the call is rejected for its NULL pointers)
    assert L.tan_reduce_add(None, None, 2, 1 << 33, None) == -1
    # ... and a `long` RESULT beyond 2^31 comes back whole (the kept exponentials of B = 1024, S * R * Mc = 3.2e9 elements)
    assert L.tan_simnce_keep_elems(6, 65536, 8192) == 6 * 65536 * 8192
    assert L.tan_simfam_ws_bytes(6, 6, 128, 64, 16, 1344) > 0


def test_reference_import_names_resolve_with_one_sys_path_entry():
    """`from tan_model import TemporalAligner, TwinTemporalAligner` (train/main.py:21) and
    `from loss import get_loss, get_mask_from_time, get_text_pos` (main.py:16) must work with ONE sys.path entry."""
    import importlib
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tan_model import TemporalAligner, TwinTemporalAligner\n"
            "from loss import get_loss, get_mask_from_time, get_text_pos\n"
            "from tfm_model import TemporalEncoder, ResidualAttentionBlock_Step, QuickGELU, get_position_embedding_sine\n"
            "from word2vec_model import Word2VecModel, Word2VecTokenizer\n"
            "import temporalalignnet_amd.tan_model as t\n"
            "assert TemporalAligner is t.TemporalAligner\n"
            "print('ok')\n") % os.path.join(root, "dropin")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr
