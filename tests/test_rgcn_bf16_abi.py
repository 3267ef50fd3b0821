"""CPU-side checks of the RGCN layer's bf16 entries (include/het_amd.h: het_rgcn_layer_forward_bf16 / _backward_bf16): the header
declares them with het_bf16 activation rows, the library exports them, the ctypes table types them, and argument validation
answers before any launch.  (The checks that need a grouping -- K = 48, a misaligned x, a grouping of the wrong R -- build one on
the device: tests/test_gpu_rgcn_bf16.py.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("het_rgcn_layer_forward_bf16", "het_rgcn_layer_backward_bf16")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "het_amd.h")).read(), flags=re.S)


def test_header_declares_the_bf16_entries_with_bf16_rows():
    src = _header()
    assert re.search(r"typedef\s+uint16_t\s+het_bf16\s*;", src)
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        base = re.search(r"\bint\s+" + name[:-len("_bf16")] + r"\s*\(([^;]*)\)\s*;", src)
        fp32 = [p.strip() for p in base.group(1).split(",")]
        assert len(params) == len(fp32), name
        bf16_args = {p.split()[-1].lstrip("*") for p in params if "het_bf16" in p}
        # exactly the activation rows change type; every other argument is the fp32 entry's
        assert bf16_args == ({"x", "ret"} if "forward" in name else {"gradout", "grad_x"}), (name, bf16_args)
        for p, q in zip(params, fp32):
            if "het_bf16" not in p:
                assert p.split() == q.split(), (name, p, q)


def test_library_exports_and_ctypes_types_the_bf16_entries():
    from het_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in _lib._SIGNATURES, name
        assert _lib._SIGNATURES[name] == _lib._SIGNATURES[name[:-len("_bf16")]], name
        assert getattr(_lib.lib(), name).argtypes is not None


def test_bf16_entries_validate_before_any_launch():
    from het_amd import _lib
    L = _lib.lib()
    # no grouping: refused with the message, nothing launched (no device is needed to get the answer)
    rc = L.het_rgcn_layer_forward_bf16(None, 3, 10, None, None, None, None, None, None, None, None, None, 64, 64, None)
    assert rc == 1 and b"het_rgcn_layer_forward_bf16" in L.het_last_error() and b"grouping" in L.het_last_error()
    rc = L.het_rgcn_layer_backward_bf16(None, None, 3, 10, 10, None, None, None, None, None, None, None, None, None, None, 64, 64,
                                        None, 0, None)
    assert rc == 1 and b"het_rgcn_layer_backward_bf16" in L.het_last_error() and b"grouping" in L.het_last_error()


def test_bf16_argument_check_of_the_python_wrappers():
    """kernels.rgcn_layer_forward_bf16 refuses fp32 activation rows (and CPU tensors) by name, before the library is called."""
    import pytest
    import torch
    import het_amd.kernels as k
    plan = (None, None, torch.zeros((3, 4), dtype=torch.int32), None, None, None)
    with pytest.raises(k._lib.HetError, match="rgcn_layer_forward_bf16: expected contiguous bfloat16"):
        k.rgcn_layer_forward_bf16(plan, torch.zeros(4, 64), torch.zeros(3, 64, 64), torch.zeros(8), None)
    with pytest.raises(k._lib.HetError, match="rgcn_layer_backward_bf16: expected contiguous bfloat16"):
        k.rgcn_layer_backward_bf16((None, None, None, None, torch.zeros((3, 4), dtype=torch.int32), None), torch.zeros(4, 64),
                                   torch.zeros(3, 64, 64), torch.zeros(8), torch.zeros(4, 64, dtype=torch.bfloat16).t(), True)
