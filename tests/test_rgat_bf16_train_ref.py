"""What tests/test_gpu_rgat_bf16_train.py relies on and no GPU is needed for: the staged emulation of the RGAT layer's bf16 training
contract (tests/_rgat_bf16_train_ref.py) is, with its roundings off, the oracle -- output and every gradient; the C entries of the
bf16 training step are declared, exported and typed for ctypes; the layer takes the keyword."""
import ctypes
import os
import re

import pytest
import torch

from tests import _rgat_bf16_train_ref as TREF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry -> (fp32 twin or None, names of the het_bf16 pointers)
ENTRIES = {
    "het_rgat_aggregate_compact_runs_bf16": ("het_rgat_aggregate_compact_runs", {"feat_c", "h_inout"}),
    "het_rgat_backward_compact_runs_bf16": ("het_rgat_backward_compact_runs", {"feat_c", "gradout"}),
    "het_rgat_node_backward_dx_bf16": ("het_rgat_node_backward_dx", {"grad_h", "grad_x"}),
    "het_rows_dot1h_backward_dw_bf16": (None, {"x"}),
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "het_amd.h")).read(), flags=re.S)


def _params(src, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/het_amd.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_declares_the_entries_with_bf16_rows():
    src = _header()
    for name, (twin, rows) in ENTRIES.items():
        params = _params(src, name)
        assert {p.split()[-1].lstrip("*") for p in params if "het_bf16" in p} == rows, name
        if twin is not None:  # exactly the activation rows change type; every other argument is the fp32 entry's
            fp32 = _params(src, twin)
            assert len(params) == len(fp32), name
            for p, q in zip(params, fp32):
                if "het_bf16" not in p:
                    assert p.split() == q.split(), (name, p, q)


def test_library_exports_and_ctypes_types_the_entries():
    from het_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    src = _header()
    for name, (twin, _) in ENTRIES.items():
        assert hasattr(L, name), name
        assert name in _lib._SIGNATURES, name
        assert len(_lib._SIGNATURES[name]) == len(_params(src, name)), name
        if twin is not None:
            assert _lib._SIGNATURES[name] == _lib._SIGNATURES[twin], name
        assert getattr(_lib.lib(), name).argtypes is not None


def test_null_arguments_are_refused_before_anything_else():
    """No grouping, no tables: HET_ERR_INVALID_ARG (1) with a message, without a GPU."""
    from het_amd import _lib
    L = _lib.lib()
    assert L.het_rgat_aggregate_compact_runs_bf16(None, None, 4, None, None, None, None, None, 10, 4, 16, 0.2, None, 0, None, None, None, 0,
                                                  None, None, None, 0, None) == 1
    assert L.het_rgat_backward_compact_runs_bf16(None, None, None, None, None, None, None, None, None, None, None, None, None, None, None,
                                                 None, 4, None, 0, 10, 10, 10, 4, 16, 0.2, None, None, 0, None) == 1
    assert b"null argument" in L.het_last_error()
    assert L.het_rgat_node_backward_dx_bf16(0, 10, 10, 10, 9, None, None, None, None, None, None, None, None, None, 4, 64, 16, None, None) == 1
    assert b"unsupported shape" in L.het_last_error()  # (9 relations)
    one = (ctypes.c_int64 * 2)(0, 10)
    h = ctypes.c_void_p(64)
    assert L.het_rows_dot1h_backward_dw_bf16(one, 1, None, None, 10, h, h, h, 3, 64, 0, None) == 3  # (3 heads: HET_ERR_UNSUPPORTED)


def test_layer_takes_the_keyword_and_defaults_to_off():
    from het_amd.layers import HET_RGATLayer
    assert HET_RGATLayer(64, 64, 3, 4).bf16_training is False
    assert HET_RGATLayer(64, 64, 3, 4, bf16_training=True).bf16_training is True


@pytest.mark.parametrize("name", TREF.CASE_NAMES)
def test_emulation_without_rounding_is_the_oracle(name):
    """Output, grad_x and every parameter gradient to 1e-10 relative L2, on the cases of the GPU value test."""
    case = TREF.CASES[TREF.CASE_NAMES.index(name)]
    g, layer, xb, gob = TREF.build_case(case)
    ref, emu = TREF.oracle_and_emulation(case, g, layer, xb, gob, rounding=False)
    for n, r, e in zip(TREF.NAMES, ref, emu):
        assert (r is None) == (e is None) == (n.startswith("grad_") and n != "grad_x" and not hasattr(layer, n[5:])), n
        if r is not None:
            assert r.shape == e.shape and TREF.rel_l2(e, r) <= 1e-10, (n, TREF.rel_l2(e, r))


def test_emulation_rounds_where_the_contract_says():
    """With roundings on: the output and grad_x are bf16 values, the parameter gradients are not, and the output is the evaluation
    contract's (tests/_rgat_bf16_ref.py::staged_reference) exactly."""
    from tests import _rgat_bf16_ref as REF
    case = TREF.CASES[0]
    g, layer, xb, gob = TREF.build_case(case)
    _, emu = TREF.oracle_and_emulation(case, g, layer, xb, gob)
    out, gx, gw = emu[0], emu[1], emu[2]
    assert torch.equal(out, REF.bf16_round(out)) and torch.equal(gx, REF.bf16_round(gx)) and not torch.equal(gw, REF.bf16_round(gw))
    assert torch.equal(out, REF.reference_of(case, g, layer, xb))
