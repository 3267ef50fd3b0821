"""CPU checks of the RGAT layer's bf16 evaluation path: the staged reference of its precision contract (tests/_rgat_bf16_ref.py)
against the oracle, and the new entries as an interface -- declared, exported, marshalled, validated on the host.  No GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from oracle import layers as OL
from tests import _rgat_bf16_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("het_rgat_aggregate_compact_forward_bf16", "het_rows_linear_bias_bf16")
HELPERS = ("het_rgat_el_rows_bf16", "het_rows_matmul_heads_bf16", "het_rows_dot1h_bf16")
HET_ERR_INVALID_ARG, HET_ERR_UNSUPPORTED = 1, 3


def _oracle(case, g, layer, x):
    s = g.get_separate_coo_original()
    p = {n: t.detach().double() for n, t in layer.named_parameters()}
    ref = OL.rgat_layer(x.double(), p["conv_weights"], p["attn_l"], p["attn_r"], s["rel_ptrs"], s["row_indices"], s["col_indices"],
                        g.get_num_nodes(), 0.2, p.get("loop_weight"), p.get("h_bias"))
    return ref if case["nd"] is None else ref[:case["nd"]]


@pytest.mark.parametrize("name", REF.CASE_NAMES)
def test_staged_reference_without_rounding_is_the_oracle(name):
    """Self-loop and bias on and off, empty relations (random_graph leaves relation 1 empty), nodes without in-edges, a block."""
    case = REF.CASES[REF.CASE_NAMES.index(name)]
    g, layer, x = REF.build_case(case)
    ref, emu = _oracle(case, g, layer, x), REF.reference_of(case, g, layer, x, rounding=False)
    assert emu.dtype == torch.float64 and emu.shape == ref.shape
    assert float((emu - ref).norm() / ref.norm()) <= 1e-12
    assert float((emu - ref).abs().max() / ref.abs().max()) <= 1e-12
    # the distance of the contract itself (roundings on) to the plain oracle: reported, not bounded
    rounded = REF.reference_of(case, g, layer, x)
    print(f"{name}: staged bf16 reference against the oracle: rel L2 {float((rounded - ref).norm() / ref.norm()):.3e}, "
          f"max |diff| / max|ref| {float((rounded - ref).abs().max() / ref.abs().max()):.3e}")


def test_the_cases_cover_what_they_claim():
    s = REF.build_graph(("random", 720, 350, 4, 6000)).get_separate_coo_original()
    assert int((s["rel_ptrs"][1:] == s["rel_ptrs"][:-1]).sum()) >= 1  # an empty relation
    g = REF.build_graph(("random", 722, 2000, 5, 1500))
    no_in = torch.ones(g.get_num_nodes(), dtype=torch.bool)
    no_in[g.get_separate_coo_original()["col_indices"]] = False
    assert int(no_in.sum()) > 100
    indeg = torch.bincount(REF.build_graph(("ladder", 5, 3)).get_separate_coo_original()["col_indices"])
    assert int((indeg > 256).sum()) >= 2  # hub destinations above HET_RGAT_HUB_MIN


def test_nodes_without_in_edges_keep_the_rounded_self_loop_row():
    case = REF._case("sparse", ("random", 722, 2000, 5, 1500), 4, 64, 64)
    g, layer, x = REF.build_case(case)
    out = REF.reference_of(case, g, layer, x)
    no_in = torch.ones(g.get_num_nodes(), dtype=torch.bool)
    no_in[g.get_separate_coo_original()["col_indices"]] = False
    h = REF.bf16_round(x.double() @ layer.loop_weight.detach().double() + layer.h_bias.detach().double())
    assert torch.equal(out[no_in], h[no_in])
    ref = _oracle(case, g, layer, x)
    assert float((REF.reference_of(case, g, layer, x, rounding=False) - ref).abs().max() / ref.abs().max()) <= 1e-12


def test_abs_term_measurement_runs():
    """The absolute term of the GPU test's bound is 4x this measurement (recorded in tests/test_gpu_rgat_bf16.py); printed here."""
    worst, per = REF.measure_abs_term()
    for n, v in per:
        print(f"{n}: fp32 against fp64 evaluation of the staged reference needs a >= {v:.3e}")
    print(f"worst {worst:.3e}: a = max(1e-5, 4 x worst) = {max(1e-5, 4 * worst):.3e}")
    assert worst >= 0


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "het_amd.h")).read(), flags=re.S)


def test_bf16_entries_are_declared_exported_and_marshalled():
    from het_amd import _lib
    import het_amd.kernels as k
    src = _header()
    for name in ENTRIES + HELPERS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert m, name + " is not declared in include/het_amd.h"
        assert hasattr(_lib.lib(), name), name + " is not exported by libhet_amd.so"
        assert name in _lib._SIGNATURES and len(_lib._SIGNATURES[name]) == len(m.group(1).split(",")), name
        assert callable(getattr(k, name[4:], None)), name
    params = re.search(r"\bint\s+het_rgat_aggregate_compact_forward_bf16\s*\(([^;]*)\)\s*;", src).group(1)
    assert "const het_bf16* feat_c" in params and "het_bf16* h_inout" in params and "const float* er_c" in params
    params = re.search(r"\bint\s+het_rows_linear_bias_bf16\s*\(([^;]*)\)\s*;", src).group(1)
    assert "const het_bf16* x" in params and "het_bf16* out" in params and "const float* w" in params and "const float* bias" in params
    # the twin's arguments, in the twin's order
    assert _lib._SIGNATURES[ENTRIES[0]] == _lib._SIGNATURES["het_rgat_aggregate_compact_forward"]
    assert _lib._SIGNATURES[ENTRIES[1]] == _lib._SIGNATURES["het_rows_linear_bias"]


def _aligned(nbytes):
    buf = C.create_string_buffer(nbytes + 16)
    return buf, C.c_void_p((C.addressof(buf) + 15) & ~15)


def test_argument_validation_without_gpu():
    """Checked on the host, in this order, before a grouping is read or anything is enqueued (the pointers are never dereferenced)."""
    from het_amd import _lib
    L = _lib.lib()
    name = ENTRIES[0].encode()
    keep_g, fake = _aligned(4096)
    keep_h, h = _aligned(64)

    def fwd(by_dst, by_dst_rel, H, D, h_inout, feat=None):
        return L.het_rgat_aggregate_compact_forward_bf16(by_dst, by_dst_rel, 3, feat, None, None, H, D, 0.2, h_inout, 10, None, None, None, 0,
                                                         None)
    assert fwd(None, None, 4, 16, h) == HET_ERR_INVALID_ARG and name in L.het_last_error() and b"null" in L.het_last_error()
    assert fwd(fake, None, 4, 16, h) == HET_ERR_INVALID_ARG
    assert fwd(fake, fake, 4, 16, None) == HET_ERR_INVALID_ARG and b"h_inout" in L.het_last_error()
    assert fwd(fake, fake, 4, 16, C.c_void_p(h.value + 8)) == HET_ERR_INVALID_ARG and b"h_inout" in L.het_last_error()
    assert fwd(fake, fake, 4, 16, h, C.c_void_p(h.value + 8)) == HET_ERR_INVALID_ARG and b"feat_c" in L.het_last_error()
    for H, D in ((8, 8), (3, 16)):
        assert fwd(fake, fake, H, D, h) == HET_ERR_UNSUPPORTED, (H, D)
        assert name in L.het_last_error() and b"unsupported shape" in L.het_last_error()
    one = (C.c_int64 * 2)(0, 10)
    assert L.het_rows_linear_bias_bf16(None, h, h, h, h, 10, 64, 64, None) == HET_ERR_INVALID_ARG
    assert b"het_rows_linear_bias_bf16" in L.het_last_error()
    assert L.het_rows_linear_bias_bf16(one, h, h, None, None, 10, 64, 64, None) == HET_ERR_INVALID_ARG
    assert L.het_rows_linear_bias_bf16(one, h, h, None, h, 10, 48, 64, None) == HET_ERR_UNSUPPORTED
    assert b"{32, 64, 128}" in L.het_last_error()
    assert L.het_rows_linear_bias_bf16(one, C.c_void_p(h.value + 8), h, None, h, 10, 64, 64, None) == HET_ERR_UNSUPPORTED
    assert L.het_rows_matmul_heads_bf16(one, 1, None, 10, h, h, h, 4, 256, 16, None) == HET_ERR_UNSUPPORTED
    assert L.het_rows_dot1h_bf16(one, 1, None, None, 10, h, h, h, 3, 64, None) == HET_ERR_UNSUPPORTED
    assert L.het_rgat_el_rows_bf16(one, 1, h, h, h, 10, 8, 8, None) == HET_ERR_UNSUPPORTED
    del keep_g, keep_h


def test_python_wrappers_refuse_fp32_rows_by_name():
    import het_amd.kernels as k
    z = torch.zeros
    with pytest.raises(k._lib.HetError, match="rgat_aggregate_compact_forward_bf16: expected contiguous bfloat16"):
        k.rgat_aggregate_compact_forward_bf16((None,) * 4, z(4, 4, 16), None, z(4, 4), z(4, 64), 0.2, 3)
    with pytest.raises(k._lib.HetError, match="rows_linear_bias_bf16: expected contiguous bfloat16"):
        k.rows_linear_bias_bf16(z(2, dtype=torch.int64), z(4, 64), z(64, 64), None)


def test_cpu_bf16_input_is_handed_to_the_fp32_layer():
    """CPU tensors are outside the native path: the layer hands x.float() to the fp32 layer.  The library has no CPU form of any
    layer, fp32 included, so that call is refused by name -- what is checked is that the refusal is the fp32 layer's, i.e. that the
    upcast copy, not the bf16 tensor, reached it.  A CPU bf16 input is not served."""
    import het_amd.kernels as k
    case = REF._case("cpu", ("random", 720, 350, 4, 6000), 4, 64, 64)
    g, layer, x = REF.build_case(case)
    assert layer._route(g, x, None, False).path == "upcast"
    with torch.no_grad(), pytest.raises(k._lib.HetError, match="float32 GPU tensors, got torch.float32 on cpu"):
        layer(g, x)


def test_halo_call_with_bf16_rows_goes_through_the_fp32_layer(monkeypatch):
    """forward_with_halo has no bf16 form: it hands x_own.float() to the fp32 halo path and casts what comes back (None stays
    None: the caller then exchanges first and calls forward).  The halo path itself is stubbed: what is checked is the routing."""
    from het_amd.backend import rgat_fused_layer as FL
    case = REF._case("halo", ("random", 720, 350, 4, 6000), 4, 64, 64)
    g, layer, x = REF.build_case(case)
    seen = []
    decide = FL.rgat_route.decide

    def served(facts, *lazy):  # (the real decision for the bf16 call; the fp32 halo call it hands on is "served" by the stub)
        if facts.bf16:
            return decide(facts, *lazy)
        assert facts.halo
        return FL.rgat_route.Route("node", facts.R, facts.H, facts.K, facts.D, True, True, True, True, True)

    def fused(route, g_, x_, *a, **k):
        seen.append(x_.dtype)
        assert route.path == "node" and k.get("halo") is not None
        return x_ * 2.0

    monkeypatch.setattr(FL.rgat_route, "decide", served)
    monkeypatch.setattr(FL, "rgat_layer_fused", fused)
    with torch.no_grad():
        out = layer.forward_with_halo(g, x, object())
    assert seen == [torch.float32] and out.dtype == torch.bfloat16 and torch.equal(out, (x.float() * 2.0).to(torch.bfloat16))
    monkeypatch.setattr(FL.rgat_route, "decide", lambda facts, *lazy: decide(facts, *lazy) if facts.bf16 else
                        FL.rgat_route.Route("composition", facts.R, facts.H, facts.K, facts.D))
    assert layer.forward_with_halo(g, x, object()) is None
