"""CPU-side checks of the HGT layer's bf16 entries (include/het_amd.h): the header declares them with het_bf16 activation rows, the
library exports them, the ctypes table types them with matching argument counts, and argument validation answers before any
launch.  (The checks that need a grouping or device tensors are in tests/test_gpu_hgt_bf16.py.)

Also here, because they need no GPU: the two references tests/test_gpu_hgt_bf16.py measures against (tests/_hgt_bf16_ref.py) are
validated against the oracle -- the explicit fp64 backward of the attention rows (formulas of csrc/hgt_compact.hip's header comment) equals the oracle's
autograd, and the staged emulation of the layer with rounding switched off equals oracle/layers.py::hgt_layer."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry -> (fp32 twin or None, names of the het_bf16 pointers)
ENTRIES = {
    "het_hgt_aggregate_compact_bf16": ("het_hgt_aggregate_compact", {"kv_c", "q", "out"}),
    "het_hgt_backward_compact_bf16": ("het_hgt_backward_compact", {"kv_c", "q", "out", "gradout"}),
    "het_node_rows_matmul_sum_bf16": ("het_node_rows_matmul_sum", {"out"}),
    "het_rows_matmul_bf16": (None, {"x", "out"}),
    "het_rows_matmul_backward_dw_bf16": (None, {"x"}),
    "het_rows_matmul_backward_dw_bf16_bf16": (None, {"x", "gradout"}),
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "het_amd.h")).read(), flags=re.S)


def _params(src, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/het_amd.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_declares_the_bf16_entries_with_bf16_rows():
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


def test_library_exports_and_ctypes_types_the_bf16_entries():
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


def test_bf16_entries_validate_before_any_launch():
    from het_amd import _lib
    L = _lib.lib()
    rc = L.het_hgt_aggregate_compact_bf16(None, None, None, None, None, 10, 10, 8, 8, None, 0, None)
    assert rc == 1 and b"het_hgt_aggregate_compact_bf16: null argument" in L.het_last_error()
    rc = L.het_hgt_backward_compact_bf16(None, None, None, None, None, None, None, None, None, 10, 10, 8, 8, None, 0, None)
    assert rc == 1 and b"het_hgt_backward_compact_bf16: null argument" in L.het_last_error()
    rc = L.het_rows_matmul_bf16(None, 1, None, None, 10, None, None, None, 64, 64, None)
    assert rc == 1 and b"het_rows_matmul_bf16" in L.het_last_error()
    one = (ctypes.c_int64 * 2)(0, 10)
    buf = ctypes.create_string_buffer(64)  # (never read: the shape is refused first)
    rc = L.het_rows_matmul_bf16(one, 1, None, None, 10, buf, buf, buf, 48, 64, None)
    assert rc != 0 and b"K in {32, 64}" in L.het_last_error()
    rc = L.het_rows_matmul_backward_dw_bf16(one, 1, None, None, 10, buf, buf, buf, 64, 256, 0, None)
    assert rc != 0 and b"X in {32, 64, 128}" in L.het_last_error()


def test_bf16_argument_check_of_the_python_wrappers():
    """The kernels.py wrappers refuse fp32 activation rows (and CPU tensors) by name, before the library is called."""
    import het_amd.kernels as k
    z = torch.zeros
    with pytest.raises(k._lib.HetError, match="hgt_aggregate_compact_bf16: expected contiguous bfloat16"):
        k.hgt_aggregate_compact_bf16(None, z(4, 2, 64), z(4, 64), z(4, 8), z(4, 64))
    with pytest.raises(k._lib.HetError, match="hgt_backward_compact_bf16: expected contiguous bfloat16"):
        k.hgt_backward_compact_bf16(None, z(4, 2, 64), z(4, 64), z(4, 8), z(4, 64), z(4, 64), z(4, 2, 64), z(4, 64))
    with pytest.raises(k._lib.HetError, match="rows_matmul_bf16: expected contiguous bfloat16"):
        k.rows_matmul_bf16(z(2, dtype=torch.int64), None, None, z(1, 1, 64, 64), z(4, 64), z(4, 64))
    with pytest.raises(k._lib.HetError, match="rows_matmul_backward_dw_bf16: expected contiguous bfloat16"):
        k.rows_matmul_backward_dw_bf16(z(2, dtype=torch.int64), None, z(4, 64), z(4, 64), z(1, 1, 64, 64), False)
    with pytest.raises(k._lib.HetError, match="node_rows_matmul_sum_bf16: expected contiguous bfloat16"):
        k.node_rows_matmul_sum_bf16(0, 4, [(z(4, 64), 0, None, z(64, 64))], z(4, 64))


# ---- the references of the GPU tests (tests/_hgt_bf16_ref.py), checked against the oracle on the CPU --------------------------
from tests._hgt_bf16_ref import PARAMS, attention_rows_backward, staged_emulation  # noqa: E402


@pytest.mark.parametrize("H,D,n,e", [(8, 8, 300, 5000), (4, 16, 40, 9000), (1, 32, 30, 4000)])
def test_explicit_attention_backward_is_the_oracles_autograd(H, D, n, e):
    from oracle import ops as O
    from tests.util import random_graph
    g = random_graph(seed=29, n=n, r=4, e=e)
    s = g.get_separate_coo_original()
    inv = g.get_separate_unique_node_indices_single_sided_inverse_idx()
    S_row = g.get_separate_unique_node_indices_single_sided()["node_indices_row"].numel()
    srow, col, N = inv["inverse_indices_row"][s["eids"]].contiguous(), s["col_indices"], g.get_num_nodes()
    gen = torch.Generator().manual_seed(6)
    kv = (torch.randn(S_row, 2, H, D, generator=gen, dtype=torch.float64) * 0.6).requires_grad_(True)
    q = (torch.randn(N, H, D, generator=gen, dtype=torch.float64) * 0.6).requires_grad_(True)
    go = torch.randn(N, H, D, generator=gen, dtype=torch.float64)
    _, out = O.hgt_attention_rows(kv, q, srow, col, N)
    gkv_r, gq_r = torch.autograd.grad(out, [kv, q], go)
    gkv, gq = attention_rows_backward(kv.detach(), q.detach(), go, out.detach(), srow, col)
    for name, a, b in (("grad_kv", gkv, gkv_r), ("grad_q", gq, gq_r)):
        rel = float((a - b).norm() / b.norm())
        print(f"{name}: explicit vs autograd rel L2 {rel:.2e}")
        assert rel <= 1e-12, name


@pytest.mark.parametrize("fused_attn", [False, True])
@pytest.mark.parametrize("H,in_dim,out_dim", [(8, 64, 64), (2, 32, 64), (1, 32, 32)])
def test_staged_emulation_without_rounding_is_the_oracle(fused_attn, H, in_dim, out_dim):
    from het_amd.layers import HET_HGTLayerHetero
    from oracle import layers as OL
    from tests.util import mag_graph
    g = mag_graph(1.5e-3)
    torch.manual_seed(4)
    N, R, T = g.get_num_nodes(), g.get_num_rels(), g.get_num_ntypes()
    layer = HET_HGTLayerHetero(T, R, in_dim, out_dim, num_heads=H, dropout=0.0, hgt_fused_attn_score_flag=fused_attn)
    with torch.no_grad():
        layer.relation_pri.uniform_(0.5, 1.5)
        layer.skip.uniform_(-1, 1)
    h, go = torch.randn(N, in_dim, dtype=torch.float64) * 0.5, torch.randn(N, out_dim, dtype=torch.float64)
    s = g.get_separate_coo_original()
    offs = g.get_original_node_type_offsets()
    res = []
    for emu in (False, True):
        p = {n: getattr(layer, n).detach().double().requires_grad_(True) for n in PARAMS}
        h64 = h.clone().requires_grad_(True)
        if emu:
            out = staged_emulation(h64, offs, s["rel_ptrs"], s["row_indices"], s["col_indices"], N, g.get_rel_node_types()[0], p, H,
                                   fused_attn, False)
        else:
            out = OL.hgt_layer(h64, offs, s["rel_ptrs"], s["row_indices"], s["col_indices"], N, *(p[n] for n in PARAMS), H,
                               fused_attn=fused_attn)
        res.append([out.detach()] + list(torch.autograd.grad(out, [h64] + [p[n] for n in PARAMS], go)))
    for name, a, b in zip(["out", "grad_h"] + PARAMS, res[1], res[0]):
        rel = float((a - b).norm() / b.norm())
        print(f"{name}: emulation without rounding vs oracle rel L2 {rel:.2e}")
        assert rel <= 1e-10, name
