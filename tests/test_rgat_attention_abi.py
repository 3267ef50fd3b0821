"""The attention output of the compact RGAT layer (het_rgat_attention_compact) as an interface: declared, exported, marshalled and
validated on the host before anything touches a GPU; and what tests/test_gpu_rgat_attention.py rests on that needs no GPU -- the
torch composition against the fp64 reference, and the measurement its bounds come from.  Runs without a GPU.

The interface and composition tests fail on a tree without the feature.  test_reference_is_the_oracle_layer and
test_recorded_measurements check the reference helper alone (tests/_rgat_attention_ref.py against oracle/layers.py, and the figures
the GPU file's bounds are 4 x of): they are self-checks of the yardstick and pass wherever the helper exists."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, WORKSPACE = "het_rgat_attention_compact", "het_rgat_attention_compact_workspace"
HET_OK, HET_ERR_INVALID_ARG, HET_ERR_UNSUPPORTED = 0, 1, 3


def test_entries_are_declared_and_exported():
    from het_amd import _lib
    header = open(os.path.join(ROOT, "include", "het_amd.h")).read()
    for name in (ENTRY, WORKSPACE):
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in include/het_amd.h"
        assert hasattr(_lib.lib(), name), name + " is not exported by libhet_amd.so"
    assert ENTRY in _lib._SIGNATURES


def test_python_interface():
    import het_amd.kernels as k
    from het_amd.layers import HET_RGATLayer
    assert callable(getattr(k, "rgat_attention_compact", None))
    sig = inspect.signature(HET_RGATLayer.forward)
    assert sig.parameters["get_attention"].default is False
    assert "get_attention" not in inspect.signature(HET_RGATLayer.forward_with_halo).parameters


def _aligned(nbytes):
    """A zeroed host buffer and a 16-byte aligned address inside it (never dereferenced by the calls below)."""
    buf = C.create_string_buffer(nbytes + 16)
    return buf, C.c_void_p((C.addressof(buf) + 15) & ~15)


def test_argument_validation_without_gpu():
    """A null grouping, unsupported head counts, null and misaligned pointers and a grouping of another shape are refused with the
    documented code and a message that names the entry, before anything is enqueued; no edges is HET_OK."""
    from het_amd import _lib
    L = _lib.lib()
    keep_g, grouping = _aligned(4096)  # (a zeroed het_grouping: no positions)
    keep_b, buf = _aligned(256)

    def call(by_dst, el, er, H, col, srow, drow, eids, E, N, lse, attn):
        return L.het_rgat_attention_compact(by_dst, el, er, H, 0.2, col, srow, drow, eids, E, N, lse, attn, None, 0, None)

    assert call(None, buf, buf, 4, buf, buf, buf, None, 10, 10, None, buf) == HET_ERR_INVALID_ARG
    assert ENTRY.encode() in L.het_last_error() and b"null" in L.het_last_error()
    for H in (3, 16, 0):
        assert call(grouping, buf, buf, H, buf, buf, buf, None, 10, 10, None, buf) == HET_ERR_UNSUPPORTED, H
        assert ENTRY.encode() in L.het_last_error() and b"unsupported shape" in L.het_last_error()
    assert call(grouping, buf, buf, 4, buf, buf, buf, None, 10, 2 ** 31, None, buf) == HET_ERR_UNSUPPORTED
    # no edges: nothing is looked at
    assert call(grouping, None, None, 4, None, None, None, None, 0, 10, None, None) == HET_OK
    # every required pointer
    for i in range(6):
        ptrs = [buf] * 6
        ptrs[i] = None
        el, er, col, srow, drow, attn = ptrs
        assert call(grouping, el, er, 4, col, srow, drow, None, 10, 10, None, attn) == HET_ERR_INVALID_ARG, i
        assert ENTRY.encode() in L.het_last_error() and b"null" in L.het_last_error()
    # misaligned: a float tensor off 16 bytes, an id list off 8
    off8, off4 = C.c_void_p(buf.value + 8), C.c_void_p(buf.value + 4)
    assert call(grouping, off8, buf, 4, buf, buf, buf, None, 10, 10, None, buf) == HET_ERR_INVALID_ARG
    assert b"misaligned" in L.het_last_error()
    assert call(grouping, buf, buf, 4, buf, buf, buf, None, 10, 10, off8, buf) == HET_ERR_INVALID_ARG
    assert call(grouping, buf, buf, 4, buf, off4, buf, None, 10, 10, None, buf) == HET_ERR_INVALID_ARG
    assert b"misaligned" in L.het_last_error()
    # a grouping of another shape (this one has no positions)
    assert call(grouping, buf, buf, 4, buf, buf, buf, None, 10, 10, None, buf) == HET_ERR_INVALID_ARG
    assert b"by_dst must group" in L.het_last_error()
    # the workspace query
    assert L.het_rgat_attention_compact_workspace(None, 4, 10, 0) == -1
    assert L.het_rgat_attention_compact_workspace(grouping, 3, 10, 0) == -1
    assert L.het_rgat_attention_compact_workspace(grouping, 4, 10, 0) == 160  # the lse rows
    assert L.het_rgat_attention_compact_workspace(grouping, 4, 10, 1) == 0
    del keep_g, keep_b


@pytest.mark.parametrize("shuffle", [False, True])
def test_composition_matches_the_reference_on_the_cpu(shuffle):
    """attention_composition is plain torch: on CPU tensors it is held against the fp64 reference with the GPU tests' bound."""
    from het_amd.backend import rgat_fused_layer as FL
    from tests import _rgat_attention_ref as A
    g, layer, x = A.build_case("ladder", 5, 4, 16, shuffle=shuffle)
    ref, _ = A.reference_of(g, layer, x)
    attn = FL.attention_composition(g, x, layer.conv_weights, layer.attn_l, layer.attn_r, 0.2)
    assert attn.shape == ref.shape and attn.dtype == torch.float32 and not attn.requires_grad
    assert A.deviation(attn, ref) <= 4 * 1.11e-6
    if shuffle:
        eids = g.get_separate_coo_original()["eids"]
        assert A.deviation(attn, ref[eids]) > 1e-2


def test_reference_is_the_oracle_layer():
    """The reference's weights rebuild oracle/layers.py::rgat_layer's output."""
    from oracle import layers as OL
    from tests import _rgat_attention_ref as A
    g, layer, x = A.build_case("random", 5, 4, 16)
    a, feat = A.reference_of(g, layer, x)
    s = g.get_separate_coo_original()
    p = {n: t.detach().double() for n, t in layer.named_parameters()}
    N = g.get_num_nodes()
    out = OL.rgat_layer(x.double(), p["conv_weights"], p["attn_l"], p["attn_r"], s["rel_ptrs"], s["row_indices"], s["col_indices"], N, 0.2)
    mine = torch.zeros(N, 4, 16, dtype=torch.float64).index_add(0, s["col_indices"], a[s["eids"]].unsqueeze(-1) * feat).view(N, 64)
    torch.testing.assert_close(mine, out, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("family,recorded", [("fp32", 1.11e-6), ("large", 2.08e-5), ("bf16", 1.21e-4)])
def test_recorded_measurements(family, recorded):
    """The figures in the header of tests/test_gpu_rgat_attention.py are what the measurement gives (rounded up to 3 digits)."""
    from tests import _rgat_attention_ref as A
    got = A.measure(family)
    print(f"{family}: measured {got:.4e}, recorded {recorded:.3e}")
    assert 0.95 * recorded <= got <= recorded
