"""The keyed dropout entries (csrc/keyed_dropout.hip) as an interface: declared in include/het_amd.h, exported, typed in
het_amd/_lib.py, validated on the host before anything touches a GPU; the Python wrappers, the layers' opt-in flag and the training
script's option.  Runs without a GPU; fails on a tree without the feature."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests import _keyed_dropout_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("het_keyed_dropout", "het_keyed_dropout_backward", "het_keyed_dropout_bf16", "het_keyed_dropout_backward_bf16",
           "het_keyed_dropout_params")
HET_OK, HET_ERR_INVALID_ARG, HET_ERR_UNSUPPORTED = 0, 1, 3


def test_entries_are_declared_exported_and_typed():
    from het_amd import _lib
    header = open(os.path.join(ROOT, "include", "het_amd.h")).read()
    P, I64, INT, D = C.c_void_p, C.c_int64, C.c_int, C.c_double
    fwd, bwd = [P, P, I64, I64, INT, D, I64, I64, P], [P, P, P, I64, I64, INT, D, I64, I64, P]
    want = {"het_keyed_dropout": fwd, "het_keyed_dropout_bf16": fwd, "het_keyed_dropout_backward": bwd,
            "het_keyed_dropout_backward_bf16": bwd, "het_keyed_dropout_params": [D, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]}
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in include/het_amd.h"
        assert hasattr(_lib.lib(), name), name + " is not exported by libhet_amd.so"
        assert _lib._ENTRIES[name] == (C.c_int, want[name]), name
    proto = re.search(r"int\s+het_keyed_dropout_backward\s*\(([^)]*)\)", header).group(1)
    for word in ("grad_out", "const float* out", "float* grad_y", "int64_t n", "int64_t base", "int activation", "double p", "seed", "draw"):
        assert word in proto, word
    assert "grad_y MAY be grad_out" in header  # the aliasing rule is part of the interface


def test_source_unit_is_built_and_sm64_has_one_copy():
    csrc = os.path.join(ROOT, "het_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bkeyed_dropout\.hip\b", mk, flags=re.M)
    src = open(os.path.join(csrc, "keyed_dropout.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "HET_keyed_dropout" in code and "HET_keyed_dropout_backward" in code
    assert "atomic" not in code and "__shared__" not in code and "asm" not in code
    defs = [f for f in os.listdir(csrc) if f.endswith((".hip", ".h")) and re.search(r"uint64_t\s+sm64\s*\(", open(os.path.join(csrc, f)).read())]
    assert defs == ["common.hip.h"], defs


def _aligned(nbytes):
    buf = C.create_string_buffer(nbytes + 16)
    return buf, C.c_void_p((C.addressof(buf) + 15) & ~15)  # (never dereferenced by the calls below)


def test_argument_validation_without_gpu():
    """n = 0 without a look at anything, n < 0, null and misaligned pointers, base, p, the activation code, relu's backward without
    out, overlapping tensors: refused with the documented code and a message naming the entry, nothing enqueued."""
    from het_amd import _lib
    L = _lib.lib()
    keep = [_aligned(256) for _ in range(3)]
    a, b, c = (k[1] for k in keep)
    off = lambda p, d: C.c_void_p(p.value + d)  # noqa: E731
    nan = float("nan")
    for name, align in (("het_keyed_dropout", 16), ("het_keyed_dropout_bf16", 8)):
        f = getattr(L, name)
        call = lambda y=a, out=b, n=8, base=0, act=1, p=0.5: f(y, out, n, base, act, p, 1, 2, None)  # noqa: E731
        assert call(y=None, out=None, n=0, base=-3, act=9, p=nan) == HET_OK  # n = 0: nothing is looked at
        assert call(n=-1) == HET_ERR_INVALID_ARG and name.encode() in L.het_last_error()
        assert call(act=2) == HET_ERR_UNSUPPORTED and name.encode() in L.het_last_error()
        assert call(act=-1) == HET_ERR_UNSUPPORTED
        for kw in (dict(y=None), dict(out=None)):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"null" in L.het_last_error(), kw
        for kw in (dict(y=off(a, align // 2)), dict(out=off(b, align // 2)), dict(y=off(a, 2))):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"misaligned" in L.het_last_error() and name.encode() in L.het_last_error(), kw
        for base in (-4, 1, 2, 6):
            assert call(base=base) == HET_ERR_INVALID_ARG and b"base" in L.het_last_error(), base
        for p in (-0.1, 1.0, 2.0, nan, float("inf")):
            assert call(p=p) == HET_ERR_INVALID_ARG and b"p=" in L.het_last_error(), p
        assert call(out=a) == HET_ERR_INVALID_ARG and b"overlaps" in L.het_last_error()  # not an in-place operation
        assert call(out=off(a, align)) == HET_ERR_INVALID_ARG and b"overlaps" in L.het_last_error()  # (partly)
    assert L.het_keyed_dropout(a, off(b, 8), 8, 0, 1, 0.5, 1, 2, None) == HET_ERR_INVALID_ARG  # fp32 rows: 16 bytes
    for name, align in (("het_keyed_dropout_backward", 16), ("het_keyed_dropout_backward_bf16", 8)):
        f = getattr(L, name)
        call = lambda go=a, out=b, gy=c, n=8, base=0, act=1, p=0.5: f(go, out, gy, n, base, act, p, 1, 2, None)  # noqa: E731
        assert call(go=None, out=None, gy=None, n=0, base=-3, act=9, p=nan) == HET_OK
        assert call(n=-1) == HET_ERR_INVALID_ARG and name.encode() in L.het_last_error()
        assert call(act=7) == HET_ERR_UNSUPPORTED and name.encode() in L.het_last_error()
        for kw in (dict(go=None), dict(gy=None)):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"null" in L.het_last_error(), kw
        assert call(out=None) == HET_ERR_INVALID_ARG and b"relu" in L.het_last_error() and name.encode() in L.het_last_error()
        for kw in (dict(go=off(a, align // 2)), dict(out=off(b, align // 2)), dict(gy=off(c, align // 2))):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"misaligned" in L.het_last_error(), kw
        assert call(base=2) == HET_ERR_INVALID_ARG and call(base=-4) == HET_ERR_INVALID_ARG
        for p in (-0.1, 1.0, nan):
            assert call(p=p) == HET_ERR_INVALID_ARG, p
        assert call(gy=b) == HET_ERR_INVALID_ARG and b"overlaps" in L.het_last_error()   # grad_y on out
        assert call(gy=off(a, align)) == HET_ERR_INVALID_ARG and b"overlaps" in L.het_last_error()  # grad_y partly on grad_out
    del keep


def test_params_entry_gives_the_reference_constants():
    import struct
    from het_amd import _lib
    import het_amd.kernels as k
    L = _lib.lib()
    for p in ref.RATES + (1.0 - 1e-9,):
        T, scale = C.c_uint32(99), C.c_float(0.0)
        assert L.het_keyed_dropout_params(p, C.byref(T), C.byref(scale)) == HET_OK
        t, s = ref.params(p)
        assert T.value == t and struct.pack("f", scale.value) == struct.pack("f", float(s)), p
        assert k.keyed_dropout_params(p) == (t, float(s))
    T, scale = C.c_uint32(0), C.c_float(0.0)
    for bad in (-1e-9, 1.0, float("nan")):
        assert L.het_keyed_dropout_params(bad, C.byref(T), C.byref(scale)) == HET_ERR_INVALID_ARG and b"het_keyed_dropout_params" in L.het_last_error()
        with pytest.raises(_lib.HetError):
            k.keyed_dropout_params(bad)
    assert L.het_keyed_dropout_params(0.5, None, C.byref(scale)) == HET_ERR_INVALID_ARG and b"null" in L.het_last_error()


def test_wrappers_reject_what_the_kernels_do_not_take():
    import torch
    import het_amd.kernels as k
    from het_amd._lib import HetError
    y = torch.zeros(8, 64)
    for t in (y, y.to(torch.bfloat16), y.double()):
        with pytest.raises(HetError):
            k.keyed_dropout(t, 0.5, 1, 0)
        with pytest.raises(HetError):
            k.keyed_dropout_backward(t, t.clone(), 0.5, 1, 0, relu=True)
    sig = inspect.signature(k.keyed_dropout)
    assert [(n, p.default) for n, p in sig.parameters.items()][1:] == [("p", inspect._empty), ("seed", inspect._empty), ("draw", inspect._empty),
                                                                      ("relu", False), ("base", 0)]
    sig = inspect.signature(k.keyed_dropout_backward)
    assert list(sig.parameters)[:7] == ["grad_out", "out", "p", "seed", "draw", "relu", "base"]


def test_layers_keep_their_default_and_their_modules():
    import torch
    import torch.nn.functional as F
    from het_amd.layers import HET_EglRelGraphConv_EdgeParallel, HET_HGTLayerHetero, HET_RGATLayer, KeyedDropout
    for cls in (HET_RGATLayer, HET_EglRelGraphConv_EdgeParallel):
        assert inspect.signature(cls.__init__).parameters["keyed_dropout"].default is False
    assert "keyed_dropout" not in inspect.signature(HET_HGTLayerHetero.__init__).parameters
    rgat = HET_RGATLayer(16, 16, 3, 2, self_loop=True, activation=F.relu)
    rgcn = HET_EglRelGraphConv_EdgeParallel(16, 16, 3, activation=F.relu, dropout=0.5)
    assert {n: type(m) for n, m in rgat.named_modules()} == {"": HET_RGATLayer, "dropout": torch.nn.Dropout} and rgat.dropout.p == 0.5
    assert {n: type(m) for n, m in rgcn.named_modules()} == {"": HET_EglRelGraphConv_EdgeParallel, "dropout": torch.nn.Dropout}
    assert list(rgat.state_dict()) == ["conv_weights", "attn_l", "attn_r", "h_bias", "loop_weight"]
    assert list(rgcn.state_dict()) == ["weight", "h_bias"]
    # the default constructor draws what it drew: the parameters' initialisation only
    torch.manual_seed(3)
    HET_RGATLayer(16, 16, 3, 2, self_loop=True, activation=F.relu)
    after_default = torch.rand(4)
    torch.manual_seed(3)
    keyed = HET_RGATLayer(16, 16, 3, 2, self_loop=True, activation=F.relu, keyed_dropout=True)
    assert not torch.equal(torch.rand(4), after_default)  # (only the opted-in layer draws a seed)
    assert isinstance(keyed.dropout, KeyedDropout) and keyed.dropout.activation == "relu" and keyed.dropout.p == 0.5
    assert list(keyed.state_dict()) == list(rgat.state_dict())
    for act, fused in ((torch.relu, "relu"), (torch.tanh, None), (None, None)):
        layer = HET_EglRelGraphConv_EdgeParallel(16, 16, 3, activation=act, dropout=0.25, keyed_dropout=True)
        assert isinstance(layer.dropout, KeyedDropout) and layer.dropout.activation == fused and layer.dropout.p == 0.25


def test_training_script_option():
    import argparse
    import json
    from het_amd import train
    p = argparse.ArgumentParser()
    train.add_generic_RGNN_args(p, "x.json")
    assert p.parse_args([]).keyed_dropout is False and p.parse_args(["--keyed_dropout"]).keyed_dropout is True
    with pytest.raises(SystemExit, match="keyed_dropout"):
        train.main(["--model", "hgt", "--keyed_dropout"])
    for cls in (train.HET_RGATModel, train.HET_RGCNModel):
        assert inspect.signature(cls.__init__).parameters["keyed_dropout"].default is False
    src = inspect.getsource(train.main)
    assert 'del res["args"]["keyed_dropout"]' in src  # (absent from the log line when off, like --use_norm)
    assert json.dumps({})  # (json: the log line's format)


def test_no_torch_hrt_op_was_added():
    import het_amd.kernels as k
    assert not any("dropout" in n for n in k.REGISTERED_OPS) and len(k.REGISTERED_OPS) == 31  # (the 31 it had)
    assert "dropout" not in open(os.path.join(ROOT, "het_amd", "csrc", "torch_export.cpp")).read()
