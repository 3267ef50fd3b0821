"""The softmax cross-entropy entries (csrc/softmax_xent.hip) as an interface: declared in include/het_amd.h, exported, typed in
het_amd/_lib.py, validated on the host before anything touches a GPU; the Python wrappers, the launch constants and the training
script's option.  Runs without a GPU; fails on a tree without the feature."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("het_softmax_xent_workspace", "het_softmax_xent", "het_softmax_xent_bf16", "het_softmax_xent_backward",
           "het_softmax_xent_backward_bf16", "het_softmax_xent_params")
HET_OK, HET_ERR_INVALID_ARG, HET_ERR_UNSUPPORTED = 0, 1, 3


def test_entries_are_declared_exported_and_typed():
    from het_amd import _lib
    header = open(os.path.join(ROOT, "include", "het_amd.h")).read()
    P, I64, INT = C.c_void_p, C.c_int64, C.c_int
    fwd, bwd = [P, P, I64, I64, I64, INT, P, P, P, P, I64, P], [P, P, P, P, P, I64, I64, I64, INT, P, P]
    want = {"het_softmax_xent_workspace": (I64, [I64, I64]), "het_softmax_xent": (INT, fwd), "het_softmax_xent_bf16": (INT, fwd),
            "het_softmax_xent_backward": (INT, bwd), "het_softmax_xent_backward_bf16": (INT, bwd),
            "het_softmax_xent_params": (INT, [C.POINTER(I64)])}
    for name in ENTRIES:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header), name + " is not declared in include/het_amd.h"
        assert hasattr(_lib.lib(), name), name + " is not exported by libhet_amd.so"
        assert _lib._ENTRIES[name] == want[name], name
    assert list(_lib._ENTRIES)[-len(ENTRIES):] == list(ENTRIES)  # (the header's order)
    proto = " ".join(re.search(r"int\s+het_softmax_xent_backward\s*\(([^)]*)\)", header).group(1).split())
    for word in ("const float* logits", "const int64_t* labels", "const float* lse", "const int64_t* stats", "const float* grad_loss", "int64_t n",
                 "int64_t c", "int64_t ignore_index", "int reduction", "float* grad_logits", "het_stream stream"):
        assert word in proto, word
    proto = " ".join(re.search(r"int\s+het_softmax_xent_bf16\s*\(([^)]*)\)", header).group(1).split())
    for word in ("const het_bf16* logits", "float* loss", "float* lse", "int64_t* stats", "void* workspace", "int64_t workspace_bytes"):
        assert word in proto, word
    assert re.search(r"#define\s+HET_XENT_MEAN\s+0\b", header) and re.search(r"#define\s+HET_XENT_SUM\s+1\b", header)


def test_source_unit_is_built_without_float_atomics_or_lds():
    csrc = os.path.join(ROOT, "het_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bsoftmax_xent\.hip\b", mk, flags=re.M)
    code = re.sub(r"//.*", "", open(os.path.join(csrc, "softmax_xent.hip")).read())
    for kernel in ("HET_softmax_xent", "HET_softmax_xent_finish", "HET_softmax_xent_backward"):
        assert kernel in code
    assert "atomic" not in code and "__shared__" not in code and "asm" not in code and "hipMemset" not in code
    assert "ldrow4" in code and "strow4" in code and "to_f32" in code  # (the row helpers of common.hip.h)
    assert not re.search(r"\bint\s+(row|j|k)\b", code)  # rows and columns are 64-bit


def test_mapping_constants_read_from_python_equal_the_source():
    import het_amd.kernels as k
    src = open(os.path.join(ROOT, "het_amd", "csrc", "softmax_xent.hip")).read()
    common = open(os.path.join(ROOT, "het_amd", "csrc", "common.hip.h")).read()
    const = lambda text, name: re.search(r"constexpr\s+int\s+%s\s*=\s*(\w+)\s*;" % name, text).group(1)  # noqa: E731
    wave = int(re.search(r"#define\s+HET_WAVE\s+(\d+)", common).group(1))
    assert const(src, "kXentMaxLanes") == "HET_WAVE"
    p = k.softmax_xent_params()
    assert p == {"lane_elems": int(const(src, "kXentLaneElems")), "max_lanes": wave, "max_blocks": int(const(src, "kXentMaxBlocks")),
                 "block": int(const(common, "kBlock"))}
    e, m = p["lane_elems"], p["max_lanes"]
    assert k.softmax_xent_thresholds() == tuple(e << i for i in range(m.bit_length() - 1)) and len(k.softmax_xent_thresholds()) >= 2
    for g, t in zip((1 << i for i in range(16)), k.softmax_xent_thresholds()):
        assert k.softmax_xent_lanes(t) == g and k.softmax_xent_lanes(t + 1) == 2 * g
    assert k.softmax_xent_lanes(1) == 1 and k.softmax_xent_lanes(10 ** 6) == m
    assert k.softmax_xent_rows_per_pass(1) == p["max_blocks"] * p["block"]
    assert k.softmax_xent_rows_per_pass(10 ** 6) == p["max_blocks"] * p["block"] // m
    L = __import__("het_amd._lib", fromlist=["lib"]).lib()
    assert L.het_softmax_xent_params(None) == HET_ERR_INVALID_ARG and b"het_softmax_xent_params" in L.het_last_error()
    # the workspace: 32 bytes per wave of the grid
    assert L.het_softmax_xent_workspace(0, 8) == 0 and L.het_softmax_xent_workspace(1, 8) == 32 * p["block"] // m
    assert L.het_softmax_xent_workspace(10 ** 9, 8) == 32 * p["max_blocks"] * p["block"] // m
    assert L.het_softmax_xent_workspace(-1, 8) == -1 and L.het_softmax_xent_workspace(4, 0) == -1


def _aligned(nbytes):
    buf = C.create_string_buffer(nbytes + 16)
    return buf, C.c_void_p((C.addressof(buf) + 15) & ~15)  # (never dereferenced by the calls below)


def test_argument_validation_without_gpu():
    """n = 0 without a launch, n < 0, c < 1, an unknown reduction, null and misaligned pointers, a workspace that is too small,
    grad_logits on the logits: refused with the documented code and a message naming the entry, nothing enqueued."""
    from het_amd import _lib
    L = _lib.lib()
    keep = [_aligned(4096) for _ in range(7)]
    z, lab, loss, lse, stats, ws, gz = (k[1] for k in keep)
    off = lambda p, d: C.c_void_p(p.value + d)  # noqa: E731
    n, c = 8, 8
    need = L.het_softmax_xent_workspace(n, c)
    assert 0 < need <= 4096
    for name, align in (("het_softmax_xent", 16), ("het_softmax_xent_bf16", 8)):
        f = getattr(L, name)
        call = lambda z=z, lab=lab, n=n, c=c, red=0, loss=loss, lse=lse, stats=stats, ws=ws, nb=need: f(z, lab, n, c, -100, red, loss, lse, stats, ws, nb, None)  # noqa: E731,E501
        err = lambda: L.het_last_error()  # noqa: E731
        assert call(z=None, lab=None, n=0, loss=None, lse=None, stats=None, ws=None, nb=0) == HET_OK  # n = 0: no launch
        assert call(n=-1) == HET_ERR_INVALID_ARG and name.encode() in err() and b"n=-1" in err()
        assert call(c=0) == HET_ERR_INVALID_ARG and name.encode() in err() and b"c=0" in err()
        assert call(n=0, c=0) == HET_ERR_INVALID_ARG
        for red in (2, -1):
            assert call(red=red) == HET_ERR_UNSUPPORTED and name.encode() in err() and b"reduction" in err()
        assert call(n=0, red=5) == HET_ERR_UNSUPPORTED
        for kw in (dict(z=None), dict(lab=None), dict(loss=None), dict(stats=None)):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"null" in err() and name.encode() in err(), kw
        for kw in (dict(z=off(z, align // 2)), dict(z=off(z, 2)), dict(lab=off(lab, 4)), dict(loss=off(loss, 2)), dict(lse=off(lse, 2)),
                   dict(stats=off(stats, 4)), dict(ws=off(ws, 4))):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"misaligned" in err() and name.encode() in err(), kw
        assert call(ws=None) == HET_ERR_INVALID_ARG and b"workspace" in err()
        assert call(nb=need - 1) == HET_ERR_INVALID_ARG and b"workspace" in err() and name.encode() in err()
        assert call(n=2 ** 61, c=2 ** 10) == HET_ERR_INVALID_ARG  # n * c beyond 64-bit byte offsets
    assert L.het_softmax_xent(off(z, 8), lab, n, c, -100, 0, loss, lse, stats, ws, need, None) == HET_ERR_INVALID_ARG  # fp32 rows: 16 bytes
    g = loss
    for name, align, size in (("het_softmax_xent_backward", 16, 4), ("het_softmax_xent_backward_bf16", 8, 2)):
        f = getattr(L, name)
        call = lambda z=z, lab=lab, lse=lse, stats=stats, g=g, n=n, c=c, red=0, gz=gz: f(z, lab, lse, stats, g, n, c, -100, red, gz, None)  # noqa: E731
        assert call(z=None, lab=None, lse=None, stats=None, g=None, n=0, gz=None) == HET_OK
        assert call(n=-1) == HET_ERR_INVALID_ARG and name.encode() in L.het_last_error()
        assert call(c=0) == HET_ERR_INVALID_ARG and name.encode() in L.het_last_error()
        assert call(red=7) == HET_ERR_UNSUPPORTED and name.encode() in L.het_last_error() and b"reduction" in L.het_last_error()
        for kw in (dict(z=None), dict(lab=None), dict(lse=None), dict(stats=None), dict(g=None), dict(gz=None)):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"null" in L.het_last_error(), kw
        for kw in (dict(z=off(z, align // 2)), dict(gz=off(gz, align // 2)), dict(lab=off(lab, 4)), dict(lse=off(lse, 2)), dict(g=off(g, 2)),
                   dict(stats=off(stats, 4))):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"misaligned" in L.het_last_error() and name.encode() in L.het_last_error(), kw
        assert call(gz=z) == HET_ERR_INVALID_ARG and b"overlaps" in L.het_last_error() and name.encode() in L.het_last_error()
        assert call(gz=off(z, n * c * size - 16)) == HET_ERR_INVALID_ARG and b"overlaps" in L.het_last_error()  # (its last 16 bytes)
        assert call(z=off(gz, 16)) == HET_ERR_INVALID_ARG and b"overlaps" in L.het_last_error()
    del keep


def test_wrappers_reject_what_the_kernels_do_not_take():
    import torch
    import het_amd.kernels as k
    from het_amd._lib import HetError
    z, lab = torch.zeros(8, 4), torch.zeros(8, dtype=torch.int64)
    for t in (z, z.to(torch.bfloat16), z.double(), z.half()):
        assert not k.softmax_xent_ok(t, lab)
        with pytest.raises(HetError, match="softmax_xent"):
            k.softmax_xent(t, lab)
        with pytest.raises(HetError, match="softmax_xent_backward"):
            k.softmax_xent_backward(t, lab, torch.zeros(8), torch.zeros(3, dtype=torch.int64), torch.ones(()))
    sig = inspect.signature(k.softmax_xent)
    assert [(n, p.default) for n, p in sig.parameters.items()][2:] == [("ignore_index", -100), ("reduction", "mean"), ("want_lse", True)]
    sig = inspect.signature(k.softmax_xent_backward)
    assert list(sig.parameters) == ["logits", "labels", "lse", "stats", "grad_loss", "ignore_index", "reduction"]
    assert k.XENT_REDUCTIONS == {"mean": 0, "sum": 1}


def test_module_interface():
    import torch
    from het_amd.layers import SoftmaxCrossEntropy, SoftmaxCrossEntropyFunction
    sig = inspect.signature(SoftmaxCrossEntropy.__init__)
    assert [(n, p.default) for n, p in sig.parameters.items()][1:] == [("ignore_index", -100), ("reduction", "mean"), ("check_labels", False)]
    assert issubclass(SoftmaxCrossEntropyFunction, torch.autograd.Function)
    mod = SoftmaxCrossEntropy()
    assert mod.last_stats is None and not list(mod.parameters()) and not list(mod.buffers())
    for bad in ((torch.zeros(4), torch.zeros(4, dtype=torch.int64)), (torch.zeros(4, 3), torch.zeros(5, dtype=torch.int64)),
                (torch.zeros(4, 0), torch.zeros(4, dtype=torch.int64))):
        with pytest.raises(ValueError):
            mod(*bad)


def test_training_script_option():
    import argparse
    from het_amd import train
    p = argparse.ArgumentParser()
    train.add_generic_RGNN_args(p, "x.json")
    assert p.parse_args([]).fused_loss is False and p.parse_args(["--fused_loss"]).fused_loss is True
    src = inspect.getsource(train.main)
    assert 'del res["args"]["fused_loss"]' in src and 'res["loss"] = "fused"' in src  # (absent from the log line when off)
    body = inspect.getsource(train.HET_RGNN_train)
    assert body.count("-logits.log_softmax(dim=-1).gather(1, cur_labels.view(-1, 1)).mean()") == 2  # the default expression, both passes
    assert body.count("loss_fn(logits, cur_labels)") == 2 and 'getattr(args, "fused_loss", False)' in body


def test_no_torch_hrt_op_was_added():
    import het_amd.kernels as k
    assert not any("xent" in n or "softmax_xent" in n for n in k.REGISTERED_OPS) and len(k.REGISTERED_OPS) == 31  # (the 31 it had)
    assert "xent" not in open(os.path.join(ROOT, "het_amd", "csrc", "torch_export.cpp")).read()
