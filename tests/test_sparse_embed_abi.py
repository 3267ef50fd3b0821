"""The row-sparse embedding entries (csrc/rows_embed.hip) as an interface: declared in include/het_amd.h, exported, typed in
het_amd/_lib.py, and validated on the host before anything touches a GPU.  Runs without a GPU; fails on a tree without the feature."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("het_rows_embed_ok", "het_rows_embed_gather", "het_rows_embed_gather_bf16", "het_rows_adam")
HET_OK, HET_ERR_INVALID_ARG, HET_ERR_UNSUPPORTED = 0, 1, 3


def test_entries_are_declared_exported_and_typed():
    from het_amd import _lib
    header = open(os.path.join(ROOT, "include", "het_amd.h")).read()
    P, I64, D = C.c_void_p, C.c_int64, C.c_double
    want = {"het_rows_embed_ok": [I64], "het_rows_embed_gather": [P, P, I64, I64, I64, P, P],
            "het_rows_embed_gather_bf16": [P, P, I64, I64, I64, P, P],
            "het_rows_adam": [P, P, P, P, P, P, I64, I64, I64, D, D, D, D, D, D, P]}
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in include/het_amd.h"
        assert hasattr(_lib.lib(), name), name + " is not exported by libhet_amd.so"
        assert _lib._ENTRIES[name] == (C.c_int, want[name]), name
    # the prototype of the Adam entry names its scalars as the rule does
    proto = re.search(r"int\s+het_rows_adam\s*\(([^)]*)\)", header).group(1)
    for word in ("rows_sorted", "perm", "double lr", "double beta1", "double beta2", "double eps", "double bias_correction1",
                 "double bias_correction2"):
        assert word in proto, word
    # the halo gather of the multi-GPU path keeps its own entry and signature
    assert _lib._ENTRIES["het_rows_gather"] == (C.c_int, [P, P, I64, I64, P, P])


def test_source_unit_is_built():
    mk = open(os.path.join(ROOT, "het_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\brows_embed\.hip\b", mk, flags=re.M)
    src = open(os.path.join(ROOT, "het_amd", "csrc", "rows_embed.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "atomic" not in code and "rsqrt" not in code and "__frcp" not in code and "rcp" not in code


def test_python_interface():
    import het_amd.kernels as k
    from het_amd.layers import HET_RelGraphEmbed
    from het_amd.optim import RowSparseAdam
    for name in ("rows_embed_ok", "rows_embed_gather", "rows_adam_"):
        assert callable(getattr(k, name, None)), name
    sig = inspect.signature(HET_RelGraphEmbed.forward)
    assert list(sig.parameters) == ["self", "nodes", "dtype"] and sig.parameters["nodes"].default is None and sig.parameters["dtype"].default is None
    assert inspect.signature(HET_RelGraphEmbed.__init__).parameters["sparse"].default is False
    sig = inspect.signature(RowSparseAdam.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[2:]] == [("lr", 1e-3), ("betas", (0.9, 0.999)), ("eps", 1e-8)]
    assert not any("embed" in n or "adam" in n for n in k.REGISTERED_OPS)  # (no torch.ops.torch_hrt op was added)


def test_width_predicate():
    import het_amd.kernels as k
    ok = [K for K in range(0, 1100) if k.rows_embed_ok(K)]
    assert ok == list(range(4, 1025, 4))
    assert not k.rows_embed_ok(-4)


def _aligned(nbytes):
    buf = C.create_string_buffer(nbytes + 16)
    return buf, C.c_void_p((C.addressof(buf) + 15) & ~15)  # (never dereferenced by the calls below)


def test_argument_validation_without_gpu():
    """Unsupported widths before anything else, B = 0 without a launch, null and misaligned pointers, bad scalars: refused with the
    documented code and a message naming the entry, nothing enqueued."""
    from het_amd import _lib
    L = _lib.lib()
    keep, buf = _aligned(256)
    off4, off8 = C.c_void_p(buf.value + 4), C.c_void_p(buf.value + 8)
    adam = lambda p=buf, m=buf, v=buf, rows=buf, perm=None, grad=buf, B=10, N=10, K=64, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, bc1=0.1, bc2=0.001: \
        L.het_rows_adam(p, m, v, rows, perm, grad, B, N, K, lr, b1, b2, eps, bc1, bc2, None)  # noqa: E731
    for name in ("het_rows_embed_gather", "het_rows_embed_gather_bf16"):
        f = getattr(L, name)
        for K in (0, 2, 10, 66, 1028):
            assert f(buf, buf, 10, 10, K, buf, None) in ((HET_ERR_UNSUPPORTED,) if K > 0 else (HET_ERR_INVALID_ARG, HET_ERR_UNSUPPORTED)), (name, K)
        assert f(buf, buf, 10, 10, 10, buf, None) == HET_ERR_UNSUPPORTED and name.encode() in L.het_last_error()
        assert f(None, None, 0, 10, 64, None, None) == HET_OK  # B = 0: nothing is looked at
        assert f(buf, buf, 0, 10, 10, buf, None) == HET_ERR_UNSUPPORTED  # (the width is refused even then)
        for args in ((None, buf, buf), (buf, None, buf), (buf, buf, None)):
            assert f(args[0], args[1], 10, 10, 64, args[2], None) == HET_ERR_INVALID_ARG and b"null" in L.het_last_error()
        assert f(off8, buf, 10, 10, 64, buf, None) == HET_ERR_INVALID_ARG and b"misaligned" in L.het_last_error()
        assert f(buf, off4, 10, 10, 64, buf, None) == HET_ERR_INVALID_ARG
        assert f(buf, buf, 10, 10, 64, off4, None) == HET_ERR_INVALID_ARG and name.encode() in L.het_last_error()
        assert f(buf, buf, -1, 10, 64, buf, None) == HET_ERR_INVALID_ARG
    assert L.het_rows_embed_gather(buf, buf, 10, 10, 64, off8, None) == HET_ERR_INVALID_ARG  # fp32 rows: 16 bytes
    assert adam(K=10) == HET_ERR_UNSUPPORTED and b"het_rows_adam" in L.het_last_error()
    assert adam(K=1028) == HET_ERR_UNSUPPORTED
    assert adam(p=None, m=None, v=None, rows=None, grad=None, B=0) == HET_OK
    for k in ("p", "m", "v", "rows", "grad"):
        assert adam(**{k: None}) == HET_ERR_INVALID_ARG and b"null" in L.het_last_error(), k
    for k in ("p", "m", "v", "grad"):
        assert adam(**{k: off8}) == HET_ERR_INVALID_ARG and b"misaligned" in L.het_last_error(), k
    assert adam(rows=off4) == HET_ERR_INVALID_ARG and adam(perm=off4) == HET_ERR_INVALID_ARG
    for bad in (dict(lr=-1.0), dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0), dict(bc1=0.0), dict(bc2=0.0), dict(B=-1)):
        assert adam(**bad) == HET_ERR_INVALID_ARG, bad
    del keep


def test_wrappers_reject_cpu_tensors():
    import pytest
    import torch
    import het_amd.kernels as k
    from het_amd._lib import HetError
    t, ids = torch.zeros(8, 64), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(HetError):
        k.rows_embed_gather(t, ids)
    with pytest.raises(HetError):
        k.rows_adam_(t, t.clone(), t.clone(), ids, None, torch.zeros(3, 64), 1e-3, 0.9, 0.999, 1e-8, 1)
