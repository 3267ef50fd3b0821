"""The forward-only RGAT aggregation (het_rgat_aggregate_compact_forward) as an interface: declared, exported, marshalled, and
validated on the host before anything touches a GPU.  Runs without one."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, WORKSPACE = "het_rgat_aggregate_compact_forward", "het_rgat_aggregate_compact_forward_workspace"
HET_ERR_INVALID_ARG, HET_ERR_UNSUPPORTED = 1, 3


def test_forward_only_entries_are_declared_and_exported():
    from het_amd import _lib
    header = open(os.path.join(ROOT, "include", "het_amd.h")).read()
    for name in (ENTRY, WORKSPACE):
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in include/het_amd.h"
        assert hasattr(_lib.lib(), name), name + " is not exported by libhet_amd.so"
    assert ENTRY in _lib._SIGNATURES


def test_kernels_module_marshals_the_entry():
    import het_amd.kernels as k
    assert callable(getattr(k, "rgat_aggregate_compact_forward", None))


def _aligned(nbytes):
    """A zeroed host buffer and a 16-byte aligned address inside it (never dereferenced by the calls below)."""
    buf = C.create_string_buffer(nbytes + 16)
    return buf, C.c_void_p((C.addressof(buf) + 15) & ~15)


def _forward(L, by_dst, by_dst_rel, H, D, h_inout, num_rels=3):
    return L.het_rgat_aggregate_compact_forward(by_dst, by_dst_rel, num_rels, None, None, None, H, D, 0.2, h_inout, 10, None, None,
                                                None, 0, None)


def test_argument_validation_without_gpu():
    """Null groupings, a null or misaligned h_inout and a shape outside the run-sum form are refused with the documented code and
    a message that names the entry -- checked in that order, before a grouping is read or anything is enqueued."""
    from het_amd import _lib
    L = _lib.lib()
    keep_g, fake_grouping = _aligned(4096)
    keep_h, h = _aligned(64)
    # null groupings
    assert _forward(L, None, None, 4, 16, h) == HET_ERR_INVALID_ARG
    assert ENTRY.encode() in L.het_last_error() and b"null" in L.het_last_error()
    assert _forward(L, fake_grouping, None, 4, 16, h) == HET_ERR_INVALID_ARG
    # null h_inout: it is the only output
    assert _forward(L, fake_grouping, fake_grouping, 4, 16, None) == HET_ERR_INVALID_ARG
    assert ENTRY.encode() in L.het_last_error() and b"h_inout" in L.het_last_error()
    # misaligned h_inout
    assert _forward(L, fake_grouping, fake_grouping, 4, 16, C.c_void_p(h.value + 4)) == HET_ERR_INVALID_ARG
    assert b"h_inout" in L.het_last_error()
    # shapes outside compact_shape_ok / coop_shape_ok: heads of 8 floats, a row of 48
    for H, D in ((8, 8), (3, 16)):
        assert _forward(L, fake_grouping, fake_grouping, H, D, h) == HET_ERR_UNSUPPORTED, (H, D)
        msg = L.het_last_error()
        assert ENTRY.encode() in msg and b"unsupported shape" in msg
    # the workspace query names its failure the same way
    assert L.het_rgat_aggregate_compact_forward_workspace(None, None, 3, 4, 16, None) == -1
    del keep_g, keep_h


def test_train_help_lists_inference():
    r = subprocess.run([sys.executable, "-m", "het_amd.train", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--inference" in r.stdout
