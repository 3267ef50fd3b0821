"""The keyed-sampler entries (csrc/block_sample.hip) as an interface: declared in include/het_amd.h, exported, typed in het_amd/_lib.py,
and validated on the host before anything touches a GPU.  Runs without a GPU; fails on a tree without the feature."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HET_OK, HET_ERR_INVALID_ARG = 0, 1
P, I64 = C.c_void_p, C.c_int64
WANT = {"het_sample_workgroup_degree": [], "het_sample_chunk": [],
        "het_sample_count": [P, P, I64, I64, I64, P, P, P],
        "het_sample_select": [P, P, I64, I64, I64, I64, I64, P, I64, P, P, P],
        "het_block_renumber": [P, I64, P, I64, P, I64, P, I64, P, P, P, P],
        "het_block_relation_major": [P, P, I64, P, P, P, I64, I64, P, P, P, P, P, P]}


def test_entries_are_declared_exported_and_typed():
    from het_amd import _lib
    header = open(os.path.join(ROOT, "include", "het_amd.h")).read()
    for name, args in WANT.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in include/het_amd.h"
        assert hasattr(_lib.lib(), name), name + " is not exported by libhet_amd.so"
        assert _lib._ENTRIES[name] == (C.c_int, args), name
    proto = re.search(r"int\s+het_sample_select\s*\(([^)]*)\)", header).group(1)
    for word in ("int64_t fanout", "int64_t seed", "int64_t draw", "offsets", "int64_t total", "out_pos", "out_owner"):
        assert word in proto, word
    proto = re.search(r"int\s+het_block_renumber\s*\(([^)]*)\)", header).group(1)
    for word in ("int64_t* map", "out_nodes", "out_local_src", "int64_t* out_num_extra"):
        assert word in proto, word


def test_source_unit_is_built_and_thresholds_are_exported():
    import het_amd.kernels as k
    mk = open(os.path.join(ROOT, "het_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bblock_sample\.hip\b", mk, flags=re.M)
    t = k.sample_thresholds()
    assert set(t) == {"workgroup_degree", "chunk"}
    assert t["workgroup_degree"] >= 64 and t["workgroup_degree"] % 64 == 0 and t["chunk"] % 64 == 0 and 64 <= t["chunk"] <= 1024
    src = open(os.path.join(ROOT, "het_amd", "csrc", "block_sample.hip")).read()
    for name, v in (("kSampleWorkgroupDegree", t["workgroup_degree"]), ("kSampleChunk", t["chunk"])):
        assert re.search(r"constexpr int %s = %d;" % (name, v), src), name


def test_python_interface():
    import het_amd.kernels as k
    from het_amd.graph import HetGraph
    from het_amd.sampling import NeighborSampler
    for name in ("sample_thresholds", "sample_count", "sample_select", "block_renumber", "block_relation_major"):
        assert callable(getattr(k, name, None)), name
    sig = inspect.signature(NeighborSampler.__init__)
    assert list(sig.parameters) == ["self", "g", "fanouts", "seed", "full_layouts", "by_type", "method"]
    assert sig.parameters["method"].default == "sort"
    assert inspect.signature(NeighborSampler.sample_block).parameters["draw"].default is None
    sig = inspect.signature(HetGraph.from_block_separate_coo)
    assert list(sig.parameters) == ["num_nodes", "num_rels", "node_type_offsets", "rel_ptrs", "row", "col", "rel", "full"]
    assert sig.parameters["full"].default is True
    assert not any("sample" in n or "block" in n for n in k.REGISTERED_OPS)  # (no torch.ops.torch_hrt op was added)


def test_argument_validation_without_gpu():
    """Negative counts and num_rels < 1 first, then B == 0 / total == 0 without a launch (host counts set to 0), then null
    pointers: refused with HET_ERR_INVALID_ARG and a message naming the entry, nothing enqueued."""
    from het_amd import _lib
    L = _lib.lib()
    keep = C.create_string_buffer(256)
    buf = C.c_void_p(C.addressof(keep))  # (never dereferenced by the calls below)
    out = C.c_int64(77)
    ref = C.byref(out)

    def refused(rc, name, word=None):
        assert rc == HET_ERR_INVALID_ARG, (name, rc)
        msg = L.het_last_error()
        assert name.encode() in msg and (word is None or word in msg), msg

    # het_sample_count(row_ptrs, dst, num_dst, num_nodes, fanout, out_offsets, out_total, stream)
    n = "het_sample_count"
    refused(L.het_sample_count(buf, buf, -1, 10, 5, buf, ref, None), n)
    refused(L.het_sample_count(buf, buf, 4, -1, 5, buf, ref, None), n)
    assert L.het_sample_count(None, None, 0, 10, 5, None, ref, None) == HET_OK and out.value == 0
    for args in ((None, buf, buf, ref), (buf, None, buf, ref), (buf, buf, None, ref), (buf, buf, buf, None)):
        refused(L.het_sample_count(args[0], args[1], 4, 10, 5, args[2], args[3], None), n, b"null")
    # het_sample_select(row_ptrs, dst, num_dst, num_nodes, fanout, seed, draw, offsets, total, out_pos, out_owner, stream)
    n = "het_sample_select"
    refused(L.het_sample_select(buf, buf, -1, 10, 5, 0, 0, buf, 8, buf, buf, None), n)
    refused(L.het_sample_select(buf, buf, 4, -2, 5, 0, 0, buf, 8, buf, buf, None), n)
    refused(L.het_sample_select(buf, buf, 4, 10, 5, 0, 0, buf, -8, buf, buf, None), n)
    assert L.het_sample_select(None, None, 0, 10, 5, 0, 0, None, 8, None, None, None) == HET_OK
    assert L.het_sample_select(None, None, 4, 10, 5, 0, 0, None, 0, None, None, None) == HET_OK
    for i in range(5):
        a = [buf] * 5
        a[i] = None
        refused(L.het_sample_select(a[0], a[1], 4, 10, 5, -3, 1 << 40, a[2], 8, a[3], a[4], None), n, b"null")
    # het_block_renumber(src, num_edges, pos, total, dst, num_dst, map, num_nodes, out_nodes, out_local_src, out_num_extra, stream)
    n = "het_block_renumber"
    for bad in (dict(E=-1), dict(total=-1), dict(B=-1), dict(N=-1)):
        v = {**dict(E=20, total=8, B=4, N=10), **bad}
        refused(L.het_block_renumber(buf, v["E"], buf, v["total"], buf, v["B"], buf, v["N"], buf, buf, ref, None), n)
    out.value = 77
    assert L.het_block_renumber(None, 20, None, 8, None, 0, None, 10, None, None, ref, None) == HET_OK and out.value == 0
    out.value = 77
    assert L.het_block_renumber(None, 20, None, 0, None, 4, None, 10, None, None, ref, None) == HET_OK and out.value == 0
    for i in range(7):
        a = [buf, buf, buf, buf, buf, buf, ref]
        a[i] = None
        refused(L.het_block_renumber(a[0], 20, a[1], 8, a[2], 4, a[3], 10, a[4], a[5], a[6], None), n, b"null")
    # het_block_relation_major(rel, eids, num_edges, pos, owner, local_src, total, num_rels, out_rel_ptrs, out_row, out_col, out_rel,
    #                          out_eids, stream)
    n = "het_block_relation_major"
    refused(L.het_block_relation_major(buf, buf, -1, buf, buf, buf, 8, 3, buf, buf, buf, buf, buf, None), n)
    refused(L.het_block_relation_major(buf, buf, 20, buf, buf, buf, -8, 3, buf, buf, buf, buf, buf, None), n)
    for R in (0, -1):
        refused(L.het_block_relation_major(buf, buf, 20, buf, buf, buf, 8, R, buf, buf, buf, buf, buf, None), n, b"num_rels")
        refused(L.het_block_relation_major(buf, buf, 20, buf, buf, buf, 0, R, buf, buf, buf, buf, buf, None), n, b"num_rels")
    assert L.het_block_relation_major(None, None, 20, None, None, None, 0, 3, None, None, None, None, None, None) == HET_OK
    for i in range(10):
        a = [buf] * 10
        a[i] = None
        refused(L.het_block_relation_major(a[0], a[1], 20, a[2], a[3], a[4], 8, 3, a[5], a[6], a[7], a[8], a[9], None), n, b"null")
    del keep


def test_wrappers_reject_cpu_tensors():
    import torch
    import het_amd.kernels as k
    from het_amd._lib import HetError
    ptr, ids = torch.zeros(9, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(HetError):
        k.sample_count(ptr, ids, 4)
    with pytest.raises(HetError):
        k.sample_select(ptr, ids, 4, 0, 0, torch.zeros(4, dtype=torch.int64), 0)
    with pytest.raises(HetError):
        k.block_renumber(ids, ids, ids, torch.full((8,), -1))
    with pytest.raises(HetError):
        k.block_relation_major(ids, ids, ids, ids, ids, 2)


def test_driver_flag_is_declared():
    """--keyed_sampler exists and is off by default (a run without it logs what it logged before)."""
    import argparse
    from het_amd import train
    p = argparse.ArgumentParser()
    train.add_generic_RGNN_args(p, "x.json")
    assert p.parse_args([]).keyed_sampler is False and p.parse_args(["--keyed_sampler"]).keyed_sampler is True
