"""CPU-side checks of the bdd RGCN layer's C entries (include/het_amd.h: het_grouping_node_rows, het_rgcn_bdd_layer_*): declared,
exported and typed; argument validation answers with the documented code and the entry's name before anything is enqueued (no
device is needed to get the answer); het_rgcn_bdd_params equals the constants in the source; the route table; the training option;
the op count; and what the new unit must not contain."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("het_grouping_node_rows", "het_rgcn_bdd_layer_ok", "het_rgcn_bdd_layer_backward_workspace", "het_rgcn_bdd_layer_forward",
           "het_rgcn_bdd_layer_backward", "het_rgcn_bdd_params")
INVALID, UNSUPPORTED = 1, 3  # HET_ERR_INVALID_ARG, HET_ERR_UNSUPPORTED


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def _lib():
    from het_amd import _lib
    return _lib.lib()


def test_entries_are_declared_exported_and_typed_after_the_bf16_pair():
    from het_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _read("include", "het_amd.h"), flags=re.S)
    declared = re.findall(r"\b(?:int|int64_t|void|const char\*)\s+(het_\w+)\s*\(", src)
    at = declared.index("het_rgcn_layer_backward_bf16")
    assert tuple(declared[at + 1:at + 1 + len(ENTRIES)]) == ENTRIES
    names = list(_lib._ENTRIES)
    at = names.index("het_rgcn_layer_backward_bf16")
    assert tuple(names[at + 1:at + 1 + len(ENTRIES)]) == ENTRIES
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(L, name), name
        m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        params = [p.strip() for p in m.group(2).split(",")]
        restype, argtypes = _lib._ENTRIES[name]
        assert restype is (ctypes.c_int64 if m.group(1) == "int64_t" else ctypes.c_int), name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for p, t in zip(params, argtypes):
            want = ctypes.c_int64 if p.startswith("int64_t ") else ctypes.POINTER(ctypes.c_int64) if p.startswith("int64_t*") else ctypes.c_void_p
            assert t is want or (t is ctypes.c_void_p and "*" in p) or (p.startswith("het_stream") and t is ctypes.c_void_p), (name, p, t)
        assert getattr(_lib.lib(), name).argtypes is not None
    assert "rgcn_bdd.hip" in re.search(r"^SRCS := (.*)$", _read("het_amd", "csrc", "Makefile"), flags=re.M).group(1).split()


def _fwd(L, g=None, R=3, N=10, x=None, w=None, norm=None, bias=None, nptr=None, erow=None, erel=None, ssum=None, ret=None, K=64, D=64, B=8):
    return L.het_rgcn_bdd_layer_forward(g, R, N, x, w, norm, None, bias, nptr, erow, erel, ssum, ret, K, D, B, None)


def _bwd(L, gs=None, gd=None, R=3, Ns=10, Nd=10, ssum=None, wt=None, norm=None, go=None, nptr=None, erow=None, erel=None, gx=None,
         gw=None, gb=None, K=64, D=64, B=8, ws=None, nbytes=0):
    return L.het_rgcn_bdd_layer_backward(gs, gd, R, Ns, Nd, ssum, wt, norm, None, go, nptr, erow, erel, gx, gw, gb, K, D, B, ws, nbytes, None)


def _refused(rc, code, *words):
    msg = _lib().het_last_error()
    assert rc == code, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def test_validation_answers_before_any_launch():
    L = _lib()
    a = 1 << 20  # (an aligned address that is never read: every call below is refused first)
    # unsupported (K, D, B): the documented code, the entry's name
    for K, D, B in ((48, 64, 8), (64, 64, 32), (64, 64, 1), (256, 256, 8), (64, 60, 4), (64, 64, 3)):
        _refused(_fwd(L, K=K, D=D, B=B), UNSUPPORTED, "het_rgcn_bdd_layer_forward", "unsupported")
        _refused(_bwd(L, K=K, D=D, B=B), UNSUPPORTED, "het_rgcn_bdd_layer_backward", "unsupported")
        assert L.het_rgcn_bdd_layer_ok(3, K, D, B) == 0
        assert L.het_rgcn_bdd_layer_backward_workspace(10, 10, 3, K, D, B) == -1
    for K, D, B in ((32, 32, 8), (64, 64, 8), (64, 64, 4), (64, 64, 16), (64, 32, 2), (32, 64, 4), (128, 128, 4)):
        assert L.het_rgcn_bdd_layer_ok(535, K, D, B) == 1
    # sizes that make no sense, negative counts
    _refused(_fwd(L, R=0), INVALID, "het_rgcn_bdd_layer_forward", "bad sizes")
    _refused(_fwd(L, B=0), INVALID, "het_rgcn_bdd_layer_forward", "bad sizes")
    _refused(_fwd(L, N=-1), INVALID, "het_rgcn_bdd_layer_forward", "node count")
    _refused(_fwd(L, N=1 << 31), INVALID, "het_rgcn_bdd_layer_forward", "node count")
    _refused(_bwd(L, Ns=-1), INVALID, "het_rgcn_bdd_layer_backward", "node counts")
    _refused(_bwd(L, Nd=-5), INVALID, "het_rgcn_bdd_layer_backward", "node counts")
    assert L.het_rgcn_bdd_layer_backward_workspace(-1, 10, 3, 64, 64, 8) == -1 and b"het_rgcn_bdd_layer_backward_workspace" in L.het_last_error()
    # misaligned pointers
    _refused(_fwd(L, x=a + 4, w=a, norm=a, nptr=a, ssum=a, ret=a), INVALID, "het_rgcn_bdd_layer_forward", "16-byte")
    _refused(_fwd(L, x=a, w=a, norm=a, nptr=a, ssum=a, ret=a + 8), INVALID, "het_rgcn_bdd_layer_forward", "16-byte")
    _refused(_bwd(L, ssum=a, wt=a, go=a + 4, gw=a, ws=a, nbytes=1 << 30), INVALID, "het_rgcn_bdd_layer_backward", "16-byte")
    # a short workspace (the part of it that no graph can do without), a missing one
    need = L.het_rgcn_bdd_layer_backward_workspace(0, 0, 3, 64, 64, 8)
    assert need > 0 and need % 16 == 0
    _refused(_bwd(L, ssum=a, wt=a, go=a, gw=a, ws=a, nbytes=need - 4), INVALID, "het_rgcn_bdd_layer_backward", "workspace too small")
    _refused(_bwd(L, ssum=a, wt=a, go=a, gw=a, ws=None, nbytes=need), INVALID, "het_rgcn_bdd_layer_backward", "workspace too small")
    # nulls: no grouping
    _refused(_fwd(L, x=a, w=a, norm=a, nptr=a, ssum=a, ret=a), INVALID, "het_rgcn_bdd_layer_forward", "grouping")
    _refused(_bwd(L, ssum=a, wt=a, go=a, gw=a, ws=a, nbytes=need), INVALID, "het_rgcn_bdd_layer_backward", "grouping")
    _refused(L.het_grouping_node_rows(None, 10, a, a, a, None), INVALID, "het_grouping_node_rows", "null")
    _refused(L.het_grouping_node_rows(None, -1, a, a, a, None), INVALID, "het_grouping_node_rows", "num_keys")
    _refused(L.het_rgcn_bdd_params(None), INVALID, "het_rgcn_bdd_params", "null")


def test_workspace_formula():
    L = _lib()
    import het_amd.kernels as k
    p = k.rgcn_bdd_params()
    for (ns, nd, R, K, D, B) in ((0, 0, 1, 32, 32, 8), (1000, 5000, 535, 64, 64, 8), (7, 1023, 4, 128, 128, 4), (7, 1024, 4, 64, 32, 2)):
        floats = max(1, ns) * D + p["colsum_blocks"] * D + (nd // p["chunk_rows"] + R) * (K // B) * D
        assert L.het_rgcn_bdd_layer_backward_workspace(ns, nd, R, K, D, B) == 4 * floats


def test_params_equal_the_constants_in_the_source():
    import het_amd.kernels as k
    src = _read("het_amd", "csrc", "rgcn_bdd.hip") + _read("het_amd", "csrc", "rgcn_rows.hip.h")

    def const(name):
        return int(eval(re.search(r"constexpr int[^;]*\b" + name + r" = ([0-9* ]+)[,;]", src).group(1)))  # noqa: S307 -- digits and '*'
    p = k.rgcn_bdd_params()
    assert p == {"chunk_rows": const("kBddChunkRows"), "lds_weight_bytes": const("kBddLdsWeightBytes"), "block": const("kBddBlock"),
                 "min_side": const("kBddMinSide"), "max_side": const("kBddMaxSide"), "colsum_blocks": const("kColsumBlocks")}
    assert k.rgcn_bdd_lds_relations(64, 64, 8) == p["lds_weight_bytes"] // 2048
    assert k.rgcn_bdd_ok(535, 64, 64, 8) and not k.rgcn_bdd_ok(474, 500, 500, 100)  # (fb15k's 5 x 5 blocks: the dense route)


def test_route_table():
    from het_amd.backend import rgcn_bdd_route
    facts = dict(cuda=True, fp32=True, groupings=True, shape_ok=True, compact_flag=False, env_on=True, few_rels_dense=False)
    assert rgcn_bdd_route(**facts) == "native"
    for name in facts:  # every fact alone sends the call to the dense route
        assert rgcn_bdd_route(**{**facts, name: not facts[name]}) == "dense", name
    assert rgcn_bdd_route(cuda=True, fp32=True, groupings=True, shape_ok=True) == "native"  # (the defaults: no compact flag, switch on)


def test_route_of_reads_the_switch_and_the_plan(monkeypatch):
    import torch
    from het_amd import plan
    from het_amd.backend import rgcn_layers_and_funcs as RB
    from tests.util import random_graph
    g = random_graph(seed=5, n=40, r=4, e=300)
    seen = []
    monkeypatch.setattr(RB, "rgcn_bdd_route", lambda **facts: seen.append(facts) or "dense")
    x, w, norm = torch.randn(40, 64), torch.randn(4, 8, 8, 8), torch.rand(300, 1)
    RB.rgcn_bdd_route_of(g, x, w, norm)
    assert seen[-1] == dict(cuda=False, fp32=True, groupings=True, shape_ok=False, compact_flag=False, env_on=True, few_rels_dense=False)
    monkeypatch.setenv("HET_RGCN_BDD", "0")
    with plan.forced(False):
        RB.rgcn_bdd_route_of(g, x.bfloat16(), w, norm, None, True)
    assert seen[-1] == dict(cuda=False, fp32=False, groupings=False, shape_ok=False, compact_flag=True, env_on=False, few_rels_dense=False)


def test_training_option():
    import argparse
    from het_amd import train
    p = argparse.ArgumentParser()
    train.add_generic_RGNN_args(p, "x.json")
    assert p.parse_args([]).regularizer == "basis"
    assert p.parse_args(["--model", "rgcn", "--regularizer", "bdd", "--n_bases", "8"]).regularizer == "bdd"
    with pytest.raises(SystemExit):
        p.parse_args(["--regularizer", "diag"])
    for argv, word in ((["--model", "rgat", "--regularizer", "bdd", "--n_bases", "8"], "--model rgcn"),
                       (["--model", "rgcn", "--regularizer", "bdd"], "--n_bases"),
                       (["--model", "rgcn", "--regularizer", "bdd", "--n_bases", "7", "--n_infeat", "64", "--num_classes", "64"], "--n_bases"),
                       (["--model", "rgcn", "--regularizer", "bdd", "--n_bases", "8", "--n_infeat", "64", "--num_classes", "12"], "--n_bases")):
        with pytest.raises(SystemExit) as e:
            train.main(argv)
        assert word in str(e.value), (argv, e.value)
    m = train.HET_RGCNModel(5, 64, 32, num_layers=2, num_bases=8, regularizer="bdd")
    assert [tuple(l.weight.shape) for l in m.layers] == [(5, 8, 8, 8), (5, 8, 8, 4)] and all(l.regularizer == "bdd" for l in m.layers)
    assert all(l.regularizer == "basis" for l in train.HET_RGCNModel(5, 64, 32, num_layers=2).layers)


def test_no_new_torch_op():
    import het_amd.kernels as k
    assert len(k.REGISTERED_OPS) == 31 and not any("bdd" in n for n in k.REGISTERED_OPS)


def test_the_unit_has_no_float_atomic_copy_or_synchronise():
    src = _read("het_amd", "csrc", "rgcn_bdd.hip")
    for word in ("atomic", "hipMemcpy", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemset"):
        assert word not in src, word
    assert '#include "rgcn_rows.hip.h"' in src and "launch_segment_sum(" not in src  # the gather-sum is reached through the header
