"""The filtered-ranking entries (csrc/triple_rank.hip) as an interface: declared in include/het_amd.h, exported, typed in
het_amd/_lib.py, validated on the host before anything touches a GPU; the launch constants, the workspace formula, the Python
wrappers, the module het_amd/linkpred.py and the training script's option.  Runs without a GPU; fails on a tree without the feature."""
import ctypes as C
import hashlib
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("het_triple_rank_workspace", "het_triple_rank", "het_triple_rank_bf16", "het_triple_rank_params")
HET_OK, HET_ERR_INVALID_ARG, HET_ERR_UNSUPPORTED = 0, 1, 3
# sha256 of inspect.getsource(het_amd.train.HET_RGNN_train): the classification step is the function it was before link prediction
RGNN_TRAIN_SHA256 = "92304c54ee8ef7082f98e260b3b8b514e5e1bd4459bae6fb5158b1ceaf4e1bce"


def _lib():
    from het_amd import _lib
    return _lib


def test_entries_are_declared_exported_and_typed():
    _l = _lib()
    header = open(os.path.join(ROOT, "include", "het_amd.h")).read()
    P, I64 = C.c_void_p, C.c_int64
    rank = [P, P, P, P, P, I64, P, P, I64, P, I64, I64, I64, I64, P, P, P, P, P, I64, P]
    want = {"het_triple_rank_workspace": (I64, [I64, I64, I64, I64]), "het_triple_rank": (C.c_int, rank),
            "het_triple_rank_bf16": (C.c_int, rank), "het_triple_rank_params": (C.c_int, [C.POINTER(I64)])}
    for name in ENTRIES:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header), name + " is not declared in include/het_amd.h"
        assert hasattr(_l.lib(), name), name + " is not exported by libhet_amd.so"
        assert _l._ENTRIES[name] == want[name], name
    # the header's order: the four side by side, before keyed dropout (the sections behind it are pinned to their neighbours)
    names = list(_l._ENTRIES)
    at = names.index(ENTRIES[0])
    assert tuple(names[at:at + len(ENTRIES)]) == ENTRIES and names[at + len(ENTRIES)] == "het_keyed_dropout"
    pos = [header.index(" " + n + "(") for n in ENTRIES + ("het_keyed_dropout",)]
    assert pos == sorted(pos)
    proto = " ".join(re.search(r"int\s+het_triple_rank_bf16\s*\(([^)]*)\)", header).group(1).split())
    for word in ("const het_bf16* h", "const float* w", "const int64_t* anchor", "const int64_t* rel", "const int64_t* truth",
                 "int64_t num_queries", "const int64_t* pair_query", "const int64_t* pair_cand", "int64_t num_pairs",
                 "const int64_t* node_type_offsets", "int64_t num_types", "int64_t num_nodes", "int64_t num_rels", "int64_t dim",
                 "int32_t* greater", "int32_t* equal", "int32_t* cands", "int64_t* bad", "void* workspace", "int64_t workspace_bytes",
                 "het_stream stream"):
        assert word in proto, word
    # the rule and how the counters start at zero are stated in the header
    text = " ".join(header.split())
    for word in ("fmaf(q_j[d], h[c, d], acc)", "greater[j]", "equal[j]", "cands[j]", "The counters start at zero by the library's own doing",
                 "hipMemsetAsync", "No float atomic"):
        assert word in text, word


def test_source_unit_is_built_with_integer_counters_only():
    csrc = os.path.join(ROOT, "het_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\btriple_rank\.hip\b", mk, flags=re.M) and len(re.findall(r"^SRCS\s*:=", mk, flags=re.M)) == 1
    code = open(os.path.join(csrc, "triple_rank.hip")).read()
    for kernel in ("HET_rank_prelude", "HET_rank_pair_keys", "HET_rank_tile_ptr", "HET_triple_rank"):
        assert kernel in code
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in code and "fmaf(" in code and "ldrow4" in code and "__shared__" in code
    assert "hipcub::DeviceRadixSort::SortPairs" in code  # (the stable sort of the pairs by tile cell)
    assert "hipStreamSynchronize" not in code and "hipMemcpy" not in code and "hipDeviceSynchronize" not in code  # no read-back
    assert "asm" not in code and "atomic_add4" not in code
    # every atomic works on an integer: the counters in LDS and in memory, the mask bits, the runs of a query tile, the bad count
    body = re.sub(r"//[^\n]*", "", code)
    assert set(re.findall(r"\batomic\w+", body)) == {"atomicAdd", "atomicOr", "atomicMin", "atomicMax"}
    assert not re.search(r"atomicAdd\(\s*\(?\s*float", body) and "float* at" not in body
    assert not re.search(r"\bint\s+(j|c|c0|j0|item)\b", body)  # queries, candidates and items are 64-bit


def test_launch_constants_read_from_python_equal_the_source():
    import het_amd.kernels as k
    src = open(os.path.join(ROOT, "het_amd", "csrc", "triple_rank.hip")).read()
    common = open(os.path.join(ROOT, "het_amd", "csrc", "common.hip.h")).read()
    const = lambda text, name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))  # noqa: E731
    p = k.triple_rank_params()
    assert p == {"query_tile": const(src, "kRankQueryTile"), "cand_tile": const(src, "kRankCandTile"), "min_width": const(src, "kRankMinWidth"),
                 "max_width": const(src, "kRankMaxWidth"), "block": const(common, "kBlock"), "max_blocks": const(src, "kRankMaxBlocks"),
                 "chunk_tiles": const(src, "kRankChunkTiles"), "max_span": const(src, "kRankMaxSpan")}
    assert p["min_width"] == 4 and p["max_width"] >= 256 and p["query_tile"] % 16 == 0 and p["cand_tile"] % 32 == 0
    L = _lib().lib()
    assert L.het_triple_rank_params(None) == HET_ERR_INVALID_ARG and b"het_triple_rank_params" in L.het_last_error()
    # the workspace without pairs (no sort, so no device is asked): q [Q, D] fp32 and p, lo, hi, t [Q] of 4 bytes, each rounded to 256
    up = lambda b: (b + 255) & ~255  # noqa: E731
    for Q, N, D in ((1, 10, 4), (130, 1031, 64), (2048, 1939743, 64), (70, 515, 256)):
        assert L.het_triple_rank_workspace(Q, 0, N, D) == up(4 * Q * D) + 4 * up(4 * Q)
    assert L.het_triple_rank_workspace(0, 0, 10, 64) == 0 and L.het_triple_rank_workspace(0, 5, 10, 64) == 0
    for bad in ((-1, 0, 10, 64), (5, -1, 10, 64), (5, 0, -1, 64), (5, 0, 10, 0), (5, 0, 10, 10), (5, 0, 10, p["max_width"] + 4),
                (2 ** 30, 0, 10, 64), (5, 2 ** 30, 10, 64), (5, 0, 2 ** 31 - 1, 64)):
        assert L.het_triple_rank_workspace(*bad) == -1 and b"het_triple_rank_workspace" in L.het_last_error(), bad


def _aligned(nbytes):
    buf = C.create_string_buffer(nbytes + 16)
    return buf, C.c_void_p((C.addressof(buf) + 15) & ~15)  # (never dereferenced by the calls below)


def test_argument_validation_without_gpu():
    """No queries without a launch, negative counts, dim < 1, widths the kernels do not take, null and misaligned pointers, a
    workspace that is too small: refused with the documented code and a message naming the entry, nothing enqueued."""
    L = _lib().lib()
    keep = [_aligned(1 << 16) for _ in range(13)]
    h, w, a, r, t, pq, pc, offs, gr, eq, cn, bad, ws = (k[1] for k in keep)
    off = lambda p, d: C.c_void_p(p.value + d)  # noqa: E731
    err = lambda: L.het_last_error()  # noqa: E731
    Q, NP, N, R, D = 8, 4, 8, 3, 8
    need = L.het_triple_rank_workspace(Q, 0, N, D)
    assert 0 < need <= 1 << 16
    for entry, align in (("het_triple_rank", 16), ("het_triple_rank_bf16", 8)):
        f, name = getattr(L, entry), entry.encode()
        call = lambda h=h, w=w, a=a, r=r, t=t, q=Q, pq=pq, pc=pc, np_=NP, offs=None, nt=0, n=N, nr=R, d=D, gr=gr, eq=eq, cn=cn, bad=bad, ws=ws, nb=1 << 16: f(  # noqa: E731,E501
            h, w, a, r, t, q, pq, pc, np_, offs, nt, n, nr, d, gr, eq, cn, bad, ws, nb, None)
        assert call(h=None, w=None, a=None, r=None, t=None, q=0, pq=None, pc=None, np_=0, gr=None, eq=None, cn=None, bad=None, ws=None, nb=0) == HET_OK
        for kw in (dict(q=-1), dict(np_=-1), dict(n=-1), dict(nr=-1), dict(d=0), dict(d=-4), dict(q=2 ** 30), dict(np_=2 ** 30), dict(n=2 ** 31 - 1),
                   dict(nr=2 ** 31 - 1), dict(nt=-1), dict(offs=offs, nt=0)):
            assert call(**kw) == HET_ERR_INVALID_ARG and name in err(), kw
        assert call(q=0, d=0) == HET_ERR_INVALID_ARG
        for d in (1, 2, 10, 260, 1024):
            assert call(d=d) == HET_ERR_UNSUPPORTED and name in err() and b"dim=%d" % d in err()
        for kw in (dict(h=None), dict(w=None), dict(a=None), dict(r=None), dict(t=None), dict(pq=None), dict(pc=None), dict(gr=None), dict(eq=None),
                   dict(cn=None), dict(bad=None)):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"null" in err() and name in err(), kw
        for kw in (dict(h=off(h, align // 2)), dict(h=off(h, 2)), dict(w=off(w, 8)), dict(a=off(a, 4)), dict(t=off(t, 4)), dict(pq=off(pq, 4)),
                   dict(pc=off(pc, 4)), dict(offs=off(offs, 4), nt=2), dict(gr=off(gr, 2)), dict(eq=off(eq, 1)), dict(cn=off(cn, 2)),
                   dict(bad=off(bad, 4)), dict(ws=off(ws, 8))):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"misaligned" in err() and name in err(), kw
        for kw in (dict(ws=None, np_=0), dict(nb=0, np_=0), dict(nb=need - 1, np_=0), dict(nb=need)):  # (the last: pairs need more than `need`)
            assert call(**kw) == HET_ERR_INVALID_ARG and b"workspace" in err() and name in err(), kw
    assert L.het_triple_rank(off(h, 8), w, a, r, t, Q, pq, pc, NP, None, 0, N, R, D, gr, eq, cn, bad, ws, 1 << 16, None) == HET_ERR_INVALID_ARG
    del keep


def test_wrappers_reject_what_the_kernels_do_not_take():
    import torch
    import het_amd.kernels as k
    from het_amd._lib import HetError
    ids = tuple(torch.zeros(8, dtype=torch.int64) for _ in range(3))
    w = torch.zeros(3, 8)
    for h in (torch.zeros(8, 8), torch.zeros(8, 8, dtype=torch.bfloat16), torch.zeros(8, 8, dtype=torch.float64), torch.zeros(8, 8).half()):
        assert not k.triple_rank_ok(h, w)
        with pytest.raises(HetError, match="triple_rank"):
            k.triple_rank(h, w, *ids)
    assert list(inspect.signature(k.triple_rank).parameters) == ["h", "w", "anchor", "rel", "truth", "pair_query", "pair_cand", "node_type_offsets"]
    assert list(inspect.signature(k.triple_rank_ok).parameters) == ["h", "w"] and list(inspect.signature(k.triple_rank_params).parameters) == []
    src = inspect.getsource(k.triple_rank)
    assert '_workspace(h, "het_triple_rank_workspace"' in src  # (the one workspace path of the binding)


def test_module_interface():
    import torch
    from het_amd import linkpred as lp
    sig = inspect.signature(lp.distmult_rank)
    assert list(sig.parameters) == ["h", "w", "s", "r", "o", "sides", "filter", "node_type_offsets", "native"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("sides", "filter", "node_type_offsets", "native"))
    assert sig.parameters["sides"].default == "both" and sig.parameters["filter"].default is None and sig.parameters["native"].default is True
    sig = inspect.signature(lp.distmult_rank_torch)
    assert list(sig.parameters) == ["h", "w", "s", "r", "o", "sides", "filter", "node_type_offsets", "chunk"]
    assert list(inspect.signature(lp.ranking_metrics).parameters) == ["result", "ks"] and inspect.signature(lp.ranking_metrics).parameters["ks"].default == (1, 3, 10)
    assert list(inspect.signature(lp.FilterIndex.__init__).parameters) == ["self", "s", "r", "o", "num_nodes", "num_rels"]
    assert list(inspect.signature(lp.FilterIndex.from_graph).parameters) == ["g"]
    assert list(inspect.signature(lp.DistMultDecoder.rank).parameters) == ["self", "h", "s", "r", "o", "kw"]
    assert lp.RankResult._fields == ("greater", "equal", "candidates", "bad")
    doc = " ".join(lp.__doc__.split())
    for word in ("acc = fmaf(q_j[d], h[c, d], acc)", "rank_j = 1 + greater_j + equal_j / 2", "**counted, not asserted**",
                 "**The filter serves evaluation only: training negatives stay unfiltered.**", "**the one read-back of a ranking call**",
                 "the P tail queries first, then the P head queries"):
        assert word in doc, word
    ids = torch.zeros(4, dtype=torch.int64)
    for bad in ((torch.zeros(4, 8), torch.zeros(2, 4), ids, ids, ids), (torch.zeros(4), torch.zeros(2, 4), ids, ids, ids),
                (torch.zeros(4, 8), torch.zeros(2, 8), ids, ids[:3], ids), (torch.zeros(4, 8), torch.zeros(2, 8), ids.float(), ids, ids)):
        with pytest.raises(ValueError):
            lp.distmult_rank(*bad)


def test_training_script_option():
    import argparse
    from het_amd import train
    p = argparse.ArgumentParser()
    train.add_generic_RGNN_args(p, "x.json")
    assert p.parse_args([]).eval_ranking == 0
    assert p.parse_args(["--link_prediction", "--eval_ranking", "64"]).eval_ranking == 64
    src = inspect.getsource(train.main)
    # absent from the log line when off, a record when on
    assert 'del res["args"]["eval_ranking"]' in src and 'res["ranking"] = ranking' in src
    with pytest.raises(SystemExit, match="--link_prediction"):
        train.main(["--eval_ranking", "64"])
    with pytest.raises(SystemExit, match="--link_prediction"):
        train.main(["--eval_ranking", "64", "--full_graph_training"])
    with pytest.raises(SystemExit, match="eval_ranking"):
        train.main(["--link_prediction", "--full_graph_training", "--eval_ranking", "-1"])
    # the training steps are the functions they were: the evaluation is a function beside them
    assert hashlib.sha256(inspect.getsource(train.HET_RGNN_train).encode()).hexdigest() == RGNN_TRAIN_SHA256
    body = inspect.getsource(train.HET_linkpred_train)
    assert "rank" not in body and "FilterIndex" not in body
    ev = inspect.getsource(train.HET_linkpred_evaluate)
    for word in ("th.no_grad()", "keyed_positive_edges(g, args.eval_ranking, seed=args.seed, draw=RANKING_DRAW)", "FilterIndex.from_graph(g)",
                 'sides="both"', "ranking_metrics(res, ks=(1, 3, 10))", 'out["ms"]'):
        assert word in ev, word
    assert train.RANKING_DRAW < 0  # (the training steps draw with 2 step and 2 step + 1)


def test_no_torch_hrt_op_was_added():
    import het_amd.kernels as k
    assert not any("rank" in n and "triple" in n for n in k.REGISTERED_OPS) and len(k.REGISTERED_OPS) == 31  # (the 31 it had)
    export = open(os.path.join(ROOT, "het_amd", "csrc", "torch_export.cpp")).read()
    assert "triple_rank" not in export
