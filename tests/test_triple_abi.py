"""The link-prediction entries (csrc/triple_score.hip) as an interface: declared in include/het_amd.h before the softmax cross-entropy
section, exported, typed in het_amd/_lib.py, validated on the host before anything touches a GPU; the launch constants, the Python
wrappers, the module het_amd/linkpred.py and the training script's options.  Runs without a GPU; fails on a tree without the feature."""
import ctypes as C
import hashlib
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("het_triple_corrupt", "het_triple_plan_workspace", "het_triple_plan", "het_distmult_score", "het_distmult_score_bf16",
           "het_distmult_score_backward_workspace", "het_distmult_score_backward", "het_distmult_score_backward_bf16", "het_triple_params")
HET_OK, HET_ERR_INVALID_ARG, HET_ERR_UNSUPPORTED = 0, 1, 3
# sha256 of inspect.getsource(het_amd.train.HET_RGNN_train) on the commit before link prediction: the new path is a new function
RGNN_TRAIN_SHA256 = "92304c54ee8ef7082f98e260b3b8b514e5e1bd4459bae6fb5158b1ceaf4e1bce"


def _lib():
    from het_amd import _lib
    return _lib


def test_entries_are_declared_exported_and_typed():
    _l = _lib()
    header = open(os.path.join(ROOT, "include", "het_amd.h")).read()
    P, I64 = C.c_void_p, C.c_int64
    score = [P, P, P, P, P, I64, I64, I64, I64, P, P]
    bwd = [P] * 11 + [I64] * 4 + [P, P, P, I64, P]
    want = {"het_triple_corrupt": (C.c_int, [P, P, P, I64, I64, I64, I64, P, I64, I64, P, P, P, P]),
            "het_triple_plan_workspace": (I64, [I64, I64, I64]),
            "het_triple_plan": (C.c_int, [P, P, P, I64, I64, I64, P, P, P, P, P, P, P, I64, P]),
            "het_distmult_score": (C.c_int, score), "het_distmult_score_bf16": (C.c_int, score),
            "het_distmult_score_backward_workspace": (I64, [I64, I64, I64]),
            "het_distmult_score_backward": (C.c_int, bwd), "het_distmult_score_backward_bf16": (C.c_int, bwd),
            "het_triple_params": (C.c_int, [C.POINTER(I64)])}
    for name in ENTRIES:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header), name + " is not declared in include/het_amd.h"
        assert hasattr(_l.lib(), name), name + " is not exported by libhet_amd.so"
        assert _l._ENTRIES[name] == want[name], name
    # the header's order: after keyed dropout, before the softmax cross-entropy section (which stays last)
    names = list(_l._ENTRIES)
    at = names.index(ENTRIES[0])
    assert tuple(names[at:at + len(ENTRIES)]) == ENTRIES
    assert names[at - 1] == "het_keyed_dropout_params" and names[at + len(ENTRIES)] == "het_softmax_xent_workspace"
    pos = [header.index(" " + n + "(") for n in ("het_keyed_dropout_params",) + ENTRIES + ("het_softmax_xent_workspace",)]
    assert pos == sorted(pos)
    proto = " ".join(re.search(r"int\s+het_distmult_score_backward_bf16\s*\(([^)]*)\)", header).group(1).split())
    for word in ("const het_bf16* h", "const float* w", "const int64_t* s", "const float* grad_score", "const int64_t* node_ptr",
                 "const int64_t* node_slots", "const int64_t* rel_ptr", "const int64_t* rel_order", "const int64_t* chunk_ptr", "int64_t dim",
                 "het_bf16* grad_h", "float* grad_w", "void* workspace", "int64_t workspace_bytes", "het_stream stream"):
        assert word in proto, word
    proto = " ".join(re.search(r"int\s+het_triple_corrupt\s*\(([^)]*)\)", header).group(1).split())
    for word in ("int64_t num_pos", "int64_t num_neg", "int64_t seed", "int64_t draw", "const int64_t* node_type_offsets", "int64_t num_nodes"):
        assert word in proto, word


def test_source_unit_is_built_without_float_atomics_or_zero_fills():
    csrc = os.path.join(ROOT, "het_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\btriple_score\.hip\b", mk, flags=re.M) and len(re.findall(r"^SRCS\s*:=", mk, flags=re.M)) == 1
    code = open(os.path.join(csrc, "triple_score.hip")).read()
    for kernel in ("HET_triple_corrupt", "HET_triple_keys", "HET_triple_bounds", "HET_distmult_score", "HET_distmult_grad_chunks",
                   "HET_distmult_grad_h", "HET_distmult_grad_w"):
        assert kernel in code
    assert "atomic" not in code.lower() and "asm" not in code and "hipMemset" not in code and "__shared__" not in code
    assert "hipcub::DeviceRadixSort::SortPairs" in code  # (the stable sorts of the plan)
    assert "hipStreamSynchronize" not in code and "hipMemcpy" not in code and "hipDeviceSynchronize" not in code  # no read-back
    assert "ldrow4" in code and "strow4" in code  # (the row helpers of common.hip.h: one body for fp32 and bf16 rows)
    assert not re.search(r"\bint\s+(j|v|pos|slot|c)\b", code)  # triples, nodes, positions and chunks are 64-bit


def test_launch_constants_read_from_python_equal_the_source():
    import het_amd.kernels as k
    src = open(os.path.join(ROOT, "het_amd", "csrc", "triple_score.hip")).read()
    common = open(os.path.join(ROOT, "het_amd", "csrc", "common.hip.h")).read()
    const = lambda text, name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))  # noqa: E731
    p = k.triple_params()
    assert p == {"min_width": const(src, "kTripleMinWidth"), "max_width": const(src, "kTripleMaxWidth"), "max_lanes": const(src, "kTripleMaxLanes"),
                 "list_chunk": const(src, "kTripleListChunk"), "rel_chunk": const(src, "kTripleRelChunk"),
                 "max_blocks": const(src, "kTripleMaxBlocks"), "block": const(common, "kBlock")}
    assert p["min_width"] == 4 and p["max_width"] >= 256 and p["list_chunk"] >= 2 and p["rel_chunk"] >= 2
    assert k.triple_long_list() == p["list_chunk"]
    m = p["max_lanes"]
    assert m & (m - 1) == 0 and k.triple_lane_thresholds() == tuple(4 << i for i in range(m.bit_length() - 1)) and len(k.triple_lane_thresholds()) >= 2
    for g, t in zip((1 << i for i in range(16)), k.triple_lane_thresholds()):
        assert k.triple_lanes(t) == g and k.triple_lanes(t + 4) == 2 * g
    assert k.triple_lanes(4) == 1 and k.triple_lanes(p["max_width"]) == m
    for d, ok in ((4, True), (64, True), (256, True), (p["max_width"], True), (p["max_width"] + 4, False), (0, False), (10, False), (3, False)):
        assert k.triple_width_ok(d) is ok, d
    L = _lib().lib()
    assert L.het_triple_params(None) == HET_ERR_INVALID_ARG and b"het_triple_params" in L.het_last_error()
    # the backward's workspace: fp32 partial rows for at most 4 T / L + 1 chunks of long node lists and T / chunk + R + 1 relation chunks
    T, R, D = 10 ** 6, 7, 64
    assert L.het_distmult_score_backward_workspace(T, R, D) == (4 * T // p["list_chunk"] + 1 + T // p["rel_chunk"] + R + 1) * D * 4
    assert L.het_distmult_score_backward_workspace(0, R, D) == 0
    for bad in ((-1, R, D), (T, -1, D), (T, R, 0), (T, R, 10), (2 ** 30, R, D)):
        assert L.het_distmult_score_backward_workspace(*bad) == -1 and b"het_distmult_score_backward_workspace" in L.het_last_error()
    assert L.het_triple_plan_workspace(0, 10, 3) == 0
    for bad in ((-1, 10, 3), (5, -1, 3), (5, 10, -1), (2 ** 30, 10, 3), (5, 2 ** 31 - 1, 3)):
        assert L.het_triple_plan_workspace(*bad) == -1 and b"het_triple_plan_workspace" in L.het_last_error()


def _aligned(nbytes):
    buf = C.create_string_buffer(nbytes + 16)
    return buf, C.c_void_p((C.addressof(buf) + 15) & ~15)  # (never dereferenced by the calls below)


def test_argument_validation_without_gpu():
    """No triples without a launch, negative counts, dim < 1, widths the kernels do not take, null and misaligned pointers, a workspace
    that is too small, grad_h on h: refused with the documented code and a message naming the entry, nothing enqueued."""
    L = _lib().lib()
    keep = [_aligned(1 << 16) for _ in range(14)]
    h, w, s, r, o, score, g, nptr, slots, rptr, order, cptr, gh, ws = (k[1] for k in keep)
    gw = score
    off = lambda p, d: C.c_void_p(p.value + d)  # noqa: E731
    err = lambda: L.het_last_error()  # noqa: E731
    T, N, R, D = 8, 8, 3, 8

    # ---- het_triple_corrupt
    name = b"het_triple_corrupt"
    call = lambda src=s, rel=r, dst=o, P=4, K=2, offs=None, nt=0, n=N, so=nptr, ro=rptr, oo=order: L.het_triple_corrupt(  # noqa: E731
        src, rel, dst, P, K, 1, 2, offs, nt, n, so, ro, oo, None)
    assert call(src=None, rel=None, dst=None, P=0, so=None, ro=None, oo=None) == HET_OK  # no positives: no launch
    for kw in (dict(P=-1), dict(K=-1), dict(n=-1), dict(n=2 ** 31), dict(nt=-1), dict(P=2 ** 29, K=1), dict(offs=cptr, nt=0)):
        assert call(**kw) == HET_ERR_INVALID_ARG and name in err(), kw
    for kw in (dict(src=None), dict(rel=None), dict(dst=None), dict(so=None), dict(ro=None), dict(oo=None)):
        assert call(**kw) == HET_ERR_INVALID_ARG and b"null" in err() and name in err(), kw
    for kw in (dict(src=off(s, 4)), dict(oo=off(order, 4)), dict(offs=off(cptr, 4), nt=2)):
        assert call(**kw) == HET_ERR_INVALID_ARG and b"misaligned" in err() and name in err(), kw

    # ---- het_triple_plan
    name = b"het_triple_plan"
    call = lambda s=s, r=r, o=o, t=T, n=N, nr=R, nptr=nptr, slots=slots, rptr=rptr, order=order, cptr=cptr, bad=gh, ws=ws, nb=1 << 16: L.het_triple_plan(  # noqa: E731,E501
        s, r, o, t, n, nr, nptr, slots, rptr, order, cptr, bad, ws, nb, None)
    assert call(s=None, r=None, o=None, t=0, nptr=None, slots=None, rptr=None, order=None, cptr=None, bad=None, ws=None, nb=0) == HET_OK
    for kw in (dict(t=-1), dict(n=-1), dict(nr=-1), dict(t=2 ** 30), dict(n=2 ** 31 - 1), dict(nr=2 ** 31)):
        assert call(**kw) == HET_ERR_INVALID_ARG and name in err(), kw
    for kw in (dict(s=None), dict(o=None), dict(nptr=None), dict(slots=None), dict(rptr=None), dict(order=None), dict(cptr=None), dict(bad=None)):
        assert call(**kw) == HET_ERR_INVALID_ARG and b"null" in err() and name in err(), kw
    for kw in (dict(r=off(r, 4)), dict(slots=off(slots, 4)), dict(bad=off(gh, 4)), dict(ws=off(ws, 8))):
        assert call(**kw) == HET_ERR_INVALID_ARG and b"misaligned" in err() and name in err(), kw
    for kw in (dict(ws=None), dict(nb=0), dict(nb=64)):
        assert call(**kw) == HET_ERR_INVALID_ARG and b"workspace" in err() and name in err(), kw

    # ---- the score
    for entry, align in (("het_distmult_score", 16), ("het_distmult_score_bf16", 8)):
        f, name = getattr(L, entry), entry.encode()
        call = lambda h=h, w=w, s=s, r=r, o=o, t=T, n=N, nr=R, d=D, score=score: f(h, w, s, r, o, t, n, nr, d, score, None)  # noqa: E731
        assert call(h=None, w=None, s=None, r=None, o=None, t=0, score=None) == HET_OK  # no triples: no launch
        for kw in (dict(t=-1), dict(n=-1), dict(nr=-1), dict(d=0), dict(d=-4), dict(t=2 ** 30), dict(n=2 ** 31)):
            assert call(**kw) == HET_ERR_INVALID_ARG and name in err(), kw
        assert call(t=0, d=0) == HET_ERR_INVALID_ARG
        for d in (1, 2, 10, 1028):
            assert call(d=d) == HET_ERR_UNSUPPORTED and name in err() and b"dim=%d" % d in err()
        for kw in (dict(h=None), dict(w=None), dict(s=None), dict(r=None), dict(o=None), dict(score=None)):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"null" in err() and name in err(), kw
        for kw in (dict(h=off(h, align // 2)), dict(h=off(h, 2)), dict(w=off(w, 8)), dict(s=off(s, 4)), dict(o=off(o, 4)), dict(score=off(score, 2))):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"misaligned" in err() and name in err(), kw
    assert L.het_distmult_score(off(h, 8), w, s, r, o, T, N, R, D, score, None) == HET_ERR_INVALID_ARG  # fp32 rows: 16 bytes

    # ---- the backward
    need = L.het_distmult_score_backward_workspace(T, R, D)
    assert 0 < need <= 1 << 16
    for entry, align, size in (("het_distmult_score_backward", 16, 4), ("het_distmult_score_backward_bf16", 8, 2)):
        f, name = getattr(L, entry), entry.encode()
        call = lambda h=h, w=w, s=s, r=r, o=o, g=g, nptr=nptr, slots=slots, rptr=rptr, order=order, cptr=cptr, t=T, n=N, nr=R, d=D, gh=gh, gw=gw, ws=ws, nb=need: f(  # noqa: E731,E501
            h, w, s, r, o, g, nptr, slots, rptr, order, cptr, t, n, nr, d, gh, gw, ws, nb, None)
        for kw in (dict(t=-1), dict(n=-1), dict(nr=-1), dict(d=0), dict(t=2 ** 30)):
            assert call(**kw) == HET_ERR_INVALID_ARG and name in err(), kw
        assert call(d=12 + 1) == HET_ERR_UNSUPPORTED and name in err()
        for kw in (dict(h=None), dict(w=None), dict(s=None), dict(r=None), dict(o=None), dict(g=None), dict(nptr=None), dict(slots=None),
                   dict(rptr=None), dict(order=None), dict(cptr=None)):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"null" in err() and name in err(), kw
        for kw in (dict(h=off(h, align // 2)), dict(gh=off(gh, align // 2)), dict(w=off(w, 8)), dict(gw=off(gw, 8)), dict(s=off(s, 4)),
                   dict(nptr=off(nptr, 4)), dict(cptr=off(cptr, 4)), dict(g=off(g, 2)), dict(ws=off(ws, 8))):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"misaligned" in err() and name in err(), kw
        for kw in (dict(ws=None), dict(nb=need - 1), dict(nb=0)):
            assert call(**kw) == HET_ERR_INVALID_ARG and b"workspace" in err() and name in err(), kw
        assert call(gh=h) == HET_ERR_INVALID_ARG and b"overlaps" in err() and name in err()
        assert call(gh=off(h, N * D * size - 16)) == HET_ERR_INVALID_ARG and b"overlaps" in err()  # (its last 16 bytes)
        assert call(h=off(gh, 16)) == HET_ERR_INVALID_ARG and b"overlaps" in err()
    del keep


def test_wrappers_reject_what_the_kernels_do_not_take():
    import torch
    import het_amd.kernels as k
    from het_amd._lib import HetError
    ids = tuple(torch.zeros(8, dtype=torch.int64) for _ in range(3))
    w = torch.zeros(3, 8)
    for h in (torch.zeros(8, 8), torch.zeros(8, 8, dtype=torch.bfloat16), torch.zeros(8, 8, dtype=torch.float64), torch.zeros(8, 8).half()):
        assert not k.distmult_ok(h, w)
        with pytest.raises(HetError, match="distmult_score"):
            k.distmult_score(h, w, *ids)
        with pytest.raises(HetError, match="distmult_score_backward"):
            k.distmult_score_backward(h, w, *ids, torch.zeros(8), None)
    with pytest.raises(HetError, match="triple_corrupt"):
        k.triple_corrupt(*ids, 2, 0, 0, None, 10)
    with pytest.raises(HetError, match="triple_plan"):
        k.triple_plan(*ids, 10, 3)
    assert list(inspect.signature(k.triple_corrupt).parameters) == ["src", "rel", "dst", "num_neg", "seed", "draw", "node_type_offsets", "num_nodes"]
    assert list(inspect.signature(k.triple_plan).parameters) == ["s", "r", "o", "num_nodes", "num_rels"]
    assert list(inspect.signature(k.distmult_score).parameters) == ["h", "w", "s", "r", "o"]
    sig = inspect.signature(k.distmult_score_backward)
    assert [(n, p.default) for n, p in sig.parameters.items()][5:] == [("grad_score", inspect.Parameter.empty), ("plan", inspect.Parameter.empty),
                                                                       ("want_h", True), ("want_w", True)]
    assert k.TriplePlan._fields == ("node_ptr", "node_slots", "rel_ptr", "rel_order", "chunk_ptr", "bad", "num_nodes", "num_rels")


def test_module_interface():
    import torch
    from het_amd import linkpred as lp
    sig = inspect.signature(lp.keyed_corruptions)
    assert list(sig.parameters) == ["src", "rel", "dst", "num_neg", "seed", "draw", "node_type_offsets", "num_nodes"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("seed", "draw", "node_type_offsets", "num_nodes"))
    assert sig.parameters["node_type_offsets"].default is None
    sig = inspect.signature(lp.keyed_positive_edges)
    assert list(sig.parameters) == ["g", "batch_size", "seed", "draw"] and sig.parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(lp.link_prediction_loss).parameters) == ["scores", "num_pos"]
    assert issubclass(lp.DistMultScoreFunction, torch.autograd.Function)
    assert list(inspect.signature(lp.DistMultDecoder.__init__).parameters)[1:3] == ["num_rels", "dim"]
    assert list(inspect.signature(lp.DistMultDecoder.forward).parameters) == ["self", "h", "s", "r", "o"]
    torch.manual_seed(0)
    dec = lp.DistMultDecoder(5, 16)
    w = dec.w_relation
    assert [n for n, _ in dec.named_parameters()] == ["w_relation"] and w.shape == (5, 16) and w.dtype == torch.float32 and dec.last_bad is None
    bound = (6.0 / (5 + 16)) ** 0.5  # xavier-uniform
    assert 0.5 * bound < float(w.detach().abs().max()) <= bound
    ids = torch.zeros(4, dtype=torch.int64)
    for bad in ((torch.zeros(4, 8), ids, ids, ids), (torch.zeros(4), ids, ids, ids), (torch.zeros(4, 16), ids, ids[:3], ids),
                (torch.zeros(4, 16), ids.float(), ids, ids)):
        with pytest.raises(ValueError):
            dec(*bad)
    for bad in (dict(num_neg=-1, num_nodes=4), dict(num_neg=1, num_nodes=2 ** 31), dict(num_neg=1, num_nodes=-1)):
        with pytest.raises(ValueError):
            lp.keyed_corruptions(ids, ids, ids, bad["num_neg"], seed=0, draw=0, num_nodes=bad["num_nodes"])
    # the documentation states what the sampler does not do, in bold
    doc = lp.__doc__
    assert "**Unfiltered: v_new == v_old and collisions with" in doc and "(hi - lo) / 2^32" in doc and "**counted, not asserted**" in doc


def test_training_script_options():
    import argparse
    from het_amd import train
    p = argparse.ArgumentParser()
    train.add_generic_RGNN_args(p, "x.json")
    a = p.parse_args([])
    assert a.link_prediction is False and a.num_negatives == 1
    a = p.parse_args(["--link_prediction", "--num_negatives", "16"])
    assert a.link_prediction is True and a.num_negatives == 16
    src = inspect.getsource(train.main)
    # absent from the log line when off, named when on
    assert 'del res["args"]["link_prediction"]' in src and 'del res["args"]["num_negatives"]' in src and 'res["task"] = "link_prediction"' in src
    with pytest.raises(SystemExit, match="full_graph_training"):
        train.main(["--link_prediction"])
    with pytest.raises(SystemExit, match="inference"):
        train.main(["--link_prediction", "--full_graph_training", "--inference"])
    # the classification step is the function it was: the new path is a function beside it
    assert hashlib.sha256(inspect.getsource(train.HET_RGNN_train).encode()).hexdigest() == RGNN_TRAIN_SHA256
    body = inspect.getsource(train.HET_linkpred_train)
    for word in ("keyed_positive_edges", "keyed_corruptions", "link_prediction_loss", "draw=2 * step", "draw=2 * step + 1", "optimizer.step()"):
        assert word in body, word
    # "forward" is the encoder; the batch, the decoder and the loss count inside "backward"
    assert body.index("ev[1].record()") < body.index("ev[2].record()") < body.index("keyed_positive_edges(g") < body.index("loss.backward()")


def test_no_torch_hrt_op_was_added():
    import het_amd.kernels as k
    assert not any("triple" in n or "distmult" in n for n in k.REGISTERED_OPS) and len(k.REGISTERED_OPS) == 31  # (the 31 it had)
    export = open(os.path.join(ROOT, "het_amd", "csrc", "torch_export.cpp")).read()
    assert "triple" not in export and "distmult" not in export
