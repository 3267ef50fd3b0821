"""CPU-side checks of HGT's CSR edge-softmax / aggregation ops (include/het_amd.h a10c): both registrations carry them with
one schema and the reference's written positions, the C ABI declares and exports them and validates its arguments before
any launch, and the distances between the reference's literal behaviour and the intended one."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# op -> positions of the arguments its launcher writes (HGTOps.inc.h:190-204, 180-188, 477-487, 553-566, 282-325)
CSR_OPS = {
    "hgt_full_graph_edge_softmax_ops_csr": (6, 7, 8),
    "hgt_full_graph_message_mean_aggregation_csr": (8,),
    "backward_hgt_full_graph_message_mean_aggregation_csr": (7,),
    "backward_hgt_full_graph_edge_softmax_ops_csr": (10, 11),
    "backward_hgt_full_graph_enorm_to_unnormalized_attn_score_csr": (8, 9),
}


def _schemas(setup: str):
    code = (setup + "\nimport json, torch\nK = torch.ops.torch_hrt\n"
            "print('SCHEMAS' + json.dumps({n: str(getattr(K, n).default._schema) for n in %r if hasattr(K, n)}))" % (list(CSR_OPS),))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("HET_TORCH_HRT_LIB", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("SCHEMAS")][-1][len("SCHEMAS"):])


def test_python_registration_has_the_csr_ops():
    import het_amd.kernels as k
    for name in CSR_OPS:
        assert hasattr(k.K, name) and name in k.REGISTERED_OPS, name
    assert len(k.REGISTERED_OPS) == 31


def test_both_registrations_agree_and_mark_the_written_arguments():
    lib = os.path.join(ROOT, "het_amd", "libtorch_hrt.so")
    assert os.path.exists(lib), "libtorch_hrt.so not built (make -C het_amd/csrc torch_hrt)"
    compiled = _schemas("import sys, torch\ntorch.ops.load_library(%r)\nassert 'het_amd' not in sys.modules" % lib)
    python = _schemas("import het_amd.kernels")
    assert set(compiled) == set(python) == set(CSR_OPS)
    for name, written in CSR_OPS.items():
        assert compiled[name] == python[name], f"{name}:\n  compiled {compiled[name]}\n  python   {python[name]}"
        for i, a in enumerate(torch._C.parse_schema(compiled[name]).arguments):
            is_mut = a.alias_info is not None and a.alias_info.is_write
            assert is_mut == (i in written), f"{name}: argument {i} ({a.name}) mutable={is_mut}, the launcher writes {written}"


def test_header_declares_and_library_exports_the_entry_points():
    from het_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "het_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(het_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in CSR_OPS:
        sym = "het_" + name
        assert sym in declared, sym
        assert hasattr(L, sym), sym
        assert sym in _lib._SIGNATURES, sym


def test_argument_validation_returns_an_error_code():
    """Null pointers and a row_ptrs array that is not num_nodes + 1 long are refused on the host, before any launch."""
    from het_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_int64 * 16)()  # a host buffer: never read, the checks come first
    p = ctypes.cast(buf, ctypes.c_void_p)
    # null index pointers with edges
    rc = L.het_hgt_full_graph_edge_softmax_ops_csr(p, 5, None, None, None, 4, 10, p, p, p, p, p, 8, None, None)
    assert rc == 1 and b"null" in L.het_last_error()
    # null data pointers with edges
    rc = L.het_hgt_full_graph_message_mean_aggregation_csr(p, 5, p, p, p, 4, 10, None, p, p, p, p, 8, 8, None, None)
    assert rc == 1 and b"null" in L.het_last_error()
    # row_ptrs length != num_nodes + 1, for every op
    for call in (
        lambda: L.het_hgt_full_graph_edge_softmax_ops_csr(p, 4, p, p, p, 4, 10, p, p, p, p, p, 8, None, None),
        lambda: L.het_hgt_full_graph_message_mean_aggregation_csr(p, 6, p, p, p, 4, 10, p, p, p, p, p, 8, 8, None, None),
        lambda: L.het_backward_hgt_full_graph_message_mean_aggregation_csr(p, 3, p, p, p, 4, 10, p, p, p, p, 8, 8, None),
        lambda: L.het_backward_hgt_full_graph_edge_softmax_ops_csr(p, 4, p, p, p, 4, 10, 2, p, p, p, p, p, p, p, p, 8, 8, None, None),
        lambda: L.het_backward_hgt_full_graph_enorm_to_unnormalized_attn_score_csr(p, 0, p, p, p, 4, 10, 2, p, p, p, p, p, p, 8, None,
                                                                                   None, 0, None),
    ):
        assert call() == 1 and b"row_ptrs" in L.het_last_error()
    # bad sizes
    rc = L.het_backward_hgt_full_graph_message_mean_aggregation_csr(p, 5, p, p, p, 4, -1, p, p, p, p, 8, 8, None)
    assert rc == 1 and b"sizes" in L.het_last_error()


# ---- quirk distances: the reference's literal forms, computed here in fp64 -------------------
def _case(seed=3):
    from tests.util import random_graph
    g = random_graph(seed=seed, n=200, r=4, e=3000)
    s = g.get_separate_coo_original()
    N, R, E, H, dk = g.get_num_nodes(), g.get_num_rels(), g.get_num_edges(), 4, 8
    gen = torch.Generator().manual_seed(seed)
    score = torch.randn(E, H, generator=gen, dtype=torch.float64)
    mu = torch.rand(R, H, generator=gen, dtype=torch.float64) + 0.5
    msg = torch.randn(E, H, dk, generator=gen, dtype=torch.float64)
    gout = torch.randn(N, H, dk, generator=gen, dtype=torch.float64)
    col, eids = s["col_indices"], s["eids"]
    rel = torch.repeat_interleave(torch.arange(R), s["rel_ptrs"][1:] - s["rel_ptrs"][:-1])
    m = torch.zeros(E, H, dtype=torch.float64)
    m[eids] = torch.exp(score[eids] * mu[rel])
    sm = torch.zeros(N, H, dtype=torch.float64).index_add_(0, col, m[eids])
    a = torch.zeros_like(m)
    a[eids] = m[eids] / sm[col]
    return dict(N=N, R=R, H=H, col=col, eids=eids, rel=rel, score=score, mu=mu, msg=msg, gout=gout, m=m, sm=sm, a=a)


def _aggregate(c, attn, row_of_pos):
    """the aggregation launcher (switch 1): ret[v] = SUM attn[x] / sum[v] * msg[x], x = row_of_pos of each in-edge"""
    ret = torch.zeros(c["N"], c["H"], c["msg"].shape[2], dtype=torch.float64)
    return ret.index_add_(0, c["col"], (attn[row_of_pos] / c["sm"][c["col"]]).unsqueeze(-1) * c["msg"][row_of_pos])


def _softmax_bwd(c, out, rel_mu, rel_acc):
    c_ = c["a"][c["eids"]] * (c["gout"][c["col"]] * (c["msg"][c["eids"]] - out[c["col"]])).sum(-1)
    gs = torch.zeros_like(c["a"])
    gs[c["eids"]] = c_ * c["mu"][rel_mu]
    gmu = torch.zeros(c["R"], c["H"], dtype=torch.float64).index_add_(0, rel_acc, c_ * c["score"][c["eids"]])
    return gs, gmu


def _rel(x, ref):
    return float((x - ref).norm() / ref.norm())


def quirk_distances():
    c = _case()
    intended = _aggregate(c, c["m"], c["eids"])
    q11 = _aggregate(c, c["a"], c["eids"])      # the wrapper hands the NORMALISED score to a launcher that divides again
    q12 = _aggregate(c, c["m"], c["rel"])       # (eids, reltypes) in swapped slots: edge data read at the relation id
    gs, gmu = _softmax_bwd(c, intended, c["rel"], c["rel"])
    zero = torch.zeros_like(c["rel"])
    gs13, gmu13 = _softmax_bwd(c, intended, zero, zero)  # etype stays 0 on the non-compact path: mu[0], all grad_mu on relation 0
    return {"Q11_ret": _rel(q11, intended), "Q12_ret": _rel(q12, intended), "Q13_grad_attn_score": _rel(gs13, gs),
            "Q13_grad_mu": _rel(gmu13, gmu)}


def test_reference_quirk_distances():
    d = quirk_distances()
    print(d)
    # each literal form is a different function, not a rounding: far above fp64 noise (values quoted in DESIGN.md section 3)
    assert all(v > 0.1 for v in d.values()), d
    # ... and the intended forms agree with the fused COO path's definition: SUM a * msg is the normalised mean
    c = _case()
    assert torch.allclose(_aggregate(c, c["m"], c["eids"]),
                          torch.zeros_like(_aggregate(c, c["m"], c["eids"])).index_add_(
                              0, c["col"], c["a"][c["eids"]].unsqueeze(-1) * c["msg"][c["eids"]]))
