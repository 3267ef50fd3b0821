"""GPU parity of HGT's CSR edge-softmax / message-aggregation ops (include/het_amd.h a10c) against fp64, and of the autograd
composition HGTFullGraphEdgeSoftmaxAndMessageMeanAggregationOpsCSR against the fused COO path."""
import subprocess
import sys

import pytest
import torch

from oracle import ops as O
from tests._hgt_csr_ref import ref_backward, ref_forward
from tests.util import assert_close, random_graph, to64

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(8, 8), (4, 16), (16, 4), (2, 32), (1, 128), (3, 5), (1, 4)]


@pytest.fixture(scope="module")
def K():
    import het_amd.kernels as k
    return k.K


@pytest.fixture(params=[True, False], ids=["grouped", "plain"])
def plan_mode(request):
    import het_amd.plan as plan
    old = plan.enabled
    plan.enabled = request.param
    plan.clear()
    yield request.param
    plan.enabled = old
    plan.clear()


def hub_graph(seed, N=500, E=6000, R=3):
    """One destination with half of all edges (split over several work items), many destinations without in-edges."""
    from het_amd.graph import HetGraph
    from het_amd.synth import IntegratedCOO
    gen = torch.Generator().manual_seed(seed)
    col = torch.randint(0, 40, (E,), generator=gen)
    col[: E // 2] = 7
    row = torch.randint(0, N, (E,), generator=gen)
    rel = torch.sort(torch.randint(0, R, (E,), generator=gen)).values
    return HetGraph.from_integrated_coo(IntegratedCOO(N, R, torch.tensor([0, N]), row, col, rel, torch.randperm(E, generator=gen)))


def layouts(g):
    """(separate COO, in-CSR, out-CSR) on the CPU (int64)."""
    return g.get_separate_coo_original(), g.get_in_csr(), g.get_out_csr()


def dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def run_ops(K, s, i, o, N, R, H, dk, seed=21):
    gen = torch.Generator().manual_seed(seed)
    E = s["eids"].numel()
    score, mu = torch.randn(E, H, generator=gen), torch.rand(R, H, generator=gen) + 0.5
    msg, go = torch.randn(E, H, dk, generator=gen), torch.randn(N, H, dk, generator=gen)
    ga = torch.randn(E, H, generator=gen)
    s = dict(s, num_nodes=N)
    sm_r, m_r, a_r, ret_r = ref_forward(s, score, mu, msg)
    out = ret_r.float()
    gmsg_r, gs_r, gmu_r = ref_backward(s, score, mu, a_r, msg, out, go, R)
    gs2_r, gmu2_r, tmp_r = torch.zeros(E, H, dtype=torch.float64), torch.zeros(R, H, dtype=torch.float64), torch.zeros(N, H, dtype=torch.float64)
    O.backward_hgt_full_graph_enorm_to_unnormalized_attn_score_separate_coo(s["row_indices"], s["col_indices"], s["eids"], s["rel_ptrs"],
                                                                            to64(score), a_r, to64(ga), to64(mu), gs2_r, gmu2_r, tmp_r)
    di, do = dev(i), dev(o)
    inc = (di["row_ptrs"], di["col_indices"], di["eids"], di["rel_types"])
    score_d, mu_d, msg_d, go_d = score.to(DEV), mu.to(DEV), msg.to(DEV), go.to(DEV)
    nan = float("nan")
    # every overwritten output prefilled with NaN (sum with 5.0: rows of destinations without in-edges must become 0)
    sm, m, a = torch.full((N, H), 5.0, device=DEV), torch.full((E, H), nan, device=DEV), torch.full((E, H), nan, device=DEV)
    K.hgt_full_graph_edge_softmax_ops_csr(*inc, score_d, mu_d, sm, m, a)
    assert_close(sm, sm_r, what="sum"); assert_close(m, m_r, what="m"); assert_close(a, a_r, what="a")
    ret = torch.full((N, H, dk), nan, device=DEV)
    K.hgt_full_graph_message_mean_aggregation_csr(di["row_ptrs"], di["col_indices"], di["rel_types"], di["eids"], msg_d, m, sm, mu_d, ret)
    assert_close(ret, ret_r, what="ret")
    gmsg = torch.full((E, H, dk), nan, device=DEV)
    K.backward_hgt_full_graph_message_mean_aggregation_csr(do["row_ptrs"], do["col_indices"], do["rel_types"], do["eids"], sm, a, go_d, gmsg)
    assert_close(gmsg, gmsg_r, what="grad_message")
    gs, gmu = torch.full((E, H), nan, device=DEV), torch.full((R, H), 0.25, device=DEV)
    K.backward_hgt_full_graph_edge_softmax_ops_csr(do["row_ptrs"], do["col_indices"], do["eids"], do["rel_types"], msg_d, score_d, a,
                                                   out.to(DEV), go_d, mu_d, gs, gmu)
    assert_close(gs, gs_r, what="grad_attn_score"); assert_close(gmu, gmu_r + 0.25, what="grad_mu (accumulated)")
    gs2, gmu2 = torch.full((E, H), nan, device=DEV), torch.full((R, H), 0.25, device=DEV)
    K.backward_hgt_full_graph_enorm_to_unnormalized_attn_score_csr(*inc, score_d, a, ga.to(DEV), mu_d, gs2, gmu2)
    assert_close(gs2, gs2_r, what="enorm grad_score"); assert_close(gmu2, gmu2_r + 0.25, what="enorm grad_mu (accumulated)")


@pytest.mark.parametrize("H,dk", SHAPES)
@pytest.mark.parametrize("graph", ["random", "hub"])
def test_hgt_csr_ops_against_fp64(K, plan_mode, graph, H, dk):
    g = hub_graph(9) if graph == "hub" else random_graph(seed=71, n=260, r=4, e=4000)
    s, i, o = layouts(g)
    run_ops(K, s, i, o, g.get_num_nodes(), g.get_num_rels(), H, dk)


@pytest.mark.parametrize("H,dk", [(8, 8), (3, 5)])
def test_hgt_csr_ops_zero_edges(K, plan_mode, H, dk):
    """No edges: sum and ret are overwritten with zeros, the edge outputs and grad_mu are left alone."""
    N, R = 6, 2
    rp, z = torch.zeros(N + 1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV)
    e2, mu = torch.zeros(0, H, device=DEV), torch.rand(R, H, device=DEV) + 0.5
    sm = torch.full((N, H), 5.0, device=DEV)
    K.hgt_full_graph_edge_softmax_ops_csr(rp, z, z, z, e2, mu, sm, e2, e2)
    assert torch.equal(sm.cpu(), torch.zeros(N, H))
    ret = torch.full((N, H, dk), 5.0, device=DEV)
    K.hgt_full_graph_message_mean_aggregation_csr(rp, z, z, z, torch.zeros(0, H, dk, device=DEV), e2, sm, mu, ret)
    assert torch.equal(ret.cpu(), torch.zeros(N, H, dk))
    gm = torch.zeros(0, H, dk, device=DEV)
    K.backward_hgt_full_graph_message_mean_aggregation_csr(rp, z, z, z, sm, e2, torch.randn(N, H, dk, device=DEV), gm)
    gmu = torch.full((R, H), 0.25, device=DEV)
    K.backward_hgt_full_graph_edge_softmax_ops_csr(rp, z, z, z, gm, e2, e2, ret, ret, mu, e2, gmu)
    K.backward_hgt_full_graph_enorm_to_unnormalized_attn_score_csr(rp, z, z, z, e2, e2, e2, mu, e2, gmu)
    torch.cuda.synchronize()
    assert torch.equal(gmu.cpu(), torch.full((R, H), 0.25))


def composition_case(g, H, dk, seed=5, gradout_seed=6):
    """new_h and the gradients of (score, mu, v, relation_msg) through the CSR composition and through the fused COO path."""
    import het_amd.backend as B
    N, R, E = g.get_num_nodes(), g.get_num_rels(), g.get_num_edges()
    gen = torch.Generator().manual_seed(seed)
    v0, W0 = torch.randn(N, H, dk, generator=gen), torch.randn(R, H, dk, dk, generator=gen) * 0.4
    s0, mu0 = torch.randn(E, H, generator=gen), torch.rand(R, H, generator=gen) + 0.5
    gout = torch.randn(N, H, dk, generator=torch.Generator().manual_seed(gradout_seed)).to(DEV)
    g.get_in_csr(), g.get_out_csr()
    g.cuda_()
    results = []
    for path in ("coo", "csr"):
        v, W, sc, mu = (t.to(DEV).requires_grad_() for t in (v0, W0, s0, mu0))
        if path == "coo":
            new_h = B.hgt_full_graph_message_calc_edge_softmax_and_message_mean_aggregation_coo(W, v, g, mu, sc)
        else:
            sep, i, o = g.get_separate_coo_original(), g.get_in_csr(), g.get_out_csr()
            msg = B.rgnn_relational_matmul({"separate_coo_rel_ptrs": sep["rel_ptrs"], "separate_coo_node_indices": sep["row_indices"],
                                            "separate_coo_eids": sep["eids"]}, W, v, False, 0)
            new_h = B.HGTFullGraphEdgeSoftmaxAndMessageMeanAggregationOpsCSR.apply(
                i["row_ptrs"], i["col_indices"], i["eids"], i["rel_types"], o["row_ptrs"], o["col_indices"], o["eids"], o["rel_types"],
                sc, mu, torch.empty(N, H, device=DEV), torch.empty(E, H, device=DEV), torch.empty(E, H, device=DEV), msg,
                torch.empty(N, H, dk, device=DEV))
        new_h.backward(gout)
        results.append({"new_h": new_h.detach(), "score": sc.grad, "mu": mu.grad, "v": v.grad, "relation_msg": W.grad})
    return results


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("graph", ["random", "hub"])
@pytest.mark.parametrize("H,dk", [(8, 8), (4, 16), (3, 5)])
def test_hgt_csr_composition_matches_fused_coo(plan_mode, graph, H, dk):
    g = hub_graph(11) if graph == "hub" else random_graph(seed=73, n=300, r=4, e=5000)
    coo, csr = composition_case(g, H, dk)
    for k in coo:
        assert csr[k] is not None, k
        assert_close(csr[k], coo[k].cpu(), rtol=1e-4, atol=1e-5, what=k)


FULLSIZE = r"""
import sys, json, torch
sys.path.insert(0, sys.argv[1])
from het_amd.graph import HetGraph
from het_amd.synth import make_mag_like
from tests.test_gpu_hgt_csr import composition_case, rel_l2
coo = make_mag_like(scale=1.0)
for f in ("row", "col", "rel", "eids", "node_type_offsets"):
    setattr(coo, f, getattr(coo, f).to("cuda"))
g = HetGraph.from_integrated_coo(coo, full=False)
H, dk = 8, 16
assert g.get_num_edges() * H * dk > 2 ** 31
coo, csr = composition_case(g, H, dk)
err = {k: rel_l2(csr[k], coo[k]) for k in coo}
print("RELL2 " + json.dumps(err))
"""


def test_hgt_csr_composition_full_size_ogbn_mag():
    """ogbn-mag topology at H=8, dk=16 (E*H*dk > 2^31: 64-bit offsets), forward and backward of the CSR composition against
    the fused COO path, relative L2 <= 1e-5 (in a child process under a time limit)."""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", FULLSIZE, root], capture_output=True, text=True, timeout=1500, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    err = json.loads([l for l in r.stdout.splitlines() if l.startswith("RELL2 ")][-1][6:])
    print(err)
    assert all(v <= 1e-5 for v in err.values()), err
