"""The HIP ops against the reference's OWN Python outputs (tests/golden/*_rgcn_hgt.npz; tests/golden/make_golden.py::main_rgcn_hgt):
the RGCN compact aggregation and its backward, HGT's CSR edge softmax, message aggregation and its backward, and the separate-COO
softmax twin -- on the toy graph, the 6 x 4096-edge slice and the whole shipped ogbn_mag_0.1 topology, with canonical edge ids
and with every layout renumbered by one random permutation, with the plan's groupings on and off.  H = 2, D = 4 (recipe.H / D); RGCN
width 16 (8 on the whole topology).  The ops always run on the whole graph; the comparison is on the rows the fixtures store
(recipe.pinned_rows).  The oracle's side, and the proof that a wrong convention is rejected, is tests/test_rgcn_hgt_golden.py; the
tolerances are those of tests/_rgcn_hgt_pins.py.  The softmax's exp and sum stay HIP-vs-oracle (tests/test_gpu_hgt_csr.py)."""
import pytest
import torch

from tests._rgcn_hgt_pins import GRAPHS, by_id, load_case, pin_close, rgcn_dict
from tests.util import cpu

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


@pytest.fixture(params=[False, True], ids=["canonical", "permuted"])
def permuted(request):
    return request.param


@pytest.fixture(params=GRAPHS)
def case(request, permuted):
    return load_case(request.param, permuted)


def dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


@pytest.mark.parametrize("direct", [False, True])
def test_rgcn_compact_aggregation_forward_and_backward(K, plan_mode, case, direct):
    """ret (overwritten: prefilled with 3.0) on feat_c[u] = feat_node[node_indices_row[u]] against ref_rgcn.py's node-indexed ret;
    grad_feat [U,X], summed per node, against its grad_feat_src."""
    g, inp, n = case["g"], case["inp"], case["n"]
    s = g.get_separate_coo_original()
    node_of_row = g.get_separate_unique_node_indices_single_sided()["node_indices_row"]
    feat_c = inp["rgcnc_feat_node"][node_of_row].contiguous().to(DEV)
    enorm = by_id(inp["rgcnc_enorm"], s["eids"]).to(DEV)
    a = tuple(s[k].to(DEV) for k in ("eids", "rel_ptrs", "row_indices", "col_indices"))
    d = dev(rgcn_dict(g, direct))
    ret = torch.full((n, feat_c.shape[1]), 3.0, device=DEV)
    K.rgcn_node_mean_aggregation_compact_as_of_node_separate_coo(*a, d, feat_c, enorm, ret, direct)
    gf = torch.zeros_like(feat_c)
    K.backward_rgcn_node_mean_aggregation_compact_as_of_node_separate_coo(*a, d, feat_c, enorm, ret, inp["rgcncb_gradout"].to(DEV), gf, direct)
    pin_close(ret, case, "rgcnc_ret", "hip", what=f"direct={direct}")
    per_node = torch.zeros(n, gf.shape[1], dtype=torch.float64).index_add_(0, node_of_row, cpu(gf).double())
    pin_close(per_node, case, "rgcncb_grad_feat_src", "hip", what=f"direct={direct}")


def test_hgt_csr_softmax_aggregation_and_message_backward(K, plan_mode, case):
    """a of the in-CSR softmax on (score, mu) against hgts_a; the aggregation fed the op's own m and sum and the message by edge id
    against hgta_new_h; the aggregation's backward on the op's own a against hgtab_grad_message (toy graph and slice)."""
    g, inp, n, E, R = case["g"], case["inp"], case["n"], case["E"], case["R"]
    eids = g.get_separate_coo_original()["eids"]
    i, o = dev(g.get_in_csr()), dev(g.get_out_csr())
    H, D = inp["hgta_message"].shape[1:]
    score, mu = by_id(inp["hgts_score"], eids).to(DEV), inp["hgts_mu"].to(DEV)
    nan = float("nan")
    sm, m, a = torch.full((n, H), 5.0, device=DEV), torch.full((E, H), nan, device=DEV), torch.full((E, H), nan, device=DEV)
    K.hgt_full_graph_edge_softmax_ops_csr(i["row_ptrs"], i["col_indices"], i["eids"], i["rel_types"], score, mu, sm, m, a)
    pin_close(cpu(a)[eids], case, "hgts_a", "hip", edge=True, what="in-CSR")
    msg = by_id(inp["hgta_message"], eids).to(DEV)
    ret = torch.full((n, H, D), nan, device=DEV)
    K.hgt_full_graph_message_mean_aggregation_csr(i["row_ptrs"], i["col_indices"], i["rel_types"], i["eids"], msg, m, sm, mu, ret)
    pin_close(ret, case, "hgta_new_h", "hip")
    if "hgtab_grad_message" in case["gold"]:
        gmsg = torch.full((E, H, D), nan, device=DEV)
        K.backward_hgt_full_graph_message_mean_aggregation_csr(o["row_ptrs"], o["col_indices"], o["rel_types"], o["eids"], sm, a,
                                                               inp["hgtab_gradout"].to(DEV), gmsg)
        pin_close(cpu(gmsg)[eids], case, "hgtab_grad_message", "hip", edge=True)
    else:
        assert case["which"] == "mag01_full"


def test_hgt_separate_coo_softmax(K, plan_mode, case):
    """The separate-COO twin of the softmax against the same hgts_a."""
    g, inp, n, E = case["g"], case["inp"], case["n"], case["E"]
    s = g.get_separate_coo_original()
    H = inp["hgts_mu"].shape[1]
    nan = float("nan")
    sm, m, a = torch.full((n, H), 5.0, device=DEV), torch.full((E, H), nan, device=DEV), torch.full((E, H), nan, device=DEV)
    K.hgt_full_graph_edge_softmax_ops_separate_coo(*(s[k].to(DEV) for k in ("row_indices", "col_indices", "eids", "rel_ptrs")),
                                                   by_id(inp["hgts_score"], s["eids"]).to(DEV), inp["hgts_mu"].to(DEV), sm, m, a)
    pin_close(cpu(a)[s["eids"]], case, "hgts_a", "hip", edge=True, what="separate COO")
