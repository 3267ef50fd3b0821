"""fp64 compositions of HGT's CSR edge-softmax / message-aggregation ops on the oracle (shared by tests/test_gpu_hgt_csr.py and
the reference-output pins of tests/test_rgcn_hgt_golden.py; importing this module needs no GPU)."""
import torch

from oracle import ops as O
from tests.util import to64


def ref_forward(s, score, mu, msg):
    """fp64: (sum, m, a) of the separate-COO twin, then ret[v] = SUM m / sum[v] * msg over the in-edges of v."""
    N, (E, H) = s["num_nodes"], score.shape
    sm, m, a = torch.empty(N, H, dtype=torch.float64), torch.empty(E, H, dtype=torch.float64), torch.empty(E, H, dtype=torch.float64)
    O.hgt_full_graph_edge_softmax_ops_separate_coo(s["row_indices"], s["col_indices"], s["eids"], s["rel_ptrs"], to64(score),
                                                   to64(mu), sm, m, a)
    col, eids = s["col_indices"], s["eids"]
    ret = torch.zeros((N,) + tuple(msg.shape[1:]), dtype=torch.float64)
    ret.index_add_(0, col, (m[eids] / sm[col]).unsqueeze(-1) * to64(msg)[eids])
    return sm, m, a, ret


def ref_backward(s, score, mu, a, msg, out, gradout, R):
    """fp64 message gradient and softmax backward of the composition (destination = col of the separate COO)."""
    col, eids = s["col_indices"], s["eids"]
    rel = O.rel_of_position(s["rel_ptrs"])
    gmsg = torch.zeros_like(to64(msg))
    gmsg[eids] = a[eids].unsqueeze(-1) * to64(gradout)[col]
    c = a[eids] * (to64(gradout)[col] * (to64(msg)[eids] - to64(out)[col])).sum(-1)
    gs = torch.zeros_like(a)
    gs[eids] = c * to64(mu)[rel]
    gmu = torch.zeros(R, a.shape[1], dtype=torch.float64).index_add_(0, rel, c * to64(score)[eids])
    return gmsg, gs, gmu
