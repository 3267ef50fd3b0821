"""CPU checks around the bdd RGCN layer: the numpy reference (tests/_rgcn_bdd_ref.py) against torch autograd on the dense expansion,
bdd_dense_weight against torch.block_diag, the layer's parameters and errors, and the condition that makes the GPU tests' integer
grids exact in fp32 whatever the order of the additions."""
import numpy as np
import pytest
import torch

from tests import _rgcn_bdd_cases as CS
from tests import _rgcn_bdd_ref as REF
from tests.util import random_graph


def _dense(weight):
    return torch.stack([torch.block_diag(*weight[r]) for r in range(weight.shape[0])])


@pytest.mark.parametrize("K,D,B", [(8, 12, 4), (6, 6, 1), (16, 8, 8)])
def test_reference_equals_autograd_on_the_dense_expansion(K, D, B):
    g = random_graph(seed=3, n=57, r=5, e=400)
    src, dst, rel, eid = CS.coo_of(g)
    N, R, E = g.get_num_nodes(), g.get_num_rels(), g.get_num_edges()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(N, K, generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn(R, B, K // B, D // B, generator=gen, dtype=torch.float64, requires_grad=True)
    bias = torch.randn(D, generator=gen, dtype=torch.float64, requires_grad=True)
    norm, go = torch.rand(E, 1, generator=gen, dtype=torch.float64), torch.randn(N, D, generator=gen, dtype=torch.float64)
    # a plain per-edge composition: message_e = norm_e * x[src_e] . block_diag(weight[rel_e]), summed per destination
    msg = torch.einsum("ek,ekd->ed", norm[eid] * x[src], _dense(w)[rel])
    out = torch.zeros(N, D, dtype=torch.float64).index_add(0, dst, msg) + bias
    gx, gw, gb = torch.autograd.grad(out, [x, w, bias], go)
    np.testing.assert_allclose(REF.bdd_forward(N, src, dst, rel, eid, norm, x, w, bias), out.detach().numpy(), rtol=1e-12, atol=1e-12)
    rx, rw, rb = REF.bdd_backward(N, src, dst, rel, eid, norm, x, w, go)
    for a, b in ((rx, gx), (rw, gw), (rb, gb)):
        np.testing.assert_allclose(a, b.numpy(), rtol=1e-12, atol=1e-12)


def test_bdd_dense_weight_is_block_diag():
    from het_amd.backend import bdd_dense_weight
    w = torch.randn(3, 4, 2, 5, requires_grad=True)
    d = bdd_dense_weight(w)
    assert d.shape == (3, 8, 20) and torch.equal(d, _dense(w))
    (g,) = torch.autograd.grad(d, w, torch.ones_like(d))  # differentiable: every block element appears once
    assert torch.equal(g, torch.ones_like(w))


def test_layer_parameters_errors_and_the_unchanged_basis_layer():
    from het_amd.layers import HET_EglRelGraphConv_EdgeParallel as Layer
    layer = Layer(64, 32, 7, 8, regularizer="bdd")
    assert tuple(layer.weight.shape) == (7, 8, 8, 4) and not hasattr(layer, "w_comp")
    assert set(layer.state_dict()) == {"weight", "h_bias"}
    bound = torch.nn.init.calculate_gain("relu") * (6.0 / (8 * 8 * 4 + 7 * 8 * 4)) ** 0.5  # xavier_uniform_ at the relu gain
    assert float(layer.weight.detach().abs().max()) <= bound and float(layer.weight.detach().abs().max()) > 0.5 * bound
    for bad in ((64, 32, 7, 3), (64, 30, 7, 4), (64, 32, 7, -1), (64, 32, 7, 0)):
        with pytest.raises(ValueError):
            Layer(*bad, regularizer="bdd")
    with pytest.raises(ValueError, match="either 'basis' or 'bdd'"):
        Layer(64, 32, 7, 2, regularizer="diag")
    # a layer built without the keyword: the parameters and state_dict it had, to the bit
    torch.manual_seed(11)
    a = Layer(16, 8, 5, 2)
    torch.manual_seed(11)
    b = Layer(16, 8, 5, 2, regularizer="basis")
    assert list(a.state_dict()) == ["weight", "w_comp", "h_bias"] == list(b.state_dict()) and a.last_route is None
    assert all(torch.equal(a.state_dict()[k], b.state_dict()[k]) for k in a.state_dict())
    torch.manual_seed(11)
    gain = torch.nn.init.calculate_gain("relu")
    w = torch.nn.init.xavier_uniform_(torch.empty(2, 16, 8), gain=gain)
    wc = torch.nn.init.xavier_uniform_(torch.empty(5, 2), gain=gain)
    assert torch.equal(a.weight, w) and torch.equal(a.w_comp, wc)
    assert list(Layer(16, 8, 5).state_dict()) == ["weight", "h_bias"]


def test_a_cpu_call_is_routed_dense():
    from het_amd.backend import rgcn_bdd_route_of
    g = random_graph(seed=5, n=40, r=4, e=300)
    assert rgcn_bdd_route_of(g, torch.randn(40, 64), torch.randn(4, 8, 8, 8), torch.rand(300, 1)) == "dense"


GRID_CASES = ([("ladder", 0, s) for s in CS.SHAPES] + [("relcount", 0, s) for s in CS.SHAPES] +
              [("rowladder", 1024, (64, 64, 8)), ("rowladder", 1024, (128, 128, 4)), ("repeat", 0, (64, 64, 8))])


@pytest.mark.parametrize("name,arg,shape", GRID_CASES, ids=[f"{n}-{s[0]}x{s[1]}b{s[2]}" for n, _, s in GRID_CASES])
def test_integer_grid_inputs_are_exact_in_fp32_in_any_order(name, arg, shape):
    """Every partial sum, in any order, is a whole number of units below 2^24 units: fp32 holds it exactly, so the GPU tests may ask
    for torch.equal against the fp64 reference."""
    K, D, B = shape
    g = CS.graph(name, arg)
    src, dst, rel, eid = CS.coo_of(g)
    N, R, E = g.get_num_nodes(), g.get_num_rels(), g.get_num_edges()
    c = REF.grid_case(N, E, R, K, D, B, seed=7)
    assert REF.grid_units_bound(N, src, dst, rel, eid, c) < 2 ** 24
    out = REF.bdd_forward(N, src, dst, rel, eid, c["norm"], c["x"], c["weight"], c["bias"])
    grads = REF.bdd_backward(N, src, dst, rel, eid, c["norm"], c["x"], c["weight"], c["go"])
    assert all(REF.on_grid(t) for t in (out,) + grads)
    assert (c["x"] == 0).all(1).any() and (c["go"] == 0).all(1).any()  # some all-zero rows
    assert np.abs(out).max() > 0 and all(np.abs(t).max() > 0 for t in grads)


def test_the_test_graphs_have_their_rungs():
    per_dst, per_src = CS.rel_counts_of(CS.graph("relcount"))
    n = len(CS.REL_COUNTS)
    assert per_dst[:n].tolist() == list(CS.REL_COUNTS) and per_src[n:2 * n].tolist() == list(CS.REL_COUNTS)
    assert CS.rows_per_relation(CS.graph("rowladder", 1024)).tolist() == list(CS.row_ladder_counts(1024))
    g = CS.graph("repeat")
    s = g.get_separate_coo_original()
    N, R = g.get_num_nodes(), g.get_num_rels()
    rel = torch.repeat_interleave(torch.arange(R), s["rel_ptrs"][1:] - s["rel_ptrs"][:-1])
    for idx in (s["col_indices"], s["row_indices"]):
        assert int(torch.bincount(rel * N + idx).max()) <= 32
    assert int(CS.rows_per_relation(g).min()) > 2 * 1024 and int(CS.rel_counts_of(g)[0].float().mean()) >= 4
