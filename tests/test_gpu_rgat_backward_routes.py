"""The training node of the RGAT layer (het_amd/backend/rgat_fused_layer.py: RgatLayerFunction, forward + backward) on the
distinct-row dataflow, on every route of its backward and with the self-loop and the bias on and off: output and all gradients
against the fp64 oracle (oracle/layers.py::rgat_layer, first num_dst rows).  tests/test_gpu_layers.py runs the node with self-loop
and bias both on, on whole graphs, with the side stream on; the two halo forms are in tests/test_gpu_dist.py.

Routes (every case names the one it expects and asserts that it ran, by counting the calls of the two kernels.py functions that
tell them apart):
  node-major   grad_x from one pass over the nodes (kernels.rgat_node_backward_dx): er from the folded weight, a shape
               het_rgat_node_gemm_ok takes, every edge ending below num_dst
  generic      grad_x by per-relation read-modify-write (kernels.matmul_backward(..., distinct_rows=True)): everything else"""
import functools

import pytest
import torch

from oracle import layers as OL
from tests._rgat_bf16_ref import build_graph
from tests.util import assert_close, rgat_min_abs_preactivation

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAPHS = {"whole": (("random", 41, 400, 4, 6000), None),          # tests/test_gpu_layers.py: test_rgat_layer_variants
          "block": (("block", 5, 900, 4, 7000, 200), 200),        # every edge ends below num_dst = 200
          "whole_num_dst": (("random", 41, 400, 4, 6000), 200),   # num_dst < N and edges that end at or above it
          # tests/test_gpu_rgat_kink.py: the ladder graph (hubs of 257 .. 769 in-edges), the block a sampler makes of its first 120
          # nodes (all the destination rungs) with all their in-edges, and num_dst = its 43 destination rungs with the edges into the pool kept
          "ladder": (("ladder", 5, 0), None),
          "ladder_block": (("ladder_block", 5, 0, 120), 120),
          "ladder_num_dst": (("ladder", 5, 0), 43)}
NAMES = ["conv_weights", "attn_l", "attn_r", "loop_weight", "h_bias"]


def _build(spec):
    if spec[0] != "ladder_block":
        return build_graph(spec)
    from het_amd.sampling import NeighborSampler
    _, R, seed, nd = spec
    block = NeighborSampler(build_graph(("ladder", R, seed)), [-1]).sample_block(torch.arange(nd), -1)
    assert block.num_dst == nd
    return block.graph


@functools.lru_cache(maxsize=None)
def _case(graph, H, K, X, mulfirst, self_loop, bias, slope=0.2, case=None):
    """(layer state, x, gradout, oracle output [nd,X], oracle gradients by name) of a case, computed once: the cases that differ in
    the side stream alone share it.  Nothing here is changed by a test.  case: the seed of pre-made inputs and parameters ON the
    leaky-ReLU kink (tests/util.py: exact_rgat_case) in place of the random draw: no nudge, and the ties are asserted."""
    from het_amd.layers import HET_RGATLayer
    spec, nd = GRAPHS[graph]
    g = _build(spec)
    R, N = g.get_num_rels(), g.get_num_nodes()
    nd = N if nd is None else nd
    torch.manual_seed(7)
    layer = HET_RGATLayer(K, X, R, H, bias=bias, self_loop=self_loop, compact_as_of_node_flag=True, compact_direct_indexing_flag=True,
                          multiply_among_weights_first_flag=mulfirst, dropout=0.0)
    if bias:
        with torch.no_grad():
            layer.h_bias.uniform_(-0.1, 0.1)
    x = torch.randn(N, K) * 0.5
    go = torch.randn(nd, X)
    s = g.get_separate_coo_original()
    if case is not None:
        from tests.util import assert_ties_on_hub_edges, exact_rgat_case, load_rgat_case
        c = exact_rgat_case(g, H, K, X // H, case, bias=bias, self_loop=self_loop)
        x, go = load_rgat_case(layer, c)
        go = go[:nd]
        assert_ties_on_hub_edges(c, s, N)
    for _ in range(64 if case is None else 0):  # no (edge, head) on the leaky-ReLU kink (tests/util.py)
        if rgat_min_abs_preactivation(x, layer.conv_weights, layer.attn_l, layer.attn_r, s) >= 2e-6:
            break
        x = x + 1e-3 * torch.randn(N, K)
    p = {n: t.detach().double().requires_grad_(True) for n, t in layer.named_parameters()}
    x64 = x.double().requires_grad_(True)
    ref = OL.rgat_layer(x64, p["conv_weights"], p["attn_l"], p["attn_r"], s["rel_ptrs"], s["row_indices"], s["col_indices"], N, slope,
                        p.get("loop_weight"), p.get("h_bias"))[:nd]
    wrt = {"x": x64, **p}
    grads = dict(zip(wrt, torch.autograd.grad(ref, list(wrt.values()), go.double())))
    return {n: t.detach().clone() for n, t in layer.state_dict().items()}, x, go, ref.detach(), grads


def _run(monkeypatch, route, graph, H, K, X, mulfirst, self_loop, bias, overlap, slope=0.2, case=None):
    from het_amd import kernels as _k
    from het_amd.backend import rgat_fused_layer as FL
    from het_amd.layers import HET_RGATLayer
    monkeypatch.setattr(FL, "OVERLAP", overlap)
    monkeypatch.setattr(FL, "LITERAL_ER", not mulfirst)  # (False: er from the folded weight whatever the layer flag says)
    monkeypatch.setattr(FL, "PER_EDGE", False)
    state, x, go, ref, grads_ref = _case(graph, H, K, X, mulfirst, self_loop, bias, slope, case)
    spec, nd = GRAPHS[graph]
    g = _build(spec)
    R = g.get_num_rels()
    assert _k.rgat_node_gemm_ok(R, H, K, X // H) == (X == 64), "the shapes of the routes are not what this file assumes"
    calls = {"node-major": 0, "generic": 0}
    node_dx, matmul_backward = _k.rgat_node_backward_dx, _k.matmul_backward

    def counted_node_dx(*a, **kw):
        calls["node-major"] += 1
        return node_dx(*a, **kw)

    def counted_matmul_backward(*a, **kw):
        calls["generic"] += bool(kw.get("distinct_rows"))
        return matmul_backward(*a, **kw)

    monkeypatch.setattr(_k, "rgat_node_backward_dx", counted_node_dx)
    monkeypatch.setattr(_k, "matmul_backward", counted_matmul_backward)
    layer = HET_RGATLayer(K, X, R, H, bias=bias, self_loop=self_loop, compact_as_of_node_flag=True, compact_direct_indexing_flag=True,
                          multiply_among_weights_first_flag=mulfirst, dropout=0.0, leaky_relu_slope=slope)
    layer.load_state_dict(state)
    g.to_(DEV)
    layer = layer.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    out = layer(g, xd, num_dst=nd)
    out.backward(go.to(DEV))
    torch.cuda.synchronize()
    g.cpu_()
    other = "generic" if route == "node-major" else "node-major"
    assert calls[route] > 0 and calls[other] == 0, f"expected the {route} route: {calls}"
    assert_close(out, ref, what="out")
    assert_close(xd.grad, grads_ref["x"], what="grad_x")
    params = dict(layer.named_parameters())
    assert set(params) == set(grads_ref) - {"x"}
    for n in NAMES:
        if n in params:
            assert_close(params[n].grad, grads_ref[n], what="grad_" + n)


LOOP_BIAS = [(True, True), (True, False), (False, True), (False, False)]


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("self_loop,bias", LOOP_BIAS)
@pytest.mark.parametrize("graph", ["whole", "block"])
def test_node_major_route(graph, self_loop, bias, overlap, monkeypatch):
    _run(monkeypatch, "node-major", graph, 4, 64, 64, True, self_loop, bias, overlap)


@pytest.mark.parametrize("self_loop,bias", LOOP_BIAS)
@pytest.mark.parametrize("mulfirst", [True, False])
def test_generic_route(mulfirst, self_loop, bias, monkeypatch):
    """A shape the node-major pass refuses (rows of 128 floats), er from the folded weight and in its literal form."""
    _run(monkeypatch, "generic", "whole", 4, 64, 128, mulfirst, self_loop, bias, True)


def test_edges_ending_at_or_above_num_dst_take_the_generic_route(monkeypatch):
    """The node-major shape, but num_dst < N with edges that end at or above it: the per-destination tensors of the backward are
    not their first num_dst rows, which the node-major pass assumes."""
    spec, nd = GRAPHS["whole_num_dst"]
    assert int(build_graph(spec).get_separate_coo_original()["col_indices"].max()) >= nd
    _run(monkeypatch, "generic", "whole_num_dst", 4, 64, 64, True, True, True, True)
