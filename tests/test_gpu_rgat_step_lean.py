"""The RGAT training step with its parameter forms made once per step in the forward (W^T and loop_w^T in one launch, one folded
weight), the attention-gradient finish on the side stream beside the node-major pass, the unfold as one launch
and no q_sum fill where every er row has an edge (het_amd/backend/rgat_fused_layer.py, csrc/gat_compact.hip, csrc/node_gemm.hip):
the step against the unchanged fp64 oracle with the tolerances of tests/test_gpu_layers.py, twice per process; a block whose lists
hold er rows without edges, poisoned and unpoisoned; and the bits of grad_attn_l over 20 steps."""
import pytest
import torch

import tests.test_gpu_rgat_backward_routes as RT
from oracle import layers as OL
from tests._poison import POISON_IDS, POISONS, poisoned
from tests._rgat_bf16_ref import build_graph
from tests.util import assert_close, assert_ladder, ladder_counts, rgat_min_abs_preactivation

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = RT.NAMES


def _count(monkeypatch, owner, name, calls):
    fn = getattr(owner, name)

    def counted(*a, **kw):
        calls[name] = calls.get(name, 0) + 1
        return fn(*a, **kw)

    monkeypatch.setattr(owner, name, counted)


def test_the_toy_graph_has_a_destination_reached_through_two_relations():
    g = RT._build(RT.GRAPHS["whole"][0])
    s = g.get_separate_coo_original()
    N, R = g.get_num_nodes(), g.get_num_rels()
    assert int((ladder_counts(g)["rel"] > 0).sum()) >= 3
    rel = torch.repeat_interleave(torch.arange(R), s["rel_ptrs"][1:] - s["rel_ptrs"][:-1])
    runs = torch.bincount(rel * N + s["col_indices"], minlength=R * N).view(R, N)
    assert int(((runs > 0).sum(0) >= 2).sum()) > 0
    assert_ladder(RT._build(RT.GRAPHS["ladder"][0]))  # hubs, long and split segments: partial rows of several relations


@pytest.mark.parametrize("self_loop,bias", RT.LOOP_BIAS)
@pytest.mark.parametrize("graph", ["whole", "ladder"])
def test_step_against_the_oracle_twice(graph, self_loop, bias, monkeypatch):
    """out, grad_x and every parameter gradient against oracle/layers.py::rgat_layer in fp64 (tests/test_gpu_rgat_backward_routes.py:
    _run, the tolerances of tests/util.py::assert_close that tests/test_gpu_layers.py uses), on the node-major route with the side
    stream on.  Twice in one process: the second call runs with the plan cache warm and its own saved forms.  Per step: one launch
    of the transposes, one folded weight (the forward's; the backward makes none), one finish on the side stream."""
    from het_amd import kernels as _k
    from het_amd.backend import rgat_fused_layer as FL
    calls = {}
    _count(monkeypatch, _k, "rgat_transpose_weights", calls)
    _count(monkeypatch, _k, "rgat_attn_grad_finish", calls)
    _count(monkeypatch, _k, "rgat_unfold_weight_gradient", calls)
    _count(monkeypatch, FL, "_folded_weight", calls)
    for step in (1, 2):
        RT._run(monkeypatch, "node-major", graph, 4, 64, 64, True, self_loop, bias, True)
        assert calls == {"rgat_transpose_weights": step, "rgat_attn_grad_finish": step, "rgat_unfold_weight_gradient": step,
                         "_folded_weight": step}, calls


# ---------------------------------------------------------------- a block whose lists hold er rows without edges
BLOCK = ("block", 11, 300, 3, 900, 100)  # N = 300, 3 relations, 900 edges, every edge ends below num_dst = 100


def _add_edgeless_er_rows(g, nd):
    """Every second (relation, destination < nd) pair WITHOUT an edge gets a row in the graph's unique (relation, destination) list
    (the rows stay sorted per relation; the inverse indices follow): what a list made for more edges than the block keeps looks
    like.  Returns the number of rows added."""
    g.generate_separate_unique_node_indices_single_sided_for_each_etype()
    d = g.graph_data["separate"]["unique_node_indices_single_sided"]
    rp, nodes, inv = d["rel_ptrs_col"], d["node_indices_col"], d["inverse_indices_col"]
    new_nodes, new_rp, new_row = [], [0], torch.empty_like(nodes)
    added = 0
    for r in range(rp.numel() - 1):
        a, b = int(rp[r]), int(rp[r + 1])
        have = nodes[a:b]
        assert bool((have[1:] > have[:-1]).all())
        absent = torch.tensor(sorted(set(range(nd)) - set(have.tolist())), dtype=torch.int64)[::2]
        merged = torch.sort(torch.cat([have, absent])).values
        new_row[a:b] = new_rp[-1] + torch.searchsorted(merged, have)
        new_nodes.append(merged)
        new_rp.append(new_rp[-1] + merged.numel())
        added += absent.numel()
    d["node_indices_col"], d["rel_ptrs_col"], d["inverse_indices_col"] = torch.cat(new_nodes), torch.tensor(new_rp), new_row[inv]
    return added


def _block_case():
    from het_amd.layers import HET_RGATLayer
    g = build_graph(BLOCK)
    nd = BLOCK[-1]
    c = ladder_counts(g)  # nothing split over work items, no hub: no float atomics outside grad_attn_l (tests/test_gpu_poison.py)
    out_deg = torch.bincount(g.get_separate_coo_original()["row_indices"], minlength=g.get_num_nodes())
    assert max(int(c["in_rel"].max()), int(c["in"].max()), int(c["out_rel"].max()), int(out_deg.max())) <= 256
    added = _add_edgeless_er_rows(g, nd)
    assert added >= 5, added
    R, N = g.get_num_rels(), g.get_num_nodes()
    torch.manual_seed(5)
    layer = HET_RGATLayer(64, 64, R, 4, self_loop=True, dropout=0.0)
    with torch.no_grad():
        layer.h_bias.uniform_(-0.1, 0.1)
    x, go = torch.randn(N, 64) * 0.5, torch.randn(nd, 64)
    s = g.get_separate_coo_original()
    for _ in range(64):  # no (edge, head) on the leaky-ReLU kink (tests/util.py)
        if rgat_min_abs_preactivation(x, layer.conv_weights, layer.attn_l, layer.attn_r, s) >= 2e-6:
            break
        x = x + 1e-3 * torch.randn(N, 64)
    return g, nd, layer, x, go


def _block_step(g, nd, layer, x, go):
    for p in layer.parameters():
        p.grad = None
    xd = x.to(DEV).requires_grad_(True)
    out = layer(g, xd, num_dst=nd)
    out.backward(go.to(DEV))
    torch.cuda.synchronize()
    got = {"out": out.detach().clone(), "grad_x": xd.grad.clone()}
    got.update({"grad_" + n: p.grad.clone() for n, p in layer.named_parameters()})
    return got


def test_block_with_edgeless_er_rows_keeps_the_q_sum_fill():
    """num_dst < N and (relation, destination) rows that no edge reaches: the aggregation stores no run sums for them, so q_sum must
    still be zero-filled (q == 0 marks them: grad_er_c = 0 there).  The training step against the oracle, and its bits unpoisoned
    (twice), under NaN and under 1e30 -- out, grad_x and every parameter gradient but grad_attn_l, whose finish adds partial rows
    with float atomics (tests/test_gpu_poison.py: NOT_BIT_REPRODUCIBLE); that one is held against the oracle under every poison."""
    g, nd, layer, x, go = _block_case()
    N = g.get_num_nodes()
    s = g.get_separate_coo_original()
    p64 = {n: t.detach().double().requires_grad_(True) for n, t in layer.named_parameters()}
    x64 = x.double().requires_grad_(True)
    ref = OL.rgat_layer(x64, p64["conv_weights"], p64["attn_l"], p64["attn_r"], s["rel_ptrs"], s["row_indices"], s["col_indices"], N, 0.2,
                        p64["loop_weight"], p64["h_bias"])[:nd]
    grads_ref = dict(zip(["x"] + NAMES, torch.autograd.grad(ref, [x64] + [p64[n] for n in NAMES], go.double())))
    g.to_(DEV)
    layer = layer.to(DEV)

    def judged(got, what):
        assert_close(got["out"], ref, what=what + "out")
        for n in ["x"] + NAMES:
            assert_close(got["grad_" + n], grads_ref[n], what=what + "grad_" + n)

    plain, again = _block_step(g, nd, layer, x, go), _block_step(g, nd, layer, x, go)
    judged(plain, "")
    exact = set(plain) - {"grad_attn_l"}
    for n in exact:
        assert torch.equal(plain[n], again[n]), f"{n}: two unpoisoned steps differ"
    for value, vid in zip(POISONS, POISON_IDS):
        with poisoned(value) as rec:
            got = _block_step(g, nd, layer, x, go)
        assert rec.from_module("het_amd.kernels", "_rgat_aggregate_compact_runs"), "the run sums were not among the poisoned tensors"
        judged(got, vid + ": ")
        for n in exact:
            assert bool(torch.isfinite(got[n]).all()), f"{n} under {vid}"
            assert torch.equal(got[n], plain[n]), f"{n}: the bits depend on uninitialised memory ({vid})"
    g.cpu_()


# ---------------------------------------------------------------- the finish on the side stream: the bits of grad_attn_l
def _two_partial_rows_graph():
    """One relation; 12 sources of 3 out-edges (one workgroup of the short-segment launch) and one source of 100 (> the backward's
    pack threshold of 64: one item of the long-segment launch, on the library's side stream).  The edge pass leaves TWO partial rows
    of grad_attn_l, one per launch, and the finish adds each with one float atomic per column onto the zero fill: a sum of two
    terms, the same bits in either order.  (With three or more partial rows or a second relation the atomics' order shows in the last
    bit, before this change as after it: tests/test_gpu_poison.py, NOT_BIT_REPRODUCIBLE.)"""
    from het_amd.graph import HetGraph
    from het_amd.synth import IntegratedCOO
    gen = torch.Generator().manual_seed(2)
    N = 160
    row = torch.cat([torch.arange(12).repeat_interleave(3), torch.full((100,), 12)])
    col = torch.cat([torch.randint(20, N, (36,), generator=gen), 20 + torch.randperm(N - 20, generator=gen)[:100]])
    E = row.numel()
    return HetGraph.from_integrated_coo(IntegratedCOO(N, 1, torch.tensor([0, N]), row, col, torch.zeros(E, dtype=torch.int64), torch.arange(E)))


def test_grad_attn_l_bits_over_20_steps(monkeypatch):
    """20 steps of one layer, same input: grad_attn_l has the same bits every time, and they are the oracle's values.  A finish that
    ran before one of its two producers (the short-segment launch on the main stream, the long-segment launch on the library's side
    stream), or on a workspace that a later allocation had been handed, would miss or corrupt a partial row."""
    from het_amd import kernels as _k
    from het_amd.layers import HET_RGATLayer
    g = _two_partial_rows_graph()
    N = g.get_num_nodes()
    calls = {}
    _count(monkeypatch, _k, "rgat_attn_grad_finish", calls)
    torch.manual_seed(9)
    layer = HET_RGATLayer(64, 64, 1, 4, self_loop=True, dropout=0.0)
    x, go = torch.randn(N, 64) * 0.5, torch.randn(N, 64)
    s = g.get_separate_coo_original()
    for _ in range(64):
        if rgat_min_abs_preactivation(x, layer.conv_weights, layer.attn_l, layer.attn_r, s) >= 2e-6:
            break
        x = x + 1e-3 * torch.randn(N, 64)
    p64 = {n: t.detach().double().requires_grad_(True) for n, t in layer.named_parameters()}
    ref = OL.rgat_layer(x.double(), p64["conv_weights"], p64["attn_l"], p64["attn_r"], s["rel_ptrs"], s["row_indices"], s["col_indices"], N,
                        0.2, p64["loop_weight"], p64["h_bias"])
    ref_attn_l, = torch.autograd.grad(ref, [p64["attn_l"]], go.double())
    g.to_(DEV)
    layer = layer.to(DEV)
    xd, god = x.to(DEV), go.to(DEV)
    first = None
    for step in range(20):
        layer.attn_l.grad = None
        layer(g, xd.clone().requires_grad_(True)).backward(god)
        got = layer.attn_l.grad.clone()
        if first is None:
            first = got
            assert_close(first, ref_attn_l, what="grad_attn_l")
        assert torch.equal(got, first), f"step {step}: grad_attn_l differs from step 0 by {float((got - first).abs().max()):.3e}"
    assert calls == {"rgat_attn_grad_finish": 20}, calls
    g.cpu_()
