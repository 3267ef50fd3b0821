"""RGAT attention AT the leaky-ReLU kink and across slopes.

Every other RGAT test moves its random input off the kink first (tests/util.py: rgat_nudge_off_kink), because fp32 and fp64 may round
el + er to different sides of 0.  Here the inputs come from small integer grids (tests/util.py: exact_rgat_case, exact_gat_case; their
conditions are asserted on the CPU in tests/test_rgat_kink_inputs.py): el, er and z = el + er are exact in fp32, in bf16 and in fp64
in every association the routes use, so every format takes the same branch, thousands of (edge, head) pairs sit exactly ON z == 0 --
hundreds of them on edges into hubs -- and the op-level inputs also hold z = +-2^-30, where expf(z) rounds to 1.0f.  The rule that
is pinned: the derivative at z == 0 is `slope` (z > 0 ? 1 : slope, the reference's gradLeaky; oracle/ops.py, oracle/layers.py).  A
kernel that decides z >= 0, or a grouped kernel that recovers z > 0 from a stored exp of exactly 1, is off by a factor 1 / slope on
every tied edge: tests/test_rgat_kink_inputs.py shows that tests/util.py::assert_close rejects that.

The oracles, the case functions and the tolerances are those of the files the cases come from (tests/test_gpu_ops.py,
tests/test_gpu_layers.py::_run_rgat, tests/test_gpu_rgat_backward_routes.py::_run): fp32 results at assert_close's defaults, bf16
stores elementwise within 2^-8 |ref| + 1e-5 max|ref| (tests/_bf16_rows_ref.py::check_bf16).  Every layer-level case asserts,
before it compares, that its input has ties on hub edges.

The slope ladder (0, 1, 2.5, -0.2; 0.2 is every other case) runs on the same inputs, so the ties stay in place.  A negative slope
is outside the grouped kernels' recovery of z > 0 from the stored exp (exp(slope z) > 1 for z < 0): the guards route it elsewhere,
and whatever they pick has to match the oracle."""
import pytest
import torch

from oracle import layers as OL
from oracle import ops as O
from tests import _bf16_rows_ref as RR
from tests import _rgat_attention_ref as A
from tests import _rgat_bf16_train_ref as TREF
from tests import test_gpu_ops as OPS
from tests import test_gpu_rgat_backward_routes as ROUTES
from tests.test_gpu_layers import _run_rgat
from tests.test_gpu_ops import K, plan_mode  # noqa: F401  (fixtures: the registration under test, groupings on / off)
from tests.util import (assert_close, assert_gat_ties_on_hub_edges, assert_ties_on_hub_edges, exact_gat_case, exact_gat_case_of_kind,
                        exact_rgat_case, ladder_graph, load_rgat_case)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPES = [0.0, 1.0, 2.5, -0.2]
SEED = 3


# ---------------------------------------------------------------- 2. the ops at the kink
@pytest.mark.parametrize("kind,H,D,R", [(kind, 4, 16, 5) for kind in (0, 1, 2, 3, 4)]
                         + [(kind, H, D, 5) for kind in (0, 4) for (H, D) in ((2, 32), (1, 64), (3, 5))] + [(0, 4, 16, 9), (4, 4, 16, 9)])
def test_reference_named_pair(K, plan_mode, kind, H, D, R):  # noqa: F811
    g = ladder_graph(R=R)
    OPS.fused_gat_case(K, g, kind, H, D, inputs=exact_gat_case_of_kind(g, kind, H, D, seed=17))


@pytest.mark.parametrize("fold,bias", [(False, False), (True, True)])
@pytest.mark.parametrize("H,D,R", [(4, 16, 5), (2, 32, 5), (1, 64, 5), (4, 16, 9)])
def test_compact_passes(K, H, D, R, fold, bias):  # noqa: F811
    g = ladder_graph(R=R)
    OPS.rgat_compact_case(K, g, H, D, fold, bias, inputs=exact_gat_case_of_kind(g, 4, H, D, seed=19))


@pytest.mark.parametrize("fold,bias", [(False, False), (True, True)])
@pytest.mark.parametrize("H,D,R", [(4, 16, 5), (2, 32, 5), (1, 64, 5), (4, 16, 9)])
def test_compact_run_sums(K, H, D, R, fold, bias):  # noqa: F811
    """D = 16 with R <= 8 also forms el from the gathered row; R = 9 gathers it."""
    g = ladder_graph(R=R)
    col, N = g.get_separate_coo_original()["col_indices"], g.get_num_nodes()
    ss = g.get_separate_unique_node_indices_single_sided()

    def inputs(srow, drow):
        feat, el, er, go = exact_gat_case(srow, drow, col, ss["node_indices_row"].numel(), ss["node_indices_col"].numel(), N, H, D, seed=23)
        assert_gat_ties_on_hub_edges(el, er, srow, drow, col, N)
        return feat, el, er, go

    OPS.rgat_run_sums_case(K, g, H, D, fold, bias, inputs=inputs)


@pytest.mark.parametrize("H,D", [(4, 16), (3, 5)])
@pytest.mark.parametrize("compact", [False, True])
def test_csr_pair(K, plan_mode, compact, H, D):  # noqa: F811
    g = ladder_graph(R=5)
    i, u = g.get_in_csr(), g.get_separate_unique_node_indices()
    N = g.get_num_nodes()
    dst = torch.repeat_interleave(torch.arange(N), i["row_ptrs"][1:] - i["row_ptrs"][:-1])
    if compact:
        srow = O._search_rows(u["rel_ptrs"], u["node_indices"], i["rel_types"], i["col_indices"], N)
        drow = O._search_rows(u["rel_ptrs"], u["node_indices"], i["rel_types"], dst, N)
    else:
        srow = drow = i["eids"]

    def inputs(n_rows):
        feat, el, er, go = exact_gat_case(srow, drow, dst, n_rows, n_rows, N, H, D, seed=29)
        assert_gat_ties_on_hub_edges(el, er, srow, drow, dst, N)
        return feat, el, er, go

    OPS.fused_gat_csr_case(K, plan_mode, g, compact, H, D, inputs=inputs)


@pytest.mark.parametrize("H,D", [(4, 16), (2, 32)])
def test_backward_streams_the_sorted_exp(K, H, D):  # noqa: F811
    """The stored-exp recovery on the streamed, destination-sorted copy of exp and on the gathered one (hit and miss of
    tests/test_gpu_ops.py::sorted_exp_stream_case); its in-place edit halves exp, so that leg is off the stored-value rule by
    construction and is compared with the oracle on the tensors it is given, as there."""
    g = ladder_graph(R=5)
    OPS.sorted_exp_stream_case(K, g, H, D, inputs=exact_gat_case_of_kind(g, 0, H, D, seed=31))


@pytest.mark.parametrize("H,D,R", [(4, 16, 5), (1, 64, 5), (4, 16, 9)])
def test_folded_attn_l(H, D, R):
    """el = <feat, attn_l[r]> formed inside the node: feat in {-1, -1/2, 0, 1/2, 1} (half of it 0), attn_l in {-1/2, 0, 1/2} -- el is an
    exact multiple of 1/4 --, er = -el on a sixth of the (edge, head) pairs (exact ties) and a multiple of 1/8 elsewhere."""
    g = ladder_graph(R=R)
    s = g.get_separate_coo_original()
    N, E = g.get_num_nodes(), g.get_num_edges()
    gen = torch.Generator().manual_seed(37)
    from tests.util import _grid
    feat = _grid((E, H, D), [0.0, 0.0, 0.0, 0.0, -0.5, 0.5, -1.0, 1.0], gen)
    attn = _grid((R, H, D), [-0.5, 0.0, 0.5], gen)
    rel_of_eid = torch.empty(E, dtype=torch.int64)
    rel_of_eid[s["eids"]] = O.rel_of_position(s["rel_ptrs"])
    el = (feat * attn[rel_of_eid]).sum(-1)
    assert torch.equal(el.double(), (feat.double() * attn.double()[rel_of_eid]).sum(-1))
    er = torch.where(torch.rand(E, H, generator=gen) < 1 / 6, -el, _grid((E, H), [k / 8 for k in range(-16, 17)], gen))
    go = _grid((N, H, D), [i / 4 for i in range(-8, 9)], gen)
    tie = ((el + er) == 0).any(1)  # (by edge id, as el and er are)
    hub_eid = torch.zeros(E, dtype=torch.bool)
    hub_eid[s["eids"]] = (torch.bincount(s["col_indices"], minlength=N) > 256)[s["col_indices"]]
    assert int((tie & hub_eid).sum()) >= 100
    OPS.folded_attn_l_case(g, H, D, inputs=lambda E_, R_: (feat, attn, er, go))


# ---------------------------------------------------------------- 3. the layer at the kink, every route
def _layer_case(R=5, H=4, K=64, D=16, **kw):
    g = ladder_graph(R=R, shuffle=False)
    return g, exact_rgat_case(g, H, K, D, SEED, **kw)


@pytest.mark.parametrize("K", [64, 32])
@pytest.mark.parametrize("compact,direct,mulfirst", [(False, False, False), (False, False, True), (True, False, False),
                                                     (True, True, False), (True, True, True), (True, False, True)])
def test_layer_variants(compact, direct, mulfirst, K):
    g, c = _layer_case(K=K)
    _run_rgat(g, H=4, K=K, X=64, compact=compact, direct=direct, mulfirst=mulfirst, case=c)


@pytest.mark.parametrize("K,mulfirst", [(64, False), (32, False), (64, True)])
@pytest.mark.parametrize("literal_er", [False, True])
def test_layer_per_edge_dataflow(literal_er, K, mulfirst, monkeypatch):
    from het_amd.backend import rgat_fused_layer as FL
    monkeypatch.setattr(FL, "PER_EDGE", True)
    monkeypatch.setattr(FL, "LITERAL_ER", literal_er)
    g, c = _layer_case(K=K)
    _run_rgat(g, H=4, K=K, X=64, compact=False, direct=False, mulfirst=mulfirst, case=c)


@pytest.mark.parametrize("K", [64, 32])
def test_layer_default_flags_literal_er(K, monkeypatch):
    from het_amd.backend import rgat_fused_layer as FL
    monkeypatch.setattr(FL, "LITERAL_ER", True)
    g, c = _layer_case(K=K)
    _run_rgat(g, H=4, K=K, X=64, compact=False, direct=False, mulfirst=False, case=c)


@pytest.mark.parametrize("mode,compact,K", [("atomics", False, 64), ("atomics", True, 64), ("op_by_op", False, 64), ("op_by_op", True, 64),
                                            ("atomics", False, 32), ("op_by_op", False, 32)])
def test_layer_fallback_paths(mode, compact, K, monkeypatch):
    import het_amd.plan as plan
    from het_amd.backend import rgat_fused_layer as FL
    old = plan.enabled
    try:
        if mode == "atomics":
            plan.enabled = False
            plan.clear()
        else:
            monkeypatch.setattr(FL, "rgat_layer_fused_ok", lambda *a, **k: False)
        g, c = _layer_case(K=K)
        _run_rgat(g, H=4, K=K, X=64, compact=compact, direct=compact, mulfirst=False, case=c)
    finally:
        plan.enabled = old
        plan.clear()


@pytest.mark.parametrize("mulfirst", [False, True])
def test_layer_reference_op_sequence(mulfirst):
    g, c = _layer_case()
    _run_rgat(g, H=4, K=64, X=64, compact=False, direct=False, mulfirst=mulfirst, reference_op_sequence=True, case=c)


def test_layer_csr_path():
    g, c = _layer_case()
    _run_rgat(g, H=4, K=64, X=64, compact=False, direct=False, mulfirst=False, edge_parallel=False, case=c)


@pytest.mark.parametrize("compact,mulfirst", [(False, False), (True, True)])
def test_layer_nine_relations(compact, mulfirst):
    g, c = _layer_case(R=9)
    _run_rgat(g, H=4, K=64, X=64, compact=compact, direct=compact, mulfirst=mulfirst, case=c)


@pytest.mark.parametrize("self_loop,bias", [(True, False), (False, True), (False, False)])
def test_layer_without_self_loop_or_bias(self_loop, bias):
    g, c = _layer_case(self_loop=self_loop, bias=bias)
    _run_rgat(g, H=4, K=64, X=64, compact=False, direct=False, mulfirst=False, self_loop=self_loop, bias=bias, case=c)


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("graph,K", [("ladder", 64), ("ladder_block", 64), ("ladder", 32)])
def test_node_major_route(graph, K, overlap, monkeypatch):
    ROUTES._run(monkeypatch, "node-major", graph, 4, K, 64, True, True, True, overlap, case=SEED)


def test_node_major_route_without_self_loop_and_bias(monkeypatch):
    ROUTES._run(monkeypatch, "node-major", "ladder", 4, 64, 64, True, False, False, True, case=SEED)


@pytest.mark.parametrize("mulfirst", [True, False])
def test_generic_route(mulfirst, monkeypatch):
    ROUTES._run(monkeypatch, "generic", "ladder", 4, 64, 128, mulfirst, True, True, True, case=SEED)


def test_generic_route_edges_ending_at_or_above_num_dst(monkeypatch):
    spec, nd = ROUTES.GRAPHS["ladder_num_dst"]
    assert int(ROUTES.build_graph(spec).get_separate_coo_original()["col_indices"].max()) >= nd
    ROUTES._run(monkeypatch, "generic", "ladder_num_dst", 4, 64, 64, True, True, True, True, case=SEED)


@pytest.mark.parametrize("compact", [False, True])
def test_halo_route_two_ranks(compact):
    """The layer's own halo exchange (forward_with_halo) on a 2-way partition, as logical ranks of this process (dist.LocalRanks:
    tests/test_gpu_dist.py), against the fp64 oracle on the whole graph."""
    from het_amd.dist import LocalRanks
    from het_amd.layers import HET_RGATLayer
    from het_amd.synth import IntegratedCOO
    g, c = _layer_case()
    s = g.get_separate_coo_original()
    N, R, E = g.get_num_nodes(), g.get_num_rels(), g.get_num_edges()
    assert_ties_on_hub_edges(c, s, N)
    layer = HET_RGATLayer(64, 64, R, 4, self_loop=True, dropout=0.0, compact_as_of_node_flag=compact, compact_direct_indexing_flag=compact)
    x, go = load_rgat_case(layer, c)
    p64 = {n: t.detach().double().requires_grad_(True) for n, t in layer.named_parameters()}
    x64 = x.double().requires_grad_(True)
    ref = OL.rgat_layer(x64, p64["conv_weights"], p64["attn_l"], p64["attn_r"], s["rel_ptrs"], s["row_indices"], s["col_indices"], N, 0.2,
                        p64["loop_weight"], p64["h_bias"])
    names = ["conv_weights", "attn_l", "attn_r", "loop_weight", "h_bias"]
    grads_ref = torch.autograd.grad(ref, [x64] + [p64[n] for n in names], go.double())
    layer = layer.to(DEV)
    coo = IntegratedCOO(N, R, torch.tensor([0, N]).to(DEV), s["row_indices"].to(DEV), s["col_indices"].to(DEV),
                        O.rel_of_position(s["rel_ptrs"]).to(DEV), torch.arange(E).to(DEV))
    lr = LocalRanks(coo, 2, layer, full_layouts=compact)
    mine = [lr.owned_nodes(r).cpu() for r in range(2)]
    x_own = [x[m].to(DEV).requires_grad_(True) for m in mine]
    outs = lr.forward(x_own)
    assert all(lr.took_halo_path), lr.took_halo_path
    lr.backward(outs, [go[m].to(DEV) for m in mine], x_own)
    for r in range(2):
        assert_close(outs[r], ref.detach()[mine[r]], what=f"rank {r} out")
        assert_close(x_own[r].grad, grads_ref[0][mine[r]], what=f"rank {r} grad_x")
    for n, gr in zip(names, grads_ref[1:]):
        assert_close(dict(layer.named_parameters())[n].grad, gr, what="grad_" + n + " (sum over the ranks)")


@pytest.mark.parametrize("K,mulfirst", [(64, False), (64, True), (32, False), (32, True)])
def test_bf16_training_step(K, mulfirst, monkeypatch):
    """x, feat_c, the self-loop + bias rows and the output gradient are bf16 numbers already (tests/test_rgat_kink_inputs.py): the only
    roundings left are the stores of the output and of grad_x, held ELEMENTWISE against the fp64 oracle within the bound of the bf16
    ladders; the parameter gradients at the fp32 tolerance."""
    from het_amd.layers import HET_RGATLayer
    from tests import test_gpu_rgat_bf16_train as T
    g, c = _layer_case(K=K)
    s = g.get_separate_coo_original()
    N = g.get_num_nodes()
    assert_ties_on_hub_edges(c, s, N)
    layer = HET_RGATLayer(K, 64, g.get_num_rels(), 4, bias=True, self_loop=True, multiply_among_weights_first_flag=mulfirst, dropout=0.0,
                          bf16_training=True)
    x, go = load_rgat_case(layer, c)
    p = {n: t.detach().double() for n, t in layer.named_parameters()}
    ref = TREF.oracle(x.double(), p, s["rel_ptrs"], s["row_indices"], s["col_indices"], N, go.double(), 0.2)
    calls = T._count_calls(monkeypatch)
    layer = layer.to(DEV)
    g.to_(DEV)
    out, gx, pg = T._step(layer, g, x.to(torch.bfloat16).to(DEV), go.to(torch.bfloat16).to(DEV))
    g.cpu_()
    T._assert_native(calls)
    RR.check_bf16("out", out, ref[0])
    RR.check_bf16("grad_x", gx, ref[1])
    for n, r in zip(TREF.PARAMS, ref[2:]):
        RR.check_f32("grad_" + n, pg[n], r)


# ---------------------------------------------------------------- 4. the slope ladder, on the same inputs
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
def test_slopes_reference_named_pair(K, kind, slope):  # noqa: F811
    g = ladder_graph(R=5)
    OPS.fused_gat_case(K, g, kind, 4, 16, inputs=exact_gat_case_of_kind(g, kind, 4, 16, seed=17), slope=slope)


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("route", ["default", "node_major", "per_edge"])
def test_slopes_layer(route, slope, monkeypatch):
    from het_amd.backend import rgat_fused_layer as FL
    if route == "per_edge":
        monkeypatch.setattr(FL, "PER_EDGE", True)
    flag = route == "node_major"  # compact + mulfirst: the node-major backward where the guards allow it
    g, c = _layer_case()
    _run_rgat(g, H=4, K=64, X=64, compact=flag, direct=flag, mulfirst=flag, slope=slope, case=c)


def _evaluation_layer(g, c, slope, **kw):
    from het_amd.layers import HET_RGATLayer
    layer = HET_RGATLayer(64, 64, g.get_num_rels(), 4, bias=True, self_loop=True, multiply_among_weights_first_flag=True, dropout=0.0,
                          leaky_relu_slope=slope, **kw)
    x, _ = load_rgat_case(layer, c)
    s = g.get_separate_coo_original()
    p = {n: t.detach().double() for n, t in layer.named_parameters()}
    ref = OL.rgat_layer(x.double(), p["conv_weights"], p["attn_l"], p["attn_r"], s["rel_ptrs"], s["row_indices"], s["col_indices"],
                        g.get_num_nodes(), slope, p["loop_weight"], p["h_bias"])
    return layer.to(DEV), x.to(DEV), ref


@pytest.mark.parametrize("slope", SLOPES + [0.2])
def test_slopes_forward_only(slope, monkeypatch):
    """The evaluation call in fp32 -- bit-identical to the training forward, on the forward-only entry where the slope allows it
    (tests/test_gpu_rgat_forward_only.py) -- and in bf16, both against the fp64 oracle."""
    from tests import test_gpu_rgat_forward_only as F
    g, c = _layer_case()
    assert_ties_on_hub_edges(c, g.get_separate_coo_original(), g.get_num_nodes())
    layer, x, ref = _evaluation_layer(g, c, slope)
    g.to_(DEV)
    if slope >= 0:
        out_f, out_t = F._both(g, layer, x, F._count_calls(monkeypatch))
    else:  # whatever the guards pick
        with torch.no_grad():
            out_f = layer(g, x)
        out_t = layer(g, x).detach()
    with torch.no_grad():
        out_b = layer(g, x.to(torch.bfloat16))
    torch.cuda.synchronize()
    g.cpu_()
    if slope >= 0:
        assert torch.equal(out_f, out_t)
    assert_close(out_f, ref, what="out")
    assert_close(out_t, ref, what="out (training forward)")
    RR.check_bf16("out (bf16)", out_b, ref)


@pytest.mark.parametrize("slope", SLOPES + [0.2])
def test_slopes_get_attention(slope):
    from tests.test_gpu_rgat_attention import _evaluate
    g, c = _layer_case()
    s = g.get_separate_coo_original()
    assert_ties_on_hub_edges(c, s, g.get_num_nodes())
    layer, x, ref = _evaluation_layer(g, c, slope)
    a_ref, _ = A.attention_reference(c["x"].double(), c["W"].double(), c["attn_l"].double(), c["attn_r"].double(), s["rel_ptrs"],
                                     s["row_indices"], s["col_indices"], s["eids"], g.get_num_nodes(), slope)
    h, attn = _evaluate(g, layer, x)
    assert_close(attn, a_ref, what="attention")
    assert_close(h, ref, what="out")
